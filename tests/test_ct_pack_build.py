"""CPU-side checks of slot packing: the entry is declared, exported and wrapped; the example is plain C; what
kernels/ct_pack.hip compiles to for gfx950 -- exactly the six kernels, none with scratch, none at fewer waves per SIMD than
the switch-key ring's sum kernel of the same degree, whose body they share (no GPU needed)."""
import os

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)

ENTRIES = ("se_amd_ct_pack_sp_device",)
METHODS = ("ct_pack_sp",)
KERNELS = {f"k_ct_pack_sp<{logn}, {form}>": logn for logn in (12, 13, 14) for form in ("false", "true")}


def test_header_declares_and_library_exports_the_entry(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    assert "Five facts" in text and "a per-record element list," not in text   # the block, and the gap it closes


def test_slot_pack_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "slot_pack_roundtrip.c"), tmp_path, hip=True)


def test_pack_kernels_use_no_scratch_and_keep_the_switch_sums_waves():
    rows = resource_rows("ct_pack")
    assert rows, "tools/resource_usage.py gave no table for ct_pack"
    assert set(rows) == set(KERNELS), (sorted(rows), sorted(KERNELS))
    siblings = resource_rows("ct_ops")
    assert siblings, "tools/resource_usage.py gave no table for ct_ops"
    bad = []
    for k, logn in KERNELS.items():
        vgpr, scratch, occ = rows[k]
        sib = siblings[f"k_ct_switch_sum_sp<{logn}>"]
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD (k_ct_switch_sum_sp<{logn}>: {sib[2]})")
        if scratch != 0 or occ < sib[2]:
            bad.append(f"{k}: built {rows[k]}, sibling {sib}")
    assert not bad, "(VGPRs, scratch bytes, waves per SIMD):\n" + "\n".join(bad)
