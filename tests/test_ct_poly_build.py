"""CPU-side checks of the slot-wise polynomials: the entries are declared, exported and wrapped; the example is plain C;
what kernels/ct_poly.hip compiles to for gfx950 -- exactly k_ct_affine_rescale<12 | 13 | 14>, none with scratch, none at
fewer waves per SIMD than the lower of the two kernels whose bodies it joins, k_ct_rescale and k_ct_dot_sp of the same
degree (no GPU needed)."""
import os
import re

from build_support import ROOT, assert_entries, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)

ENTRIES = ("se_amd_ct_affine_rescale_device", "se_amd_poly_create", "se_amd_poly_result", "se_amd_ct_poly_sp_device")
OTHERS = ("se_amd_poly_destroy", "se_amd_poly_terms", "se_amd_poly_workspace_bytes")       # void and size_t entries
METHODS = ("ct_affine_rescale", "ct_poly_sp", "poly_workspace_bytes")
KERNELS = {f"k_ct_affine_rescale<{logn}>": logn for logn in (12, 13, 14)}


def test_header_declares_and_library_exports_the_entries(pkg):
    assert_entries(pkg, ENTRIES, methods=METHODS)
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    for nm in OTHERS:
        assert re.search(r"\b(void|size_t)\s+%s\s*\(" % nm, text), nm
        assert nm in pkg.EXPORTED_SYMBOLS and hasattr(pkg.lib(), nm), nm
    for nm in ("poly_create", "poly_terms", "poly_result", "PolyPlan"):
        assert callable(getattr(pkg, nm, None)), nm
    assert re.search(r"^#define\s+SE_AMD_AFFINE_MAX_TERMS\s+16\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+SE_AMD_POLY_MAX_DEGREE\s+15\s*$", text, flags=re.M)


def test_poly_activation_example_compiles_as_plain_c(tmp_path):
    compile_only(os.path.join(ROOT, "examples", "poly_activation_roundtrip.c"), tmp_path, hip=True)


def test_affine_rescale_kernels_use_no_scratch_and_keep_their_siblings_waves():
    rows = resource_rows("ct_poly")
    assert rows, "tools/resource_usage.py gave no table for ct_poly"
    assert set(rows) == set(KERNELS), (sorted(rows), sorted(KERNELS))
    siblings = resource_rows("ct_ops")
    assert siblings, "tools/resource_usage.py gave no table for ct_ops"
    bad = []
    for k, logn in KERNELS.items():
        vgpr, scratch, occ = rows[k]
        floor = min(siblings[f"k_ct_rescale<{logn}>"][2], siblings[f"k_ct_dot_sp<{logn}>"][2])
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD (k_ct_rescale<{logn}>: "
              f"{siblings[f'k_ct_rescale<{logn}>'][2]}, k_ct_dot_sp<{logn}>: {siblings[f'k_ct_dot_sp<{logn}>'][2]})")
        if scratch != 0 or occ < floor:
            bad.append(f"{k}: built {rows[k]}, floor {floor}")
    assert not bad, "(VGPRs, scratch bytes, waves per SIMD):\n" + "\n".join(bad)
