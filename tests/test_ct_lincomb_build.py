"""CPU-side checks of the key-free weighted sum of ciphertexts: the two entries are declared, exported and wrapped, the
ct_ops kernels compile for gfx950 without private memory, and the aggregation example is plain C (no GPU needed)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LINCOMB_ENTRIES = ("se_amd_ct_lincomb_device", "se_amd_set_lincomb_split")
LINCOMB_KERNELS = ("k_ct_lincomb<false>", "k_ct_lincomb<true>", "k_ct_lincomb_sum")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.load_package()
    p.build_library()
    return p


def test_header_declares_lincomb_entries():
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for nm in LINCOMB_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % nm, text), nm


def test_library_exports_lincomb_entries(pkg):
    L = pkg.lib()
    for nm in LINCOMB_ENTRIES:
        assert nm in pkg.EXPORTED_SYMBOLS
        assert hasattr(L, nm), nm


def test_context_has_the_methods(pkg):
    assert callable(getattr(pkg.Context, "ct_lincomb", None))
    assert callable(getattr(pkg.Context, "set_lincomb_split", None))


def test_lincomb_kernels_use_no_scratch():
    """A wave-uniform entry loop and 16-byte accesses: nothing of these kernels lives in private memory."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "ct_ops"],
                         capture_output=True, text=True, timeout=1200).stdout
    rows = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if len(f) >= 6:
            rows[" ".join(f[:-5]).replace("seamd::", "")] = (int(f[-5]), int(f[-3]), int(f[-2]))  # VGPR, scratch, occ
    assert rows, out
    for k in LINCOMB_KERNELS:
        assert k in rows, (k, sorted(rows))
        vgpr, scratch, occ = rows[k]
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {occ} waves/SIMD")
        assert scratch == 0, (k, rows[k])


def test_aggregate_example_compiles_as_plain_c(tmp_path):
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-c",
                    os.path.join(ROOT, "examples", "aggregate_roundtrip.c"), "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", str(tmp_path / "aggregate_roundtrip.o")],
                   check=True)
