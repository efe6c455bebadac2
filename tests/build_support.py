"""What the CPU-side build tests (tests/test_cabi.py, tests/test_*_build.py) share.  Tests import helpers from here
(`from build_support import pkg, assert_entries, ...`), never from another test module; a helper that a second module
needs moves here.

- pkg: the module-scoped fixture (the loaded package with its library built).
- assert_entries: C entries are declared in the public header, exported and loadable; Context methods are callable.
- compile_only: gcc -std=gnu11 -Wall -Wextra -Werror -c of one C file.
- resource_rows: the per-kernel register / scratch / occupancy table of a kernel source, compiled once per session.
"""
import os
import re
import subprocess

import pytest

from tools import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.load_package()
    p.build_library()
    return p


def assert_entries(pkg, entries, methods=()):
    """Each entry is declared as `int name(` in include/seal_embedded_amd.h (comments stripped), listed in
    EXPORTED_SYMBOLS and present on the loaded library; each method is callable on Context."""
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = pkg.lib()
    for nm in entries:
        assert re.search(r"\bint\s+%s\s*\(" % nm, text), nm
        assert nm in pkg.EXPORTED_SYMBOLS, nm
        assert hasattr(L, nm), nm
    for nm in methods:
        assert callable(getattr(pkg.Context, nm, None)), nm


def compile_only(path, tmp_path, hip=False, extra=()):
    """Compile (not link: linking needs the HIP runtime's GPU-side dependencies at run time) one C file against
    include/.  hip: a caller that owns device memory through the HIP runtime's C API."""
    cmd = ["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-c", str(path), "-I" + os.path.join(ROOT, "include")]
    if hip:
        cmd += ["-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
    obj = tmp_path / (os.path.splitext(os.path.basename(str(path)))[0] + ".o")
    subprocess.run(cmd + list(extra) + ["-o", str(obj)], check=True)


_ROWS = {}


def resource_rows(source):
    """{kernel name without "seamd::": (VGPRs, scratch bytes, waves per SIMD)} of kernels/<source>.hip.  One compile per
    source and session (encode_encrypt takes minutes).  A compile that fails or runs out of time is cached as the
    empty table it gives, so every caller asserts that its rows are not empty."""
    if source not in _ROWS:
        try:
            table = resource_usage.table(source)
        except subprocess.TimeoutExpired:
            table = []
        _ROWS[source] = {r["kernel"].replace("seamd::", ""): (int(r["VGPRs"]), int(r["ScratchSize [bytes/lane]"]),
                                                             int(r["Occupancy [waves/SIMD]"])) for r in table}
    return _ROWS[source]
