"""CPU checks of the owning handles in seal-embedded_amd/csrc/se_devmem.h: the header is compiled with plain g++ into
tests/c/devmem_driver.cpp, whose stub of the HIP runtime logs every call the handles make (no GPU, no runtime
library).  Plus a source guard: the host code allocates, frees and destroys GPU resources through that header only."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seal-embedded_amd", "csrc")
HEADER = os.path.join(CSRC, "se_devmem.h")


@pytest.fixture(scope="module")
def log(tmp_path_factory):
    if not shutil.which("g++") or not os.path.exists(HEADER):
        pytest.skip("needs g++ and se_devmem.h")
    exe = str(tmp_path_factory.mktemp("devmem") / "devmem_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I" + CSRC, os.path.join(ROOT, "tests", "c", "devmem_driver.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    scenarios, cur = {}, None
    for line in out.splitlines():
        if line.startswith("== "):
            cur = scenarios.setdefault(line[3:], [])
        else:
            cur.append(line)
    return scenarios


def test_secret_devbuf_is_zeroed_then_freed_on_growth_and_destruction(log):
    assert log["secret_grow"] == [
        "hipMalloc 400 -> a1",
        "grow 0",
        "grow 0",                      # at capacity: no call
        "grow 0",                      # below capacity: no call
        "hipMemset a1 0 400 of 400",   # growth: the whole old allocation is zeroed ...
        "hipFree a1 zero=1",           # ... before it is freed
        "hipMalloc 800 -> a2",
        "grow 0",
        "size 200",
        "hipMemset a2 0 800 of 800",   # destruction: the same
        "hipFree a2 zero=1",
    ]


def test_plain_devbuf_is_freed_without_a_memset(log):
    assert log["plain"] == ["hipMalloc 20 -> a3", "hipFree a3 zero=0", "hipMalloc 60 -> a4", "hipFree a4 zero=0"]


def test_failed_allocation_leaves_the_buffer_empty_and_returns_the_error(log):
    assert log["failed_alloc"] == [
        "hipMalloc 16 -> a5", "hipMemset a5 0 16 of 16", "hipFree a5 zero=1", "hipMalloc 32 -> error",
        "error 1 null=1 size 0",       # and its destruction makes no call
    ]


def test_moved_from_buffer_frees_nothing_and_the_allocation_is_freed_once(log):
    assert log["move"] == [
        "hipMalloc 32 -> a6",
        "moved null=1 size 0",
        "hipMalloc 16 -> a7",
        "hipFree a7 zero=0",           # move assignment releases what the target held
        "moved null=1 size 0",
        "holder size 4",
        "hipMemset a6 0 32 of 32",     # the secret allocation keeps its policy through the moves
        "hipFree a6 zero=1",
    ]
    assert log["end"] == ["live 0"]


def test_secret_pinned_buffer_is_all_zero_when_freed(log):
    assert log["pinned"] == [
        "hipHostMalloc 64 -> a8",
        "hipHostMalloc 64 -> a9",
        "hipHostFree a8 zero=1",       # growth of the secret one
        "hipHostMalloc 128 -> a10",
        "hipHostFree a9 zero=0",       # not secret: left as it is
        "hipHostFree a10 zero=1",
    ]


def test_streams_and_events_are_destroyed_once_and_only_when_created(log):
    assert log["handles_empty"] == ["null=1"]
    assert log["handles"] == [
        "hipStreamCreateWithFlags 1 -> s1",   # a second create() on a held stream makes no call
        "hipEventCreateWithFlags 2 -> e1",
        "moved null=1",
        "hipEventDestroy e1",
        "hipStreamDestroy s1",
    ]


def test_host_code_owns_gpu_resources_only_through_se_devmem_h():
    calls = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree|hipStreamDestroy|hipEventDestroy)\(")
    found = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.h"))):
        if os.path.basename(path) == "se_devmem.h":
            continue
        with open(path) as f:
            for i, line in enumerate(f, 1):
                if calls.search(line):
                    found.append(f"{os.path.relpath(path, ROOT)}:{i}: {line.strip()}")
    assert not found, "raw GPU resource calls outside se_devmem.h:\n" + "\n".join(found)
