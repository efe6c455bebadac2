"""CPU-side checks of the drop-in boundary: the shared library loads, exports every symbol that
include/seal_embedded_amd.h declares, and refuses to run without a GPU (no CPU fallback).
No compute calls are made here."""
import ctypes as C
import os
import re

import pytest

from build_support import ROOT, compile_only, pkg, resource_rows  # noqa: F401  (pkg is a fixture)
from gpu_support import check_host_tables


def declared_functions():
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\b(se_[a-z0-9_]+)\s*\(", text)
    return sorted(set(names))


def test_library_exports_every_declared_symbol(pkg):
    L = pkg.lib()
    names = declared_functions()
    assert len(names) >= 30
    for nm in names:
        assert hasattr(L, nm), f"{nm} declared in include/seal_embedded_amd.h but not exported"
    assert set(names) == set(pkg.EXPORTED_SYMBOLS)


def declared_lower_functions():
    """Every prototype of include/seal_embedded_amd_lower.h (the reference-named lower surface)."""
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd_lower.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    names = re.findall(r"\b([a-z][a-z0-9_]+)\s*\([^;{]*\)\s*;", text)
    return sorted(set(names))


def test_library_exports_the_reference_named_lower_surface(pkg):
    """ckks_encode_base, ckks_setup, reduce_set_pte, ckks_setup_s, ckks_sym_init,
    ckks_encode_encrypt_sym, ckks_next_prime_sym, gen_pk, ckks_asym_init, ckks_encode_encrypt_asym,
    ckks_next_prime_asym, ntt_roots_initialize, ntt_inpl, ifft_inpl ... under the reference's names."""
    L = pkg.lib()
    names = declared_lower_functions()
    must = {"ckks_encode_base", "ckks_setup", "reduce_set_pte", "ckks_setup_s", "ckks_sym_init",
            "ckks_encode_encrypt_sym", "ckks_next_prime_sym", "gen_pk", "ckks_asym_init",
            "ckks_encode_encrypt_asym", "ckks_next_prime_asym", "ntt_roots_initialize", "ntt_inpl",
            "ifft_inpl", "ckks_mempool_setup_sym", "ckks_set_ptrs_sym", "ckks_reset_primes",
            "sample_poly_uniform", "prng_fill_buffer", "load_sk", "load_pki"}
    assert must <= set(names), sorted(must - set(names))
    for nm in names:
        assert hasattr(L, nm), f"{nm} declared in seal_embedded_amd_lower.h but not exported"


def test_reference_named_shim_headers_and_callers_compile(tmp_path):
    """A caller that includes the reference's header NAMES (seal_embedded.h, ckks_sym.h, ntt.h, ...)
    compiles as C11 and C++17 against include/ + include/compat/; the reference-style test callers
    under tests/c/ build with -Wall -Wextra -Werror."""
    import subprocess
    inc = os.path.join(ROOT, "include")
    flags = ["-Wall", "-Wextra", "-Werror", "-I", inc, "-I", os.path.join(inc, "compat")]
    src = tmp_path / "t.c"
    src.write_text("""#include <complex.h>
#include "seal_embedded.h"
#include "defines.h"
#include "ckks_common.h"
#include "ckks_sym.h"
#include "ckks_asym.h"
#include "fft.h"
#include "ntt.h"
#include "intt.h"
#include "parameters.h"
#include "modulus.h"
#include "rng.h"
#include "sample.h"
#include "fileops.h"
int main(void)
{
    /* the reference's exact prototypes (ckks_common.h:134, ckks_sym.h:110, ntt.h:54, fft.h:98) */
    bool (*f1)(const Parms *, const flpt *, size_t, uint16_t *, double complex *, double complex *) = ckks_encode_base;
    void (*f2)(const Parms *, const int64_t *, const int8_t *, SE_PRNG *, ZZ *, ZZ *, ZZ *, ZZ *, ZZ *, ZZ *,
               ZZ *) = ckks_encode_encrypt_sym;
    void (*f3)(const Parms *, const ZZ *, ZZ *) = ntt_inpl;
    void (*f4)(double complex *, size_t, size_t, const double complex *) = ifft_inpl;
    void (*f5)(const Parms *, ZZ *, ZZ *, uint8_t *, SE_PRNG *, ZZ *, int8_t *, ZZ *, ZZ *, ZZ *) = gen_pk;
    RND_FNCT_PTR r = 0;
    SE_UNUSED(r);
    return !(f1 && f2 && f3 && f4 && f5);
}
""")
    compat = ("-I" + os.path.join(inc, "compat"),)
    compile_only(src, tmp_path, extra=compat)
    cxx = tmp_path / "t.cpp"
    cxx.write_text('#include "seal_embedded.h"\n#include "ckks_sym.h"\nint main(){ SE_PRNG p; prng_clear(&p); return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", *flags, "-c", str(cxx), "-o", str(tmp_path / "t2.o")])
    for name in ("lower_sym_caller", "lower_asym_caller"):
        compile_only(os.path.join(ROOT, "tests", "c", name + ".c"), tmp_path, extra=compat)


def test_header_cites_reference_interfaces():
    text = open(os.path.join(ROOT, "include", "seal_embedded_amd.h")).read()
    for cite in ("seal_embedded.h:91-130", "ckks_common.c:105-215", "ntt.c:168-189",
                 "sample.c:39-57", "rng.h:78-91", "fileops.c:140-204"):
        assert cite in text


def test_header_compiles_as_c_and_cxx(tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "seal_embedded_amd.h"\nint main(void){ SE_PARMS p; (void)p; return SE_SUCCESS; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", inc, "-c", str(src), "-o",
                           str(tmp_path / "t.o")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-x", "c++", "-I", inc, "-c",
                           str(src), "-o", str(tmp_path / "t2.o")])


def test_reference_struct_layouts(pkg):
    """Modulus / SE_PARMS layouts the reference's callers rely on (modulus.h:22-30,
    seal_embedded.h:52-56)."""
    class Modulus(C.Structure):
        _fields_ = [("value", C.c_uint32), ("const_ratio", C.c_uint32 * 2)]
    assert C.sizeof(Modulus) == 12


def test_no_gpu_means_loud_failure(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.SealEmbeddedAmdError) as ei:
        pkg.Context(4096, 3)
    assert "no HIP device" in str(ei.value) or "HIP" in str(ei.value)


def test_product_does_not_touch_oracle():
    """The oracle is test infrastructure: nothing under seal-embedded_amd/ may reference it."""
    bad = []
    pdir = os.path.join(ROOT, "seal-embedded_amd")
    for dp, _, files in os.walk(pdir):
        if "build" in dp.split(os.sep):
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip", ".cuh", "Makefile")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                if re.search(r"se_oracle|pyoracle|libse_ref|oracle/", txt):
                    bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_product_sources_carry_no_ab_hooks_or_wrong_result_ablations():
    """Round 6: rejected experiment forms and compile-time A/B hooks live under experiments/ as
    re-applicable diffs, not in the product sources -- a default build compiles everything that is in the kernel files,
    and no setting of the debug-flag word changes a result.  Guards: no SEAMD_* conditional compilation outside the
    test-hook build of se_api.cpp, no kernel a launcher never reaches, every experiments/*.patch is a diff with a header
    that names its evidence."""
    cdir = os.path.join(ROOT, "seal-embedded_amd", "csrc")
    hooks = []
    for dp, _, files in os.walk(cdir):
        if os.path.basename(dp).startswith("build"):
            continue
        for f in files:
            if f.endswith((".cpp", ".h", ".hip", ".cuh")):
                for i, ln in enumerate(open(os.path.join(dp, f), errors="replace"), 1):
                    m = re.match(r"\s*#\s*(?:ifdef|ifndef|if|elif)\b.*\b(SEAMD_\w+)", ln)
                    if m and m.group(1) != "SEAMD_TEST_HOOKS":
                        hooks.append((f, i, m.group(1)))
    assert not hooks, hooks
    samplers = open(os.path.join(cdir, "kernels", "samplers.hip")).read()
    for gone in ("k_bulk_lane", "keccak_f1600_sync", "spec_window", "debug_flags & 2)"):
        assert gone not in samplers, gone
    # every __global__ kernel of the kernel files is launched from the same file
    for name in ("samplers.hip", "encode_encrypt.hip", "stage_ops.hip"):
        txt = open(os.path.join(cdir, "kernels", name)).read()
        code = re.sub(r"//[^\n]*", "", txt)
        for k in set(re.findall(r"void\s+(k_\w+)\s*\(", code)):
            assert len(re.findall(r"\b" + k + r"\b", code)) >= 2, (name, k, "defined but never launched")
    edir = os.path.join(ROOT, "experiments")
    patches = [f for f in os.listdir(edir) if f.endswith(".patch")]
    assert len(patches) >= 4
    for f in patches:
        txt = open(os.path.join(edir, f)).read()
        assert txt.startswith("# experiments/" + f) and "profiles/" in txt.split("diff --git")[0] and "diff --git" in txt, f


def test_pack_ternary_host_matches_reference_format(pkg):
    import numpy as np
    L = pkg.lib()
    codes = np.array([0, 1, 2, 1, 2, 2, 0, 0], dtype=np.int8)
    out = np.zeros(2, dtype=np.uint8)
    L.se_amd_pack_ternary_host(codes.ctypes.data_as(C.c_void_p), 8, out.ctypes.data_as(C.c_void_p))
    # MSB-first 2-bit fields (sample.c:61-87): 00 01 10 01 | 10 10 00 00
    assert list(out) == [0b00011001, 0b10100000]


def test_examples_compile_as_plain_c(tmp_path):
    """The public header is valid C11 and the example callers build with gcc -Wall -Werror
    (compile only: linking needs the HIP runtime's GPU-side dependencies at run time)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("api_digest", "batch_encrypt"):
        subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-c",
                        os.path.join(root, "examples", name + ".c"), "-I" + os.path.join(root, "include"),
                        "-o", str(tmp_path / (name + ".o"))], check=True)


@pytest.mark.parametrize("shape", [(1024, 1), (2048, 1), (4096, 3), (8192, 6), (16384, 13)])
def test_host_tables_match_oracle_and_golden(pkg, shape):
    """Every setup-time table the context uploads (host logic, no GPU): gpu_support.check_host_tables."""
    check_host_tables(pkg, shape)


def _hot_path_has_no_scratch(root):
    """k_encode_encrypt<12, 0 | 2> (two plaintexts per workgroup): every scratch instruction of the compiled kernel lies in
    the exact-redo branch -- laid out behind the kernel's main body, entered by a forward branch -- i.e. none in front of the
    first prime loop and none inside a loop that carries the NTT (7-op Harvey butterflies: v_mad_u64_u32)."""
    import subprocess
    src = os.path.join(root, "seal-embedded_amd", "csrc")
    out = "/tmp/se_enc_isa.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I" + src,
                    "-I" + os.path.join(root, "include"), "-S", "--cuda-device-only",
                    os.path.join(src, "kernels", "encode_encrypt.hip"), "-o", out], check=True, capture_output=True, timeout=900)
    isa = open(out).read().split("\n")
    for mode in (0, 2):
        start = next(i for i, ln in enumerate(isa) if re.match(r"^_ZN5seamd16k_encode_encryptILi12ELi%dEEEv\w*:" % mode, ln))
        end = next(i for i in range(start, len(isa)) if isa[i].startswith(".Lfunc_end"))
        body = isa[start:end]
        scratch = [i for i, ln in enumerate(body) if "scratch_" in ln]
        mads = [i for i, ln in enumerate(body) if "v_mad_u64_u32" in ln]
        assert mads, mode
        if not scratch:
            continue
        # the hot path: everything up to the end of the FIRST block of butterflies (the tail's prime loop)
        gaps = [j for j in range(1, len(mads)) if mads[j] - mads[j - 1] > 600]
        first_loop_end = mads[gaps[0] - 1] if gaps else mads[-1]
        assert min(scratch) > first_loop_end, (mode, min(scratch), first_loop_end)


def test_hot_kernels_keep_their_register_budget():
    """Regression guard for the register budgets the throughput numbers rest on (hipcc
    -Rpass-analysis=kernel-resource-usage, tools/resource_usage.py): the fast fused kernels of
    n <= 8192 and the split kernels do not spill, and at n = 4096 the symmetric / encode-only forms fit
    4 workgroups per CU (<= 128 VGPRs), the public-key form 3 (<= 168 VGPRs: round 4, global addresses formed per
    prime from an opaque thread index instead of being carried across the prime loop -- 206 VGPRs before)."""
    rows = resource_rows("encode_encrypt")
    assert len(rows) > 30, rows
    for logn in (10, 11, 12, 13):
        for mode in (0, 1, 2):
            vgpr, scratch, occ = rows[f"k_encode_encrypt<{logn}, {mode}>"]
            if logn == 12 and mode != 1:
                # round 6: the pair form keeps the SECOND plaintext's coefficients in registers across the exact redo of a
                # plaintext in the guard band (about 1 workgroup in 25): that branch may spill, the hot path must not --
                # _hot_path_has_no_scratch below reads the ISA
                assert scratch <= 96, (logn, mode, scratch)
            else:
                assert scratch == 0, (logn, mode, scratch)
    _hot_path_has_no_scratch(ROOT)
    for mode in (0, 2):
        assert rows[f"k_encode_encrypt<12, {mode}>"][0] <= 128 and rows[f"k_encode_encrypt<12, {mode}>"][2] >= 4
    assert rows["k_encode_encrypt<12, 1>"][0] <= 168 and rows["k_encode_encrypt<12, 1>"][2] >= 3
    assert rows["k_encode_encrypt<13, 1>"][0] <= 128          # n = 8192 public key: 4 waves per SIMD (159 VGPRs before)
    assert rows["k_encode_encrypt<14, 1>"][1] <= 32           # n = 16384 public key: 440 B of scratch before round 4
    for k in ("k_ntt_fuse<12, 0>", "k_ntt_fuse<14, 0>", "k_encode_rns<12, true>", "k_encode_rns<14, true>",
              "k_encode_encrypt<14, 0>", "k_encode_encrypt<14, 2>"):
        assert rows[k][1] == 0, (k, rows[k])
    # the samplers: the batch form of the chain kernel at 160 VGPRs without spills (its per-lane-prime form must
    # not leak into it), the staged kernels light enough to sit beside a transform workgroup
    rows = resource_rows("samplers")
    assert rows, "tools/resource_usage.py gave no table for samplers"
    assert rows["k_sample_uniform<12, 512, false>"][0] <= 168 and rows["k_sample_uniform<12, 512, false>"][1] == 0
    assert rows["k_sample_uniform<14, 512, false>"][1] == 0
    for k, vg in (("k_bulk_pair<14>", 80), ("k_bulk_pair<12>", 80), ("k_candidates", 80), ("k_resolve_light<14>", 40),
                  ("k_sample_cbd", 80)):
        assert rows[k][0] <= vg and rows[k][1] == 0, (k, rows[k])
