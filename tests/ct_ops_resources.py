"""The resource table of kernels/ct_ops.hip: every kernel the file compiles to, as build_support.resource_rows("ct_ops")
names it, with what tests/test_ct_ops_build.py holds it to.  Plain data, imported like build_support.  A rule has at most
    scratch   exact bytes per lane
    waves     ("==", n) or (">=", n) waves per SIMD; absent: no floor of its own
    vgprs     exact count
    at_least  names of siblings: at least the waves per SIMD the same report gives each of them
Adding a kernel to the file means adding a row here.  The VGPR figures in the comments are as built (python
tools/resource_usage.py ct_ops), for logn 10 .. 14 or, in the special-prime families, 12 / 13 / 14."""
ALL = range(10, 15)
SP = (12, 13, 14)          # a context with a special prime has np >= 2, which the default chains give from n = 4096 on


def family(names, logns, at_least=(), **rule):
    """{name: rule} at 0 scratch for every logn; `names` (one or a tuple) and the siblings in `at_least` are written with
    {logn}, as in "k_ct_galois_hoist<{logn}, true>"."""
    names = (names,) if isinstance(names, str) else names
    return {n.format(logn=logn): {"scratch": 0, **rule,
                                  **({"at_least": tuple(a.format(logn=logn) for a in at_least)} if at_least else {})}
            for n in names for logn in logns}


KERNELS = {
    # a wave-uniform entry loop and 16-byte accesses; the tensor kernel, the key plumbing and the fold kernel: nothing of
    # these lives in private memory.  k_ct_mul_sum is k_ct_mul with the pair loop inside and three 64-bit accumulator
    # quads: 66 VGPRs beside k_ct_mul's 45
    **{k: {"scratch": 0} for k in ("k_ct_lincomb<false>", "k_ct_lincomb<true>", "k_ct_lincomb_sum", "k_ct_mul_plain",
                                   "k_ct_mul", "k_ct_mul_sum", "k_relin_key_rows", "k_lintrans_fold")},
    # a tile of four records, 64-bit sums
    "k_ct_mul_plain_sum": {"scratch": 0, "waves": ("==", 8), "vgprs": 64},
    # the 16 signed values a rescale thread carries across the prime loop, its transform tile and the input row all stay
    # in registers: 95 / 101 / 131 / 125 / 127 VGPRs (a floor of its own per degree, so no family())
    **{f"k_ct_rescale<{logn}>": {"scratch": 0, "waves": ("==", w)} for logn, w in zip(ALL, (5, 4, 3, 4, 4))},
    # k_ct_mod_down_sp<logn> has the rows of k_ct_rescale<logn>: 131 / 125 / 127 VGPRs, 3 / 4 / 4 waves
    **family("k_ct_mod_down_sp<{logn}>", SP, at_least=("k_ct_rescale<{logn}>",)),
    # the two digit key-switch kernels: two 16-value accumulators, the coefficient tile, the digit tile and two key rows
    # per thread.  Their waves before they shared their device code (106 / 107 / 107 / 109 / 114 VGPRs for k_ct_relin,
    # 124 / 125 / 125 / 106 / 105 for k_ct_galois): the floor the shared helpers must not cost a wave of
    **family(("k_ct_relin<{logn}>", "k_ct_galois<{logn}>"), ALL, waves=(">=", 4)),
    # k_ct_galois_accum<logn> is k_ct_galois<logn> with the element loop inside: ONE accumulator pair across the
    # elements, sigma(c0) added to it.  118 / 119 / 120 / 122 / 108 VGPRs beside the rotation's 124 / 125 / 125 / 102 / 105
    **family("k_ct_galois_accum<{logn}>", ALL, at_least=("k_ct_galois<{logn}>",)),
    **family("k_bsgs_permute<{logn}>", ALL),
    # k_ct_galois_hoist<logn, SUM>: the sum form carries one accumulator pair like its siblings k_ct_relin / k_ct_galois
    # and keeps their 4 (107 / 122 / 121 / 127 / 111 VGPRs); the many form carries kHoistGroup = 2 pairs, 139 / 154 / 153 /
    # 159 VGPRs and 3 waves for logn 10 .. 13, and at logn 14, where the workgroup of 1024 threads is 4 waves per SIMD by
    # itself, 128 VGPRs with the coefficients of the input row parked in LDS
    **family("k_ct_galois_hoist<{logn}, true>", ALL, waves=("==", 4)),
    **family("k_ct_galois_hoist<{logn}, false>", (10, 11, 12, 13), waves=("==", 3)),
    **family("k_ct_galois_hoist<{logn}, false>", (14,), waves=("==", 4)),
    # k_ct_lintrans<logn> carries the accumulator pair of k_ct_galois_hoist<logn, true> and a weighted epilogue that
    # starts when the transform's registers are dead: 127 / 121 / 121 / 126 / 111 VGPRs beside the sibling's
    **family("k_ct_lintrans<{logn}>", ALL, waves=("==", 4), at_least=("k_ct_galois_hoist<{logn}, true>",)),
    # the diagonal kernels of the key generators exist for every degree
    **family(("k_evk_diag<{logn}, true>", "k_evk_diag<{logn}, false>", "k_evk_diag_sp<{logn}, true>",
              "k_evk_diag_sp<{logn}, false>", "k_evk_diag_switch_sp<{logn}>"), ALL),
    # the special-prime key switch, the family's 4 everywhere: 113 / 115 / 119 VGPRs for k_ct_relin_sp, 113 / 97 / 97 for
    # k_ct_galois_sp; the hoisted sum and the linear transform on the same key share their helpers and their 4
    **family(("k_ct_relin_sp<{logn}>", "k_ct_galois_sp<{logn}>", "k_ct_galois_sum_sp<{logn}>", "k_ct_lintrans_sp<{logn}>"),
             SP, waves=("==", 4)),
    # k_ct_galois_many_ext_sp<logn> is one pass of k_ct_galois_sum_sp<logn> with kManyExtGroup = 2 accumulator pairs:
    # 123 / 124 / 124 VGPRs beside the sum form's 122 / 115 / 126
    **family("k_ct_galois_many_ext_sp<{logn}>", SP, at_least=("k_ct_galois_sum_sp<{logn}>",)),
    # k_ct_galois_accum_sp<logn> is k_ct_galois_sp<logn> with the element loop inside each pass: 122 / 119 / 121 VGPRs
    # beside the single rotation's 113 / 97 / 97
    **family("k_ct_galois_accum_sp<{logn}>", SP, at_least=("k_ct_galois_sp<{logn}>",)),
    # k_ct_switch_sp<logn> and k_ct_switch_sum_sp<logn> are k_ct_relin_sp<logn> with the record loop inside each pass and
    # the key pointer taken per record: 101 / 117 / 120 and 117 / 121 / 120 VGPRs beside the relinearisation's
    **family(("k_ct_switch_sp<{logn}>", "k_ct_switch_sum_sp<{logn}>"), SP, waves=(">=", 4)),
    # k_ct_dot_sp<logn> is k_ct_relin_sp<logn> with every row it would load formed in registers, a quad at a time:
    # 95 / 120 / 122 VGPRs beside the relinearisation's 113 / 115 / 119
    **family("k_ct_dot_sp<{logn}>", SP, waves=(">=", 4)),
}
