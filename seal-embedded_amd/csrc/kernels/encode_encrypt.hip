// encode_encrypt.hip -- one workgroup per plaintext: CKKS encode (FP64 inverse FFT) -> add the
// sampled error -> per RNS prime {signed reduction -> forward NTT -> fused ciphertext arithmetic}.
//
// Replaces, for a whole batch at once:
//   ckks_encode_base          /root/reference/device/lib/ckks_common.c:105-215
//   ifft_inpl                 /root/reference/device/lib/fft.c:69-144
//   reduce_set_pte / _e_small /root/reference/device/lib/ckks_common.c:224-265
//   ntt_inpl                  /root/reference/device/lib/ntt.c:124-189
//   the per-prime bodies of ckks_encode_encrypt_sym (ckks_sym.c:199-301) and
//   ckks_encode_encrypt_asym (ckks_asym.c:205-286) incl. poly_*_mod_inpl (polymodarith.h:39-101)
//
// Data never leaves the CU between encode and the final store: the plaintext stays in VGPRs
// (int32 x 16 per thread in the fast form, int64 in the general form -- see encrypt_one) across all
// primes; LDS is only the re-deal buffer of the transforms.
// HBM traffic per ciphertext = values (2n B) + error bytes + a (read back, 4n*np) + c0 (4n*np).
//
// NTT(s) is a per-key constant: it is computed once when the key is set (k_ntt_polys below)
// instead of once per ciphertext as the reference does -- same values, 1/2 of the NTT work.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../se_types.h"
#include "kernel_args.h"
#include "launch.h"
#include "transform.cuh"

namespace seamd {

__device__ __forceinline__ void load16(uint32_t (&v)[16], const uint32_t *p)
{
    const uint4 *p4 = reinterpret_cast<const uint4 *>(p);
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
        uint4 w      = p4[i];
        v[4 * i]     = w.x;
        v[4 * i + 1] = w.y;
        v[4 * i + 2] = w.z;
        v[4 * i + 3] = w.w;
    }
}

__device__ __forceinline__ void store16(uint32_t *p, const uint32_t (&v)[16])
{
    uint4 *p4 = reinterpret_cast<uint4 *>(p);
#pragma unroll
    for (int i = 0; i < 4; i++) p4[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}

// 16 interleaved (value, shoup) pairs starting at pair index `first`
__device__ __forceinline__ void load16_pairs(uint32_t (&w)[16], uint32_t (&wp)[16],
                                             const uint32_t *tab, size_t first)
{
    const uint4 *p4 = reinterpret_cast<const uint4 *>(tab + 2 * first);
#pragma unroll
    for (int i = 0; i < 8; i++)
    {
        uint4 v       = p4[i];
        w[2 * i]      = v.x;
        wp[2 * i]     = v.y;
        w[2 * i + 1]  = v.z;
        wp[2 * i + 1] = v.w;
    }
}

// (the quad-layout accessors load_quads / store_quads live beside tile_to_quads in transform.cuh)
//
// Key rings (kernel_args.h, KeyRing): the keyed kernels read the key rows of record b from key idx[b] of the ring.  b is
// workgroup-uniform (one plaintext per workgroup, or per half of the pair form), so the key's offset is one scalar word
// (readfirstlane of the index) times the key stride: SGPRs only, and the per-prime offsets (kb) are the single key's.
__device__ __forceinline__ size_t key_base(const KeyRing &R, size_t b)
{
    return (size_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)R.idx[b]) * R.stride;
}

// the tables with the key rows of the ring key at word offset kb
__device__ __forceinline__ DevTables with_key(const DevTables &T, const KeyRing &R, size_t kb)
{
    DevTables Tk = T;
    Tk.s_hat     = R.k0 + kb;
    Tk.pk0       = R.k0 + kb;
    Tk.pk1       = R.k1 + kb;
    return Tk;
}

// interleaved (value, shoup) pairs of one polynomial's table, quad layout
__device__ __forceinline__ void load_quads_pairs(uint32_t (&w)[16], uint32_t (&wp)[16], const uint32_t *tab,
                                                 int t)
{
    const uint32_t *base = tab + 2 * (size_t)quad_index(t, 0);
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
        const uint4 *p4 = reinterpret_cast<const uint4 *>(base + (i << 9));
        const uint4 a = p4[0], b = p4[1];
        w[4 * i] = a.x, wp[4 * i] = a.y, w[4 * i + 1] = a.z, wp[4 * i + 1] = a.w;
        w[4 * i + 2] = b.x, wp[4 * i + 2] = b.y, w[4 * i + 3] = b.z, wp[4 * i + 3] = b.w;
    }
}

// epilogue accessors in whichever layout the kernel's outputs are in: quad layout after tile_to_quads,
// else the thread's 16 consecutive coefficients
template <bool QUADS>
__device__ __forceinline__ void ld_poly(uint32_t (&v)[16], const uint32_t *poly, int t)
{
    if constexpr (QUADS) load_quads(v, poly, t); else load16(v, poly + 16 * t);
}
template <bool QUADS>
__device__ __forceinline__ void st_poly(uint32_t *poly, const uint32_t (&v)[16], int t)
{
    if constexpr (QUADS) store_quads(poly, v, t); else store16(poly + 16 * t, v);
}
template <bool QUADS>
__device__ __forceinline__ void ld_pairs(uint32_t (&w)[16], uint32_t (&wp)[16], const uint32_t *tab, int t)
{
    if constexpr (QUADS) load_quads_pairs(w, wp, tab, t); else load16_pairs(w, wp, tab, (size_t)16 * t);
}

// ------------------------------------------------------------------------------------------
// Encode front end shared by the fused and the split kernels: values -> LDS -> gather through the
// inverse index map -> inverse FFT -> round to int64 (+ overflow status).  On return thread t owns
// the plaintext coefficients k = t + (n/16)*e, e = 0..15, and the workgroup is synchronised.
// ------------------------------------------------------------------------------------------
//
// MT = int64_t: the general form.  MT = int32_t: the FAST form of the fused kernel -- the coefficients are
// only meaningful when `small` comes back true for every wave of the workgroup (|m| < 2 q_min - 64 < 2^31);
// the caller hands every other plaintext to the general kernel (k_encode_encrypt_general).
// The general kernel walks a list in a loop; seen as loop-invariant, the thread's table loads (twiddles,
// gather map, roots, key rows) would be hoisted out of that loop and the kernel spills.  Its thread index
// therefore passes through an opaque asm (a fresh value per iteration as far as the compiler knows).
template <bool OPAQUE>
__device__ __forceinline__ int thread_index()
{
    if constexpr (OPAQUE)
    {
        int t = threadIdx.x;
        __asm__ volatile("" : "+v"(t));
        return t;
    }
    else
        return threadIdx.x;
}

// C round() (half away from zero; ckks_common.c:183,192) as trunc(x + copysign(0.5 - 2^-54, x)): 3 operations
// (v_bfi, v_add_f64, v_trunc_f64) instead of the 6-7 of the library form (trunc, subtract, compare, select,
// copysign, add).  Exact for every double: with c = pred(0.5), a fraction below 0.5 can never be carried to the
// next integer (x + c stays below it by more than half an ulp), a fraction of 0.5 or more always is (x + c is
// within 2^-54 of the next integer, less than half a spacing -- and for x = 0.5 the tie 1 - 2^-54 rounds to even =
// 1.0); |x| >= 2^52 is an integer already and absorbs c; NaN / infinity pass through.  Checked exhaustively
// through the parity suite (every record of C2 / C3 / C4 / C5 against the oracle's round()) and on the host for
// the boundary cases (tests/test_oracle.py::test_round_half_away_form).
__device__ __forceinline__ double round_half_away(double x)
{
    const double c = 0.49999999999999994;   // 0.5 - 2^-54
    return trunc(__dadd_rn(x, dev_copysign(c, x)));
}

// Workgroup-wide outcome of the encoder (one OR-reduction over the workgroup, returned in `wg`):
constexpr int kWgOverflow  = 1;   // a coefficient fails the reference's overflow test (ckks_common.c:195)
constexpr int kWgNotSmall  = 2;   // some |m| >= 2 q_min - 64 (or a non-finite value in the fast form)
constexpr int kWgNonfinite = 4;   // int64 form: the plaintext holds a NaN or an infinite value
// BRANCH_EXACT (int64 form only): a plaintext with a NaN / infinite value takes the EXACT transform
// (transform.cuh, cmul_annexg), chosen by a workgroup-uniform branch -- the general kernels.  Without it the
// int64 form (k_encode_rns, whose register budget the second transform would cost 30 VGPRs) only REPORTS
// kWgNonfinite: its outputs are then meaningless, no status is written and the caller hands the plaintext
// to its general kernel.
template <int LOGN, typename MT, bool BRANCH_EXACT>
__device__ __forceinline__ void encode_plaintext(const DevParams &P, const DevTables &T,
                                                 const float *values, uint8_t *status, size_t b,
                                                 unsigned char *smem, MT (&m)[16], bool &small, int &wg)
{
    static_assert(sizeof(MT) == 8 || !BRANCH_EXACT, "the fast form never sees a non-finite plaintext through");
    const int t = thread_index<sizeof(MT) == 8>();
    using G          = XformGeom<LOGN>;
    constexpr int N  = G::N;
    constexpr int TH = G::THREADS;
    double *plane    = reinterpret_cast<double *>(smem);
    float *sv        = reinterpret_cast<float *>(smem);

    // ckks_common.c:139-153 scatters values[i] to both conjugate slots; the map is a bijection
    // onto [0,n), so slot k is filled from values[inv_map[k] mod n/2].  The staging array is laid out
    // through sv_slot() (se_types.h) so that the gather is bank-conflict-free; gather_map holds the
    // LDS position directly.
    //
    // NaN and infinite values are legal inputs of the reference (a NaN coefficient passes its overflow
    // test and is stored as INT64_MIN, ckks_common.c:195-206; an infinite one is the `return false`), and
    // they are the ONLY way a non-finite number enters the transform (|value| <= FLT_MAX keeps every
    // intermediate below 2^143).  Each thread folds the values it stages into v * 0 + acc, which is NaN
    // exactly when one of them is NaN or infinite (four v_pk_fma_f32): the fast form declines such a
    // plaintext (`small` comes back false), the general form takes the EXACT transform (transform.cuh,
    // cmul_annexg) for it.
    typedef float v2f __attribute__((ext_vector_type(2)));
    v2f nfacc = {0.0f, 0.0f};
    {
        const float4 *src = reinterpret_cast<const float4 *>(values + b * (N / 2));
        static_assert((N / 8) % TH == 0, "every thread stages the same number of float4 pieces");
#pragma unroll
        for (int k = 0; k < (N / 8) / TH; k++)
        {
            const int i    = t + k * TH;
            const float4 v = src[i];
            nfacc          = __builtin_elementwise_fma(v2f{v.x, v.y}, v2f{0.0f, 0.0f}, nfacc);
            nfacc          = __builtin_elementwise_fma(v2f{v.z, v.w}, v2f{0.0f, 0.0f}, nfacc);
            sv[sv_slot(4u * i, LOGN)]      = v.x;
            sv[sv_slot(4u * i + 1u, LOGN)] = v.y;
            sv[sv_slot(4u * i + 2u, LOGN)] = v.z;
            sv[sv_slot(4u * i + 3u, LOGN)] = v.w;
        }
    }
    const float nfsum    = nfacc.x + nfacc.y;
    const bool nonfinite = nfsum != nfsum;   // this thread staged a NaN or an infinity
    bool wg_nonfinite    = false;            // workgroup-uniform
    if constexpr (BRANCH_EXACT)
        wg_nonfinite = __syncthreads_or(nonfinite) != 0;
    else
        __syncthreads();
    double re[16], im[16];
    {
        // [2][n/16] uint4: half h of thread t's 16 entries at row h -- a wave load covers 1 KiB contiguous
        const uint4 *mp = reinterpret_cast<const uint4 *>(T.gather_map);
        uint4 m0 = mp[t], m1 = mp[TH + t];
        uint32_t packed[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            uint32_t idx = (packed[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
            re[e]        = (double)sv[idx];
            im[e]        = 0.0;
        }
    }
    __syncthreads();

    // inverse FFT (no 1/n: folded into n_inv, ckks_common.c:183); real input: short butterflies in pass 0
    if constexpr (BRANCH_EXACT)
    {
        if (wg_nonfinite)
            ifft_tiles<LOGN, false, true>(re, im, T.ifft_w, plane, t);
        else
            ifft_tiles<LOGN, true>(re, im, T.ifft_w, plane, t);
    }
    else
        ifft_tiles<LOGN, true>(re, im, T.ifft_w, plane, t);

    // round to int64, overflow check (ckks_common.c:183-206).  The largest magnitude of the thread
    // serves both the overflow test and the wave-uniform "small" flag: when every coefficient of
    // the wave stays below 2 q_min - 64 (< 2^31; the normal case, |m| ~ scale * |value|; the margin
    // covers the error term added later, |e| <= 21) the int64 conversion is one v_cvt_i32_f64 plus a
    // sign extension, and the per-prime "reduction" is the single add m + 2q (modarith.cuh).
    double amax = 0.0;
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        re[e] = round_half_away(__dmul_rn(re[e], P.n_inv));
        amax  = fmax(amax, fabs(re[e]));
    }
    // fmax() skips NaNs: a NaN coefficient is not an overflow for the reference (ckks_common.c:195)
    const int ok = !(amax > 9223372036854775808.0);
    if constexpr (sizeof(MT) == 4)
    {
        small = __all(amax < P.small_bound && !nonfinite);
#pragma unroll
        for (int e = 0; e < 16; e++) m[e] = (int32_t)re[e];
    }
    else
    {
        small = __all(amax < P.small_bound && !nonfinite) && !wg_nonfinite;
        if (small)
        {
#pragma unroll
            for (int e = 0; e < 16; e++) m[e] = (int64_t)(int32_t)re[e];
        }
        else
        {
            // the reference's x86-64 build converts with cvttsd2si: NaN and +2^63 (which passes its check: it
            // rejects only > 2^63) come out as the "integer indefinite" INT64_MIN; the device conversion
            // saturates and maps NaN to 0
#pragma unroll
            for (int e = 0; e < 16; e++)
                m[e] = (fabs(re[e]) < 9223372036854775808.0) ? (int64_t)re[e] : INT64_MIN;
        }
    }
    // ONE reduction over the workgroup carries everything the callers need
    wg = __ockl_wgred_or_i32((ok ? 0 : kWgOverflow) | (small ? 0 : kWgNotSmall) | (nonfinite ? kWgNonfinite : 0));
    if constexpr (sizeof(MT) == 4)
    {
        // fast form: `small` for the whole workgroup (it implies "no overflow"); a plaintext that is not
        // small gets its status from the general kernel
        small = !(wg & kWgNotSmall);
        if (status && t == 0 && small) status[b] = 1;
    }
    else
    {
        const bool declined = !BRANCH_EXACT && (wg & kWgNonfinite);
        if (status && t == 0 && !declined) status[b] = (wg & kWgOverflow) ? 0 : 1;
    }
}

// ------------------------------------------------------------------------------------------
// The fused kernel comes in two forms.
//   FAST (GENERAL = false): the plaintext is carried as int32 -- every |m + e| of a normal plaintext is
//     below 2 q_min (|m| ~ scale * |value| ~ 2^30) -- which frees the 16 VGPRs of the high words and the
//     code of the 64-bit reduction: 164 -> 126 VGPRs (n = 4096 symmetric: 4 workgroups per CU instead of
//     3), the public-key form fits the quad-layout epilogue without spills.  A workgroup whose plaintext
//     is NOT small (any wave) appends its index to A.general and leaves without writing outputs.
//   GENERAL: int64 plaintext, the exact signed 64-bit reduction (reduce_pte_core, ckks_common.c:224-237);
//     k_encode_encrypt_general walks the list the fast launch produced (normally empty: the launch costs
//     a few microseconds).
// ------------------------------------------------------------------------------------------
template <int MODE>
constexpr int enc_quad_stride()
{
    return MODE == kModeAsym ? 28 : 20;
}

// pair form of the fast kernels (encrypt_pair below)
constexpr int kWgRisky          = 8;   // a coefficient within the guard band of a half-integer
constexpr double kHalfDelta     = 3.0e-14 * 1.001;
constexpr size_t kPairParkWords = 5120;   // parked coefficients start here (32-bit words into the dynamic LDS)

// Everything behind the encoder for ONE plaintext whose coefficients k = t + (n/16) e sit in m[]: + error, per prime
// {representative, NTT, fused ciphertext arithmetic}.  PAIR: the caller transforms two plaintexts per workgroup
// (encrypt_pair) and parks the second one's coefficients in LDS behind the first 5 120 words (kPairParkWords) -- the
// transpose region then lives inside the NTT plane (one workgroup barrier more per prime: measured neutral,
// profiles/r05_ab_qalias28.log).
template <int LOGN, int MODE, bool GENERAL, bool PAIR, typename MT>
__device__ __forceinline__ void encrypt_tail(const DevParams &P, const DevTables &T, const EncArgs &A,
                                             const size_t b, unsigned char *smem, MT (&m)[16], const bool small)
{
    const int t = thread_index<GENERAL>();
    using G            = XformGeom<LOGN>;
    constexpr bool ASYM3 = LOGN <= 12;  // three-way NTT per prime (three LDS planes; spills at n = 8192)
    constexpr int N    = G::N;
    constexpr int CTOP = LOGN - 4;
    uint32_t *lds32 = reinterpret_cast<uint32_t *>(smem);

    const int np   = P.nprimes;

    // thread t owns points k = t + (n/16)*e
    if constexpr (MODE == kModeSym)
    {
#pragma unroll
        for (int e = 0; e < 16; e++) m[e] += A.err[b * N + (e << CTOP) + t];
    }
    else if constexpr (MODE == kModeAsym)
    {
#pragma unroll
        for (int e = 0; e < 16; e++) m[e] += A.err[b * 2 * N + (e << CTOP) + t];
    }
    if (A.pte)
    {
#pragma unroll
        for (int e = 0; e < 16; e++) A.pte[b * N + (e << CTOP) + t] = m[e];
    }

    // ---- 4. per prime ----------------------------------------------------------------------
    if constexpr (MODE == kModeEncodeOnly)
    {
        if (!A.c0) return;  // plain ckks_encode_base: only the int64 plaintext was requested
    }
    // Outputs leave the kernel in quad layout (n <= 4096): the wave-local transpose region sits behind the
    // NTT plane(s), so it needs no barrier against the next prime's exchanges.  Symmetric / encode-only:
    // rows of 20 words (32 conflict cycles per transpose instead of the 16 of 28-word rows,
    // tools/lds_conflicts.py) keep plane + region at 37 KiB -- 4 workgroups per CU.  Public-key form: rows
    // of 28 INSIDE the three planes (QALIAS below: 51 KiB, 3 workgroups per CU at 150 VGPRs); its general form
    // keeps the tile layout (three transposes beside the int64 plaintext spill).
    constexpr bool QUADS   = LOGN <= 12 && (MODE != kModeAsym || !GENERAL);
    constexpr int QSTRIDE  = enc_quad_stride<MODE>();
    // The public-key form's transpose region lives INSIDE its three planes (free after the last exchange's
    // trailing barrier; one workgroup barrier per prime keeps the next prime's first exchange off it): 51 KiB per
    // workgroup instead of 79, THREE workgroups per CU -- possible since the kernel needs 150 VGPRs (opaque_index
    // above; 206 before).  Fused stage 5.09 -> 4.83 ms per 65 536 (profiles/r04_ab_transform.log).  (The same alias
    // for the symmetric / encode-only forms, 28-word rows: no gain, profiles/r05_ab_qalias28.log.)
    constexpr bool QALIAS  = (MODE == kModeAsym && ASYM3 && !GENERAL) || PAIR;
    static_assert(!PAIR || (size_t)(G::N / 16) * QSTRIDE <= kPairParkWords, "the transpose region ends below the parked plaintext");
    static_assert(!PAIR || (size_t)G::SLOTS <= kPairParkWords, "the NTT plane ends below the parked plaintext");
    uint32_t *qlds         = lds32 + (QALIAS ? 0 : (MODE == kModeAsym && ASYM3 ? 3 : 1)) * G::SLOTS;
    auto to_quads = [&](uint32_t (&v)[16]) {
        if constexpr (QUADS) tile_to_quads<QSTRIDE>(v, qlds, t);
    };
    for (int j = 0; j < np; j++)
    {
        const uint32_t q = P.q[j], two_q = q << 1;
        const uint32_t crh = P.cr_hi[j], crl = P.cr_lo[j];
        const uint32_t *RW = T.ntt_rw + 2 * xform_table_len(N) * j;
        const size_t pb    = (b * np + j) * N;            // this polynomial in the [ct][prime][coeff] slabs
        const size_t kb    = (size_t)2 * N * j;           // this prime's rows of the (value, shoup) key tables
        // thread index for this prime's GLOBAL addresses (opaque_index above; the encode-only form has one store
        // per prime and nothing to hoist: measured 1 % slower with it)
        // (the transforms keep the plain index: with the opaque one the symmetric form needs 100 VGPRs instead of
        // 120 but recomputes its LDS and root addresses per prime and runs 12 % slower, profiles/r04_ab_transform.log)
        const int tg       = MODE == kModeEncodeOnly ? t : opaque_index(t);
        uint32_t x[16];

        if constexpr (MODE == kModeAsym && ASYM3)
        {
            // the three transforms of this prime side by side (ntt_tiles3): u_hat = NTT(expand(u))
            // (ckks_asym.c:235-241; code 0 -> q-1, 1 -> 0, 2 -> 1), NTT(e1) (:263-272) and
            // NTT(m + e0) (:280-284)
            uint32_t uh[16], y[16];
            const int8_t *up = A.ucodes + b * N + tg, *ep = A.err + b * 2 * N + N + tg;
#pragma unroll
            for (int e = 0; e < 16; e++)
            {
                uint32_t code = (uint32_t)up[e << CTOP];
                uh[e]         = code + q - 1u;            // q-1, q, q+1 == -1, 0, 1 (sample.c:98-111 mod q)
                int32_t e1    = ep[e << CTOP];
                y[e]          = q + (uint32_t)e1;          // == reduce_set_e_small (ckks_common.c:259-265) mod q
            }
            reduce_signed16(m, x, q, crh, crl, small);
            ntt_tiles3<LOGN>(uh, y, x, RW, q, lds32, t);
            to_quads(uh);
            {
                // c1 = pk1 . u_hat + NTT(e1)   (:251): the lazy transform outputs go through the transpose as they
                // are; one canonicalisation at the end (modarith.cuh, add_mul_canon)
                uint32_t w[16], wp[16];
                to_quads(y);
                ld_pairs<QUADS>(w, wp, T.pk1 + kb, tg);
#pragma unroll
                for (int e = 0; e < 16; e++) y[e] = add_mul_canon(y[e], uh[e], w[e], wp[e], q, two_q);
                st_poly<QUADS>(A.c1 + pb, y, tg);
            }
            to_quads(x);
            if (A.ntt_pte)
            {
                uint32_t cx[16];
#pragma unroll
                for (int e = 0; e < 16; e++) cx[e] = canon4(x[e], q, two_q);
                st_poly<QUADS>(A.ntt_pte + pb, cx, tg);
            }
            {
                // c0 = pk0 . u_hat + NTT(m + e0)   (:255)
                uint32_t w[16], wp[16], out[16];
                ld_pairs<QUADS>(w, wp, T.pk0 + kb, tg);
#pragma unroll
                for (int e = 0; e < 16; e++) out[e] = add_mul_canon(x[e], uh[e], w[e], wp[e], q, two_q);
                st_poly<QUADS>(A.c0 + pb, out, tg);
            }
            if constexpr (QALIAS) __syncthreads();
        }
        else if constexpr (MODE == kModeAsym)
        {
            // one transform at a time (n >= 8192)
            // u_hat = NTT(expand(u))   (ckks_asym.c:235-241; code 0 -> q-1, 1 -> 0, 2 -> 1)
            uint32_t uh[16];
            const int8_t *up = A.ucodes + b * N + tg;
#pragma unroll
            for (int e = 0; e < 16; e++)
            {
                uint32_t code = (uint32_t)up[e << CTOP];
                uh[e]         = code + q - 1u;
            }
            ntt_tiles<LOGN>(uh, RW, q, lds32, t);
            to_quads(uh);
            // n = 16384 (1 024 threads: 128 VGPRs): u_hat waits in LDS while the other two transforms run -- the
            // encoder's FP64 plane is twice the NTT plane, so the upper half of the allocation is free after the
            // encode; thread-private slots ([e][t]: conflict-free, no barrier).  76 B of scratch per lane without it, 28 B with (three
            // root-table addresses the compiler still carries across the prime loop).
            constexpr bool PARK = LOGN == 14 && !GENERAL;
            uint32_t *park = lds32 + G::SLOTS + t;
            static_assert(!PARK || (size_t)G::SLOTS * sizeof(double) >= ((size_t)G::SLOTS + 16 * G::THREADS) * sizeof(uint32_t),
                          "the parked polynomial fits behind the NTT plane inside the encoder's plane");
            auto park_store = [&]() {
                if constexpr (PARK)
                {
#pragma unroll
                    for (int e = 0; e < 16; e++) park[e * G::THREADS] = uh[e];
                }
            };
            auto park_load = [&]() {
                if constexpr (PARK)
                {
#pragma unroll
                    for (int e = 0; e < 16; e++) uh[e] = park[e * G::THREADS];
                }
            };
            park_store();
            // c1 = pk1 . u_hat + NTT(e1)   (:251, :263-272)
            const int8_t *ep = A.err + b * 2 * N + N + tg;
#pragma unroll
            for (int e = 0; e < 16; e++)
            {
                int32_t e1 = ep[e << CTOP];
                x[e]       = q + (uint32_t)e1;
            }
            ntt_tiles<LOGN>(x, RW, q, lds32, t);
#pragma unroll
            for (int e = 0; e < 16; e++) x[e] = canon4(x[e], q, two_q);
            to_quads(x);
            park_load();
            {
                uint32_t w[16], wp[16], out[16];
                ld_pairs<QUADS>(w, wp, T.pk1 + kb, tg);
#pragma unroll
                for (int e = 0; e < 16; e++)
                {
                    uint32_t pr = csub(mul_shoup_lazy(uh[e], w[e], wp[e], q), q);
                    out[e]      = csub(pr + x[e], q);
                }
                st_poly<QUADS>(A.c1 + pb, out, tg);
            }
            // c0 = pk0 . u_hat + NTT(m + e0)   (:255, :280-284)
            reduce_signed16(m, x, q, crh, crl, small);
            ntt_tiles<LOGN>(x, RW, q, lds32, t);
#pragma unroll
            for (int e = 0; e < 16; e++) x[e] = canon4(x[e], q, two_q);
            to_quads(x);
            if (A.ntt_pte) st_poly<QUADS>(A.ntt_pte + pb, x, tg);
            park_load();
            {
                uint32_t w[16], wp[16], out[16];
                ld_pairs<QUADS>(w, wp, T.pk0 + kb, tg);
#pragma unroll
                for (int e = 0; e < 16; e++)
                {
                    uint32_t pr = csub(mul_shoup_lazy(uh[e], w[e], wp[e], q), q);
                    out[e]      = csub(pr + x[e], q);
                }
                st_poly<QUADS>(A.c0 + pb, out, tg);
            }
        }
        else
        {
            // a_j comes from HBM: requested before the transform, it lands while the NTT runs (fused stage
            // 2.60 -> 2.38 ms per 65 536, profiles/r04_ab_transform.log; 16 VGPRs the NTT phase has to spare)
            uint32_t a_pre[16];
            if constexpr (MODE == kModeSym && QUADS) ld_poly<QUADS>(a_pre, A.c1 + pb, tg);
            // NTT(m + e mod q_j)   (ckks_sym.c:286-292)
            reduce_signed16(m, x, q, crh, crl, small);  // see modarith.cuh: the fused
                                                                          // symmetric kernel keeps the exact form
            ntt_tiles<LOGN>(x, RW, q, lds32, t);
            if constexpr (MODE != kModeSym)
            {
#pragma unroll
                for (int e = 0; e < 16; e++) x[e] = canon4(x[e], q, two_q);
            }
            to_quads(x);   // symmetric: the lazy values in [0,4q); sub_mul_canon canonicalises once at the end
            if (A.ntt_pte)
            {
                uint32_t cx[16];
#pragma unroll
                for (int e = 0; e < 16; e++) cx[e] = canon4(x[e], q, two_q);
                st_poly<QUADS>(A.ntt_pte + pb, cx, tg);
            }
            if constexpr (MODE == kModeSym)
            {
                // c0 = -(s_hat . a) + NTT(m+e)   (ckks_sym.c:273-300); a was written to c1
                uint32_t a[16], w[16], wp[16], out[16];
                if constexpr (QUADS)
                {
#pragma unroll
                    for (int e = 0; e < 16; e++) a[e] = a_pre[e];
                }
                else
                    ld_poly<QUADS>(a, A.c1 + pb, tg);
                ld_pairs<QUADS>(w, wp, T.s_hat + kb, tg);
#pragma unroll
                for (int e = 0; e < 16; e++) out[e] = sub_mul_canon(x[e], a[e], w[e], wp[e], q, two_q);
                st_poly<QUADS>(A.c0 + pb, out, tg);
            }
            else
            {
                st_poly<QUADS>(A.c0 + pb, x, tg);
            }
            if constexpr (QALIAS) __syncthreads();   // the transpose region is the next prime's exchange plane
        }
    }
}

// KEYED: the key rows come from the ring (key_base above); everything else is the unkeyed form
template <int LOGN, int MODE, bool GENERAL, bool KEYED = false>
__device__ __forceinline__ void encrypt_one(const DevParams &P, const DevTables &T, const EncArgs &A,
                                            const KeyRing &R, const size_t b, unsigned char *smem)
{
    size_t kb = 0;
    if constexpr (KEYED) kb = key_base(R, b);
    const int t = thread_index<GENERAL>();
    using MT = typename std::conditional<GENERAL, int64_t, int32_t>::type;
    MT m[16];
    bool small;  // wave-uniform: every |m + e| of this wave is below 2 q_min
    int wg;
    encode_plaintext<LOGN, MT, GENERAL>(P, T, A.values, A.status, b, smem, m, small, wg);
    if constexpr (!GENERAL)
    {
        if (!small)   // workgroup-uniform in the fast form (encode_plaintext)
        {
            if (t == 0) A.general[1 + atomicAdd(A.general, 1u)] = (uint32_t)b;
            return;
        }
    }
    if constexpr (KEYED)
        encrypt_tail<LOGN, MODE, GENERAL, false>(P, with_key(T, R, kb), A, b, smem, m, small);
    else
        encrypt_tail<LOGN, MODE, GENERAL, false>(P, T, A, b, smem, m, small);
}

// ------------------------------------------------------------------------------------------
// Round 6: the fast (int32) symmetric / encode-only forms at n = 4096 take TWO plaintexts per workgroup and encode
// them through the half-size transform (transform.cuh, ifft_pair_real_half), keeping the reference's bits by a guard:
//
//   * Through stage 10 the lower half's values are the reference's own, bit for bit.  The reference's last stage uses
//     v, its COMPUTED upper-half value, where we use conj(u); in exact arithmetic they are equal, so the two outputs
//     of a pair differ by at most |Re v - Re u| + |Im v + Im u| (+ 3 roundings) <= sqrt(2) |v - conj(u)|, and
//     |v - conj(u)| <= the forward errors of v and of u after 11 stages.  A butterfly row carries a relative error
//     <= 6u on (|u| + |v|) (sum: u; difference x root: u + 2 sqrt(2) u for the Annex-G product + 2u for libm's
//     root, u = 2^-53); a stage multiplies the 2-norm by sqrt(2) and the norm of the absolute-value matrix is 2, so
//     11 stages leave ||x^ - x||_2 <= 11 sqrt(2) 6u ||x||_2 = 1.04e-14 ||x||_2 with ||x||_2 = ||y||_2 / sqrt(2), y =
//     the exact output vector.  Every output therefore differs from the reference's by less than 2.2e-14 ||y||_2 (incl.
//     the roundings of the last stage and of the scaling); ||y||_2 = sqrt(n) ||A||_2 = sqrt(2 n sum values^2) exactly.
//   * kHalfDelta = 3e-14 (x 1.001 for the float accumulation of the sum) is that bound with 36 % of slack -- and the
//     bound itself assumes every rounding error aligned: the measured maximum deviation is 1.9e-17 ||m||_2, 1 300 times
//     smaller.  A coefficient whose scaled value lies within delta of a half-integer could round differently from the
//     reference's: the workgroup then REDOES that plaintext with the full transform (encode_plaintext; about one
//     plaintext in nine at the bench distribution).  Everything else about the fast form is unchanged: a plaintext
//     that is not small, or holds a non-finite value, is declined to the general kernel.
// The second plaintext's coefficients wait in LDS (thread-private slots behind the NTT plane + transpose region)
// while the first one's primes run.
// ------------------------------------------------------------------------------------------

// flags of plaintext A in bits 0..7, of plaintext B in bits 8..15 (kWgNotSmall | kWgNonfinite | kWgRisky)
template <int LOGN>
__device__ __forceinline__ int encode_pair_half(const DevParams &P, const DevTables &T, const float *values,
                                                const size_t bA, const size_t bB, unsigned char *smem,
                                                int32_t (&mA)[16], int32_t (&mB)[16])
{
    using G          = XformGeom<LOGN>;
    constexpr int N  = G::N;
    constexpr int TH = G::THREADS;
    static_assert((N / 8) / TH == 2, "two float4 pieces per thread and plaintext");
    const int t      = threadIdx.x;
    double *plane    = reinterpret_cast<double *>(smem);
    float *sv        = reinterpret_cast<float *>(smem);   // A's values at [0, n/2), B's at [n/2, n)
    float *part      = sv + N;                            // [wave][plaintext] sums of squares

    typedef float v2f __attribute__((ext_vector_type(2)));
    v2f nf[2]   = {{0.0f, 0.0f}, {0.0f, 0.0f}};
    float ss[2] = {0.0f, 0.0f};
#pragma unroll
    for (int p = 0; p < 2; p++)
    {
        const float4 *src = reinterpret_cast<const float4 *>(values + (p ? bB : bA) * (N / 2));
#pragma unroll
        for (int k = 0; k < 2; k++)
        {
            const int i    = t + k * TH;
            const float4 v = src[i];
            nf[p]          = __builtin_elementwise_fma(v2f{v.x, v.y}, v2f{0.0f, 0.0f}, nf[p]);
            nf[p]          = __builtin_elementwise_fma(v2f{v.z, v.w}, v2f{0.0f, 0.0f}, nf[p]);
            ss[p]          = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, ss[p]))));
            float *dst     = sv + p * (N / 2);
            dst[sv_slot(4u * i, LOGN)]      = v.x;
            dst[sv_slot(4u * i + 1u, LOGN)] = v.y;
            dst[sv_slot(4u * i + 2u, LOGN)] = v.z;
            dst[sv_slot(4u * i + 3u, LOGN)] = v.w;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss[0] += __shfl_xor(ss[0], off), ss[1] += __shfl_xor(ss[1], off);
    if ((t & 63) == 0) part[2 * (t >> 6)] = ss[0], part[2 * (t >> 6) + 1] = ss[1];
    bool nonfinite[2];
#pragma unroll
    for (int p = 0; p < 2; p++)
    {
        const float s = nf[p].x + nf[p].y;
        nonfinite[p]  = s != s;   // this thread staged a NaN or an infinity of plaintext p
    }
    __syncthreads();
    const float ss_all[2] = {(part[0] + part[2]) + (part[4] + part[6]), (part[1] + part[3]) + (part[5] + part[7])};
    double re[16], im[16];
    {
        const int Tl    = t & 127;
        const float *my = sv + (t >> 7) * (N / 2);
        const uint4 *mp = reinterpret_cast<const uint4 *>(T.gather_map);
        uint4 m0 = mp[Tl], m1 = mp[TH + Tl];
        uint32_t packed[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            uint32_t idx = (packed[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
            re[e]        = (double)my[idx];
            im[e]        = 0.0;
        }
    }
    __syncthreads();
    ifft_pair_real_half<LOGN>(re, im, T.ifft_w, plane, t);

    int flags = 0;
#pragma unroll
    for (int p = 0; p < 2; p++)
    {
        // |fast - reference| < delta for every scaled coefficient (see above); ||m||_2 = n_inv sqrt(2 n sum values^2)
        const double delta = kHalfDelta * P.n_inv * sqrt(2.0 * (double)N * (double)ss_all[p]);
        double amax = 0.0;
        bool risky  = false;
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            const double x = e < 8 ? re[8 * p + e] : im[8 * p + e - 8];
            const double v = __dmul_rn(x, P.n_inv);
            const double a = fabs(v);
            const double g = __dsub_rn(a, trunc(a));        // exact; distance to the rounding boundary = |g - 0.5|
            risky          = risky || (fabs(__dsub_rn(g, 0.5)) < delta);
            const double r = round_half_away(v);
            amax           = fmax(amax, fabs(r));
            if (p == 0) mA[e] = (int32_t)r; else mB[e] = (int32_t)r;
        }
        const bool sm = amax < P.small_bound && !nonfinite[p];
        flags |= ((sm ? 0 : kWgNotSmall) | (nonfinite[p] ? kWgNonfinite : 0) | (risky ? kWgRisky : 0)) << (8 * p);
    }
    return __ockl_wgred_or_i32(flags);
}

template <int LOGN, int MODE, bool KEYED = false>
__device__ __forceinline__ void encrypt_pair(const DevParams &P, const DevTables &T, const EncArgs &A,
                                             const KeyRing &R, const size_t bA, const bool haveB, unsigned char *smem)
{
    const int t     = threadIdx.x;
    const size_t bB = haveB ? bA + 1 : bA;   // an odd batch ends with a workgroup that carries its plaintext twice
    size_t kbA = 0, kbB = 0;                 // keyed: the two plaintexts' key offsets (SGPRs)
    if constexpr (KEYED) kbA = key_base(R, bA), kbB = key_base(R, bB);
    int32_t m[16], mo[16];                   // A's coefficients / B's
    const int flags = encode_pair_half<LOGN>(P, T, A.values, bA, bB, smem, m, mo);
    // Per plaintext: declined (general kernel), or coefficients valid -- after an exact redo when one of them sat in the
    // guard band (two call sites of the full encoder: a loop over the two register arrays would put them in scratch).
    int run = 0;
    auto settle = [&](int32_t (&mm)[16], const int f, const size_t b, const bool live, const int bit) {
        bool small = !(f & (kWgNotSmall | kWgNonfinite));
        if (small && (f & kWgRisky) && live)
        {
            int wg;   // the full transform decides (it writes the status and may still decline)
            encode_plaintext<LOGN, int32_t, false>(P, T, A.values, A.status, b, smem, mm, small, wg);
        }
        else if (small && live && A.status && t == 0)
            A.status[b] = 1;
        if (!small && live && t == 0) A.general[1 + atomicAdd(A.general, 1u)] = (uint32_t)b;
        run |= (small && live) ? bit : 0;
    };
    settle(m, flags & 0xFF, bA, true, 1);
    settle(mo, (flags >> 8) & 0xFF, bB, haveB, 2);
    // B's coefficients wait in thread-private LDS slots behind the NTT plane and the transpose region while A's
    // primes run (ONE call site of the tail: the loop below is not unrolled)
    uint32_t *park = reinterpret_cast<uint32_t *>(smem) + kPairParkWords + t;
    __syncthreads();   // an exact redo may still be reading the plane the slots lie in
    if (run & 2)
    {
#pragma unroll
        for (int e = 0; e < 16; e++) park[e * XformGeom<LOGN>::THREADS] = (uint32_t)mo[e];
    }
#pragma nounroll
    for (int p = 0; p < 2; p++)
    {
        if (run & (1 << p))
        {
            if constexpr (KEYED)
                encrypt_tail<LOGN, MODE, false, true>(P, with_key(T, R, p ? kbB : kbA), A, p ? bB : bA, smem, m, true);
            else
                encrypt_tail<LOGN, MODE, false, true>(P, T, A, p ? bB : bA, smem, m, true);
        }
        if (p == 0 && (run & 2))
        {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 16; e++) m[e] = (int32_t)park[e * XformGeom<LOGN>::THREADS];
        }
    }
}

// ------------------------------------------------------------------------------------------
// The two-way pair form (k_encode_encrypt_pair2): the same pair encoder, guard band and exact redo, but BOTH plaintexts
// stay in registers and the tail runs prime-major -- per prime ONE two-way transform (transform.cuh, ntt_tiles2) whose
// root pairs are loaded once for the two butterfly streams under one barrier pair per exchange, and ONE load of the
// (NTT(s), Shoup) quads for the two epilogues.  Its resource plan is the public-key kernel's: three workgroups per CU
// (<= 168 VGPRs), two independent butterfly streams per thread.
// LDS: the encoder's two f64 half-planes and the two u32 NTT planes are the same 2 SLOTS words; the wave-local transpose
// region (rows of 20 words) lies INSIDE the planes, free after the transform's last barrier, and one workgroup barrier
// per prime keeps the next prime's first exchange off it.  Nothing is parked.
// run: bit 0 / bit 1 = plaintext A / B is live (not declined to the general kernel); a declined partner still goes
// through the transform (its registers hold whatever the encoder left) and is never stored.
// ------------------------------------------------------------------------------------------
template <int LOGN, int MODE>
__device__ __forceinline__ void encrypt_pair2_tail(const DevParams &P, const DevTables &T, const EncArgs &A,
                                                   const size_t bA, const size_t bB, unsigned char *smem,
                                                   int32_t (&mA)[16], int32_t (&mB)[16], const int run)
{
    static_assert(LOGN <= 12 && MODE != kModeAsym, "quad-layout outputs, one key row per prime");
    const int t = threadIdx.x;
    using G            = XformGeom<LOGN>;
    constexpr int N    = G::N;
    constexpr int CTOP = LOGN - 4;
    constexpr int QSTRIDE = enc_quad_stride<MODE>();
    static_assert((size_t)(G::N / 16) * QSTRIDE <= (size_t)2 * G::SLOTS, "the transpose region lies inside the two planes");
    uint32_t *lds32 = reinterpret_cast<uint32_t *>(smem);
    const int np    = P.nprimes;
    const bool doA = run & 1, doB = run & 2;   // workgroup-uniform

    if constexpr (MODE == kModeSym)
    {
#pragma unroll
        for (int e = 0; e < 16; e++) mA[e] += A.err[bA * N + (e << CTOP) + t];
#pragma unroll
        for (int e = 0; e < 16; e++) mB[e] += A.err[bB * N + (e << CTOP) + t];
    }
    // (the int64 stores take an opaque 32-bit copy: sign-extended in place, every coefficient would stay the low half of a
    // 64-bit register pair across the prime loop -- 32 VGPRs of unused high halves and 124 B of spills on the hot path)
    if (A.pte)
    {
        if (doA)
        {
#pragma unroll
            for (int e = 0; e < 16; e++) A.pte[bA * N + (e << CTOP) + t] = opaque_index(mA[e]);
        }
        if (doB)
        {
#pragma unroll
            for (int e = 0; e < 16; e++) A.pte[bB * N + (e << CTOP) + t] = opaque_index(mB[e]);
        }
    }
    if constexpr (MODE == kModeEncodeOnly)
    {
        if (!A.c0) return;  // plain ckks_encode_base: only the int64 plaintexts were requested
    }
    for (int j = 0; j < np; j++)
    {
        const uint32_t q = P.q[j], two_q = q << 1;
        const uint32_t *RW = T.ntt_rw + 2 * xform_table_len(N) * j;
        const size_t pbA   = (bA * np + j) * N, pbB = (bB * np + j) * N;
        const size_t kb    = (size_t)2 * N * j;
        const int tg       = MODE == kModeEncodeOnly ? t : opaque_index(t);   // see encrypt_tail
        uint32_t xA[16], xB[16];
        // a_j of both plaintexts comes from HBM: requested before the transform, it lands while the NTT runs
        uint32_t aA[16], aB[16];
        if constexpr (MODE == kModeSym)
        {
            load_quads(aA, A.c1 + pbA, tg);
            load_quads(aB, A.c1 + pbB, tg);
        }
        reduce_signed16(mA, xA, q, 0u, 0u, true);   // m + 2q (modarith.cuh)
        reduce_signed16(mB, xB, q, 0u, 0u, true);
        ntt_tiles2<LOGN>(xA, xB, RW, q, lds32, t);
        if constexpr (MODE != kModeSym)
        {
#pragma unroll
            for (int e = 0; e < 16; e++) xA[e] = canon4(xA[e], q, two_q), xB[e] = canon4(xB[e], q, two_q);
        }
        // one wave-local region for both transposes: LDS executes a wave's accesses in order
        tile_to_quads<QSTRIDE>(xA, lds32, t);
        tile_to_quads<QSTRIDE>(xB, lds32, t);
        if (A.ntt_pte)
        {
            uint32_t cx[16];
            if (doA)
            {
#pragma unroll
                for (int e = 0; e < 16; e++) cx[e] = canon4(xA[e], q, two_q);
                store_quads(A.ntt_pte + pbA, cx, tg);
            }
            if (doB)
            {
#pragma unroll
                for (int e = 0; e < 16; e++) cx[e] = canon4(xB[e], q, two_q);
                store_quads(A.ntt_pte + pbB, cx, tg);
            }
        }
        if constexpr (MODE == kModeSym)
        {
            // c0 = -(s_hat . a) + NTT(m+e)   (ckks_sym.c:273-300) for both plaintexts from ONE load of the key quads
            uint32_t w[16], wp[16];
            load_quads_pairs(w, wp, T.s_hat + kb, tg);
#pragma unroll
            for (int e = 0; e < 16; e++) xA[e] = sub_mul_canon(xA[e], aA[e], w[e], wp[e], q, two_q);
            if (doA) store_quads(A.c0 + pbA, xA, tg);
#pragma unroll
            for (int e = 0; e < 16; e++) xB[e] = sub_mul_canon(xB[e], aB[e], w[e], wp[e], q, two_q);
            if (doB) store_quads(A.c0 + pbB, xB, tg);
        }
        else
        {
            if (doA) store_quads(A.c0 + pbA, xA, tg);
            if (doB) store_quads(A.c0 + pbB, xB, tg);
        }
        __syncthreads();   // the transpose region is the next prime's exchange plane
    }
}

// plaintexts bA and bA + 1 (the launcher sends only whole pairs here)
template <int LOGN, int MODE>
__device__ __forceinline__ void encrypt_pair2(const DevParams &P, const DevTables &T, const EncArgs &A, const size_t bA,
                                              unsigned char *smem)
{
    const int t     = threadIdx.x;
    const size_t bB = bA + 1;
    int32_t mA[16], mB[16];
    const int flags = encode_pair_half<LOGN>(P, T, A.values, bA, bB, smem, mA, mB);
    // per plaintext as in encrypt_pair: declined, or coefficients valid after an exact redo where the guard band asks
    int run = 0;
    auto settle = [&](int32_t (&mm)[16], const int f, const size_t b, const int bit) {
        bool small = !(f & (kWgNotSmall | kWgNonfinite));
        if (small && (f & kWgRisky))
        {
            int wg;   // the full transform decides (it writes the status and may still decline)
            encode_plaintext<LOGN, int32_t, false>(P, T, A.values, A.status, b, smem, mm, small, wg);
        }
        else if (small && A.status && t == 0)
            A.status[b] = 1;
        if (!small && t == 0) A.general[1 + atomicAdd(A.general, 1u)] = (uint32_t)b;
        run |= small ? bit : 0;
    };
    settle(mA, flags & 0xFF, bA, 1);
    settle(mB, (flags >> 8) & 0xFF, bB, 2);
    if (!run) return;   // workgroup-uniform
    __syncthreads();    // an exact redo may still be reading the planes
    encrypt_pair2_tail<LOGN, MODE>(P, T, A, bA, bB, smem, mA, mB, run);
}

// Bytes of dynamic LDS the pair forms address, which launch_enc_mode holds against the size it launches with.
// encrypt_pair: the pair encoder's two f64 half-planes; the NTT plane and the transpose region end below the parked
// plaintext (static_asserts of encrypt_tail), which ends N words behind kPairParkWords.
template <int LOGN>
constexpr size_t pair_lds_extent()
{
    using G = XformGeom<LOGN>;
    return std::max((size_t)G::SLOTS * sizeof(double), (kPairParkWords + (size_t)G::N) * sizeof(uint32_t));
}
// encrypt_pair2: the same half-planes, two NTT planes, the transpose region from word 0
template <int LOGN, int MODE>
constexpr size_t pair2_lds_extent()
{
    using G = XformGeom<LOGN>;
    return std::max(std::max((size_t)G::SLOTS * sizeof(double), (size_t)2 * G::SLOTS * sizeof(uint32_t)),
                    (size_t)(G::N / 16) * enc_quad_stride<MODE>() * sizeof(uint32_t));
}

// two plaintexts per workgroup (encrypt_pair)
template <int LOGN, int MODE>
constexpr bool enc_pairs()
{
    return LOGN == 12 && MODE != kModeAsym;
}

// workgroups per CU the register budget is set for (n <= 4096: 256 threads = one wave per SIMD each)
template <int LOGN, int MODE, bool GENERAL>
constexpr int enc_blocks()
{
    if (LOGN > 12) return 1;
    if (MODE == kModeAsym && !GENERAL) return 3;   // transpose region inside the planes (encrypt_one, QALIAS)
    if (MODE == kModeAsym) return 2;   // 3 (with the transpose region aliased) spills: 5.45 -> 7.07 ms
    return GENERAL ? 3 : 4;
}

template <int LOGN, int MODE, bool KEYED>
__device__ __forceinline__ void encode_encrypt_fast(const DevParams &P, const DevTables &T, const EncArgs &A,
                                                    const KeyRing &R, unsigned char *smem)
{
    if constexpr (enc_pairs<LOGN, MODE>())
    {
        const size_t bA = A.first + (size_t)2 * blockIdx.x;
        encrypt_pair<LOGN, MODE, KEYED>(P, T, A, R, bA, bA + 1 < A.count, smem);
    }
    else
        encrypt_one<LOGN, MODE, false, KEYED>(P, T, A, R, blockIdx.x, smem);
}

template <int LOGN, int MODE, bool KEYED>
__device__ __forceinline__ void encode_encrypt_general(const DevParams &P, const DevTables &T, const EncArgs &A,
                                                       const KeyRing &R, unsigned char *smem)
{
    const uint32_t count = A.general[0];
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x)
    {
        encrypt_one<LOGN, MODE, true, KEYED>(P, T, A, R, A.general[1 + i], smem);
        __syncthreads();
    }
}

template <int LOGN, int MODE>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS, (enc_blocks<LOGN, MODE, false>()))
void k_encode_encrypt(DevParams P, DevTables T, EncArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    encode_encrypt_fast<LOGN, MODE, false>(P, T, A, KeyRing{}, smem);
}

template <int LOGN, int MODE>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS, (enc_blocks<LOGN, MODE, true>()))
void k_encode_encrypt_general(DevParams P, DevTables T, EncArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t count = A.general[0];
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x)
    {
        encrypt_one<LOGN, MODE, true>(P, T, A, KeyRing{}, A.general[1 + i], smem);
        __syncthreads();
    }
}

// the two-way pair form (encrypt_pair2): fast, unkeyed, n = 4096 symmetric / encode-only; workgroup i takes the plaintexts
// 2 i and 2 i + 1.  Three workgroups per CU.
template <int LOGN, int MODE>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS, 3)
void k_encode_encrypt_pair2(DevParams P, DevTables T, EncArgs A)
{
    static_assert(3 * (pair2_lds_extent<LOGN, MODE>() + 256) <= 160 * 1024, "three workgroups per CU fit the 160 KiB of LDS");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    encrypt_pair2<LOGN, MODE>(P, T, A, (size_t)2 * blockIdx.x, smem);
}

// keyed twins (symmetric / public-key modes): the same bodies, key rows of record b from ring key R.idx[b]
template <int LOGN, int MODE>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS, (enc_blocks<LOGN, MODE, false>()))
void k_encode_encrypt_keyed(DevParams P, DevTables T, EncArgs A, KeyRing R)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    encode_encrypt_fast<LOGN, MODE, true>(P, T, A, R, smem);
}

template <int LOGN, int MODE>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS, (enc_blocks<LOGN, MODE, true>()))
void k_encode_encrypt_general_keyed(DevParams P, DevTables T, EncArgs A, KeyRing R)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    encode_encrypt_general<LOGN, MODE, true>(P, T, A, R, smem);
}

// ------------------------------------------------------------------------------------------
// Split form of the symmetric path, used so that everything that does not need `a` overlaps with
// the (long, one-wave-per-SIMD) uniform sampler:
//   k_encode_rns : encode -> + e -> per prime signed reduction, residues stored (natural order)
//                  into the c0 slab itself -- no extra scratch.
//   k_ntt_fuse   : prime j of every ciphertext: load residues from c0_j, forward NTT, then
//                  c0_j = NTT(m+e) - s_hat . a_j  with a_j read from c1_j (ckks_sym.c:273-300).
// ------------------------------------------------------------------------------------------
// Like the fused kernel it comes as a fast / general pair: the fast launch declines a plaintext that holds
// a NaN or an infinite value (it appends the index to A.general and writes nothing); k_encode_rns_general
// walks that list with the EXACT transform.  Keeping the second transform out of the fast kernel is what
// keeps its registers (120 VGPRs, 104 at n = 16384; with a branch to the exact form inside: 150, and 128 +
// 92 B of spills at n = 16384).
template <int LOGN, bool ADD_ERR, bool GENERAL>
__device__ __forceinline__ void encode_rns_one(const DevParams &P, const DevTables &T, const EncArgs &A,
                                               const size_t b, unsigned char *smem)
{
    using G            = XformGeom<LOGN>;
    constexpr int N    = G::N;
    constexpr int CTOP = LOGN - 4;
    const int t    = thread_index<GENERAL>();
    const int np   = P.nprimes;

    int64_t m[16];
    bool small;  // wave-uniform: every |m + e| of this wave is below 2 q_min
    int wg;
    encode_plaintext<LOGN, int64_t, GENERAL>(P, T, A.values, A.status, b, smem, m, small, wg);
    if constexpr (!GENERAL)
    {
        if (wg & kWgNonfinite)
        {
            if (t == 0) A.general[1 + atomicAdd(A.general, 1u)] = (uint32_t)b;
            return;
        }
    }
    if constexpr (ADD_ERR)
    {
#pragma unroll
        for (int e = 0; e < 16; e++) m[e] += A.err[b * N + (e << CTOP) + t];
    }
    if (A.pte)
    {
#pragma unroll
        for (int e = 0; e < 16; e++) A.pte[b * N + (e << CTOP) + t] = m[e];
    }
    // A small plaintext (every |m + e| < 2 q_min: the normal case) crosses to k_ntt_fuse as ONE row of
    // int32 -- parked in the c0 row of the LAST prime, which its own launch reads before it overwrites it --
    // instead of np rows of residues: k_ntt_fuse forms the representative m + 2 q_j itself.  At n = 16384
    // this kernel is HBM-bound (6 x 64 KiB of residues per plaintext against 48 KiB of inputs).
    if (A.compact)
    {
        const bool compact = !(wg & kWgNotSmall);
        if (t == 0) A.compact[b] = compact ? 1 : 0;
        if (compact)
        {
            uint32_t *dst = A.c0 + (b * np + (np - 1)) * N;
#pragma unroll
            for (int e = 0; e < 16; e++) dst[(e << CTOP) + t] = (uint32_t)(int32_t)m[e];
            return;
        }
    }
    for (int j = 0; j < np; j++)
    {
        uint32_t x[16];
        reduce_signed16(m, x, P.q[j], P.cr_hi[j], P.cr_lo[j], small);
        uint32_t *dst = A.c0 + (b * np + j) * N;
#pragma unroll
        for (int e = 0; e < 16; e++) dst[(e << CTOP) + t] = x[e];
    }
}

template <int LOGN, bool ADD_ERR>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_encode_rns(DevParams P, DevTables T,
                                                                      EncArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    encode_rns_one<LOGN, ADD_ERR, false>(P, T, A, blockIdx.x, smem);
}

template <int LOGN, bool ADD_ERR>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_encode_rns_general(DevParams P, DevTables T,
                                                                              EncArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t count = A.general[0];
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x)
    {
        encode_rns_one<LOGN, ADD_ERR, true>(P, T, A, A.general[1 + i], smem);
        __syncthreads();
    }
}

// n = 16384: at most 96 VGPRs (5 waves per SIMD instead of the 4 the 1024-thread workgroup needs) so
// that a workgroup fits beside the uniform sampler's chain waves (128 VGPRs, one wave per SIMD).
// KEYED: NTT(s) of ring key R.idx[b] (key_base above) instead of the installed key
template <int LOGN, int MODE, bool KEYED>
__device__ __forceinline__ void ntt_fuse_body(const DevParams &P, const DevTables &T, const EncArgs &A,
                                              const KeyRing &R, int j, unsigned char *smem)
{
    using G            = XformGeom<LOGN>;
    constexpr int N    = G::N;
    constexpr int CTOP = LOGN - 4;
    uint32_t *lds32  = reinterpret_cast<uint32_t *>(smem);
    const int t      = threadIdx.x;
    const size_t b   = blockIdx.x;
    const int np     = P.nprimes;
    const uint32_t q = P.q[j], two_q = q << 1;
    uint32_t *poly   = A.c0 + (b * np + j) * N;
    const uint32_t *s_hat = T.s_hat;
    if constexpr (KEYED) s_hat = R.k0 + key_base(R, b);

    // residues of this prime, or the compact int32 plaintext from the last prime's row (k_encode_rns):
    // m + 2 q_j is a representative in (0, 4q) the NTT accepts (modarith.cuh, reduce_signed16)
    const bool compact  = A.compact != nullptr && A.compact[b] != 0;
    const uint32_t *src = compact ? A.c0 + (b * np + (np - 1)) * N : poly;
    const uint32_t bias = compact ? two_q : 0u;
    uint32_t x[16];
#pragma unroll
    for (int e = 0; e < 16; e++) x[e] = src[(e << CTOP) + t] + bias;
    // issue the epilogue operands now; they land while the NTT runs.  At n = 16384 only `a` (HBM) is
    // prefetched; the L2-resident s_hat pairs are fetched after the NTT to stay within 96 VGPRs.
    // All epilogue accesses are in quad layout (transform.cuh, tile_to_quads): 1 KiB contiguous per wave
    // instruction instead of 16-byte pieces at a 64 / 128-byte lane stride.
    constexpr bool LATE_KEY = LOGN == 14;
    uint32_t a[16], w[16], wp[16];
    if constexpr (MODE == kModeSym)
    {
        load_quads(a, A.c1 + (b * np + j) * N, t);
        if constexpr (!LATE_KEY) load_quads_pairs(w, wp, s_hat + (size_t)2 * N * j, t);
    }
    ntt_tiles<LOGN>(x, T.ntt_rw + 2 * xform_table_len(N) * j, q, lds32, t);
    if constexpr (MODE == kModeSym && LATE_KEY) load_quads_pairs(w, wp, s_hat + (size_t)2 * N * j, t);
    // n <= 4096: the symmetric epilogue takes the LAZY transform output and canonicalises once (modarith.cuh,
    // sub_mul_canon); at n >= 8192 that form costs registers the kernel does not have (96-VGPR cap at n = 16384:
    // 36 B of spills) and the separate canonicalisation stays
    constexpr bool LAZY_EPI = MODE == kModeSym && LOGN <= 12;
    if constexpr (!LAZY_EPI)
    {
#pragma unroll
        for (int e = 0; e < 16; e++) x[e] = canon4(x[e], q, two_q);
    }
    // one prime per launch: the exchange plane is free after the NTT's last barrier, the wave-local
    // transpose runs inside it (unpadded rows: the plane has no room for more at n = 16384 beside the chains)
    tile_to_quads<16>(x, lds32, t);
    if (A.ntt_pte)
    {
        uint32_t cx[16];
#pragma unroll
        for (int e = 0; e < 16; e++) cx[e] = LAZY_EPI ? canon4(x[e], q, two_q) : x[e];
        store_quads(A.ntt_pte + (b * np + j) * N, cx, t);
    }
    if constexpr (MODE == kModeSym)
    {
        uint32_t out[16];
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            if constexpr (LAZY_EPI)
                out[e] = sub_mul_canon(x[e], a[e], w[e], wp[e], q, two_q);
            else
                out[e] = csub(x[e] + q - csub(mul_shoup_lazy(a[e], w[e], wp[e], q), q), q);
        }
        store_quads(poly, out, t);
    }
    else
    {
        store_quads(poly, x, t);
    }
}

template <int LOGN, int MODE>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS)
__attribute__((amdgpu_waves_per_eu(LOGN == 14 ? 5 : (XformGeom<LOGN>::THREADS + 255) / 256))) void k_ntt_fuse(DevParams P, DevTables T, EncArgs A,
                                                                    int j)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ntt_fuse_body<LOGN, MODE, false>(P, T, A, KeyRing{}, j, smem);
}

template <int LOGN, int MODE>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS)
__attribute__((amdgpu_waves_per_eu(LOGN == 14 ? 5 : (XformGeom<LOGN>::THREADS + 255) / 256))) void k_ntt_fuse_keyed(DevParams P, DevTables T,
                                                                    EncArgs A, KeyRing R, int j)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ntt_fuse_body<LOGN, MODE, true>(P, T, A, R, j, smem);
}

// Batched stand-alone forward NTT (ntt_inpl, ntt.c:168-189) of `count` polynomials mod q_j,
// in place, natural-order in, bit-reversed-order canonical out.  Also emits the Shoup companion
// table when `pairs_out` is given (used once per key for NTT(s) and the public key).
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ntt_polys(DevParams P, DevTables T, int j,
                                                                     uint32_t *polys,
                                                                     uint32_t *pairs_out)
{
    using G            = XformGeom<LOGN>;
    constexpr int N    = G::N;
    constexpr int CTOP = LOGN - 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds32 = reinterpret_cast<uint32_t *>(smem);
    const int t     = threadIdx.x;
    uint32_t *poly  = polys + (size_t)blockIdx.x * N;
    const uint32_t q = P.q[j], two_q = q << 1;
    uint32_t x[16];
#pragma unroll
    for (int e = 0; e < 16; e++) x[e] = poly[(e << CTOP) + t];
    ntt_tiles<LOGN>(x, T.ntt_rw + 2 * xform_table_len(N) * j, q, lds32, t);
#pragma unroll
    for (int e = 0; e < 16; e++) x[e] = canon4(x[e], q, two_q);
    store16(poly + 16 * t, x);
    if (pairs_out)
    {
        uint32_t *po = pairs_out + ((size_t)blockIdx.x * N + 16 * t) * 2;
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            po[2 * e]     = x[e];
            po[2 * e + 1] = (uint32_t)((((uint64_t)x[e]) << 32) / q);
        }
    }
}

// Shoup companions for a table that is already in NTT form (public-key slabs): pairs[i] =
// (v[i], floor(v[i] * 2^32 / q_j)).  (A tile-major layout that makes the public-key kernel's pair loads
// contiguous over the wave was measured 4 % SLOWER on that kernel, gpurun_out/ab_pk_tiled.log: at 256
// VGPRs / 2 waves it is not the access pattern that limits it.)
__global__ void k_make_pairs(const uint32_t *vals, uint32_t *pairs, uint32_t q, int count)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count)
    {
        uint32_t v       = vals[i];
        pairs[2 * i]     = v;
        pairs[2 * i + 1] = (uint32_t)((((uint64_t)v) << 32) / q);
    }
}

// ------------------------------------------------------------------------------------------
// Verification side: the reference's round-trip check, batched.
//   ckks_decrypt   device/test/ckks_tests_common.c:136-153   d = c0 + c1 . NTT(s)
//   intt_inpl      device/lib/intt.c:144-222 (+ n^-1)        pt = INTT(d)
//   ckks_decode    device/test/ckks_tests_common.c:59-115    centred lift, / scale, fft_inpl
//                  (device/lib/fft.c:146-213), slot pick through the index map
// One workgroup per ciphertext, one prime per launch.  Decode is bit-exact with the reference's
// (same butterflies, same root table, IEEE division and float conversion).
// ------------------------------------------------------------------------------------------
struct VerifyArgs
{
    const uint32_t *c0;   // [B][np][n]
    const uint32_t *c1;   // [B][np][n]   (NULL: c0 slab already holds the value to invert)
    uint32_t *dec_ntt;    // optional [B][n]: c0 + c1 . NTT(s) mod q_j   (NTT form)
    uint32_t *pt;         // optional [B][n]: INTT of it, canonical, natural order
    float *values;        // optional [B][n/2]: decoded slots
    uint32_t in_primes;   // polynomials per record in c0/c1 (np, or 1 for a bare polynomial batch)
    int j;                // prime
};

template <int LOGN, bool KEYED>
__device__ __forceinline__ void decrypt_decode_body(const DevParams &P, const DevTables &T, const VerifyArgs &A,
                                                    const KeyRing &R, unsigned char *smem)
{
    using G            = XformGeom<LOGN>;
    constexpr int N    = G::N;
    constexpr int CTOP = LOGN - 4;
    uint32_t *lds32  = reinterpret_cast<uint32_t *>(smem);
    double *plane    = reinterpret_cast<double *>(smem);
    const int t      = threadIdx.x;
    const size_t b   = blockIdx.x;
    const int j      = A.j;
    const uint32_t q = P.q[j];
    const size_t rec = (b * A.in_primes + (A.in_primes > 1 ? j : 0)) * N + 16 * t;

    uint32_t x[16];
    load16(x, A.c0 + rec);
    if (A.c1)
    {
        uint32_t a[16], w[16], wp[16];
        load16(a, A.c1 + rec);
        load16_pairs(w, wp, KEYED ? R.k0 + key_base(R, b) : T.s_hat, (size_t)j * N + 16 * t);
#pragma unroll
        for (int e = 0; e < 16; e++)
            x[e] = csub(csub(mul_shoup_lazy(a[e], w[e], wp[e], q), q) + x[e], q);
    }
    if (A.dec_ntt) store16(A.dec_ntt + b * N + 16 * t, x);
    if (!A.pt && !A.values) return;

    intt_tiles<LOGN>(x, T.intt_rw + (size_t)2 * N * j, q, lds32, t);
    const uint32_t inv_n = P.inv_n[j], inv_n_sh = P.inv_n_sh[j];
#pragma unroll
    for (int e = 0; e < 16; e++) x[e] = csub(mul_shoup_lazy(x[e], inv_n, inv_n_sh, q), q);
    if (A.pt)
    {
#pragma unroll
        for (int e = 0; e < 16; e++) A.pt[b * N + (e << CTOP) + t] = x[e];
    }
    if (!A.values) return;

    double re[16], im[16];
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        // representative in (-q/2, q/2], then 1/scale (ckks_tests_common.c:74-83)
        double dval = (x[e] > q / 2) ? -(double)(q - x[e]) : (double)x[e];
        re[e]       = __ddiv_rn(dval, P.scale);
        im[e]       = 0.0;
    }
    fft_tiles<LOGN>(re, im, T.ifft_w, plane, t);
    // values_decoded[i] = (flpt) Re res[index_map[i]]: this thread holds res[16t + e]; the slot
    // that reads it is inv_map[16t + e] when that is < n/2
    const uint4 *mp = reinterpret_cast<const uint4 *>(T.inv_map + 16 * t);
    uint4 m0 = mp[0], m1 = mp[1];
    uint32_t packed[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        uint32_t i = (packed[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
        if (i < (uint32_t)(N / 2)) A.values[b * (N / 2) + i] = (float)re[e];
    }
}

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_decrypt_decode(DevParams P, DevTables T,
                                                                          VerifyArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    decrypt_decode_body<LOGN, false>(P, T, A, KeyRing{}, smem);
}

// keyed twin: ciphertext b decrypted under ring key R.idx[b]
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_decrypt_decode_keyed(DevParams P, DevTables T,
                                                                                VerifyArgs A, KeyRing R)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    decrypt_decode_body<LOGN, true>(P, T, A, R, smem);
}

hipError_t launch_decrypt_decode(const DevParams &P, const DevTables &T, const uint32_t *c0,
                                 const uint32_t *c1, uint32_t in_primes, int j, uint32_t *dec_ntt,
                                 uint32_t *pt, float *values, size_t B, hipStream_t st, const KeyRing *ring)
{
    if (B == 0) return hipSuccess;
    VerifyArgs A{};
    A.c0        = c0;
    A.c1        = c1;
    A.dec_ntt   = dec_ntt;
    A.pt        = pt;
    A.values    = values;
    A.in_primes = in_primes;
    A.j         = j;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        using G         = XformGeom<L>;
        const dim3 grid((unsigned)B), block(G::THREADS);
        const size_t shmem = (size_t)G::SLOTS * sizeof(double);
        if (ring) return launch(k_decrypt_decode_keyed<L>, grid, block, shmem, st, P, T, A, *ring);
        return launch(k_decrypt_decode<L>, grid, block, shmem, st, P, T, A);
    });
}

// ------------------------------------------------------------------------------------------
// Full-modulus decrypt and decode: the receiving side for plaintexts larger than one prime.
// One workgroup per ciphertext, ALL primes in one launch.  Per prime j: pt_j = INTT(c0_j + c1_j . NTT(s)_j) as in
// decrypt_decode_body (same tiling, thread t holds the coefficients (e << (LOGN-4)) + t), then one step of the
// incremental Garner recombination folds pt_j into the centred value y of the coefficient:
//     y_0 = centred(pt_0),   c = centred((pt_j - y_{j-1}) . Q_{j-1}^-1 mod q_j),   y_j = y_{j-1} + Q_{j-1} c
// with Q_{j-1} = q_0 ... q_{j-1}; y_j is THE representative of the value mod Q_j in (-Q_j/2, Q_j/2] (Q_j odd:
// |y_j| <= (Q_{j-1} - 1)/2 + Q_{j-1} (q_j - 1)/2 = (Q_j - 1)/2).
// The state between primes is the int64 y plus one flag per thread.  Q_1 < 2^60, so y_1 always fits; y_2 = y_1 +
// Q_1 c is formed in 128 bits (|y_2| < 2^89) and the flag is raised when it leaves int64.  From the fourth prime on
// a value that fits int64 has c = 0 (|y| < 2^63 < Q_{j-1}/2 is already its centred representative), and a non-zero c
// gives |y_j| >= Q_{j-1}/2 > 2^63: the step is "reduce y mod q_j, compare with pt_j, flag a mismatch".  A flagged
// coefficient never comes back into range, so its y may be anything afterwards.
// The decode tail is decrypt_decode_body's with the int64 in place of the single-prime lift (ckks_decode,
// device/test/ckks_tests_common.c:72-115): same never-contracted FP64 operations, same root table.
// ------------------------------------------------------------------------------------------
// DEG2: the degree-2 form a tensor product leaves (se_amd_ct_mul_device), d = c0 + s (c1 + s c2) per prime with the
// third slab A.c2; everything after the per-prime d is the same code.
template <int LOGN, bool KEYED, bool DEG2 = false>
__device__ __forceinline__ void decrypt_full_body(const DevParams &P, const DevTables &T, const CrtParams &C,
                                                  const FullArgs &A, const KeyRing &R, unsigned char *smem)
{
    using G            = XformGeom<LOGN>;
    constexpr int N    = G::N;
    constexpr int CTOP = LOGN - 4;
    uint32_t *lds32  = reinterpret_cast<uint32_t *>(smem);
    double *plane    = reinterpret_cast<double *>(smem);
    const size_t b   = blockIdx.x;
    const int np     = (int)P.nprimes;
    const uint32_t *key = T.s_hat;
    if constexpr (KEYED) key = R.k0 + key_base(R, b);

    int64_t y[16];
    bool bad = false;
    uint64_t qprod = 1;   // Q_{j-1}; used for j = 1, 2 only (< 2^60)
    for (int j = 0; j < np; j++)
    {
        const int t      = opaque_index(threadIdx.x);   // per-prime addresses are formed here, not carried
        const uint32_t q = P.q[j];
        const size_t rec = (b * np + j) * N + 16 * t;
        uint32_t x[16];
        {
            uint32_t a[16], w[16], wp[16];
            if constexpr (DEG2)
            {
                // c1 + s c2 first, in the registers of c0: the live set never exceeds the four tiles of the linear form
                load16_pairs(w, wp, key, (size_t)j * N + 16 * t);
                load16(x, A.c2 + rec);
                load16(a, A.c1 + rec);
#pragma unroll
                for (int e = 0; e < 16; e++) a[e] = csub(csub(mul_shoup_lazy(x[e], w[e], wp[e], q), q) + a[e], q);
                load16(x, A.c0 + rec);
            }
            else
            {
                load16(x, A.c0 + rec);
                load16(a, A.c1 + rec);
                load16_pairs(w, wp, key, (size_t)j * N + 16 * t);
            }
#pragma unroll
            for (int e = 0; e < 16; e++)
                x[e] = csub(csub(mul_shoup_lazy(a[e], w[e], wp[e], q), q) + x[e], q);
        }
        intt_tiles<LOGN>(x, T.intt_rw + (size_t)2 * N * j, q, lds32, t);
        const uint32_t inv_n = P.inv_n[j], inv_n_sh = P.inv_n_sh[j];
#pragma unroll
        for (int e = 0; e < 16; e++) x[e] = csub(mul_shoup_lazy(x[e], inv_n, inv_n_sh, q), q);

        if (j == 0)
        {
#pragma unroll
            for (int e = 0; e < 16; e++) y[e] = centred_lift(x[e], q);
        }
        else
        {
            const uint32_t cr_hi = P.cr_hi[j], cr_lo = P.cr_lo[j];
            if (j <= 2)
            {
                const uint32_t qi = C.inv[j], qi_sh = C.inv_sh[j];
#pragma unroll
                for (int e = 0; e < 16; e++)
                {
                    // reduce_signed gives q for a negative multiple of q; any representative below 2q serves here
                    const uint32_t r = reduce_signed(y[e], q, cr_hi, cr_lo);           // [0, q]
                    const uint32_t d = x[e] + q - r;                                   // [0, 2q)
                    const int64_t c  = centred_lift(csub(mul_shoup_lazy(d, qi, qi_sh, q), q), q);
                    // y + Q_{j-1} c in 128 bits
                    const uint64_t lo  = qprod * (uint64_t)c;
                    const int64_t hi   = __mul64hi((long long)qprod, (long long)c);
                    const uint64_t lo2 = lo + (uint64_t)y[e];
                    const int64_t hi2  = hi + (y[e] >> 63) + (int64_t)(lo2 < lo);
                    y[e]               = (int64_t)lo2;
                    bad |= hi2 != (y[e] >> 63);
                }
            }
            else
            {
#pragma unroll
                for (int e = 0; e < 16; e++)
                    bad |= csub(reduce_signed(y[e], q, cr_hi, cr_lo), q) != x[e];
            }
        }
        qprod *= q;
    }

    const int t = threadIdx.x;
    const bool any_bad = __syncthreads_or(bad) != 0;
    if (A.status && t == 0) A.status[b] = any_bad ? 0 : 1;
    if (A.pte)
    {
#pragma unroll
        for (int e = 0; e < 16; e++) A.pte[b * N + (e << CTOP) + t] = y[e];
    }
    if (!A.values && !A.values_f64) return;

    double re[16], im[16];
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        re[e] = __ddiv_rn((double)y[e], P.scale);
        im[e] = 0.0;
    }
    fft_tiles<LOGN>(re, im, T.ifft_w, plane, t);
    // this thread holds res[16t + e]; the slot that reads it is inv_map[16t + e] when that is < n/2
    const uint4 *mp = reinterpret_cast<const uint4 *>(T.inv_map + 16 * t);
    uint4 m0 = mp[0], m1 = mp[1];
    uint32_t packed[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        uint32_t i = (packed[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
        if (i < (uint32_t)(N / 2))
        {
            if (A.values) A.values[b * (N / 2) + i] = (float)re[e];
            if (A.values_f64) A.values_f64[b * (N / 2) + i] = re[e];
        }
    }
}

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_decrypt_full(DevParams P, DevTables T, CrtParams C,
                                                                        FullArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    decrypt_full_body<LOGN, false>(P, T, C, A, KeyRing{}, smem);
}

// keyed twin: ciphertext b decrypted under ring key R.idx[b]
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_decrypt_full_keyed(DevParams P, DevTables T,
                                                                              CrtParams C, FullArgs A, KeyRing R)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    decrypt_full_body<LOGN, true>(P, T, C, A, R, smem);
}

// degree-2 twins (FullArgs::c2 set): d = c0 + s (c1 + s c2)
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_decrypt3_full(DevParams P, DevTables T, CrtParams C,
                                                                         FullArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    decrypt_full_body<LOGN, false, true>(P, T, C, A, KeyRing{}, smem);
}

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_decrypt3_full_keyed(DevParams P, DevTables T,
                                                                               CrtParams C, FullArgs A, KeyRing R)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    decrypt_full_body<LOGN, true, true>(P, T, C, A, R, smem);
}

hipError_t launch_decrypt_full(const DevParams &P, const DevTables &T, const CrtParams &C, const FullArgs &A, size_t B,
                               hipStream_t st, const KeyRing *ring)
{
    if (B == 0) return hipSuccess;
    if (!A.c0 || !A.c1 || (!A.pte && !A.values && !A.values_f64 && !A.status)) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        using G         = XformGeom<L>;
        const dim3 grid((unsigned)B), block(G::THREADS);
        // the INTT exchange takes SLOTS words; the FFT plane (SLOTS doubles) only when slots are decoded
        const size_t shmem = (size_t)G::SLOTS * ((A.values || A.values_f64) ? sizeof(double) : sizeof(uint32_t));
        if (A.c2)
        {
            if (ring) return launch(k_decrypt3_full_keyed<L>, grid, block, shmem, st, P, T, C, A, *ring);
            return launch(k_decrypt3_full<L>, grid, block, shmem, st, P, T, C, A);
        }
        if (ring) return launch(k_decrypt_full_keyed<L>, grid, block, shmem, st, P, T, C, A, *ring);
        return launch(k_decrypt_full<L>, grid, block, shmem, st, P, T, C, A);
    });
}

// reduce_set_e_small (ckks_common.c:259-265) for every prime: int8 error -> residues, natural order,
// into a [count][np][n] slab (public-key generation feeds them to k_ntt_fuse).
__global__ void k_reduce_small(DevParams P, const int8_t *e, uint32_t *out, int count)
{
    const int n = P.n, np = P.nprimes;
    size_t i    = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)count * n) return;
    size_t b = i / n, k = i - b * n;
    int32_t v = e[i];
    for (int j = 0; j < np; j++) out[(b * np + j) * n + k] = (v < 0 ? P.q[j] : 0u) + (uint32_t)v;
}

hipError_t launch_reduce_small(const DevParams &P, const int8_t *e, uint32_t *out, size_t count,
                               hipStream_t st)
{
    if (count == 0) return hipSuccess;
    size_t total = count * P.n;
    return launch(k_reduce_small, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P, e, out, (int)count);
}

// ------------------------------------------------------------------------------------------
// Key rings (se_context.cpp, set_*_keyring and the keyed entries)
// ------------------------------------------------------------------------------------------
// Prime j of K secret keys at once: workgroup k expands packed key k (2-bit codes, sample.c:98-129: 0 -> q-1, 1 -> 0,
// 2 -> 1; the host has refused code 3), forward NTT (as k_ntt_polys), (value, Shoup) pairs into ring key k's row j.
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ring_secret_ntt(DevParams P, DevTables T, int j,
                                                                           const uint8_t *packed, uint32_t *ring)
{
    using G            = XformGeom<LOGN>;
    constexpr int N    = G::N;
    constexpr int CTOP = LOGN - 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds32  = reinterpret_cast<uint32_t *>(smem);
    const int t      = threadIdx.x;
    const size_t k   = blockIdx.x;
    const uint8_t *sk = packed + k * (N / 4);
    const uint32_t q = P.q[j], two_q = q << 1;
    uint32_t x[16];
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        const uint32_t i    = (uint32_t)(e << CTOP) + (uint32_t)t;
        const uint32_t code = (sk[i >> 2] >> (6 - 2 * (i & 3))) & 3u;
        x[e]                = code + (code == 0 ? q : 0u) - 1u;
    }
    ntt_tiles<LOGN>(x, T.ntt_rw + 2 * xform_table_len(N) * j, q, lds32, t);
    uint32_t *po = ring + ((k * P.nprimes + j) * N + 16 * t) * 2;
#pragma unroll
    for (int e = 0; e < 16; e++)
    {
        const uint32_t v = canon4(x[e], q, two_q);
        po[2 * e]        = v;
        po[2 * e + 1]    = (uint32_t)((((uint64_t)v) << 32) / q);
    }
}

// k_make_pairs over K whole public-key slabs [K][np][n]: the prime of word i is (i / n) mod np
__global__ void k_ring_pairs(DevParams P, const uint32_t *vals, uint32_t *pairs, size_t total)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    {
        const uint32_t q = P.q[(i / P.n) % P.nprimes];
        const uint32_t v = vals[i];
        pairs[2 * i]     = v;
        pairs[2 * i + 1] = (uint32_t)((((uint64_t)v) << 32) / q);
    }
}

// The keyed kernels read only the clamped copy: no index the caller passes can form an address outside the ring.
__global__ void k_key_sanitize(const uint32_t *raw, uint32_t *idx, uint32_t *bad, uint32_t K, size_t B)
{
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t k = raw[b];
    idx[b]           = k < K ? k : K - 1;
    if (k >= K) bad[1 + atomicAdd(bad, 1u)] = (uint32_t)b;
}

// records with an out-of-range index (normally none: the workgroups read a zero count and leave)
__global__ void k_key_reject(KeyRejectArgs A)
{
    const uint32_t count = A.bad[0];
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x)
    {
        const size_t b = A.bad[1 + i];
        if (A.status && threadIdx.x == 0) A.status[b] = 2;
        for (int r = 0; r < 3; r++)
        {
            if (!A.rows[r]) continue;
            uint32_t *row = A.rows[r] + b * A.words[r];
            for (size_t w = threadIdx.x; w < A.words[r]; w += blockDim.x) row[w] = 0;
        }
    }
}

hipError_t launch_ring_secret_ntt(const DevParams &P, const DevTables &T, int j, const uint8_t *packed, uint32_t *ring,
                                  size_t K, hipStream_t st)
{
    if (K == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        using G = XformGeom<decltype(l)::value>;
        return launch(k_ring_secret_ntt<decltype(l)::value>, dim3((unsigned)K), dim3(G::THREADS),
                      (size_t)G::SLOTS * sizeof(uint32_t), st, P, T, j, packed, ring);
    });
}

hipError_t launch_ring_pairs(const DevParams &P, const uint32_t *vals, uint32_t *pairs, size_t K, hipStream_t st)
{
    const size_t total = K * P.nprimes * P.n;
    if (total == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, (size_t)64 * cus_or_default(P.num_cus));
    return launch(k_ring_pairs, dim3(grid), dim3(256), 0, st, P, vals, pairs, total);
}

hipError_t launch_key_sanitize(const uint32_t *raw, uint32_t *idx, uint32_t *bad, size_t K, size_t B, hipStream_t st)
{
    if (B == 0) return hipSuccess;
    if (K == 0 || K > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    return launch(k_key_sanitize, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, raw, idx, bad, (uint32_t)K, B);
}

hipError_t launch_key_reject(const DevParams &P, const KeyRejectArgs &A, size_t B, hipStream_t st)
{
    if (B == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>(B, (size_t)4 * cus_or_default(P.num_cus));
    return launch(k_key_reject, dim3(grid), dim3(256), 0, st, A);
}

// ------------------------------------------------------------------------------------------
// launchers (called from se_context.cpp)
// ------------------------------------------------------------------------------------------
template <int LOGN, int MODE>
static hipError_t launch_enc_mode(const DevParams &P, const DevTables &T, const EncArgs &A, size_t B,
                                  hipStream_t st, const KeyRing *ring)
{
    using G             = XformGeom<LOGN>;
    const size_t planes = (size_t)G::SLOTS * sizeof(double);   // the IFFT's two f64 half-planes
    const size_t quads  = (size_t)(G::N / 16) * enc_quad_stride<MODE>() * sizeof(uint32_t);
    // n <= 4096: one u32 NTT plane (public key: three, for the three-way NTT) + the transpose region
    // behind it (not in the general public-key form)
    size_t shmem_fast = planes, shmem_gen = planes;
    if (LOGN <= 12)
    {
        const size_t ntt_planes = (size_t)(MODE == kModeAsym ? 3 : 1) * G::SLOTS * sizeof(uint32_t);
        // public key: the transpose region is aliased into the three planes (encrypt_one, QALIAS)
        shmem_fast = MODE == kModeAsym ? std::max(planes, std::max(ntt_planes, quads)) : std::max(planes, ntt_planes + quads);
        // (the general forms never alias the region; the general public-key form keeps the tile layout)
        shmem_gen  = MODE == kModeAsym ? std::max(planes, ntt_planes) : std::max(planes, ntt_planes + quads);
    }
    hipError_t e = hipMemsetAsync(A.general, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    EncArgs Af = A;
    Af.count   = B;
    Af.first   = 0;
    if (enc_pairs<LOGN, MODE>())
    {
        shmem_fast = std::max(shmem_fast, (kPairParkWords + (size_t)G::N) * sizeof(uint32_t));
        if (shmem_fast < pair_lds_extent<LOGN>()) return hipErrorInvalidValue;
    }
    const unsigned grid_fast = (unsigned)(enc_pairs<LOGN, MODE>() ? (B + 1) / 2 : B);   // two plaintexts per workgroup
    // the plaintexts the fast form declined (normally none: the workgroups read a zero count and leave)
    const dim3 fast(grid_fast), gen((unsigned)std::min<size_t>(B, (size_t)4 * cus_or_default(P.num_cus))), block(G::THREADS);
    if constexpr (MODE != kModeEncodeOnly)
    {
        if (ring)
        {
            e = launch(k_encode_encrypt_keyed<LOGN, MODE>, fast, block, shmem_fast, st, P, T, Af, *ring);
            if (e != hipSuccess) return e;
            return launch(k_encode_encrypt_general_keyed<LOGN, MODE>, gen, block, shmem_gen, st, P, T, A, *ring);
        }
    }
    if constexpr (enc_pairs<LOGN, MODE>())
    {
        // The whole pairs of a fast, unkeyed launch take the two-way pair form; an odd last plaintext takes the one-plane
        // form, and so does everything under kEncFlagOnePlane (A.debug_flags: the forms are bit-identical).
        if (!(A.debug_flags & kEncFlagOnePlane) && B >= 2)
        {
            // two u32 NTT planes = the encoder's two f64 half-planes; the transpose region lies inside them
            const size_t shmem_pair2 = std::max(planes, (size_t)2 * G::SLOTS * sizeof(uint32_t));
            if (shmem_pair2 < pair2_lds_extent<LOGN, MODE>()) return hipErrorInvalidValue;
            e = launch(k_encode_encrypt_pair2<LOGN, MODE>, dim3((unsigned)(B / 2)), block, shmem_pair2, st, P, T, Af);
            if (e != hipSuccess) return e;
            if (B & 1)
            {
                Af.first = B - 1;
                e = launch(k_encode_encrypt<LOGN, MODE>, dim3(1), block, shmem_fast, st, P, T, Af);
                if (e != hipSuccess) return e;
            }
            return launch(k_encode_encrypt_general<LOGN, MODE>, gen, block, shmem_gen, st, P, T, A);
        }
    }
    e = launch(k_encode_encrypt<LOGN, MODE>, fast, block, shmem_fast, st, P, T, Af);
    if (e != hipSuccess) return e;
    return launch(k_encode_encrypt_general<LOGN, MODE>, gen, block, shmem_gen, st, P, T, A);
}

hipError_t launch_encode_encrypt(const DevParams &P, const DevTables &T, const EncArgs &A, int mode,
                                 size_t B, hipStream_t st, const KeyRing *ring)
{
    if (B == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        if (!A.general) return hipErrorInvalidValue;   // the context's list of declined plaintexts
        switch (mode)
        {
            case kModeSym: return launch_enc_mode<L, kModeSym>(P, T, A, B, st, ring);
            case kModeAsym: return launch_enc_mode<L, kModeAsym>(P, T, A, B, st, ring);
            default:
                if (ring) return hipErrorInvalidValue;   // encode-only reads no key
                return launch_enc_mode<L, kModeEncodeOnly>(P, T, A, B, st, nullptr);
        }
    });
}

template <int LOGN, bool ADD_ERR>
static hipError_t launch_enc_rns_e(const DevParams &P, const DevTables &T, const EncArgs &A, size_t B,
                                   hipStream_t st)
{
    using G      = XformGeom<LOGN>;
    size_t shmem = (size_t)G::SLOTS * sizeof(double);
    if (!A.general) return hipErrorInvalidValue;   // the context's list of declined plaintexts
    hipError_t e = hipMemsetAsync(A.general, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    e = launch(k_encode_rns<LOGN, ADD_ERR>, dim3((unsigned)B), dim3(G::THREADS), shmem, st, P, T, A);
    if (e != hipSuccess) return e;
    // plaintexts with NaN / infinite values (normally none: the workgroups read a zero count and leave)
    const unsigned grid = (unsigned)std::min<size_t>(B, (size_t)cus_or_default(P.num_cus));
    return launch(k_encode_rns_general<LOGN, ADD_ERR>, dim3(grid), dim3(G::THREADS), shmem, st, P, T, A);
}

hipError_t launch_encode_rns(const DevParams &P, const DevTables &T, const EncArgs &A, bool add_err,
                             size_t B, hipStream_t st)
{
    if (B == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        return add_err ? launch_enc_rns_e<L, true>(P, T, A, B, st) : launch_enc_rns_e<L, false>(P, T, A, B, st);
    });
}

hipError_t launch_ntt_fuse(const DevParams &P, const DevTables &T, const EncArgs &A, int mode, int j,
                           size_t B, hipStream_t st, const KeyRing *ring)
{
    if (B == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        using G         = XformGeom<L>;
        const dim3 grid((unsigned)B), block(G::THREADS);
        const size_t shmem = (size_t)G::SLOTS * sizeof(uint32_t);
        if (ring)
        {
            if (mode != kModeSym) return hipErrorInvalidValue;   // only the symmetric epilogue reads a key
            return launch(k_ntt_fuse_keyed<L, kModeSym>, grid, block, shmem, st, P, T, A, *ring, j);
        }
        if (mode == kModeSym) return launch(k_ntt_fuse<L, kModeSym>, grid, block, shmem, st, P, T, A, j);
        return launch(k_ntt_fuse<L, kModeEncodeOnly>, grid, block, shmem, st, P, T, A, j);
    });
}

hipError_t launch_ntt_polys(const DevParams &P, const DevTables &T, int j, uint32_t *polys,
                            uint32_t *pairs, size_t count, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        using G = XformGeom<decltype(l)::value>;
        return launch(k_ntt_polys<decltype(l)::value>, dim3((unsigned)count), dim3(G::THREADS),
                      (size_t)G::SLOTS * sizeof(uint32_t), st, P, T, j, polys, pairs);
    });
}

hipError_t launch_make_pairs(const uint32_t *vals, uint32_t *pairs, uint32_t q, size_t count,
                             hipStream_t st)
{
    if (count == 0) return hipSuccess;
    return launch(k_make_pairs, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, vals, pairs, q, (int)count);
}

}  // namespace seamd
