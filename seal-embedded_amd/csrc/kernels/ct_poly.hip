// ct_poly.hip -- the last step of a slot-wise polynomial: se_amd_ct_affine_rescale_device (AffineRescaleArgs).  Up to 16
// term records that live at their own levels, each times a wide integer weight, are summed, the sum is rescaled ONCE and
// a constant joins slab 0:
//   acc_s[b][j] = sum_t w[t][j] . term_s[t][b][j]  mod q_j   (j < primes; w[t][j] = w_t mod q_j, formed on the host),
//   out_s[b]    = rescale(acc_s[b]) + (s == 0 ? c : 0)        (c[i] = c_after mod q_i in every position of row i).
// The body of k_ct_rescale (ct_ops.hip) in its geometry -- one workgroup of n/16 threads per (record, slab), LDS the
// exchange plane alone, no scratch, no global temporary, one launch -- with every row it would load formed in registers
// instead, in the quad layout load_quads gives (affine_row), the way k_ct_dot_sp forms its rows: the sum never touches
// memory and no term is copied to the level of the call.  A term record has term_primes[t] >= primes rows and only the
// first `primes` are read: the record stride is the term's own, the row index the call's.
//   last row: affine_row(last) -> quads_to_tile -> intt_tiles mod q_last -> . n^-1 -> centred lift: 16 signed values per
//             thread, kept across the prime loop as in k_ct_rescale;
//   per lower prime i: affine_row(i), then delta mod q_i -> ntt_tiles -> tile_to_quads -> (row - NTT) . q_last^-1,
//             canonical; then + c[i] on slab 0, canonical (slab 1 adds 0 through the same two operations: the slab is
//             blockIdx.y, wave-uniform) -> quad store.
// k_ct_rescale requests ONE row before the transform and lets it land while the transform runs.  A row here is T rows of
// loads and 16 64-bit sums; held in flight across ntt_tiles they would cost the kernel its fourth wave, so the row is
// formed BEFORE the transform (its loads overlap the other workgroups of the compute unit, 3 to 4 per SIMD) and only its
// 16 canonical words are carried across it, exactly the registers k_ct_rescale carries.
// Lazy accumulation: the range argument.  Every prime of the chains is below 2^30 (se_host_tables.cpp), a weight residue
// is w <= q - 1 (canonical: the host reduces the int64 to [0, q)) and a residue of a slab is x <= q - 1, so one product
// is at most (q - 1)^2 < 2^60.  The 64-bit sum starts at 0 and takes T <= 16 products:
//   16 (q - 1)^2 < 16 . 2^60 = 2^64,
// so SE_AMD_AFFINE_MAX_TERMS = 16 weighted terms fit between reductions -- one barrett64 (exact for every 64-bit input)
// per word at the end of the row and none inside it; a 17th term would not fit (17 (q - 1)^2 > 2^64 already for the
// smallest prime of the 30-bit chain, 1 053 818 881), which is why the entry stops at 16.  The all-maximal test (every
// residue and every weight q_j - 1, T = 16) sits on that bound.
// The map is plain modular arithmetic on whatever words the slabs hold (defined for residues in [0, q_j)); the weights,
// the constant, the term pointers and the term levels are ordinary kernel arguments (wave-uniform, read through the
// scalar cache); no word of a slab is used as an address.  grid (B, 2).
#include "kernel_args.h"
#include "launch.h"
#include "modarith.cuh"
#include "transform.cuh"

namespace seamd {
namespace {

// x = row j of the weighted sum of record b, slab `slab`, canonical, in quad layout (as load_quads with index tq)
template <int LOGN>
__device__ __forceinline__ void affine_row(uint32_t (&x)[16], const AffineRescaleArgs &A, uint32_t slab, size_t b,
                                           uint32_t j, const DevParams &P, int tq)
{
    constexpr size_t N = (size_t)1 << LOGN;
    uint64_t acc[16];
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0;
#pragma unroll 1
    for (uint32_t t = 0; t < A.T; t++)
    {
        const uint32_t *rec = (slab ? A.term1[t] : A.term0[t]) + b * A.term_primes[t] * N;
        const uint32_t w    = A.w[t][j];
        uint32_t v[16];
        load_quads(v, rec + (size_t)j * N, tq);
#pragma unroll
        for (int e = 0; e < 16; e++) acc[e] += (uint64_t)v[e] * w;
    }
    const uint32_t q = P.q[j], cr_hi = P.cr_hi[j], cr_lo = P.cr_lo[j];
#pragma unroll
    for (int e = 0; e < 16; e++) x[e] = barrett64(acc[e], q, cr_hi, cr_lo);
}

}  // namespace

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_affine_rescale(const DevParams P, const DevTables T,
                                                                             const RescaleParams R,
                                                                             const AffineRescaleArgs A)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds       = reinterpret_cast<uint32_t *>(smem);
    const int t         = threadIdx.x;
    const size_t b      = blockIdx.x;
    const uint32_t slab = blockIdx.y;
    const uint32_t last = A.primes - 1;
    uint32_t *out       = (slab ? A.out1 : A.out0) + b * last * N;

    int32_t delta[16];
    {
        const uint32_t q = P.q[last];
        uint32_t x[16];
        affine_row<LOGN>(x, A, slab, b, last, P, t);
        quads_to_tile<16>(x, lds, t);
        __syncthreads();
        intt_tiles<LOGN>(x, T.intt_rw + (size_t)2 * N * last, q, lds, t);
        const uint32_t inv_n = P.inv_n[last], inv_n_sh = P.inv_n_sh[last];
#pragma unroll
        for (int e = 0; e < 16; e++)
            delta[e] = (int32_t)centred_lift(csub(mul_shoup_lazy(x[e], inv_n, inv_n_sh, q), q), q);
    }
    for (uint32_t j = 0; j < last; j++)
    {
        const uint32_t q = P.q[j], two_q = q << 1;
        uint32_t c[16], x[16];
        affine_row<LOGN>(c, A, slab, b, j, P, opaque_index(t));
#pragma unroll
        for (int e = 0; e < 16; e++) x[e] = (uint32_t)delta[e] + ((uint32_t)(delta[e] >> 31) & q);   // [0, q)
        ntt_tiles<LOGN>(x, T.ntt_rw + 2 * xform_table_len(N) * j, q, lds, t);
        tile_to_quads<16>(x, lds, t);
        const uint32_t w = R.inv[j], wp = R.inv_sh[j];
        const uint32_t cj = slab ? 0u : A.c[j];   // the constant polynomial is constant in NTT form
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            const uint32_t u = min(x[e], x[e] - two_q);                                  // NTT output [0, 4q) -> [0, 2q)
            const uint32_t r = csub(mul_shoup_lazy(c[e] + two_q - u, w, wp, q), q);      // the rescale's word, canonical
            x[e]             = csub(r + cj, q);
        }
        store_quads(out + (size_t)j * N, x, t);
        __syncthreads();
    }
}

// LOGN 12 .. 14: the degrees whose default chains have two or more primes.
hipError_t launch_ct_affine_rescale(const DevParams &P, const DevTables &T, const RescaleParams &R,
                                    const AffineRescaleArgs &A, size_t B, hipStream_t st)
{
    if (B == 0) return hipSuccess;
    if (P.logn < 12) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value < 12 ? 12 : decltype(l)::value;
        using G         = XformGeom<L>;
        return launch(k_ct_affine_rescale<L>, dim3((unsigned)B, 2), dim3(G::THREADS), (size_t)G::SLOTS * sizeof(uint32_t),
                      st, P, T, R, A);
    });
}

}  // namespace seamd
