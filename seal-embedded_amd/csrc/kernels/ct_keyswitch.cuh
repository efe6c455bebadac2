// ct_keyswitch.cuh -- the device steps the key-switch kernels of ct_ops.hip and ct_pack.hip share: the coefficients of a
// row (evk_quads_coeffs, evk_row_coeffs), THE multiply-accumulate against a key column (load_pair_quad, evk_mac), the grid
// (evk_grid), the automorphism of a row in either domain (galois_src_of, galois_src, park_row_quads, gather_row,
// load_row_sigma) and the pieces of the special-prime key switch (sp_quads_digit, sp_row_digit, sp_delta).  What each is
// for, its lazy ranges and the LDS protocol stand at the kernels that use them first, in ct_ops.hip: above k_ct_relin
// (evk_*), above k_ct_galois (sigma) and above ct_key_switch_sp (sp_*).
#pragma once
#include "kernel_args.h"
#include "launch.h"
#include "modarith.cuh"
#include "transform.cuh"

namespace seamd {

// the part behind the load: x = a row of prime j in quad layout in registers (k_ct_dot_sp forms its rows there)
template <int LOGN>
__device__ __forceinline__ void evk_quads_coeffs(uint32_t (&x)[16], uint32_t j, const DevParams &P, const DevTables &T,
                                                 uint32_t *lds, int tj)
{
    constexpr int N   = XformGeom<LOGN>::N;
    const uint32_t qj = P.q[j];
    quads_to_tile<16>(x, lds, tj);
    __syncthreads();
    intt_tiles<LOGN>(x, T.intt_rw + (size_t)2 * N * j, qj, lds, tj);
    const uint32_t inv_n = P.inv_n[j], inv_n_sh = P.inv_n_sh[j];
#pragma unroll
    for (int e = 0; e < 16; e++) x[e] = csub(mul_shoup_lazy(x[e], inv_n, inv_n_sh, qj), qj);
}

template <int LOGN>
__device__ __forceinline__ void evk_row_coeffs(uint32_t (&x)[16], const uint32_t *row, uint32_t j, const DevParams &P,
                                               const DevTables &T, uint32_t *lds, int tj)
{
    load_quads(x, row, tj);
    evk_quads_coeffs<LOGN>(x, j, P, T, lds, tj);
}

// One quad of a (word, Shoup) row pair, the layout of every key column and plan diagonal (kernel_args.h): the words
// p[256 m .. 256 m + 3] and their companions N further.
template <int N>
__device__ __forceinline__ void load_pair_quad(const uint32_t *p, int m, uint32_t (&w)[4], uint32_t (&s)[4])
{
    const uint4 a = *reinterpret_cast<const uint4 *>(p + (m << 8));
    const uint4 b = *reinterpret_cast<const uint4 *>(p + N + (m << 8));
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
    s[0] = b.x, s[1] = b.y, s[2] = b.z, s[3] = b.w;
}

// THE multiply-accumulate of every key switch of this file: acc_h += y . key_h[row][column] on both halves h, lazy as
// described above.  `key` = the thread's first quad of that column in half 0; word(c, k) = the 32-bit y of word 4c + k
// of the thread's quads (any value: see the range argument).
template <int LOGN, class Word>
__device__ __forceinline__ void evk_mac(uint32_t (&acc0)[16], uint32_t (&acc1)[16], const uint32_t *key, size_t half,
                                        uint32_t q, Word word)
{
    constexpr int N      = XformGeom<LOGN>::N;
    const uint32_t two_q = q << 1;
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        uint32_t w0[4], s0[4], w1[4], s1[4];
        load_pair_quad<N>(key, c, w0, s0);
        load_pair_quad<N>(key + half, c, w1, s1);
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const int e       = 4 * c + k;
            const uint32_t y  = word(c, k);
            const uint32_t u0 = acc0[e] + mul_shoup_lazy(y, w0[k], s0[k], q);
            const uint32_t u1 = acc1[e] + mul_shoup_lazy(y, w1[k], s1[k], q);
            acc0[e]           = min(u0, u0 - two_q);
            acc1[e]           = min(u1, u1 - two_q);
        }
    }
}

// the same on y in quad layout in registers
template <int LOGN>
__device__ __forceinline__ void evk_mac(uint32_t (&acc0)[16], uint32_t (&acc1)[16], const uint32_t (&y)[16],
                                        const uint32_t *key, size_t half, uint32_t q)
{
    evk_mac<LOGN>(acc0, acc1, key, half, q, [&](int c, int k) { return y[4 * c + k]; });
}

// The grid of every key-switch kernel: (min(B, 2^31 - 1), primes); a workgroup walks the records blockIdx.x,
// blockIdx.x + gridDim.x, ...
static dim3 evk_grid(size_t B, uint32_t primes)
{
    return dim3((unsigned)(B < 0x7fffffffu ? B : 0x7fffffffu), primes);
}

// src_g of the word whose (2 brev(k) + 1) g is u (any bits above 2n are dropped by the shift, the odd bit by the mask):
// the form of the hoisted kernels.  galois_src below keeps its own: as galois_src_of((2 brev(k) + 1) g), with the scatter
// shared too, k_ct_galois_sp<12> ran 10.597 ms against the parent's 10.566 (spread of the parent's rounds 0.025).
template <int LOGN>
__device__ __forceinline__ uint32_t galois_src_of(uint32_t u)
{
    return (__brev(u) >> (31 - LOGN)) & ((1u << LOGN) - 1);
}

template <int LOGN>
__device__ __forceinline__ uint32_t galois_src(uint32_t k, uint32_t g)
{
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t r     = __brev(k) >> (32 - LOGN);
    const uint32_t u     = ((2 * r + 1) * g) & (2 * N - 1);   // odd: (2r + 1) g < 2^30
    return __brev(u >> 1) >> (32 - LOGN);
}

// A row in quad layout (load_quads) parked in the plane as it lies in memory, word k at lds[k]: four ds_write_b128.  k4 =
// the thread's first quad (quad_index(t, 0)); word 4 m + k of the thread is k4 + (m << 8) + k.
__device__ __forceinline__ void park_row_quads(const uint32_t (&c)[16], uint32_t *lds, int k4)
{
#pragma unroll
    for (int m = 0; m < 4; m++)
        *reinterpret_cast<uint4 *>(lds + k4 + (m << 8)) = make_uint4(c[4 * m], c[4 * m + 1], c[4 * m + 2], c[4 * m + 3]);
}

// The thread's 16 words of sigma_g of a parked row: word k = lds[src_g(k)].
template <int LOGN>
__device__ __forceinline__ void gather_row(uint32_t (&c)[16], const uint32_t *lds, int k4, uint32_t g)
{
#pragma unroll
    for (int e = 0; e < 16; e++) c[e] = lds[galois_src<LOGN>((uint32_t)(k4 + ((e >> 2) << 8) + (e & 3)), g)];
}

// The row `row` of a record as it lies in memory, in quad layout; GALOIS: sigma_g of it, word k = row[src_g(k)], through
// the plane (which must be free; ends with the plane read but not yet released: the caller's next barrier releases it).
template <int LOGN, bool GALOIS>
__device__ __forceinline__ void load_row_sigma(uint32_t (&c)[16], const uint32_t *row, uint32_t g, uint32_t *lds, int te)
{
    load_quads(c, row, te);
    if constexpr (GALOIS)
    {
        const int k4 = quad_index(te, 0);
        park_row_quads(c, lds, k4);
        __syncthreads();
        gather_row<LOGN>(c, lds, k4, g);
    }
}

// NTT_c(D_j mod q) in quad layout, q = q_c the prime of key column c and rw its roots: the centred coefficients of input
// row j (GALOIS: of sigma_g of it) reduced mod q and transformed.  Ends with the plane in use by the wave-local
// transpose: the caller's barrier after the multiply-accumulate releases it.
// sp_quads_digit: the same on x = row j in quad layout in registers, as load_quads with the opaque index tj leaves it.
template <int LOGN, bool GALOIS>
__device__ __forceinline__ void sp_quads_digit(uint32_t (&x)[16], uint32_t j, uint32_t g, uint32_t q, const uint32_t *rw,
                                               const DevParams &P, const DevTables &T, uint32_t *lds, int t, int tj)
{
    const uint32_t qj = P.q[j], hj = qj >> 1, up = q - qj;   // up: mod 2^32 where q < q_j
    evk_quads_coeffs<LOGN>(x, j, P, T, lds, tj);
    constexpr int N = XformGeom<LOGN>::N;
    if constexpr (GALOIS)
    {
        // sigma, the scatter of k_ct_galois (its own copy: see there)
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            const uint32_t u = (uint32_t)(tj + (N / 16) * e) * g;
            lds[u & (N - 1)] = (u & N) && x[e] ? qj - x[e] : x[e];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; e++) x[e] = lds[tj + (N / 16) * e];
        __syncthreads();
    }
    // centred: c > (q_j - 1) / 2 stands for c - q_j, whose residue mod q is c - q_j + q, in (0, q) for every pair of
    // primes of the chains (they lie within 1 % of one another); c <= (q_j - 1) / 2 is its own residue
#pragma unroll
    for (int e = 0; e < 16; e++) x[e] += x[e] > hj ? up : 0u;
    const int td = opaque_index(t);
    ntt_tiles<LOGN>(x, rw, q, lds, td);
    tile_to_quads<16>(x, lds, td);
}

template <int LOGN, bool GALOIS>
__device__ __forceinline__ void sp_row_digit(uint32_t (&x)[16], const uint32_t *row, uint32_t j, uint32_t g, uint32_t q,
                                             const uint32_t *rw, const DevParams &P, const DevTables &T, uint32_t *lds,
                                             int t)
{
    const int tj = opaque_index(t);
    load_quads(x, row, tj);
    sp_quads_digit<LOGN, GALOIS>(x, j, g, q, rw, P, T, lds, t, tj);
}

// Between the passes of every special-prime kernel (ct_key_switch_sp, ct_hoist_sp): the accumulators hold acc_k[p] in
// quad layout, lazy in [0, 2 P); delta_k = centred(INTT_p(acc_k)), and the accumulator of pass 1 starts at
// -NTT_i(delta_k mod q_i), lazy in (0, 2 q_i].  The two halves take the same code: not unrolled, the halves change
// places after each turn.  Ends behind a barrier with the plane free.
template <int LOGN>
__device__ __forceinline__ void sp_delta(uint32_t (&acc0)[16], uint32_t (&acc1)[16], uint32_t i, uint32_t sp,
                                         const DevParams &P, const DevTables &T, uint32_t *lds, int t)
{
    constexpr int N      = XformGeom<LOGN>::N;
    const uint32_t q     = P.q[sp], qi = P.q[i], two_qi = qi << 1;
    const uint32_t *rwi  = T.ntt_rw + 2 * xform_table_len(N) * i;
    const uint32_t inv_n = P.inv_n[sp], inv_n_sh = P.inv_n_sh[sp], hp = q >> 1, down = qi - q;
#pragma unroll 1
    for (uint32_t k = 0; k < 2; k++)
    {
        const int td = opaque_index(t);
        quads_to_tile<16>(acc0, lds, td);
        __syncthreads();
        intt_tiles<LOGN>(acc0, T.intt_rw + (size_t)2 * N * sp, q, lds, td);
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            const uint32_t v = csub(mul_shoup_lazy(acc0[e], inv_n, inv_n_sh, q), q);
            acc0[e]          = v + (v > hp ? down : 0u);   // delta mod q_i in [0, q_i): |delta| < P / 2 < q_i
        }
        const int tn = opaque_index(t);
        ntt_tiles<LOGN>(acc0, rwi, qi, lds, tn);
        tile_to_quads<16>(acc0, lds, tn);
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            const uint32_t u = min(acc0[e], acc0[e] - two_qi);   // NTT output [0, 4q) -> [0, 2q)
            const uint32_t o = acc1[e];
            acc1[e]          = two_qi - u;                       // (0, 2q]
            acc0[e]          = o;
        }
        __syncthreads();
    }
}

}  // namespace seamd
