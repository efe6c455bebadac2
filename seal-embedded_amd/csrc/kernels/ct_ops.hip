// ct_ops.hip -- key-free operations on resident ciphertext slabs: weighted sums of records (se_amd_ct_lincomb_device),
// slot-wise products with encoded plaintexts (se_amd_ct_mul_plain_device) and the rescale that drops the last prime
// (se_amd_ct_rescale_device), and the ciphertext products: the tensor (se_amd_ct_mul_device) and the relinearisation
// that brings it back to two slabs (se_amd_ct_relin_device, with the key plumbing), and the slot rotation: a ring
// automorphism fused with its key switch (se_amd_ct_galois_device), and its hoisted form, many rotations of a record
// from one digit decomposition (se_amd_ct_galois_many_device, se_amd_ct_galois_sum_device, at the end of the file), and
// the plaintext-weighted sum of hoisted rotations under a plan (se_amd_ct_lintrans_device, behind them), and the
// special-prime key switch that relinearises and rotates at the record's own scale (se_amd_ct_relin_sp_device,
// se_amd_ct_galois_sp_device, behind k_ct_galois), and the two device steps of a baby-step / giant-step transform: the
// plaintext-weighted sum over a stack of batches and the rotate-and-accumulate over different records
// (se_amd_ct_mul_plain_sum_device, se_amd_ct_galois_accum_device, se_amd_ct_bsgs_device, behind the special-prime hoist),
// and the same transform on the special-prime keys with the division by P deferred: undivided baby steps, the division of
// extended records and the one-division giant sum (se_amd_ct_galois_many_ext_sp_device, se_amd_ct_mod_down_sp_device,
// se_amd_ct_galois_accum_sp_device, se_amd_ct_bsgs_sp_device, between the two), and the switch-key ring: the special-prime
// key switch with the key chosen per record, alone or summed over CSR rows with one division by P per row
// (se_amd_ct_switch_keyed_sp_device, se_amd_ct_switch_sum_keyed_sp_device, behind k_ct_galois_sp), and the grouped
// product sums: the tensor summed over CSR rows of pairs, key-free (se_amd_ct_mul_sum_device, behind k_ct_mul) or with
// one special-prime relinearisation per row (se_amd_ct_dot_sp_device, behind the switch-key ring).
//
// A slab is uint32 [record][prime][coeff] in NTT form, so a linear combination of records, or a product with a
// plaintext in the same form, is element-wise arithmetic mod q_j: no transform, no key, no table.  Unlike the rest of
// the tree these two are bound by HBM, not by VALU issue: every input row is read once per use and every output row
// written once.
//
// Access shape.  A row is np * n residues; n is a multiple of 1024, so a 256-thread workgroup that owns 1024
// consecutive residues (one lane = 4 residues = one 16-byte load per input row) lies inside ONE prime: q_j and its
// Barrett constants are workgroup-uniform (DevParams, scalar registers).  The entry list of an output row (record
// indices, weights) depends only on blockIdx and the loop counter, so it is read through uniform (scalar) loads.
// kLcFlight input rows are loaded before any of them is used.  Row offsets are 64-bit: B * row * 4 passes 4 GiB at
// sizes users run (4096 x 3, B = 65 536 is 3.2 GB per slab; 16384 x 13 reaches 4 GiB at B = 5 042).
#include "kernel_args.h"
#include "launch.h"
#include "modarith.cuh"
#include "transform.cuh"
// the device steps the key-switch kernels share with ct_pack.hip (evk_row_coeffs, evk_mac, evk_grid, load_row_sigma,
// sp_row_digit, sp_delta, ...): described at the kernels below that use them first
#include "ct_keyswitch.cuh"

namespace seamd {
namespace {

constexpr uint32_t kLcThreads = 256;
constexpr uint32_t kLcTileLog = 10;   // residues per workgroup = 4 * kLcThreads = 1024 <= n: one prime per workgroup
constexpr int kLcFlight       = 4;    // input rows in flight per wave
// Lazy accumulation, weighted form.  Every prime of the chains is below 2^30 (se_host_tables.cpp) and a weight is
// reduced to wq <= q (reduce_signed gives q, not 0, for a negative multiple of q), a residue is c <= q - 1, so one
// product is at most q (q - 1).  The accumulator enters a period canonical (<= q - 1) and takes kLcPeriod products:
//   (q - 1) + 16 q (q - 1) = (q - 1)(16 q + 1) < 16 q^2 < 16 (2^30)^2 = 2^64,
// so 16 products fit a uint64 before barrett64 (which is exact for every 64-bit input); 17 would not.
constexpr int kLcPeriod = 16;
// Unit weights: a term is a residue < 2^30 and a row has fewer than 2^32 entries (the entry rejects nnz >= 2^32), so
// the plain uint64 sum stays below 2^62: no reduction before the last one.  The sum of S <= 65 535 canonical partial
// rows (k_ct_lincomb_sum) is below 2^46 the same way.
static_assert(kLcPeriod % kLcFlight == 0, "a period is a whole number of load groups");
// bits of a relinearisation digit (SE_AMD_RELIN_DIGIT_BITS): two digits cover a coefficient below 2^30
constexpr int kRelinDigitBits = 15;

struct Lane4
{
    uint64_t a[4] = {0, 0, 0, 0};
    __device__ __forceinline__ void add(const uint4 &v)
    {
        a[0] += v.x;
        a[1] += v.y;
        a[2] += v.z;
        a[3] += v.w;
    }
    __device__ __forceinline__ void mad(const uint4 &v, uint32_t w)
    {
        a[0] += (uint64_t)v.x * w;
        a[1] += (uint64_t)v.y * w;
        a[2] += (uint64_t)v.z * w;
        a[3] += (uint64_t)v.w * w;
    }
    __device__ __forceinline__ void mad4(const uint4 &v, const uint4 &w)
    {
        a[0] += (uint64_t)v.x * w.x;
        a[1] += (uint64_t)v.y * w.y;
        a[2] += (uint64_t)v.z * w.z;
        a[3] += (uint64_t)v.w * w.w;
    }
    __device__ __forceinline__ void reduce(uint32_t q, uint32_t cr_hi, uint32_t cr_lo)
    {
#pragma unroll
        for (int e = 0; e < 4; e++) a[e] = barrett64(a[e], q, cr_hi, cr_lo);
    }
    __device__ __forceinline__ uint4 get() const
    {
        return make_uint4((uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3]);
    }
};

__device__ __forceinline__ uint4 load_row(const uint32_t *__restrict__ slab, size_t record, size_t row, size_t off)
{
    return *reinterpret_cast<const uint4 *>(slab + record * row + off);
}

}  // namespace

// grid (row / 1024 * slabs, S, output rows of the launch); slice blockIdx.y of output row g0 + blockIdx.z.
// S = 1: the canonical row goes to `out`, the status to `status`.  S > 1: the canonical partial row goes to
// part[slab][g * S + s] and flag[g * S + s] says whether the slice saw an invalid entry (k_ct_lincomb_sum follows).
template <bool UNIT>
__global__ __launch_bounds__(kLcThreads) void k_ct_lincomb(const DevParams P, const LincombArgs A)
{
    const size_t row      = (size_t)P.nprimes << P.logn;
    const uint32_t chunks = (uint32_t)(row >> kLcTileLog);
    const uint32_t slab   = blockIdx.x / chunks;
    const uint32_t chunk  = blockIdx.x - slab * chunks;
    const uint32_t j      = (chunk << kLcTileLog) >> P.logn;
    const uint32_t q = P.q[j], cr_hi = P.cr_hi[j], cr_lo = P.cr_lo[j];
    const uint32_t *__restrict__ in  = slab ? A.in1 : A.in0;
    const uint32_t *__restrict__ idx = A.idx;
    const int32_t *__restrict__ wt   = A.w;
    const size_t off = ((size_t)chunk << kLcTileLog) + 4 * threadIdx.x;
    const size_t g   = A.g0 + blockIdx.z;
    const uint32_t S = gridDim.y, s = blockIdx.y;

    // the entries [lo, hi) of the row; dense form: entry k is record k - lo
    uint64_t lo, hi;
    bool bad = false;
    if (A.row_ptr)
    {
        const uint32_t a = A.row_ptr[g], b = A.row_ptr[g + 1];
        bad = a > b || b > A.nnz;
        lo  = a;
        hi  = bad ? a : b;
        if (A.B == 0 && hi > lo)   // every index is out of range and there is no record to read
        {
            bad = true;
            hi  = lo;
        }
    }
    else
    {
        lo = (uint64_t)g * A.B;
        hi = lo + A.B;
    }
    const uint64_t len = hi - lo;                 // < 2^32, S < 2^16
    uint64_t k         = lo + len * s / S;
    const uint64_t end = lo + len * (s + 1) / S;

    // An invalid index marks the row (it will be all zero) and reads record 0 instead, which exists: B > 0 here.
    auto record_of = [&](uint64_t e) -> size_t {
        if (!idx) return (size_t)(e - lo);
        const uint32_t i = idx[e];
        bad |= i >= A.B;
        return i < A.B ? i : 0;
    };

    Lane4 acc;
    int pending = 0;
    for (; k + kLcFlight <= end; k += kLcFlight)
    {
        uint4 v[kLcFlight];
        uint32_t wq[kLcFlight];
#pragma unroll
        for (int u = 0; u < kLcFlight; u++)
        {
            v[u] = load_row(in, record_of(k + u), row, off);
            if constexpr (!UNIT) wq[u] = reduce_signed((int64_t)wt[k + u], q, cr_hi, cr_lo);
        }
#pragma unroll
        for (int u = 0; u < kLcFlight; u++)
        {
            if constexpr (UNIT)
                acc.add(v[u]);
            else
                acc.mad(v[u], wq[u]);
        }
        if constexpr (!UNIT)
        {
            pending += kLcFlight;
            if (pending == kLcPeriod)
            {
                acc.reduce(q, cr_hi, cr_lo);
                pending = 0;
            }
        }
    }
    // the last, short group (at most kLcFlight - 1 < kLcPeriod products on a canonical accumulator)
    if constexpr (!UNIT)
        if (pending) acc.reduce(q, cr_hi, cr_lo);
    for (; k < end; k++)
    {
        const uint4 v = load_row(in, record_of(k), row, off);
        if constexpr (UNIT)
            acc.add(v);
        else
            acc.mad(v, reduce_signed((int64_t)wt[k], q, cr_hi, cr_lo));
    }
    acc.reduce(q, cr_hi, cr_lo);

    if (S == 1)
    {
        uint32_t *out = slab ? A.out1 : A.out0;
        *reinterpret_cast<uint4 *>(out + g * row + off) = bad ? make_uint4(0, 0, 0, 0) : acc.get();
        if (A.status && blockIdx.x == 0 && threadIdx.x == 0) A.status[g] = bad ? 2 : 1;
    }
    else
    {
        const size_t p = g * S + s;
        uint32_t *out  = A.part + (size_t)slab * A.G * S * row;
        *reinterpret_cast<uint4 *>(out + p * row + off) = acc.get();
        if (blockIdx.x == 0 && threadIdx.x == 0) A.flag[p] = bad;
    }
}

// out[g] = sum of the S partial rows of g (canonical, so plain adds and one reduction); a flagged slice zeroes the row.
__global__ __launch_bounds__(kLcThreads) void k_ct_lincomb_sum(const DevParams P, const LincombArgs A, uint32_t S)
{
    const size_t row      = (size_t)P.nprimes << P.logn;
    const uint32_t chunks = (uint32_t)(row >> kLcTileLog);
    const uint32_t slab   = blockIdx.x / chunks;
    const uint32_t chunk  = blockIdx.x - slab * chunks;
    const uint32_t j      = (chunk << kLcTileLog) >> P.logn;
    const size_t off      = ((size_t)chunk << kLcTileLog) + 4 * threadIdx.x;
    const size_t g        = A.g0 + blockIdx.z;
    const uint32_t *__restrict__ part = A.part + (size_t)slab * A.G * S * row;
    const uint8_t *__restrict__ flag  = A.flag + g * S;

    bool bad = false;
    for (uint32_t s = 0; s < S; s++) bad |= flag[s] != 0;
    Lane4 acc;
    uint32_t s = 0;
    for (; s + kLcFlight <= S; s += kLcFlight)
    {
        uint4 v[kLcFlight];
#pragma unroll
        for (int u = 0; u < kLcFlight; u++) v[u] = load_row(part, g * S + s + u, row, off);
#pragma unroll
        for (int u = 0; u < kLcFlight; u++) acc.add(v[u]);
    }
    for (; s < S; s++) acc.add(load_row(part, g * S + s, row, off));
    acc.reduce(P.q[j], P.cr_hi[j], P.cr_lo[j]);

    uint32_t *out = slab ? A.out1 : A.out0;
    *reinterpret_cast<uint4 *>(out + g * row + off) = bad ? make_uint4(0, 0, 0, 0) : acc.get();
    if (A.status && blockIdx.x == 0 && threadIdx.x == 0) A.status[g] = bad ? 2 : 1;
}

hipError_t launch_ct_lincomb(const DevParams &P, const LincombArgs &args, uint32_t S, hipStream_t st)
{
    const uint32_t chunks = (uint32_t)(((size_t)P.nprimes << P.logn) >> kLcTileLog);
    const uint32_t slabs  = args.in1 ? 2 : 1;
    LincombArgs A         = args;
    // gridDim.z is limited to 65 535: more output rows take more launches
    for (size_t g0 = 0; g0 < args.G; g0 += 65535)
    {
        const uint32_t rows = (uint32_t)(args.G - g0 < 65535 ? args.G - g0 : 65535);
        A.g0                = g0;
        const dim3 grid(chunks * slabs, S, rows);
        hipError_t e = launch(args.w ? k_ct_lincomb<false> : k_ct_lincomb<true>, grid, dim3(kLcThreads), 0, st, P, A);
        if (e == hipSuccess && S > 1)
            e = launch(k_ct_lincomb_sum, dim3(chunks * slabs, 1, rows), dim3(kLcThreads), 0, st, P, A, S);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------
// Slot-wise product with an encoded plaintext: out[b][j][i] = in[b][j][i] . pt[p(b)][j][i] mod q_j.  Streaming, in the
// shape of k_ct_lincomb: a 256-thread workgroup owns 1024 consecutive residues of a record -- inside one prime, so q_j
// and its Barrett constants are scalar -- and walks the records blockIdx.y, blockIdx.y + gridDim.y, ...; p(b) is
// workgroup-uniform (a scalar load).  One 16-byte load per operand, one 16-byte store; 64-bit row offsets.  Every lane
// reads its own 16 bytes of `in` before it writes the same 16 bytes of `out`, so out == in is allowed (no __restrict__
// on the pair).  The product of two words is below 2^64 whatever the words are, and barrett64 is exact there.
// grid (primes n / 1024 * slabs, min(B, 65 535)).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLcThreads) void k_ct_mul_plain(const DevParams P, const MulPlainArgs A)
{
    const size_t row      = (size_t)A.primes << P.logn;
    const size_t pt_row   = (size_t)A.pt_primes << P.logn;
    const uint32_t chunks = (uint32_t)(row >> kLcTileLog);
    const uint32_t slab   = blockIdx.x / chunks;
    const uint32_t chunk  = blockIdx.x - slab * chunks;
    const uint32_t j      = (chunk << kLcTileLog) >> P.logn;
    const uint32_t q = P.q[j], cr_hi = P.cr_hi[j], cr_lo = P.cr_lo[j];
    const uint32_t *in = slab ? A.in1 : A.in0;
    uint32_t *out      = slab ? A.out1 : A.out0;
    const uint32_t *__restrict__ pt = A.pt;
    const size_t off = ((size_t)chunk << kLcTileLog) + 4 * threadIdx.x;   // the same offset inside a plaintext: j < primes

    for (size_t b = blockIdx.y; b < A.B; b += gridDim.y)
    {
        const uint32_t p = A.pt_idx ? A.pt_idx[b] : (A.P == 1 ? 0u : (uint32_t)b);
        const bool bad   = p >= A.P;   // nothing of such a record's plaintext is read
        uint4 r          = make_uint4(0, 0, 0, 0);
        if (!bad)
        {
            const uint4 a = load_row(in, b, row, off);
            const uint4 m = load_row(pt, p, pt_row, off);
            r.x           = barrett64((uint64_t)a.x * m.x, q, cr_hi, cr_lo);
            r.y           = barrett64((uint64_t)a.y * m.y, q, cr_hi, cr_lo);
            r.z           = barrett64((uint64_t)a.z * m.z, q, cr_hi, cr_lo);
            r.w           = barrett64((uint64_t)a.w * m.w, q, cr_hi, cr_lo);
        }
        *reinterpret_cast<uint4 *>(out + b * row + off) = r;
        if (A.status && blockIdx.x == 0 && threadIdx.x == 0) A.status[b] = bad ? 2 : 1;
    }
}

hipError_t launch_ct_mul_plain(const DevParams &P, const MulPlainArgs &A, hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    const uint32_t chunks = (uint32_t)(((size_t)A.primes << P.logn) >> kLcTileLog);
    const uint32_t slabs  = A.in1 ? 2 : 1;
    const dim3 grid(chunks * slabs, A.B < 65535u ? A.B : 65535u);
    return launch(k_ct_mul_plain, grid, dim3(kLcThreads), 0, st, P, A);
}

// ------------------------------------------------------------------------------------------
// Tensor product of two ciphertexts, the degree-2 form before relinearisation: for pair p with x = record ia[p] of
// (a0, a1) and y = record ib[p] of (b0, b1),  out0 = x0 y0,  out1 = x0 y1 + x1 y0,  out2 = x1 y1  mod q_j, element-wise.
// Streaming, in the shape of k_ct_mul_plain: a 256-thread workgroup owns 1024 consecutive residues of a pair -- inside
// one prime, so q_j and its Barrett constants are scalar -- and walks the pairs blockIdx.y, blockIdx.y + gridDim.y, ...;
// the two record indices are workgroup-uniform (scalar loads).  Four 16-byte loads and three 16-byte stores per lane,
// 64-bit row offsets.  The a and b slabs may be the same memory (squares, all pairs within one batch): they are only
// read, so no __restrict__ on them; the outputs overlap nothing.
// Residues are below q < 2^30, so one product is at most (q - 1)^2 < 2^60 and the two products of out1 sum to less than
// 2^61 < 2^64: ONE barrett64 (exact for every 64-bit input) for the sum.
// grid (primes n / 1024, min(P, 65 535)).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLcThreads) void k_ct_mul(const DevParams P, const MulArgs A)
{
    const size_t row     = (size_t)A.primes << P.logn;
    const uint32_t chunk = blockIdx.x;
    const uint32_t j     = (chunk << kLcTileLog) >> P.logn;
    const uint32_t q = P.q[j], cr_hi = P.cr_hi[j], cr_lo = P.cr_lo[j];
    const size_t off = ((size_t)chunk << kLcTileLog) + 4 * threadIdx.x;

    for (size_t p = blockIdx.y; p < A.P; p += gridDim.y)
    {
        const uint32_t ia = A.ia ? A.ia[p] : (uint32_t)p, ib = A.ib ? A.ib[p] : (uint32_t)p;
        const bool bad    = ia >= A.Ba || ib >= A.Bb;   // nothing of such a pair's records is read
        uint32_t r[3][4]  = {};
        if (!bad)
        {
            const uint4 x0 = load_row(A.a0, ia, row, off), x1 = load_row(A.a1, ia, row, off);
            const uint4 y0 = load_row(A.b0, ib, row, off), y1 = load_row(A.b1, ib, row, off);
            const uint32_t u0[4] = {x0.x, x0.y, x0.z, x0.w}, u1[4] = {x1.x, x1.y, x1.z, x1.w};
            const uint32_t v0[4] = {y0.x, y0.y, y0.z, y0.w}, v1[4] = {y1.x, y1.y, y1.z, y1.w};
#pragma unroll
            for (int e = 0; e < 4; e++)
            {
                r[0][e] = barrett64((uint64_t)u0[e] * v0[e], q, cr_hi, cr_lo);
                r[1][e] = barrett64((uint64_t)u0[e] * v1[e] + (uint64_t)u1[e] * v0[e], q, cr_hi, cr_lo);
                r[2][e] = barrett64((uint64_t)u1[e] * v1[e], q, cr_hi, cr_lo);
            }
        }
        *reinterpret_cast<uint4 *>(A.out0 + p * row + off) = make_uint4(r[0][0], r[0][1], r[0][2], r[0][3]);
        *reinterpret_cast<uint4 *>(A.out1 + p * row + off) = make_uint4(r[1][0], r[1][1], r[1][2], r[1][3]);
        *reinterpret_cast<uint4 *>(A.out2 + p * row + off) = make_uint4(r[2][0], r[2][1], r[2][2], r[2][3]);
        if (A.status && blockIdx.x == 0 && threadIdx.x == 0) A.status[p] = bad ? 2 : 1;
    }
}

hipError_t launch_ct_mul(const DevParams &P, const MulArgs &A, hipStream_t st)
{
    if (A.P == 0) return hipSuccess;
    const uint32_t chunks = (uint32_t)(((size_t)A.primes << P.logn) >> kLcTileLog);
    const dim3 grid(chunks, A.P < 65535u ? A.P : 65535u);
    return launch(k_ct_mul, grid, dim3(kLcThreads), 0, st, P, A);
}

// ------------------------------------------------------------------------------------------
// Grouped product sums (se_amd_ct_mul_sum_device; MulSumArgs): the tensor above summed over the pairs of a CSR row,
//   T0[g] = sum_k x0 y0,   T1[g] = sum_k (x0 y1 + x1 y0),   T2[g] = sum_k x1 y1   mod q_j,
// with the per-pair record (3 slabs per pair) never written.  Streaming, in the shape of k_ct_mul: a 256-thread
// workgroup owns 1024 consecutive residues of an output row -- inside one prime, q_j scalar -- walks the rows
// blockIdx.y, blockIdx.y + gridDim.y, ... and inside a row its pairs; row_ptr and the pair indices are
// workgroup-uniform (scalar loads).  A row is not sliced.
// Lazy accumulation.  Residues are below q < 2^30, so one product is at most (q - 1)^2 <= 2^60 - 2^32 + 4 and the T1
// term of a pair at most 2^61 - 2^33 + 8.  An accumulator enters a period canonical (< 2^30) and takes kMsPeriod = 8
// pairs:  2^30 + 8 (2^61 - 2^33 + 8) < 2^64,  so 8 pairs fit a uint64 before barrett64 (exact for every 64-bit input);
// 9 would not.  T0 and T2 take the same period: one rule for the three sums, here and in k_ct_dot_sp.
// The map is exact modular arithmetic: any order of the pairs and any placing of the reductions gives the bits of
// k_ct_mul followed by the unweighted k_ct_lincomb of each slab.
// grid (primes n / 1024, min(G, 65 535)).
// ------------------------------------------------------------------------------------------
constexpr uint32_t kMsPeriod = 8;   // pairs between two reductions
constexpr uint32_t kMsFlight = 2;   // pairs (8 input rows) in flight per wave
static_assert(kMsPeriod % kMsFlight == 0, "a period is a whole number of load groups");

// The pairs [lo, hi) of output row g and whether the row is invalid, decided before anything of it is read or written:
// the row_ptr pair, then every pair index against its batch.  Nothing but row_ptr[g], row_ptr[g + 1] and ia / ib[k] with
// k < hi <= nnz is read, and no index forms an address here.  Depends on g alone: wave-uniform.  Ba = 0 or Bb = 0 makes
// every non-empty row invalid.  An invalid row has lo = hi.
__device__ __forceinline__ bool mul_sum_row(const MulSumArgs &A, size_t g, uint32_t &lo, uint32_t &hi)
{
    const uint32_t a = A.row_ptr[g], b = A.row_ptr[g + 1];
    bool bad = a > b || b > A.nnz;
    lo       = a;
    hi       = bad ? a : b;
    for (uint32_t k = lo; k < hi; k++) bad |= (A.ia ? A.ia[k] : k) >= A.Ba || (A.ib ? A.ib[k] : k) >= A.Bb;
    if (bad) hi = lo;
    return bad;
}

// the end of the period that starts at pair k < hi (hi - k, not k + kMsPeriod: nnz may be close to 2^32)
__device__ __forceinline__ uint32_t mul_sum_period_end(uint32_t k, uint32_t hi)
{
    return hi - k < kMsPeriod ? hi : k + kMsPeriod;
}

__global__ __launch_bounds__(kLcThreads) void k_ct_mul_sum(const DevParams P, const MulSumArgs A)
{
    const size_t row     = (size_t)A.primes << P.logn;
    const uint32_t chunk = blockIdx.x;
    const uint32_t j     = (chunk << kLcTileLog) >> P.logn;
    const uint32_t q = P.q[j], cr_hi = P.cr_hi[j], cr_lo = P.cr_lo[j];
    const size_t off = ((size_t)chunk << kLcTileLog) + 4 * threadIdx.x;
    auto pair_of = [&](uint32_t k, size_t &ia, size_t &ib) {   // checked by mul_sum_row
        ia = A.ia ? A.ia[k] : k;
        ib = A.ib ? A.ib[k] : k;
    };

    for (size_t g = blockIdx.y; g < A.G; g += gridDim.y)
    {
        uint32_t lo, hi;
        const bool bad = mul_sum_row(A, g, lo, hi);
        Lane4 t0, t1, t2;
        for (uint32_t k = lo; k < hi;)
        {
            const uint32_t end = mul_sum_period_end(k, hi);
            for (; end - k >= kMsFlight; k += kMsFlight)
            {
                uint4 x0[kMsFlight], x1[kMsFlight], y0[kMsFlight], y1[kMsFlight];
#pragma unroll
                for (uint32_t u = 0; u < kMsFlight; u++)
                {
                    size_t ia, ib;
                    pair_of(k + u, ia, ib);
                    x0[u] = load_row(A.a0, ia, row, off), x1[u] = load_row(A.a1, ia, row, off);
                    y0[u] = load_row(A.b0, ib, row, off), y1[u] = load_row(A.b1, ib, row, off);
                }
#pragma unroll
                for (uint32_t u = 0; u < kMsFlight; u++)
                {
                    t0.mad4(x0[u], y0[u]);
                    t1.mad4(x0[u], y1[u]);
                    t1.mad4(x1[u], y0[u]);
                    t2.mad4(x1[u], y1[u]);
                }
            }
            for (; k < end; k++)   // the last, short group of a row
            {
                size_t ia, ib;
                pair_of(k, ia, ib);
                const uint4 x0 = load_row(A.a0, ia, row, off), x1 = load_row(A.a1, ia, row, off);
                const uint4 y0 = load_row(A.b0, ib, row, off), y1 = load_row(A.b1, ib, row, off);
                t0.mad4(x0, y0);
                t1.mad4(x0, y1);
                t1.mad4(x1, y0);
                t2.mad4(x1, y1);
            }
            t0.reduce(q, cr_hi, cr_lo);
            t1.reduce(q, cr_hi, cr_lo);
            t2.reduce(q, cr_hi, cr_lo);
        }
        // an empty or invalid row never entered the loop: the accumulators are zero
        *reinterpret_cast<uint4 *>(A.out0 + g * row + off) = t0.get();
        *reinterpret_cast<uint4 *>(A.out1 + g * row + off) = t1.get();
        *reinterpret_cast<uint4 *>(A.out2 + g * row + off) = t2.get();
        if (A.status && blockIdx.x == 0 && threadIdx.x == 0) A.status[g] = bad ? 2 : 1;
    }
}

hipError_t launch_ct_mul_sum(const DevParams &P, const MulSumArgs &A, hipStream_t st)
{
    if (A.G == 0) return hipSuccess;
    const uint32_t chunks = (uint32_t)(((size_t)A.primes << P.logn) >> kLcTileLog);
    const dim3 grid(chunks, A.G < 65535u ? A.G : 65535u);
    return launch(k_ct_mul_sum, grid, dim3(kLcThreads), 0, st, P, A);
}

// ------------------------------------------------------------------------------------------
// Rescale: level L -> level L - 1, the exact quotient (c - delta) / q_last with delta = c mod q_last centred, i.e.
// c / q_last rounded to nearest (SEAL's rescale_to_next on NTT-form data).  One workgroup of n/16 threads per
// (record, slab), the tiling of the rest of the tree:
//   last row (quad loads, 1 KiB per wave instruction) -> quads_to_tile -> intt_tiles mod q_last -> . n^-1 -> centred
//   lift: 16 signed values per thread, |delta| <= (q_last - 1)/2 < 2^29, kept in registers in tile layout LOGN-4;
//   per lower prime j: delta mod q_j (|delta| < q_j: one conditional add) -> ntt_tiles, which STARTS in tile layout
//   LOGN-4, so nothing is re-dealt between the inverse and the forward transforms -> tile_to_quads -> (c_j - NTT) .
//   q_last^-1 (Shoup pair, RescaleParams) -> canonical -> quad store.
// The input row of prime j is requested before its NTT and lands while it runs.  LDS is the exchange plane alone
// (XformGeom::SLOTS words): the wave-local transposes run inside it (rows of 16 words, n words in all) while no
// exchange is in flight -- every exchange ends in a barrier, and one workgroup barrier after each transpose keeps the
// next transform's first exchange off the rows other waves are still reading.
// The map is plain modular arithmetic on whatever words the slab holds (defined for residues in [0, q_j)); no word is
// used as an address.  grid (B, slabs).
// ------------------------------------------------------------------------------------------
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_rescale(const DevParams P, const DevTables T,
                                                                      const RescaleParams R, const RescaleArgs A)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds       = reinterpret_cast<uint32_t *>(smem);
    const int t         = threadIdx.x;
    const size_t b      = blockIdx.x;
    const uint32_t last = A.primes - 1;
    const uint32_t *in  = (blockIdx.y ? A.in1 : A.in0) + b * A.primes * N;
    uint32_t *out       = (blockIdx.y ? A.out1 : A.out0) + b * last * N;

    int32_t delta[16];
    {
        const uint32_t q = P.q[last];
        uint32_t x[16];
        load_quads(x, in + (size_t)last * N, t);
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
        load_quads(c, in + (size_t)j * N, t);
#pragma unroll
        for (int e = 0; e < 16; e++) x[e] = (uint32_t)delta[e] + ((uint32_t)(delta[e] >> 31) & q);   // [0, q)
        ntt_tiles<LOGN>(x, T.ntt_rw + 2 * xform_table_len(N) * j, q, lds, t);
        tile_to_quads<16>(x, lds, t);
        const uint32_t w = R.inv[j], wp = R.inv_sh[j];
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            const uint32_t u = min(x[e], x[e] - two_q);                          // NTT output [0, 4q) -> [0, 2q)
            x[e]             = csub(mul_shoup_lazy(c[e] + two_q - u, w, wp, q), q);  // c - u + 2q in (0, 3q)
        }
        store_quads(out + (size_t)j * N, x, t);
        __syncthreads();
    }
}

// The division by the special prime of extended records (se_amd_ct_mod_down_sp_device): k_ct_rescale on records of L + 1
// rows whose last row is modulo P = q_drop (A.drop = np - 1) instead of q_last; the lower rows, |delta| < P / 2 < q_j and
// the constants R (level np) are the rescale's.  At L = np - 1 the row map is the identity and the bits are the rescale's.
// A sibling with the body written out, not a shared inline: as one, k_ct_rescale<10> and <13> took one more register each
// and <12> seven fewer, and the rows of the rescale are to stay as they are.
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_mod_down_sp(const DevParams P, const DevTables T,
                                                                          const RescaleParams R, const RescaleArgs A)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds       = reinterpret_cast<uint32_t *>(smem);
    const int t         = threadIdx.x;
    const size_t b      = blockIdx.x;
    const uint32_t last = A.primes - 1;
    const uint32_t lp   = A.drop;   // the prime of row `last`
    const uint32_t *in  = (blockIdx.y ? A.in1 : A.in0) + b * A.primes * N;
    uint32_t *out       = (blockIdx.y ? A.out1 : A.out0) + b * last * N;

    int32_t delta[16];
    {
        const uint32_t q = P.q[lp];
        uint32_t x[16];
        load_quads(x, in + (size_t)last * N, t);
        quads_to_tile<16>(x, lds, t);
        __syncthreads();
        intt_tiles<LOGN>(x, T.intt_rw + (size_t)2 * N * lp, q, lds, t);
        const uint32_t inv_n = P.inv_n[lp], inv_n_sh = P.inv_n_sh[lp];
#pragma unroll
        for (int e = 0; e < 16; e++)
            delta[e] = (int32_t)centred_lift(csub(mul_shoup_lazy(x[e], inv_n, inv_n_sh, q), q), q);
    }
    for (uint32_t j = 0; j < last; j++)
    {
        const uint32_t q = P.q[j], two_q = q << 1;
        uint32_t c[16], x[16];
        load_quads(c, in + (size_t)j * N, t);
#pragma unroll
        for (int e = 0; e < 16; e++) x[e] = (uint32_t)delta[e] + ((uint32_t)(delta[e] >> 31) & q);   // [0, q)
        ntt_tiles<LOGN>(x, T.ntt_rw + 2 * xform_table_len(N) * j, q, lds, t);
        tile_to_quads<16>(x, lds, t);
        const uint32_t w = R.inv[j], wp = R.inv_sh[j];
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            const uint32_t u = min(x[e], x[e] - two_q);                          // NTT output [0, 4q) -> [0, 2q)
            x[e]             = csub(mul_shoup_lazy(c[e] + two_q - u, w, wp, q), q);  // c - u + 2q in (0, 3q)
        }
        store_quads(out + (size_t)j * N, x, t);
        __syncthreads();
    }
}

hipError_t launch_ct_rescale(const DevParams &P, const DevTables &T, const RescaleParams &R, const RescaleArgs &A,
                             size_t B, hipStream_t st)
{
    if (B == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        using G         = XformGeom<L>;
        return launch(k_ct_rescale<L>, dim3((unsigned)B, A.in1 ? 2 : 1), dim3(G::THREADS),
                      (size_t)G::SLOTS * sizeof(uint32_t), st, P, T, R, A);
    });
}

// LOGN 12 .. 14 only, by the rule of launch_ct_key_switch_sp.
hipError_t launch_ct_mod_down_sp(const DevParams &P, const DevTables &T, const RescaleParams &R, const RescaleArgs &A,
                                 size_t B, hipStream_t st)
{
    if (B == 0) return hipSuccess;
    if (P.logn < 12) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value < 12 ? 12 : decltype(l)::value;
        using G         = XformGeom<L>;
        return launch(k_ct_mod_down_sp<L>, dim3((unsigned)B, A.in1 ? 2 : 1), dim3(G::THREADS),
                      (size_t)G::SLOTS * sizeof(uint32_t), st, P, T, R, A);
    });
}

// ------------------------------------------------------------------------------------------
// The key switch under an evaluation key, shared by k_ct_relin and k_ct_galois (k_ct_galois_hoist takes the first step
// and has its own second one): for one record and output prime i,
//   acc0[i] = sum_{j < L, t < 2} NTT_i(D_{j,t}) . key0[2j + t][i]  mod q_i   (acc1: key1),
// D_{j,t} = the t-th 15-bit digit of the canonical natural-order coefficients c_j of an input row j.  Built from the
// pieces of k_ct_rescale, one workgroup of n/16 threads per (record, output prime i), in two steps per input prime j:
//   evk_row_coeffs: row j (quad loads) -> quads_to_tile -> intt_tiles mod q_j -> . n^-1 -> canonical c < q_j < 2^30 in
//     tile layout LOGN-4 (the caller may permute the coefficients before the second step: k_ct_galois);
//   evk_digits: per digit t, c & 0x7FFF resp. c >> 15 (below 2^15 < q_i: a residue of every prime as it stands)
//     -> ntt_tiles mod q_i, which STARTS in that layout -> tile_to_quads -> multiply-accumulate against row 2j + t of
//     both key halves (quad loads of the word row and of its Shoup row).
// L INTTs and 2 L NTTs per workgroup, L^2 and 2 L^2 per record, no scratch: the input row is transformed again by every
// output prime.
// Lazy range of the accumulators.  Every prime is below 2^30.  A key word is w < q_i (the key setters refuse others) and
// its companion is floor(w 2^32 / q_i), so mul_shoup_lazy(y, w, .) is in [0, 2 q_i) for ANY 32-bit y -- y is the lazy
// NTT output in [0, 4 q_i).  An accumulator enters a step in [0, 2 q_i) (it starts at 0): the sum is below
// 4 q_i < 2^32, and min(s, s - 2 q_i) brings it back into [0, 2 q_i).  So a 32-bit word per value carries any number of
// terms; the one canonicalisation is in the caller's epilogue, csub(acc) resp. csub(csub(acc) + d) with d < q_i.
// LDS is the exchange plane alone, used as in k_ct_rescale: the wave-local transposes run inside it while no exchange
// is in flight, and one workgroup barrier after each keeps the next transform's first exchange off the rows other
// waves are still reading.  No word of a slab or of the key is used as an address.
// The NTT mod q_i is the same for every j and digit, so with the plain thread index the compiler hoists its per-thread
// root loads and LDS addresses out of both loops and carries them across the inverse transform (n = 16384, 128 VGPRs per
// thread: 276 bytes of private memory).  Each transform takes an opaque copy of the index instead (opaque_index,
// transform.cuh): the caller hands one to evk_row_coeffs, evk_digits takes its own per digit from the plain index.
// ------------------------------------------------------------------------------------------
// k0: column i of key row 0 (a key row is np columns of 2 N words); rw: the NTT roots of prime i.  A: RelinArgs or
// GaloisArgs (key layout: half, np).
template <int LOGN, class Args>
__device__ __forceinline__ void evk_digits(const uint32_t (&x)[16], uint32_t (&acc0)[16], uint32_t (&acc1)[16],
                                           const Args &A, const uint32_t *k0, uint32_t j, const uint32_t *rw,
                                           uint32_t qi, uint32_t *lds, int t)
{
    constexpr int N = XformGeom<LOGN>::N;
    // the two digits take the same code with a shift of 0 resp. 15: not unrolled, one NTT body in the kernel
#pragma unroll 1
    for (uint32_t dg = 0; dg < 2; dg++)
    {
        const int td = opaque_index(t);
        uint32_t y[16];
#pragma unroll
        for (int e = 0; e < 16; e++) y[e] = (x[e] >> (kRelinDigitBits * dg)) & ((1u << kRelinDigitBits) - 1);
        ntt_tiles<LOGN>(y, rw, qi, lds, td);
        tile_to_quads<16>(y, lds, td);
        // key rows 2j + dg of both halves, a quad of words and of Shoup companions at a time
        const uint32_t *key = k0 + (size_t)(2 * j + dg) * A.np * 2 * N + quad_index(td, 0);
        evk_mac<LOGN>(acc0, acc1, y, key, A.half, qi);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// Relinearisation: (d0, d1, d2) of level L -> (out0, out1) of level L with the installed evaluation key,
//   out0[b][i] = d0[b][i] + sum_{j < L, t < 2} NTT_i(D_{j,t}) . evk0[2j + t][i]  mod q_i   (out1: d1 and evk1),
// D_{j,t} = the t-th 15-bit digit of the canonical natural-order coefficients of INTT_j(d2[b][j]) (n^-1 included): the
// key switch above on the rows of d2, and the two addends in the epilogue.
// grid evk_grid(B, L).
// ------------------------------------------------------------------------------------------
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_relin(const DevParams P, const DevTables T,
                                                                    const RelinArgs A)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds      = reinterpret_cast<uint32_t *>(smem);
    const int t        = threadIdx.x;
    const uint32_t i   = blockIdx.y;
    const uint32_t qi  = P.q[i];
    const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * i;
    const uint32_t *k0 = A.key + (size_t)i * 2 * N;

    for (size_t b = blockIdx.x; b < A.B; b += gridDim.x)
    {
        const size_t rec = b * A.primes * N;
        uint32_t acc0[16], acc1[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = acc1[e] = 0;
        for (uint32_t j = 0; j < A.primes; j++)
        {
            uint32_t x[16];
            evk_row_coeffs<LOGN>(x, A.d2 + rec + (size_t)j * N, j, P, T, lds, opaque_index(t));
            evk_digits<LOGN>(x, acc0, acc1, A, k0, j, rw, qi, lds, t);
        }
        const size_t o = rec + (size_t)i * N;
        uint32_t c[16];
        load_quads(c, A.d0 + o, t);
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = csub(csub(acc0[e], qi) + c[e], qi);
        store_quads(A.out0 + o, acc0, t);
        load_quads(c, A.d1 + o, t);
#pragma unroll
        for (int e = 0; e < 16; e++) acc1[e] = csub(csub(acc1[e], qi) + c[e], qi);
        store_quads(A.out1 + o, acc1, t);
    }
}

hipError_t launch_ct_relin(const DevParams &P, const DevTables &T, const RelinArgs &A, hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        using G         = XformGeom<L>;
        return launch(k_ct_relin<L>, evk_grid(A.B, A.primes), dim3(G::THREADS), (size_t)G::SLOTS * sizeof(uint32_t), st,
                      P, T, A);
    });
}

// The device copy of an evaluation key of any number of rows (2 np of a digit key, np - 1 of a special-prime key, both
// halves in one call): every row [np][n] of key words becomes [np][2][n], the words of a column followed by their Shoup
// companions floor(w 2^32 / q_i) (w < q_i was checked on the host).  One thread per word.
__global__ __launch_bounds__(kLcThreads) void k_relin_key_rows(const DevParams P, const uint32_t *__restrict__ in,
                                                            uint32_t *__restrict__ out, size_t words)
{
    const size_t k = (size_t)blockIdx.x * kLcThreads + threadIdx.x;
    if (k >= words) return;
    const size_t col   = k >> P.logn, c = k & (P.n - 1);
    const uint32_t q   = P.q[col % P.nprimes], w = in[k];
    out[((2 * col) << P.logn) + c]     = w;
    out[((2 * col + 1) << P.logn) + c] = (uint32_t)(((uint64_t)w << 32) / q);
}

hipError_t launch_relin_key_rows(const DevParams &P, const uint32_t *in, uint32_t *out, size_t rows, hipStream_t st)
{
    const size_t words = (rows * P.nprimes) << P.logn;
    if (words == 0) return hipSuccess;
    return launch(k_relin_key_rows, dim3((unsigned)(words / kLcThreads)), dim3(kLcThreads), 0, st, P, in, out, words);
}

// ------------------------------------------------------------------------------------------
// Slot rotation / conjugation: the automorphism sigma_g : x -> x^g of the ring (g odd, below 2n) on both slabs of a
// level-L record, and the key switch of sigma(c1) from sigma(s) back to s with the Galois key installed for g:
//   out0[b][i] = sigma(c0)[b][i] + sum_{j < L, t < 2} NTT_i(D_{j,t}) . gk0[2j + t][i]  mod q_i   (out1: no addend, gk1),
// D_{j,t} = the t-th 15-bit digit of the canonical natural-order coefficients of sigma(INTT_j(c1[b][j])).  This is
// k_ct_relin on (sigma(c0), 0, sigma(c1)) -- the same grid, thread shape, transforms, key layout and lazy ranges --
// with sigma folded into the two places where a row is in flight anyway:
//   c1: in the coefficient domain, where sigma sends coefficient k to position k g mod n with the sign (-1)^(k g div n).
//       The INTT leaves thread t with the coefficients k = t + (n/16) e (tile layout LOGN-4); they are scattered to
//       lds[k g mod n] and read back at lds[k], which is the layout the NTT starts in.  A wave's 64 lanes hold
//       consecutive k, so their targets are g apart: g is odd, every 32-lane group of a ds_write_b32 covers the 32 banks
//       once, and the read back is contiguous (tools/lds_conflicts.py: 0 conflict cycles for every element tried).  One
//       LDS round trip and two barriers per input prime, against L INTTs and 2 L NTTs.  The negated coefficient is
//       canonical: 0 stays 0, so the digits are those of the value in [0, q_j).
//   c0: in the NTT domain, where sigma is a pure permutation of a bit-reversed row, sigma(x)[k] = x[src(k)] with
//       src(k) = brev((((2 brev(k) + 1) g mod 2n) - 1) / 2).  The row of output prime i enters only the epilogue: it is
//       staged into the plane with the quad loads (1 KiB per wave instruction), and every thread gathers its 16 words
//       from lds[src(k)], src computed in registers (two v_bfrev, one multiply).  The gather is 2-way (g = 3, 3^5) to
//       4-way (3^-1, n + 1, 2n - 1) bank-conflicted, 2 to 6 extra cycles on each of 16 ds_read_b32 per record and output
//       prime (tools/lds_conflicts.py) -- beside 3 L transforms.  A dword gather of the row from global memory would
//       touch 64 cache lines per wave instruction.
// LDS stays the exchange plane alone (n <= XformGeom::SLOTS words for either use).  The only addresses formed from data
// are formed from g, a launch argument the host has checked (odd, below 2n): every target is masked to [0, n), and no
// word of a slab or of the key is used as an address.
// grid evk_grid(B, L).
// ------------------------------------------------------------------------------------------
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_galois(const DevParams P, const DevTables T,
                                                                     const GaloisArgs A)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds      = reinterpret_cast<uint32_t *>(smem);
    const int t        = threadIdx.x;
    const uint32_t i   = blockIdx.y;
    const uint32_t qi  = P.q[i];
    const uint32_t g   = A.elt;
    const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * i;
    const uint32_t *k0 = A.key + (size_t)i * 2 * N;

    for (size_t b = blockIdx.x; b < A.B; b += gridDim.x)
    {
        const size_t rec = b * A.primes * N;
        uint32_t acc0[16], acc1[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = acc1[e] = 0;
        for (uint32_t j = 0; j < A.primes; j++)
        {
            const int tj      = opaque_index(t);
            const uint32_t qj = P.q[j];
            uint32_t x[16];
            evk_row_coeffs<LOGN>(x, A.c1 + rec + (size_t)j * N, j, P, T, lds, tj);
            // sigma: coefficient k -> position k g mod n, negated when k g mod 2n >= n (k g < 2^29); 0 stays 0.  This
            // and sp_row_digit keep a copy each: as one inlined helper the scatter costs both kernels 24 - 28 instructions
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
            evk_digits<LOGN>(x, acc0, acc1, A, k0, j, rw, qi, lds, t);
        }
        const int te   = opaque_index(t);
        const size_t o = rec + (size_t)i * N;
        const int k4   = quad_index(te, 0);
        uint32_t c[16];
        load_quads(c, A.c0 + o, te);
        park_row_quads(c, lds, k4);   // sigma(c0) row i
        __syncthreads();
        gather_row<LOGN>(c, lds, k4, g);
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            acc0[e] = csub(csub(acc0[e], qi) + c[e], qi);
            acc1[e] = csub(acc1[e], qi);
        }
        store_quads(A.out0 + o, acc0, te);
        store_quads(A.out1 + o, acc1, te);
        __syncthreads();   // the next record's first transpose writes the plane the gather reads
    }
}

hipError_t launch_ct_galois(const DevParams &P, const DevTables &T, const GaloisArgs &A, hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        using G         = XformGeom<L>;
        return launch(k_ct_galois<L>, evk_grid(A.B, A.primes), dim3(G::THREADS), (size_t)G::SLOTS * sizeof(uint32_t), st,
                      P, T, A);
    });
}

// ------------------------------------------------------------------------------------------
// Special-prime (hybrid) key switch: se_amd_ct_relin_sp_device and se_amd_ct_galois_sp_device.  The digit key switch above
// adds sum_r D_r e_r with 15-bit digits D_r: about 2.5e7 per coefficient at 4096 x 3, the size of a fresh message.  Here
// the last prime of the CONTEXT, P = q_p with p = np - 1, is reserved for the key: a level-L record (L <= np - 1) is
// switched over the L + 1 primes E = {0 .. L-1, p} with ONE digit per data prime, the whole centred coefficient
//   D_j = centred(INTT_j(d[j]), q_j),   |D_j| < q_j / 2,
// under a key whose diagonal carries the factor P, and the result is divided by P, rounded, as k_ct_rescale divides by the
// last prime: the term sum_j D_j e_j (about 2^29 n^(1/2) sigma) is divided by P ~ 2^30 on the way out.
//   acc_k[i] = sum_{j < L} NTT_i(D_j mod q_i) . key_k[j][i]           i in E   (for i = j the factor is d[j] itself)
//   delta_k  = centred(INTT_p(acc_k[p]), P)
//   ks_k[i]  = (acc_k[i] - NTT_i(delta_k mod q_i)) . P^-1   mod q_i   i < L    (RescaleParams of level np)
// Relinearisation: d = d2, out_k = d_k + ks_k.  Rotation: d = sigma(c1), out0 = sigma(c0) + ks_0, out1 = ks_1.
// The geometry of k_ct_relin: one workgroup of n/16 threads per (record, output prime i < L), LDS the exchange plane
// alone, no scratch, no global temporary.  A workgroup makes two passes over the input rows with the same code
// (sp_row_digit, evk_mac), first modulo P against key column p, then modulo q_i against key column i:
//   pass 0, per j: evk_row_coeffs (the INTT mod q_j of the digit kernels) [-> sigma, the LDS scatter of k_ct_galois] ->
//     centre and reduce mod P (one conditional add: |D_j| < q_j / 2 < every prime of the chain) -> ntt_tiles mod P ->
//     tile_to_quads -> multiply-accumulate against row j, column p of both key halves;
//   between the passes, per half: quads_to_tile -> intt_tiles mod P -> . n^-1 -> centred delta reduced mod q_i (|delta| <
//     P / 2 < q_i: one conditional add) -> ntt_tiles mod q_i -> tile_to_quads -> the accumulator of pass 1 starts at
//     2 q_i - NTT(delta), lazy in (0, 2 q_i];
//   pass 1, per j != i: the coefficients AGAIN -> reduce mod q_i -> ntt_tiles mod q_i -> multiply-accumulate against
//     column i; row i enters as it lies in memory (rotation: load_row_sigma, as sigma(c0) does);
//   epilogue: . P^-1 (Shoup pair), + d_k resp. sigma(c0), canonical.
// 2 L - 1 INTTs and 2 L - 1 NTTs of rows, and 2 + 2 for the two deltas: 4 L + 2 transforms per workgroup against 3 L of
// the digit kernels.  Keeping the L centred rows of pass 0 instead would save L - 1 INTTs and cost 16 (L - 1) registers
// per thread or a global temporary; the live set here is two accumulator tiles and one row, below that of evk_digits
// (two accumulators, the coefficients AND a digit).
// Lazy ranges: those of evk_mac (above evk_row_coeffs), with an accumulator entering in [0, 2 q] instead of [0, 2 q):
// plus one product it is still below 4 q < 2^32.  The accumulators of pass 0 enter intt_tiles in [0, 2 P), which is its
// input range.
// Addresses: as in k_ct_galois (formed from the checked element only, masked to [0, n)).
// Key block [2][R'][np][2][n], R' = np - 1 rows (one per data prime) of the context's np columns, Shoup companions behind
// every column (k_relin_key_rows): row j, column c of half h at key + h half + (j np + c) 2 n.
// grid evk_grid(B, L).
// ------------------------------------------------------------------------------------------
template <int LOGN, bool GALOIS>
__device__ __forceinline__ void ct_key_switch_sp(const DevParams &P, const DevTables &T, const RescaleParams &R,
                                                 const KeySwitchSpArgs &A, uint32_t *lds)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    const int t        = threadIdx.x;
    const uint32_t i   = blockIdx.y;
    const uint32_t sp  = A.np - 1;
    const uint32_t qi  = P.q[i];
    const uint32_t g   = A.elt;

    for (size_t b = blockIdx.x; b < A.B; b += gridDim.x)
    {
        const size_t rec = b * A.primes * N;
        uint32_t acc0[16], acc1[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = acc1[e] = 0;
        // pass 0: modulo P against key column p; pass 1: modulo q_i against key column i.  One body for both.
#pragma unroll 1
        for (uint32_t pass = 0; pass < 2; pass++)
        {
            const uint32_t col = pass ? i : sp;
            const uint32_t q   = P.q[col];
            const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * col;
            for (uint32_t j = 0; j < A.primes; j++)
            {
                uint32_t y[16];
                if (pass && j == i)
                    load_row_sigma<LOGN, GALOIS>(y, A.sw + rec + (size_t)i * N, g, lds, opaque_index(t));
                else
                    sp_row_digit<LOGN, GALOIS>(y, A.sw + rec + (size_t)j * N, j, g, q, rw, P, T, lds, t);
                const uint32_t *key = A.key + ((size_t)j * A.np + col) * 2 * N + quad_index(opaque_index(t), 0);
                evk_mac<LOGN>(acc0, acc1, y, key, A.half, q);
                __syncthreads();
            }
            if (pass == 0) sp_delta<LOGN>(acc0, acc1, i, sp, P, T, lds, t);
        }
        // ks_k = acc_k . P^-1, then the addends
        const int te   = opaque_index(t);
        const size_t o = rec + (size_t)i * N;
        const uint32_t w = R.inv[i], wp = R.inv_sh[i];
        uint32_t c[16];
        load_row_sigma<LOGN, GALOIS>(c, A.a0 + o, g, lds, te);
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = csub(csub(mul_shoup_lazy(acc0[e], w, wp, qi), qi) + c[e], qi);
        store_quads(A.out0 + o, acc0, te);
        if constexpr (GALOIS)
        {
#pragma unroll
            for (int e = 0; e < 16; e++) acc1[e] = csub(mul_shoup_lazy(acc1[e], w, wp, qi), qi);
        }
        else
        {
            load_quads(c, A.a1 + o, te);
#pragma unroll
            for (int e = 0; e < 16; e++) acc1[e] = csub(csub(mul_shoup_lazy(acc1[e], w, wp, qi), qi) + c[e], qi);
        }
        store_quads(A.out1 + o, acc1, te);
        __syncthreads();   // the next record's first transpose writes the plane the gather reads
    }
}

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_relin_sp(const DevParams P, const DevTables T,
                                                                       const RescaleParams R, const KeySwitchSpArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ct_key_switch_sp<LOGN, false>(P, T, R, A, reinterpret_cast<uint32_t *>(smem));
}

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_galois_sp(const DevParams P, const DevTables T,
                                                                        const RescaleParams R, const KeySwitchSpArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ct_key_switch_sp<LOGN, true>(P, T, R, A, reinterpret_cast<uint32_t *>(smem));
}

// elt 0: the relinearisation; else the rotation by that element.  Contexts with a special prime have np >= 2, which
// the default chains give from n = 4096 on: the kernels exist for LOGN 12 .. 14 only, a smaller degree is an error (the
// host refuses np = 1 before it gets here) and the two unreachable cases of the dispatch name the LOGN = 12 kernels.
hipError_t launch_ct_key_switch_sp(const DevParams &P, const DevTables &T, const RescaleParams &R,
                                   const KeySwitchSpArgs &A, hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    if (P.logn < 12) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value < 12 ? 12 : decltype(l)::value;
        using G         = XformGeom<L>;
        const dim3 grid    = evk_grid(A.B, A.primes);
        const size_t plane = (size_t)G::SLOTS * sizeof(uint32_t);
        return A.elt ? launch(k_ct_galois_sp<L>, grid, dim3(G::THREADS), plane, st, P, T, R, A)
                     : launch(k_ct_relin_sp<L>, grid, dim3(G::THREADS), plane, st, P, T, R, A);
    });
}

// ------------------------------------------------------------------------------------------
// Switch-key ring: se_amd_ct_switch_keyed_sp_device and se_amd_ct_switch_sum_keyed_sp_device (SwitchSpArgs).  A ring
// key hides P . s_from_k under s_to, so the special-prime key switch of c1[b] under ring key key_idx[b], plus c0[b],
// is record b under s_to.  The sum form brings the records of a CSR row under s_to AND adds them, with the family's
// newest motif: the undivided terms of the whole row are accumulated and divided by P once.
// One body, ct_switch_sp, from the pieces of ct_key_switch_sp (sp_row_digit<LOGN, false>, evk_mac, sp_delta,
// load_quads / store_quads) and in its geometry: one workgroup of n/16 threads per (output row, output prime i < L),
// LDS the exchange plane alone, no scratch, no global temporary.  The single switch is the row {g} without the row tables.
//   row:    the entries [lo, hi) and their validity, decided before anything of the row is written: every record index
//           is compared with B and only then used to read key_idx, every key index is compared with K and only then
//           used to form the key pointer ring + key_idx[b] . stride.  All of these depend on blockIdx and the loop
//           counters alone: they are wave-uniform.  An invalid row (status 2) and an empty one (status 1) are all zero.
//   pass 0: per record of the row and input row j: sp_row_digit mod P -> evk_mac against row j, column p of THAT
//           record's key;   then sp_delta once for the row;
//   pass 1: the records again against column i (row i of a record enters as it lies in memory);
//   epilogue: . P^-1; out1 is finished and stored first, then the rows c0[b][i] of the records are added into the
//           divided acc0 one at a time -- exact, canonical after every step, and no third accumulator tile.
// Transforms per workgroup for a row of m records: (2 L - 1) m INTTs and as many NTTs, and 4 for the two deltas:
// (4 L - 2) m + 4, against (4 L + 2) m for m single switches and a sum; the switched records never touch memory.
// Lazy ranges: evk_mac's range argument (above evk_row_coeffs) does not depend on the number of terms -- a 32-bit word per
// value carries any number of them -- so it covers a row of any length; pass 1 enters in (0, 2 q_i] as in
// ct_key_switch_sp.  A row of one record runs the operations of k_ct_relin_sp on (c0, 0, c1) in their order: the same
// bits.  A long row is not sliced: a whole-batch sum into one row runs on L workgroups (sum in groups, then
// se_amd_ct_lincomb_device over the group sums).
// grid evk_grid(rows, L).
// ------------------------------------------------------------------------------------------
template <int LOGN, bool SUM>
__device__ __forceinline__ void ct_switch_sp(const DevParams &P, const DevTables &T, const RescaleParams &R,
                                             const SwitchSpArgs &A, uint32_t *lds)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    const int t        = threadIdx.x;
    const uint32_t i   = blockIdx.y;
    const uint32_t sp  = A.np - 1;
    const uint32_t qi  = P.q[i];
    const size_t words = (size_t)A.primes * N;   // of a record
    const uint32_t *__restrict__ idx  = A.idx;
    const uint32_t *__restrict__ kidx = A.key_idx;
    auto record_of = [&](uint32_t e) -> uint32_t {
        if constexpr (SUM)
            return idx[e];
        else
            return e;
    };

    for (size_t g = blockIdx.x; g < A.rows; g += gridDim.x)
    {
        uint32_t lo, hi;
        bool bad = false;
        if constexpr (SUM)
        {
            const uint32_t a = A.row_ptr[g], b = A.row_ptr[g + 1];
            bad = a > b || b > A.nnz;
            lo  = a;
            hi  = bad ? a : b;
        }
        else
        {
            lo = (uint32_t)g;
            hi = lo + 1;
        }
        for (uint32_t e = lo; e < hi && !bad; e++)
        {
            const uint32_t b = record_of(e);
            bad              = b >= A.B || kidx[b] >= A.K;   // key_idx is read for a record that exists only
        }
        const int te   = opaque_index(t);
        const size_t o = g * words + (size_t)i * N;
        uint32_t acc0[16], acc1[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = acc1[e] = 0;
        if (bad || lo == hi)
        {
            store_quads(A.out0 + o, acc0, te);
            store_quads(A.out1 + o, acc1, te);
            if (A.status && i == 0 && t == 0) A.status[g] = bad ? 2 : 1;
            continue;
        }
        // pass 0: modulo P against key column p; pass 1: modulo q_i against key column i.  One body for both.
#pragma unroll 1
        for (uint32_t pass = 0; pass < 2; pass++)
        {
            const uint32_t col = pass ? i : sp;
            const uint32_t q   = P.q[col];
            const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * col;
            for (uint32_t e = lo; e < hi; e++)
            {
                const uint32_t b   = record_of(e);
                const uint32_t *sw = A.c1 + b * words;
                const uint32_t *kc = A.ring + kidx[b] * A.stride + (size_t)col * 2 * N;   // column col of key row 0
                for (uint32_t j = 0; j < A.primes; j++)
                {
                    uint32_t y[16];
                    if (pass && j == i)
                        load_quads(y, sw + (size_t)i * N, opaque_index(t));
                    else
                        sp_row_digit<LOGN, false>(y, sw + (size_t)j * N, j, 0, q, rw, P, T, lds, t);
                    const uint32_t *key = kc + (size_t)j * A.np * 2 * N + quad_index(opaque_index(t), 0);
                    evk_mac<LOGN>(acc0, acc1, y, key, A.half, q);
                    __syncthreads();
                }
            }
            if (pass == 0) sp_delta<LOGN>(acc0, acc1, i, sp, P, T, lds, t);
        }
        // ks_k = acc_k . P^-1; out1 leaves first, then the c0 rows join the divided acc0
        const uint32_t w = R.inv[i], wp = R.inv_sh[i];
#pragma unroll
        for (int e = 0; e < 16; e++) acc1[e] = csub(mul_shoup_lazy(acc1[e], w, wp, qi), qi);
        store_quads(A.out1 + o, acc1, te);
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = csub(mul_shoup_lazy(acc0[e], w, wp, qi), qi);
        for (uint32_t e = lo; e < hi; e++)
        {
            uint32_t c[16];
            load_quads(c, A.c0 + record_of(e) * words + (size_t)i * N, te);
#pragma unroll
            for (int k = 0; k < 16; k++) acc0[k] = csub(acc0[k] + c[k], qi);
        }
        store_quads(A.out0 + o, acc0, te);
        if (A.status && i == 0 && t == 0) A.status[g] = 1;
    }
}

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_switch_sp(const DevParams P, const DevTables T,
                                                                        const RescaleParams R, const SwitchSpArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ct_switch_sp<LOGN, false>(P, T, R, A, reinterpret_cast<uint32_t *>(smem));
}

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_switch_sum_sp(const DevParams P, const DevTables T,
                                                                            const RescaleParams R, const SwitchSpArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ct_switch_sp<LOGN, true>(P, T, R, A, reinterpret_cast<uint32_t *>(smem));
}

// row_ptr set: the sum form.  LOGN 12 .. 14, as launch_ct_key_switch_sp.
hipError_t launch_ct_switch_sp(const DevParams &P, const DevTables &T, const RescaleParams &R, const SwitchSpArgs &A,
                               hipStream_t st)
{
    if (A.rows == 0) return hipSuccess;
    if (P.logn < 12) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value < 12 ? 12 : decltype(l)::value;
        using G         = XformGeom<L>;
        const dim3 grid    = evk_grid(A.rows, A.primes);
        const size_t plane = (size_t)G::SLOTS * sizeof(uint32_t);
        return A.row_ptr ? launch(k_ct_switch_sum_sp<L>, grid, dim3(G::THREADS), plane, st, P, T, R, A)
                         : launch(k_ct_switch_sp<L>, grid, dim3(G::THREADS), plane, st, P, T, R, A);
    });
}

// ------------------------------------------------------------------------------------------
// Encrypted inner products: se_amd_ct_dot_sp_device (MulSumArgs).  Relinearisation is linear in d2, so the products of a
// CSR row are summed as tensors (T0, T1, T2 of k_ct_mul_sum) and T2 of the ROW is key-switched once:
//   out_k[g] = T_k[g] + ks_k(T2[g]),   ks as in ct_key_switch_sp (centred digits, one division by P).
// The body of ct_key_switch_sp<LOGN, false> in its geometry -- one workgroup of n/16 threads per (output row, output
// prime i < L), LDS the exchange plane alone, no scratch, no global temporary -- with every row it would load formed in
// registers instead, in the quad layout load_quads gives (dot_rows), so the tensor sums never touch memory:
//   row:    validity first (mul_sum_row): the row_ptr pair, then every ia[k] < Ba and ib[k] < Bb, before an index forms
//           an address; blockIdx and loop counters only: wave-uniform.  Invalid (status 2) and empty (status 1) rows are
//           all zero.
//   pass 0: per j < L: row j of T2 = sum_k a1[ia[k]][j] . b1[ib[k]][j], a quad at a time (two quad loads per pair, the
//           lazy rule of k_ct_mul_sum), canonical -> sp_quads_digit mod P -> evk_mac against row j, column p;
//           then sp_delta once;
//   pass 1: the same for j != i against column i; row i of T2 enters as it was summed, with no transform;
//   epilogue: . P^-1, canonical; T1[i] is formed (four quad loads per pair) and added into the divided acc1, which is
//           stored; then T0[i] (two) into the divided acc0.  Exact and canonical at every step; no third accumulator.
// Every value that meets evk_mac, sp_delta and the epilogue is the one k_ct_relin_sp reads from the slabs k_ct_mul_sum
// wrote, and the operations on it are the same in the same order: the same bits, for a row of any length; a row of one
// pair has those of k_ct_mul and k_ct_relin_sp.  A row of m >= 2 pairs is NOT the sum of m relinearised products: one
// rounding centred(INTT_p(acc[p]), P) instead of m.
// Transforms per workgroup: 4 L + 2 whatever m is (against (4 L + 2) m).  Input rows read per workgroup: 2 m for each of
// the 2 L rows of T2 it forms and 6 m in the epilogue, (4 L + 6) m, where k_ct_mul_sum (its share: 4 m) and k_ct_relin_sp
// (2 L + 2) read 4 m + 2 L + 2: the price of no intermediate, and it grows with m L.
// Live set: two accumulator tiles, the row being formed (16) and ONE quad in flight (a 64-bit accumulator quad and the
// pair's input quads), as evk_mac works the key a quad at a time.
// A long row is not sliced: it runs on L workgroups (sum in groups, then se_amd_ct_lincomb_device over the group sums).
// grid evk_grid(G, L).
// ------------------------------------------------------------------------------------------
// r = quad c of row `off / N` of T_TERM summed over the pairs [lo, hi), canonical.  off = j N + quad_index(t, c).
template <int TERM>
__device__ __forceinline__ void dot_quad(uint32_t (&r)[4], const MulSumArgs &A, uint32_t lo, uint32_t hi, size_t words,
                                         size_t off, uint32_t q, uint32_t cr_hi, uint32_t cr_lo)
{
    auto quad = [&](const uint32_t *slab, size_t rec) { return *reinterpret_cast<const uint4 *>(slab + rec * words + off); };
    Lane4 acc;
    for (uint32_t k = lo; k < hi;)
    {
        const uint32_t end = mul_sum_period_end(k, hi);
        for (; k < end; k++)
        {
            const size_t ia = A.ia ? A.ia[k] : k, ib = A.ib ? A.ib[k] : k;   // checked by mul_sum_row
            if constexpr (TERM == 0) acc.mad4(quad(A.a0, ia), quad(A.b0, ib));
            if constexpr (TERM == 1)
            {
                acc.mad4(quad(A.a0, ia), quad(A.b1, ib));
                acc.mad4(quad(A.a1, ia), quad(A.b0, ib));
            }
            if constexpr (TERM == 2) acc.mad4(quad(A.a1, ia), quad(A.b1, ib));
        }
        acc.reduce(q, cr_hi, cr_lo);
    }
    const uint4 v = acc.get();
    r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
}

// x = row j of T_TERM in quad layout (TERM 2), or x += that row mod q_j, canonical (TERM 0, 1: the epilogue's addends)
template <int TERM>
__device__ __forceinline__ void dot_rows(uint32_t (&x)[16], const MulSumArgs &A, uint32_t lo, uint32_t hi, size_t words,
                                         size_t row_off, uint32_t j, const DevParams &P, int tq)
{
    const uint32_t q = P.q[j], cr_hi = P.cr_hi[j], cr_lo = P.cr_lo[j];
#pragma unroll
    for (int c = 0; c < 4; c++)
    {
        uint32_t r[4];
        dot_quad<TERM>(r, A, lo, hi, words, row_off + quad_index(tq, c), q, cr_hi, cr_lo);
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            if constexpr (TERM == 2)
                x[4 * c + k] = r[k];
            else
                x[4 * c + k] = csub(x[4 * c + k] + r[k], q);
        }
    }
}

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_dot_sp(const DevParams P, const DevTables T,
                                                                     const RescaleParams R, const MulSumArgs A)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds      = reinterpret_cast<uint32_t *>(smem);
    const int t        = threadIdx.x;
    const uint32_t i   = blockIdx.y;
    const uint32_t sp  = A.np - 1;
    const uint32_t qi  = P.q[i];
    const size_t words = (size_t)A.primes * N;   // of a record

    for (size_t g = blockIdx.x; g < A.G; g += gridDim.x)
    {
        uint32_t lo, hi;
        const bool bad = mul_sum_row(A, g, lo, hi);
        const int te   = opaque_index(t);
        const size_t o = g * words + (size_t)i * N;
        uint32_t acc0[16], acc1[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = acc1[e] = 0;
        if (lo == hi)   // empty, or invalid
        {
            store_quads(A.out0 + o, acc0, te);
            store_quads(A.out1 + o, acc1, te);
            if (A.status && i == 0 && t == 0) A.status[g] = bad ? 2 : 1;
            continue;
        }
        // pass 0: modulo P against key column p; pass 1: modulo q_i against key column i.  One body for both.
#pragma unroll 1
        for (uint32_t pass = 0; pass < 2; pass++)
        {
            const uint32_t col = pass ? i : sp;
            const uint32_t q   = P.q[col];
            const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * col;
            for (uint32_t j = 0; j < A.primes; j++)
            {
                uint32_t y[16];
                const int tj = opaque_index(t);
                dot_rows<2>(y, A, lo, hi, words, (size_t)j * N, j, P, tj);
                if (!(pass && j == i)) sp_quads_digit<LOGN, false>(y, j, 0, q, rw, P, T, lds, t, tj);
                const uint32_t *key = A.key + ((size_t)j * A.np + col) * 2 * N + quad_index(opaque_index(t), 0);
                evk_mac<LOGN>(acc0, acc1, y, key, A.half, q);
                __syncthreads();
            }
            if (pass == 0) sp_delta<LOGN>(acc0, acc1, i, sp, P, T, lds, t);
        }
        // ks_k = acc_k . P^-1; T1[i] joins the divided acc1, which leaves first, then T0[i] the divided acc0
        const uint32_t w = R.inv[i], wp = R.inv_sh[i];
#pragma unroll
        for (int e = 0; e < 16; e++) acc1[e] = csub(mul_shoup_lazy(acc1[e], w, wp, qi), qi);
        dot_rows<1>(acc1, A, lo, hi, words, (size_t)i * N, i, P, te);
        store_quads(A.out1 + o, acc1, te);
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = csub(mul_shoup_lazy(acc0[e], w, wp, qi), qi);
        dot_rows<0>(acc0, A, lo, hi, words, (size_t)i * N, i, P, te);
        store_quads(A.out0 + o, acc0, te);
        if (A.status && i == 0 && t == 0) A.status[g] = 1;
    }
}

// LOGN 12 .. 14, as launch_ct_key_switch_sp.
hipError_t launch_ct_dot_sp(const DevParams &P, const DevTables &T, const RescaleParams &R, const MulSumArgs &A,
                            hipStream_t st)
{
    if (A.G == 0) return hipSuccess;
    if (P.logn < 12) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value < 12 ? 12 : decltype(l)::value;
        using G         = XformGeom<L>;
        return launch(k_ct_dot_sp<L>, evk_grid(A.G, A.primes), dim3(G::THREADS), (size_t)G::SLOTS * sizeof(uint32_t), st,
                      P, T, R, A);
    });
}

// ------------------------------------------------------------------------------------------
// Hoisted rotations: G rotations of a record from ONE digit decomposition of c1 (se_amd_ct_galois_many_device,
// se_amd_ct_galois_sum_device).  k_ct_galois decomposes sigma(c1), so every element pays the L INTTs and 2 L NTTs of its
// key switch again.  Here the digits D_{j,t} are those of c1 itself and sigma is applied to the TRANSFORMED digit, where
// it is the permutation src_g of a bit-reversed row (galois_src above):
//   rot0[g][b][i][k] = c0[b][i][src_g(k)] + sum_{j < L, t < 2} NTT_i(D_{j,t})[src_g(k)] . gk0_g[2j + t][i][k]  mod q_i,
//   rot1[g][b][i][k] =                      sum_{j < L, t < 2} NTT_i(D_{j,t})[src_g(k)] . gk1_g[2j + t][i][k]  mod q_i.
// sum_t 2^(15 t) sigma(D_{j,t}) = sigma(c1_j) mod q_j and sigma(D) has coefficients of magnitude below 2^15, so this is
// a key switch under the SAME Galois keys; it is not bit-identical to k_ct_galois (a negated coefficient q - c has other
// digits than c).  The third caller of evk_row_coeffs: the same grid, thread shape, roots, key layout and lazy
// accumulator range as its two siblings (mul_shoup_lazy takes any 32-bit y: the argument above holds word for word).
// Per input prime j: evk_row_coeffs once; per digit: ntt_tiles mod q_i, which ends in tile layout 0 -- thread t holds the
// words 16 t .. 16 t + 15, lazy in [0, 4 q_i) -- with the plane free, so the thread parks them as they are, word k at
// lds[k] (4 ds_write_b128; no tile_to_quads: the gather below re-deals).  One barrier; then, per element of the group,
// every thread gathers the 16 words of its quads from lds[src_g(k)] and multiply-accumulates them against rows 2j + t of
// both halves of that element's key block; one barrier before the next transform.  An element costs a gather and a
// multiply-accumulate per digit; the transforms are shared.
//   SUM: ONE accumulator pair serves all G elements (an element listed twice counts twice); the c0 row is staged once
//     and gathered G times; with add_input the record itself (the rotation by 0, which needs no key) joins the sum.
//     Transforms per record are those of a single rotation whatever G is.
//   many: one accumulator pair (32 VGPRs) per element in flight, so the elements are taken in groups of kHoistGroup per
//     pass over the digits: ceil(G / kHoistGroup) times the transforms of one rotation.  The last group may be short.
// src_g(k) in registers: brev is additive over disjoint bit fields, so with r4 = brev(k4) of the thread's first quad and
// the compile-time offset d of a word in the quads, (2 brev(k4 + d) + 1) g = (2 r4 + 1) g + 2 brev(d) g: one per-thread
// product per element, a scalar product per word, then v_add, v_bfrev and the shift / mask to the LDS address.
// Addresses: as in k_ct_galois, per element.  The elements and their key blocks are read from the argument block with a
// workgroup-uniform index (scalar loads).
// grid evk_grid(B, L).
// ------------------------------------------------------------------------------------------
constexpr int kHoistGroup = 2;   // elements in flight of the many form: the largest without scratch at every degree
// n = 16384 is one workgroup of 16 waves, 4 per SIMD: 128 VGPRs at most, and two accumulator pairs beside the
// coefficients of the input row and a transform in flight are 9 more than that.  There the many form parks the
// coefficients in a second plane of n words behind the exchange plane while a digit is transformed: every thread reads
// back the slots it wrote itself (lane-consecutive, no conflict, no barrier).  One workgroup per CU either way.
template <int LOGN, bool SUM>
constexpr bool kHoistPark = LOGN == 14 && !SUM;

// the 16 words of the thread's quads of sigma_g(row), row parked in the plane with word k at plane[k]; word 4 c + k of
// the thread is k4 + (c << 8) + k.  u0 = (2 brev(k4) + 1) g < 2^30, the offsets add less than 2^30.
template <int LOGN>
__device__ __forceinline__ uint32_t hoist_word(const uint32_t *plane, uint32_t u0, uint32_t g, int c, int k)
{
    const uint32_t rd = __brev((uint32_t)((c << 8) + k)) >> (32 - LOGN);
    return plane[galois_src_of<LOGN>(u0 + 2 * rd * g)];
}

// One element's share of one digit: acc += sigma_g(NTT_i(D))[k] . key[k] on both halves (evk_mac on gathered words);
// `key` = the thread's first quad of row 2j + t, column i of the element's block.
template <int LOGN>
__device__ __forceinline__ void hoist_mac(uint32_t (&acc0)[16], uint32_t (&acc1)[16], const uint32_t *plane,
                                          const uint32_t *key, size_t half, uint32_t g, uint32_t r4, uint32_t qi)
{
    evk_mac<LOGN>(acc0, acc1, key, half, qi,
                  [=](int c, int k) { return hoist_word<LOGN>(plane, (2 * r4 + 1) * g, g, c, k); });
}

// The digit loop of a pass: for every input prime the coefficients of the c1 row, per digit its transform mod q_i parked
// in the plane, and the share of every element of the pass (hoist_mac).  SUM: acc[0] serves all A.G elements; else
// acc[u] is element e0 + u.  Args = GaloisHoistArgs, or LintransArgs (SUM, on folded key blocks).  Ends behind a barrier
// with the plane free.
template <int LOGN, bool SUM, int GC, class Args>
__device__ __forceinline__ void hoist_digits(uint32_t (&acc0)[GC][16], uint32_t (&acc1)[GC][16], const Args &A,
                                             size_t rec, uint32_t e0, uint32_t i, uint32_t qi, const uint32_t *rw,
                                             uint32_t r4, const DevParams &P, const DevTables &T, uint32_t *lds, int t)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    for (uint32_t j = 0; j < A.primes; j++)
    {
        uint32_t x[16];
        evk_row_coeffs<LOGN>(x, A.c1 + rec + (size_t)j * N, j, P, T, lds, opaque_index(t));
        if constexpr (kHoistPark<LOGN, SUM>)
        {
            uint32_t *park = lds + G::SLOTS + opaque_index(t);   // one base register, immediate offsets
#pragma unroll
            for (int e = 0; e < 16; e++) park[G::THREADS * e] = x[e];
        }
        // the two digits take the same code with a shift of 0 resp. 15: not unrolled, one NTT body in the kernel
#pragma unroll 1
        for (uint32_t dg = 0; dg < 2; dg++)
        {
            const int td         = opaque_index(t);
            const uint32_t *park = lds + G::SLOTS + td;
            uint32_t y[16];
#pragma unroll
            for (int e = 0; e < 16; e++)
            {
                const uint32_t xe = kHoistPark<LOGN, SUM> ? park[G::THREADS * e] : x[e];
                y[e]              = (xe >> (kRelinDigitBits * dg)) & ((1u << kRelinDigitBits) - 1);
            }
            ntt_tiles<LOGN>(y, rw, qi, lds, td);
#pragma unroll
            for (int c = 0; c < 4; c++)
                *reinterpret_cast<uint4 *>(lds + 16 * td + 4 * c) =
                    make_uint4(y[4 * c], y[4 * c + 1], y[4 * c + 2], y[4 * c + 3]);
            __syncthreads();
            // the thread's first quad of row 2j + dg, column i of a key block
            const size_t ko = ((size_t)(2 * j + dg) * A.np + i) * 2 * N + quad_index(td, 0);
            if constexpr (SUM)
            {
#pragma unroll 1
                for (uint32_t e = 0; e < A.G; e++)
                    hoist_mac<LOGN>(acc0[0], acc1[0], lds, A.key[e] + ko, A.half, A.elt[e], r4, qi);
            }
            else
            {
#pragma unroll
                for (int u = 0; u < GC; u++)
                    if (e0 + u < A.G)
                        hoist_mac<LOGN>(acc0[u], acc1[u], lds, A.key[e0 + u] + ko, A.half, A.elt[e0 + u], r4, qi);
            }
            __syncthreads();
        }
    }
}

template <int LOGN, bool SUM>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_galois_hoist(const DevParams P, const DevTables T,
                                                                           const GaloisHoistArgs A)
{
    using G          = XformGeom<LOGN>;
    constexpr int N  = G::N;
    constexpr int GC = SUM ? 1 : kHoistGroup;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds      = reinterpret_cast<uint32_t *>(smem);
    const int t        = threadIdx.x;
    const uint32_t i   = blockIdx.y;
    const uint32_t qi  = P.q[i];
    const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * i;
    const uint32_t r4  = __brev((uint32_t)quad_index(t, 0)) >> (32 - LOGN);
    const uint32_t groups = SUM ? 1u : (A.G + GC - 1) / GC;

    for (size_t b = blockIdx.x; b < A.B; b += gridDim.x)
    {
        const size_t rec = b * A.primes * N;
        for (uint32_t grp = 0; grp < groups; grp++)
        {
            const uint32_t e0 = grp * GC;
            uint32_t acc0[GC][16], acc1[GC][16];
#pragma unroll
            for (int u = 0; u < GC; u++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc0[u][e] = acc1[u][e] = 0;
            hoist_digits<LOGN, SUM, GC>(acc0, acc1, A, rec, e0, i, qi, rw, r4, P, T, lds, t);
            // the c0 row of output prime i as it lies in memory goes into the plane, word k at lds[k]; gathered per element
            const int te   = opaque_index(t);
            const size_t o = rec + (size_t)i * N;
            const int k4   = quad_index(te, 0);
            uint32_t c[16];
            load_quads(c, A.c0 + o, te);
            park_row_quads(c, lds, k4);
            __syncthreads();
            if constexpr (SUM)
            {
                // canonical sum of the G gathered rows, and of the row itself with add_input
                if (!A.add_input)
#pragma unroll
                    for (int e = 0; e < 16; e++) c[e] = 0;
#pragma unroll 1
                for (uint32_t e = 0; e < A.G; e++)
                {
                    const uint32_t g = A.elt[e], u0 = (2 * r4 + 1) * g;
#pragma unroll
                    for (int w = 0; w < 16; w++) c[w] = csub(c[w] + hoist_word<LOGN>(lds, u0, g, w >> 2, w & 3), qi);
                }
#pragma unroll
                for (int e = 0; e < 16; e++) acc0[0][e] = csub(csub(acc0[0][e], qi) + c[e], qi);
                store_quads(A.out0 + o, acc0[0], te);
#pragma unroll
                for (int e = 0; e < 16; e++) acc1[0][e] = csub(acc1[0][e], qi);
                if (A.add_input)
                {
                    load_quads(c, A.c1 + o, te);
#pragma unroll
                    for (int e = 0; e < 16; e++) acc1[0][e] = csub(acc1[0][e] + c[e], qi);
                }
                store_quads(A.out1 + o, acc1[0], te);
            }
            else
            {
#pragma unroll
                for (int u = 0; u < GC; u++)
                    if (e0 + u < A.G)
                    {
                        const uint32_t g = A.elt[e0 + u], u0 = (2 * r4 + 1) * g;
                        const size_t og  = ((size_t)(e0 + u) * A.B + b) * A.primes * N + (size_t)i * N;
#pragma unroll
                        for (int e = 0; e < 16; e++)
                        {
                            acc0[u][e] = csub(csub(acc0[u][e], qi) + hoist_word<LOGN>(lds, u0, g, e >> 2, e & 3), qi);
                            acc1[u][e] = csub(acc1[u][e], qi);
                        }
                        store_quads(A.out0 + og, acc0[u], te);
                        store_quads(A.out1 + og, acc1[u], te);
                    }
            }
            __syncthreads();   // the next pass's first transpose writes the plane the gather reads
        }
    }
}

hipError_t launch_ct_galois_hoist(const DevParams &P, const DevTables &T, const GaloisHoistArgs &A, hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        using G         = XformGeom<L>;
        const dim3 grid    = evk_grid(A.B, A.primes);
        const size_t plane = (size_t)G::SLOTS * sizeof(uint32_t), park = (size_t)G::N * sizeof(uint32_t);
        return A.sum ? launch(k_ct_galois_hoist<L, true>, grid, dim3(G::THREADS), plane, st, P, T, A)
                     : launch(k_ct_galois_hoist<L, false>, grid, dim3(G::THREADS),
                              plane + (kHoistPark<L, false> ? park : 0), st, P, T, A);
    });
}

// ------------------------------------------------------------------------------------------
// Linear transform (se_amd_ct_lintrans_device): the diagonal method  out = d0 . (c0, c1) + sum_e d_e . rot[elt[e]]  with
// the hoisted rotations above and one plaintext row d_e per entry.  The sum form keeps ONE accumulator pair because its
// loop is digit outside, element inside; a weight applied after the digit sum would need a pair per element.  But d_e
// does not depend on the key row:
//   d_e[k] . sum_r F_r[src_e(k)] . gk_e[r][i][k]  =  sum_r F_r[src_e(k)] . (d_e[k] . gk_e[r][i][k])   mod q_i,
// so the plan holds key blocks with d_e folded in (k_lintrans_fold below) and the digit loop is hoist_digits<SUM> as it
// is: the same grid, thread shape, LDS plane and lazy ranges.  Only the c0 term carries d_e itself.  Epilogue, with the
// c0 row parked in the plane: c = d0 . c0 (or 0), then per entry c += sigma_e(c0) . d_e, every product a Shoup product
// in [0, 2 q_i) added to c in [0, 2 q_i) and brought back below 2 q_i; out0 = canon4(acc0 + c).  out1 = acc1 (+ d0 . c1).
// mul_shoup_lazy takes any 32-bit word of a slab; the diagonal words are canonical (the fold kernel reduced them).
// ------------------------------------------------------------------------------------------
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_lintrans(const DevParams P, const DevTables T,
                                                                       const LintransArgs A)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds      = reinterpret_cast<uint32_t *>(smem);
    const int t        = threadIdx.x;
    const uint32_t i   = blockIdx.y;
    const uint32_t qi  = P.q[i], two_qi = qi << 1;
    const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * i;
    const uint32_t r4  = __brev((uint32_t)quad_index(t, 0)) >> (32 - LOGN);

    for (size_t b = blockIdx.x; b < A.B; b += gridDim.x)
    {
        const size_t rec = b * A.primes * N;
        uint32_t acc0[1][16], acc1[1][16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[0][e] = acc1[0][e] = 0;
        hoist_digits<LOGN, true, 1>(acc0, acc1, A, rec, 0u, i, qi, rw, r4, P, T, lds, t);
        const int te   = opaque_index(t);
        const size_t o = rec + (size_t)i * N;
        const int k4   = quad_index(te, 0);
        // the thread's first quad of the (word, Shoup) rows of column i: entry e is e np 2 n further
        const size_t dcol     = (size_t)i * 2 * N + k4;
        const uint32_t *diag0 = A.diag0 ? A.diag0 + dcol : nullptr;
        uint32_t c[16];
        load_quads(c, A.c0 + o, te);
        park_row_quads(c, lds, k4);
        __syncthreads();
        if (diag0)
        {
#pragma unroll
            for (int m = 0; m < 4; m++)
            {
                uint32_t wv[4], sv[4];
                load_pair_quad<N>(diag0, m, wv, sv);
#pragma unroll
                for (int k = 0; k < 4; k++) c[4 * m + k] = mul_shoup_lazy(c[4 * m + k], wv[k], sv[k], qi);
            }
        }
        else
        {
#pragma unroll
            for (int e = 0; e < 16; e++) c[e] = 0;
        }
#pragma unroll 1
        for (uint32_t e = 0; e < A.G; e++)
        {
            const uint32_t g = A.elt[e], u0 = (2 * r4 + 1) * g;
            const uint32_t *d = A.diag + (size_t)e * A.np * 2 * N + dcol;
#pragma unroll
            for (int m = 0; m < 4; m++)
            {
                uint32_t wv[4], sv[4];
                load_pair_quad<N>(d, m, wv, sv);
#pragma unroll
                for (int k = 0; k < 4; k++)
                {
                    const uint32_t v = c[4 * m + k] + mul_shoup_lazy(hoist_word<LOGN>(lds, u0, g, m, k), wv[k], sv[k], qi);
                    c[4 * m + k]     = min(v, v - two_qi);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[0][e] = canon4(acc0[0][e] + c[e], qi, two_qi);
        store_quads(A.out0 + o, acc0[0], te);
        if (diag0)
        {
            load_quads(c, A.c1 + o, te);
#pragma unroll
            for (int m = 0; m < 4; m++)
            {
                uint32_t wv[4], sv[4];
                load_pair_quad<N>(diag0, m, wv, sv);
#pragma unroll
                for (int k = 0; k < 4; k++)
                    acc1[0][4 * m + k] += mul_shoup_lazy(c[4 * m + k], wv[k], sv[k], qi);
            }
        }
#pragma unroll
        for (int e = 0; e < 16; e++) acc1[0][e] = canon4(acc1[0][e], qi, two_qi);
        store_quads(A.out1 + o, acc1[0], te);
        __syncthreads();   // the next record's first transpose writes the plane the gather reads
    }
}

hipError_t launch_ct_lintrans(const DevParams &P, const DevTables &T, const LintransArgs &A, hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        using G         = XformGeom<L>;
        return launch(k_ct_lintrans<L>, evk_grid(A.B, A.primes), dim3(G::THREADS), (size_t)G::SLOTS * sizeof(uint32_t), st, P, T, A);
    });
}

// ------------------------------------------------------------------------------------------
// Hoisted rotations on the special-prime key ("double hoisting"): se_amd_ct_galois_sum_sp_device and
// se_amd_ct_lintrans_sp_device.  The sum of G rotations, plain or weighted by plaintext diagonals, of a level-L record
// (L <= np - 1) at its own scale, from ONE decomposition of c1 and ONE division by P whatever G is.  With the notation of
// the special-prime block (p = np - 1, P = q_p, E = {0 .. L-1, p}) and src_e the permutation of element e:
//   D_j         = centred(INTT_j(c1[b][j]), q_j)                                          (the digits of c1 ITSELF)
//   F_{j,i}     = NTT_i(D_j mod q_i),  i in E                                              (F_{j,j} = c1[b][j] as it lies)
//   acc_k[i][x] = sum_e sum_{j < L} F_{j,i}[src_e(x)] . key_k^e[j][i][x]   mod q_i,  i in E
//   delta_k     = centred(INTT_p(acc_k[p]), P);   ks_k[i] = (acc_k[i] - NTT_i(delta_k mod q_i)) . P^-1   mod q_i,  i < L
//   sum form:   out0 = ks_0 + add_input . c0 + sum_e sigma_e(c0),   out1 = ks_1 + add_input . c1
//   weighted:   key^e = the plan's block with d_e folded in on EVERY column, p included (k_lintrans_fold), and
//               out0 = ks_0 + d_0 . c0 + sum_e d_e . sigma_e(c0),   out1 = ks_1 + d_0 . c1      (d_0 terms only with diag0).
// Centring commutes with sigma (q - c centres to -centred(c)), so sigma(D_j) IS the digit of sigma(c1): one element
// without add_input gives the bits of k_ct_galois_sp.  G >= 2 carries one rounding centred(sum_e delta^e mod P) where G
// calls carry G.
// The body is ct_key_switch_sp's two passes crossed with the park-and-gather of hoist_digits<SUM>: the same grid, one
// workgroup of n/16 threads per (record, output prime i < L), LDS the exchange plane alone, ONE accumulator pair.
//   pass 0 (mod P, key column p), per j: sp_park_digit = evk_row_coeffs -> centre and reduce mod P -> ntt_tiles mod P,
//     which ends in tile layout 0 with the plane free -> parked as it lies, word k at lds[k] (no tile_to_quads) -> barrier
//     -> per element hoist_mac against row j, column p of that element's block -> barrier;
//   between the passes: sp_delta, once per half;
//   pass 1 (mod q_i, column i): the same per j != i; row i enters as it lies in memory (park_row_quads);
//   epilogue: . P^-1, then the c0 row parked once and gathered G times (weighted: by the diagonal pairs, the epilogue of
//     k_ct_lintrans), then the terms of the record itself.  They are added after the division: exact.
// Transforms per workgroup: those of ct_key_switch_sp, 4 L + 2, whatever G is; an element costs a gather and a
// multiply-accumulate per row and pass.
// Lazy ranges: those of evk_mac.  An accumulator takes G L products in pass 0 and is brought back into [0, 2 P) after each,
// so it enters intt_tiles (sp_delta) in [0, 2 P), its input range; it starts pass 1 in (0, 2 q_i], plus one product is
// below 4 q_i < 2^32, and after the first product it is in [0, 2 q_i) again.  The parked words are the lazy NTT output in
// [0, 4 q), resp. any 32-bit word of the slab for row i: mul_shoup_lazy takes any 32-bit y.
// Addresses: as in k_ct_galois_hoist (formed from the checked elements only, masked to [0, n)).
// grid evk_grid(B, L).
// ------------------------------------------------------------------------------------------
// NTT_c(D_j mod q) parked in the plane as ntt_tiles leaves it, word k at lds[k] (the staging of hoist_digits): the centred
// coefficients of input row j reduced mod q = q_c, rw the roots of column c; td = the opaque index of the transform and of
// the park.  The 16 words live here only: written into the row loop, merged with the words of the row that enters as it
// lies, k_ct_galois_sum_sp<14> spilled 36 - 48 bytes per lane and <12> took 129 VGPRs.  The caller's barrier publishes the
// plane.
template <int LOGN>
__device__ __forceinline__ void sp_park_digit(const uint32_t *row, uint32_t j, uint32_t q, const uint32_t *rw,
                                              const DevParams &P, const DevTables &T, uint32_t *lds, int td, int t)
{
    uint32_t y[16];
    const uint32_t qj = P.q[j], hj = qj >> 1, up = q - qj;   // up: mod 2^32 where q < q_j
    evk_row_coeffs<LOGN>(y, row, j, P, T, lds, opaque_index(t));
#pragma unroll
    for (int e = 0; e < 16; e++) y[e] += y[e] > hj ? up : 0u;
    ntt_tiles<LOGN>(y, rw, q, lds, td);
#pragma unroll
    for (int c = 0; c < 4; c++)
        *reinterpret_cast<uint4 *>(lds + 16 * td + 4 * c) = make_uint4(y[4 * c], y[4 * c + 1], y[4 * c + 2], y[4 * c + 3]);
}

template <int LOGN, bool WEIGHTED>
__device__ __forceinline__ void ct_hoist_sp(const DevParams &P, const DevTables &T, const RescaleParams &R,
                                            const HoistSpArgs &A, uint32_t *lds)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    const int t        = threadIdx.x;
    const uint32_t i   = blockIdx.y;
    const uint32_t sp  = A.np - 1;
    const uint32_t qi  = P.q[i], two_qi = qi << 1;

    for (size_t b = blockIdx.x; b < A.B; b += gridDim.x)
    {
        const size_t rec = b * A.primes * N;
        uint32_t acc0[16], acc1[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = acc1[e] = 0;
        // pass 0: modulo P against key column p; pass 1: modulo q_i against key column i.  One body for both.
#pragma unroll 1
        for (uint32_t pass = 0; pass < 2; pass++)
        {
            const uint32_t col = pass ? i : sp;
            const uint32_t q   = P.q[col];
            const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * col;
            for (uint32_t j = 0; j < A.primes; j++)
            {
                const int td = opaque_index(t);
                if (pass && j == i)
                {
                    uint32_t y[16];
                    load_quads(y, A.c1 + rec + (size_t)i * N, td);
                    park_row_quads(y, lds, quad_index(td, 0));
                }
                else
                    sp_park_digit<LOGN>(A.c1 + rec + (size_t)j * N, j, q, rw, P, T, lds, td, t);
                __syncthreads();
                // the thread's first quad of row j, column col of a key block, and brev of that quad for the gathers: from
                // the opaque index, so that nothing but the accumulators lives across sp_delta
                const size_t ko   = ((size_t)j * A.np + col) * 2 * N + quad_index(td, 0);
                const uint32_t r4 = __brev((uint32_t)quad_index(td, 0)) >> (32 - LOGN);
#pragma unroll 1
                for (uint32_t e = 0; e < A.G; e++)
                    hoist_mac<LOGN>(acc0, acc1, lds, A.key[e] + ko, A.half, A.elt[e], r4, q);
                __syncthreads();
            }
            if (pass == 0) sp_delta<LOGN>(acc0, acc1, i, sp, P, T, lds, t);
        }
        // ks_k = acc_k . P^-1 (lazy, [0, 2 q_i)), then the addends; the c0 row of output prime i goes into the plane
        const int te   = opaque_index(t);
        const size_t o = rec + (size_t)i * N;
        const int k4   = quad_index(te, 0);
        const uint32_t r4 = __brev((uint32_t)k4) >> (32 - LOGN);
        const uint32_t w = R.inv[i], wp = R.inv_sh[i];
        uint32_t c[16];
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            acc0[e] = mul_shoup_lazy(acc0[e], w, wp, qi);
            acc1[e] = mul_shoup_lazy(acc1[e], w, wp, qi);
        }
        if constexpr (!WEIGHTED)
        {
            // out1 first: its accumulator is gone before the gathers begin
#pragma unroll
            for (int e = 0; e < 16; e++) acc1[e] = csub(acc1[e], qi);
            if (A.add_input)
            {
                load_quads(c, A.c1 + o, te);
#pragma unroll
                for (int e = 0; e < 16; e++) acc1[e] = csub(acc1[e] + c[e], qi);
            }
            store_quads(A.out1 + o, acc1, te);
        }
        load_quads(c, A.c0 + o, te);
        park_row_quads(c, lds, k4);
        __syncthreads();
        if constexpr (WEIGHTED)
        {
            // the thread's first quad of the (word, Shoup) rows of column i: entry e is e np 2 n further
            const size_t dcol     = (size_t)i * 2 * N + k4;
            const uint32_t *diag0 = A.diag0 ? A.diag0 + dcol : nullptr;
            if (diag0)
            {
#pragma unroll
                for (int m = 0; m < 4; m++)
                {
                    uint32_t wv[4], sv[4];
                    load_pair_quad<N>(diag0, m, wv, sv);
#pragma unroll
                    for (int k = 0; k < 4; k++) c[4 * m + k] = mul_shoup_lazy(c[4 * m + k], wv[k], sv[k], qi);
                }
            }
            else
            {
#pragma unroll
                for (int e = 0; e < 16; e++) c[e] = 0;
            }
#pragma unroll 1
            for (uint32_t e = 0; e < A.G; e++)
            {
                const uint32_t g = A.elt[e], u0 = (2 * r4 + 1) * g;
                const uint32_t *d = A.diag + (size_t)e * A.np * 2 * N + dcol;
#pragma unroll
                for (int m = 0; m < 4; m++)
                {
                    uint32_t wv[4], sv[4];
                    load_pair_quad<N>(d, m, wv, sv);
#pragma unroll
                    for (int k = 0; k < 4; k++)
                    {
                        const uint32_t v = c[4 * m + k] + mul_shoup_lazy(hoist_word<LOGN>(lds, u0, g, m, k), wv[k], sv[k], qi);
                        c[4 * m + k]     = min(v, v - two_qi);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 16; e++) acc0[e] = canon4(acc0[e] + c[e], qi, two_qi);
            store_quads(A.out0 + o, acc0, te);
            if (diag0)
            {
                load_quads(c, A.c1 + o, te);
#pragma unroll
                for (int m = 0; m < 4; m++)
                {
                    uint32_t wv[4], sv[4];
                    load_pair_quad<N>(diag0, m, wv, sv);
#pragma unroll
                    for (int k = 0; k < 4; k++) acc1[4 * m + k] += mul_shoup_lazy(c[4 * m + k], wv[k], sv[k], qi);
                }
            }
#pragma unroll
            for (int e = 0; e < 16; e++) acc1[e] = canon4(acc1[e], qi, two_qi);
            store_quads(A.out1 + o, acc1, te);
        }
        else
        {
            // the canonical ks_0 takes the G gathered rows one by one, and the row itself with add_input
#pragma unroll
            for (int e = 0; e < 16; e++) acc0[e] = csub(csub(acc0[e], qi) + (A.add_input ? c[e] : 0u), qi);
#pragma unroll 1
            for (uint32_t e = 0; e < A.G; e++)
            {
                const uint32_t g = A.elt[e], u0 = (2 * r4 + 1) * g;
#pragma unroll
                for (int k = 0; k < 16; k++) acc0[k] = csub(acc0[k] + hoist_word<LOGN>(lds, u0, g, k >> 2, k & 3), qi);
            }
            store_quads(A.out0 + o, acc0, te);
        }
        __syncthreads();   // the next record's first transpose writes the plane the gather reads
    }
}

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_galois_sum_sp(const DevParams P, const DevTables T,
                                                                            const RescaleParams R, const HoistSpArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ct_hoist_sp<LOGN, false>(P, T, R, A, reinterpret_cast<uint32_t *>(smem));
}

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_lintrans_sp(const DevParams P, const DevTables T,
                                                                          const RescaleParams R, const HoistSpArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ct_hoist_sp<LOGN, true>(P, T, R, A, reinterpret_cast<uint32_t *>(smem));
}

// LOGN 12 .. 14 only, by the rule of launch_ct_key_switch_sp.
hipError_t launch_ct_hoist_sp(const DevParams &P, const DevTables &T, const RescaleParams &R, const HoistSpArgs &A,
                              hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    if (P.logn < 12) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value < 12 ? 12 : decltype(l)::value;
        using G         = XformGeom<L>;
        const dim3 grid    = evk_grid(A.B, A.primes);
        const size_t plane = (size_t)G::SLOTS * sizeof(uint32_t);
        return A.weighted ? launch(k_ct_lintrans_sp<L>, grid, dim3(G::THREADS), plane, st, P, T, R, A)
                          : launch(k_ct_galois_sum_sp<L>, grid, dim3(G::THREADS), plane, st, P, T, R, A);
    });
}

// ------------------------------------------------------------------------------------------
// Baby-step / giant-step transforms on the special-prime keys (se_amd_ct_bsgs_sp_device): the division by P is DEFERRED.
// The baby steps leave extended records -- L + 1 rows, the last one modulo P: "P times the rotated ciphertext plus the
// key-switch sum", undivided -- the diagonals are multiplied in on all L + 1 rows (k_ct_mul_plain_sum with the row map),
// every giant step's inner sum is divided once (k_ct_mod_down_sp) and the giant steps share one more division
// (k_ct_galois_accum_sp): n2 + 1 roundings for n1 n2 diagonals.
//
// k_ct_galois_many_ext_sp: out[e][b] = the undivided rotation of record b by elt[e], from ONE decomposition of c1 (the
// digits D_j of ct_hoist_sp).  One workgroup of n/16 threads per (record, row r of the extended record); row r < L works
// modulo q_r against key column r, row L modulo P against key column p = np - 1: ONE pass of ct_hoist_sp's two, no delta.
//   per j < L: sp_park_digit (row j == r < L enters as it lies: park_row_quads) -> barrier -> per element of the group
//     hoist_mac against row j, column i_r of that element's block -> barrier;
//   epilogue, r < L: the c0 row parked once and gathered per element, (P mod q_r) . sigma_e(c0) by barrett64 (exact on any
//     64-bit word) added to the canonical accumulator.  Element 1: no key, no product; out_k = (P mod q_r) . c_k, row L zero.
// The elements are taken in groups of kManyExtGroup accumulator pairs per pass over the rows, as k_ct_galois_hoist<., false>
// does: ceil(G / kManyExtGroup) times 2 (L - 1) transforms on a row r < L and 2 L on row L, 2 L^2 per record and group.
// Lazy ranges: those of evk_mac -- an accumulator starts at 0 and is back in [0, 2 q) after every product, the parked words
// are the lazy NTT output in [0, 4 q) resp. any 32-bit word of the slab; one csub canonicalises.  (P mod q_r) . c < 2^62.
// Addresses: as in k_ct_galois_hoist (formed from the checked elements only, masked to [0, n)).
// grid evk_grid(B, L + 1).
// ------------------------------------------------------------------------------------------
constexpr int kManyExtGroup = kHoistGroup;

template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_galois_many_ext_sp(const DevParams P, const DevTables T,
                                                                                 const GaloisSetArgs A)
{
    using G          = XformGeom<LOGN>;
    constexpr int N  = G::N;
    constexpr int GC = kManyExtGroup;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds      = reinterpret_cast<uint32_t *>(smem);
    const int t        = threadIdx.x;
    const uint32_t r   = blockIdx.y;                       // row of the extended record
    const bool data    = r < A.primes;
    const uint32_t col = data ? r : A.np - 1;              // its prime and key column
    const uint32_t q = P.q[col], cr_hi = P.cr_hi[col], cr_lo = P.cr_lo[col];
    const uint32_t pm  = data ? P.q[A.np - 1] % q : 0u;    // P mod q_r
    const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * col;
    const size_t rows  = (size_t)A.primes + 1;
    const uint32_t groups = (A.G + GC - 1) / GC;

    for (size_t b = blockIdx.x; b < A.B; b += gridDim.x)
    {
        const size_t rec = b * A.primes * N;
        for (uint32_t grp = 0; grp < groups; grp++)
        {
            const uint32_t e0 = grp * GC;
            uint32_t acc0[GC][16], acc1[GC][16];
#pragma unroll
            for (int u = 0; u < GC; u++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc0[u][e] = acc1[u][e] = 0;
            for (uint32_t j = 0; j < A.primes; j++)
            {
                const int td = opaque_index(t);
                if (j == r)
                {
                    uint32_t y[16];
                    load_quads(y, A.c1 + rec + (size_t)j * N, td);
                    park_row_quads(y, lds, quad_index(td, 0));
                }
                else
                    sp_park_digit<LOGN>(A.c1 + rec + (size_t)j * N, j, q, rw, P, T, lds, td, t);
                __syncthreads();
                const size_t ko   = ((size_t)j * A.np + col) * 2 * N + quad_index(td, 0);
                const uint32_t r4 = __brev((uint32_t)quad_index(td, 0)) >> (32 - LOGN);
#pragma unroll
                for (int u = 0; u < GC; u++)
                    if (e0 + u < A.G && A.elt[e0 + u] != 1)
                        hoist_mac<LOGN>(acc0[u], acc1[u], lds, A.key[e0 + u] + ko, A.half, A.elt[e0 + u], r4, q);
                __syncthreads();
            }
            const int te      = opaque_index(t);
            const int k4      = quad_index(te, 0);
            const uint32_t r4 = __brev((uint32_t)k4) >> (32 - LOGN);
            if (data)
            {
                uint32_t c[16];
                load_quads(c, A.c0 + rec + (size_t)r * N, te);
                park_row_quads(c, lds, k4);
                __syncthreads();
            }
#pragma unroll
            for (int u = 0; u < GC; u++)
                if (e0 + u < A.G)
                {
                    const uint32_t g = A.elt[e0 + u], u0 = (2 * r4 + 1) * g;
                    const size_t og  = (((size_t)(e0 + u) * A.B + b) * rows + r) * N;
#pragma unroll
                    for (int e = 0; e < 16; e++)
                    {
                        acc0[u][e] = csub(acc0[u][e], q);
                        acc1[u][e] = csub(acc1[u][e], q);
                    }
                    if (data)
                    {
#pragma unroll
                        for (int e = 0; e < 16; e++)
                        {
                            const uint32_t w = hoist_word<LOGN>(lds, u0, g, e >> 2, e & 3);
                            acc0[u][e] = csub(acc0[u][e] + barrett64((uint64_t)w * pm, q, cr_hi, cr_lo), q);
                        }
                        if (g == 1)
                        {
                            // the record itself: the accumulators are 0, out1 = (P mod q_r) . c1
                            uint32_t c[16];
                            load_quads(c, A.c1 + rec + (size_t)r * N, te);
#pragma unroll
                            for (int e = 0; e < 16; e++) acc1[u][e] = barrett64((uint64_t)c[e] * pm, q, cr_hi, cr_lo);
                        }
                    }
                    store_quads(A.out0 + og, acc0[u], te);
                    store_quads(A.out1 + og, acc1[u], te);
                }
            __syncthreads();   // the next pass's first transpose writes the plane the gather reads
        }
    }
}

// LOGN 12 .. 14 only, by the rule of launch_ct_key_switch_sp.
hipError_t launch_ct_galois_many_ext_sp(const DevParams &P, const DevTables &T, const GaloisSetArgs &A,
                                        hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    if (P.logn < 12) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value < 12 ? 12 : decltype(l)::value;
        using G         = XformGeom<L>;
        return launch(k_ct_galois_many_ext_sp<L>, evk_grid(A.B, A.primes + 1), dim3(G::THREADS),
                      (size_t)G::SLOTS * sizeof(uint32_t), st, P, T, A);
    });
}

// ------------------------------------------------------------------------------------------
// k_ct_galois_accum_sp: the giant steps with ONE division by P.  G DIFFERENT level-L records (a^g, b^g) = in[g][b] are
// rotated by elt[g] under the special-prime keys and added.  It is ct_key_switch_sp<., true> -- the same grid, thread shape,
// two passes, sp_row_digit, evk_mac, sp_delta, lazy ranges -- with the element loop of k_ct_galois_accum inside each pass:
// ONE accumulator pair takes the products of every keyed element (evk_mac leaves it in [0, 2 q) whichever block a product
// came from), so there is one delta and one rounding centred(sum_g acc^g[p]) where G calls of k_ct_galois_sp round G times.
// The exact addends -- sigma_g(a^g) of a keyed element (load_row_sigma), both rows of an element 1 as they lie -- join the
// canonical ks_k AFTER the division.  Without a keyed element the accumulators stay 0, delta is 0 and ks is 0.
// G (4 L - 2) + 4 transforms per workgroup for G keyed elements, against G (4 L + 2) of G single rotations.
// Addresses: as in k_ct_galois (formed from the checked elements only, masked to [0, n)).
// grid evk_grid(B, L).
// ------------------------------------------------------------------------------------------
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_galois_accum_sp(const DevParams P, const DevTables T,
                                                                              const RescaleParams R,
                                                                              const GaloisSetArgs A)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds      = reinterpret_cast<uint32_t *>(smem);
    const int t        = threadIdx.x;
    const uint32_t i   = blockIdx.y;
    const uint32_t sp  = A.np - 1;
    const uint32_t qi  = P.q[i];

    for (size_t b = blockIdx.x; b < A.B; b += gridDim.x)
    {
        uint32_t acc0[16], acc1[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = acc1[e] = 0;
        // pass 0: modulo P against key column p; pass 1: modulo q_i against key column i.  One body for both.
#pragma unroll 1
        for (uint32_t pass = 0; pass < 2; pass++)
        {
            const uint32_t col = pass ? i : sp;
            const uint32_t q   = P.q[col];
            const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * col;
#pragma unroll 1
            for (uint32_t s = 0; s < A.G; s++)
            {
                const uint32_t g = A.elt[s];
                if (g == 1) continue;
                const uint32_t *sw = A.c1 + ((size_t)s * A.B + b) * A.primes * N;
                for (uint32_t j = 0; j < A.primes; j++)
                {
                    uint32_t y[16];
                    if (pass && j == i)
                        load_row_sigma<LOGN, true>(y, sw + (size_t)i * N, g, lds, opaque_index(t));
                    else
                        sp_row_digit<LOGN, true>(y, sw + (size_t)j * N, j, g, q, rw, P, T, lds, t);
                    const uint32_t *key = A.key[s] + ((size_t)j * A.np + col) * 2 * N + quad_index(opaque_index(t), 0);
                    evk_mac<LOGN>(acc0, acc1, y, key, A.half, q);
                    __syncthreads();
                }
            }
            if (pass == 0) sp_delta<LOGN>(acc0, acc1, i, sp, P, T, lds, t);
        }
        // ks_k = acc_k . P^-1, canonical; then the exact addends
        const uint32_t w = R.inv[i], wp = R.inv_sh[i];
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            acc0[e] = csub(mul_shoup_lazy(acc0[e], w, wp, qi), qi);
            acc1[e] = csub(mul_shoup_lazy(acc1[e], w, wp, qi), qi);
        }
#pragma unroll 1
        for (uint32_t s = 0; s < A.G; s++)
        {
            const uint32_t g = A.elt[s];
            const int te     = opaque_index(t);
            const size_t o   = (((size_t)s * A.B + b) * A.primes + i) * N;
            uint32_t c[16];
            if (g != 1)
            {
                load_row_sigma<LOGN, true>(c, A.c0 + o, g, lds, te);
#pragma unroll
                for (int e = 0; e < 16; e++) acc0[e] = csub(acc0[e] + c[e], qi);
                __syncthreads();   // the next park writes the plane the gather reads
            }
            else
            {
                load_quads(c, A.c0 + o, te);
#pragma unroll
                for (int e = 0; e < 16; e++) acc0[e] = csub(acc0[e] + c[e], qi);
                load_quads(c, A.c1 + o, te);
#pragma unroll
                for (int e = 0; e < 16; e++) acc1[e] = csub(acc1[e] + c[e], qi);
            }
        }
        const int te   = opaque_index(t);
        const size_t o = (b * A.primes + i) * N;
        store_quads(A.out0 + o, acc0, te);
        store_quads(A.out1 + o, acc1, te);
    }
}

// LOGN 12 .. 14 only, by the rule of launch_ct_key_switch_sp.
hipError_t launch_ct_galois_accum_sp(const DevParams &P, const DevTables &T, const RescaleParams &R,
                                     const GaloisSetArgs &A, hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    if (P.logn < 12) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value < 12 ? 12 : decltype(l)::value;
        using G         = XformGeom<L>;
        return launch(k_ct_galois_accum_sp<L>, evk_grid(A.B, A.primes), dim3(G::THREADS),
                      (size_t)G::SLOTS * sizeof(uint32_t), st, P, T, R, A);
    });
}

// ------------------------------------------------------------------------------------------
// Baby-step / giant-step linear transforms (se_amd_ct_bsgs_device): y = sum_{g, b} d[g][b] . rot_{giant[g] baby[b]}(x) as
//   rot[b] = the hoisted MANY form above (the record itself for element 1),
//   inner[g] = sum_b d'[g][b] . rot[b]                      k_ct_mul_plain_sum
//   out = sum_g rho_{giant[g]}(inner[g])                    k_ct_galois_accum
// with d' the diagonals pre-rotated by giant[g]^-1 when the plan is made (k_bsgs_permute).  n1 + n2 - 2 Galois keys serve
// n1 n2 diagonals.
//
// k_ct_mul_plain_sum: out[g][b] = sum_{e < E} pt[g][e] . in[e][b], element-wise and bound by HBM like k_ct_mul_plain,
// whose access shape it has: a 256-thread workgroup owns 1024 consecutive residues -- inside one prime, q_i and its Barrett
// constants scalar -- of kSumTile consecutive records of ONE output g, and walks e.  Per e: one plaintext quad, reduced mod
// q_i once (barrett64 takes any 64-bit word) and used by the kSumTile records, and kSumTile input quads, all requested
// before the first product.  The input quads do not depend on g: the Gout workgroups that read the same input rows follow
// one another on ONE XCD (the block order in the kernel), so all but the first find them in that die's L2; with g simply
// running first in blockIdx.x they sat on eight dies and the weighted sum of 64 diagonals took 16.1 ms instead of 9.8
// (4096 x 3, 16 384 records).
// Lazy range.  The reduced plaintext word is below q_i < 2^30 and an input word is ANY 32-bit word, so one product is below
// 2^62; the accumulator enters a period canonical (below 2^30) and takes kSumPeriod = 3 products:
//   2^30 + 3 . 2^62 < 2^64; a fourth would not fit.  (64 products of (q - 1)^2 ~ 2^60 pass 2^64: the saturation case.)
// Row offsets are 64-bit; E B and Gout B are below 2^32 (checked by the host).  grid (Gout . primes n / 1024 . slabs,
// min(ceil(B / kSumTile), 65 535)).
// ------------------------------------------------------------------------------------------
constexpr int kSumTile   = 4;
constexpr int kSumPeriod = 3;
constexpr uint32_t kXcds = 8;   // accelerator dies of an MI355X; workgroups are dealt to them round-robin

__global__ __launch_bounds__(kLcThreads) void k_ct_mul_plain_sum(const DevParams P, const MulPlainSumArgs A)
{
    const size_t row      = (size_t)A.primes << P.logn;
    const size_t pt_row   = (size_t)A.pt_primes << P.logn;
    const uint32_t chunks = (uint32_t)(row >> kLcTileLog);
    // blockIdx.x -> (g, row tile).  Consecutive workgroups go to consecutive XCDs, each with an L2 of its own: where the
    // row tiles divide by kXcds, workgroup 8 v + k (all on XCD k) takes g = v mod Gout of row tile 8 (v / Gout) + k, so the
    // Gout readers of one input tile follow one another on ONE XCD.  Elsewhere g simply runs first.
    const uint32_t tiles_x = chunks * (A.in1 ? 2u : 1u);
    const bool by_xcd      = tiles_x % kXcds == 0;
    const uint32_t v       = by_xcd ? blockIdx.x / kXcds : blockIdx.x;
    const uint32_t g       = v % A.Gout;
    const uint32_t rest    = by_xcd ? v / A.Gout * kXcds + blockIdx.x % kXcds : v / A.Gout;
    const uint32_t slab   = rest / chunks;
    const uint32_t chunk  = rest - slab * chunks;
    // row -> prime: the identity but for the last row, which is modulo q_{last_prime} (the special prime on extended
    // records) and meets that row of the plaintext: a shift of the plaintext's base, scalar like the rest
    const uint32_t r      = (chunk << kLcTileLog) >> P.logn;
    const uint32_t j      = r == A.primes - 1 ? A.last_prime : r;
    const uint32_t q = P.q[j], cr_hi = P.cr_hi[j], cr_lo = P.cr_lo[j];
    const uint32_t *__restrict__ in = slab ? A.in1 : A.in0;
    const uint32_t *__restrict__ pt = A.pt + ((size_t)(j - r) << P.logn);
    uint32_t *__restrict__ out      = slab ? A.out1 : A.out0;
    const size_t off   = ((size_t)chunk << kLcTileLog) + 4 * threadIdx.x;   // the same offset inside a plaintext
    const size_t tiles = ((size_t)A.B + kSumTile - 1) / kSumTile;

    for (size_t tile = blockIdx.y; tile < tiles; tile += gridDim.y)
    {
        const size_t b0 = tile * kSumTile;
        // a record past the end of the last tile reads the last record again and is not stored
        size_t rec[kSumTile];
#pragma unroll
        for (int r = 0; r < kSumTile; r++) rec[r] = b0 + r < A.B ? b0 + r : (size_t)A.B - 1;
        Lane4 acc[kSumTile];
        int pending = 0;
        for (uint32_t e = 0; e < A.E; e++)
        {
            uint4 m = load_row(pt, (size_t)g * A.E + e, pt_row, off);
            uint4 v[kSumTile];
#pragma unroll
            for (int r = 0; r < kSumTile; r++) v[r] = load_row(in, (size_t)e * A.B + rec[r], row, off);
            m.x = barrett64((uint64_t)m.x, q, cr_hi, cr_lo);
            m.y = barrett64((uint64_t)m.y, q, cr_hi, cr_lo);
            m.z = barrett64((uint64_t)m.z, q, cr_hi, cr_lo);
            m.w = barrett64((uint64_t)m.w, q, cr_hi, cr_lo);
#pragma unroll
            for (int r = 0; r < kSumTile; r++) acc[r].mad4(v[r], m);
            if (++pending == kSumPeriod)
            {
#pragma unroll
                for (int r = 0; r < kSumTile; r++) acc[r].reduce(q, cr_hi, cr_lo);
                pending = 0;
            }
        }
#pragma unroll
        for (int r = 0; r < kSumTile; r++)
        {
            if (pending) acc[r].reduce(q, cr_hi, cr_lo);
            if (b0 + r < A.B) *reinterpret_cast<uint4 *>(out + ((size_t)g * A.B + b0 + r) * row + off) = acc[r].get();
        }
    }
}

hipError_t launch_ct_mul_plain_sum(const DevParams &P, const MulPlainSumArgs &A, hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    const uint32_t chunks = (uint32_t)(((size_t)A.primes << P.logn) >> kLcTileLog);
    const uint32_t slabs  = A.in1 ? 2 : 1;
    const uint32_t tiles  = (A.B - 1) / kSumTile + 1;
    const dim3 grid(A.Gout * chunks * slabs, tiles < 65535u ? tiles : 65535u);
    return launch(k_ct_mul_plain_sum, grid, dim3(kLcThreads), 0, st, P, A);
}

// ------------------------------------------------------------------------------------------
// k_ct_galois_accum: out[b] = sum_g rho_g(in[g][b]), rho_g = k_ct_galois's map with elt[g] and its installed key -- the
// giant steps of a baby-step / giant-step product, G rotations of G DIFFERENT records into one.  It is k_ct_galois with the
// element loop inside the record loop: the same grid, thread shape, transforms (3 L per keyed element), key layout and lazy
// ranges, LDS the exchange plane alone.  ONE accumulator pair lives across the G elements: evk_mac leaves it in
// [0, 2 q_i) after every product, whichever key block the product came from, so the digits of element g + 1 accumulate on
// top of those of element g and the one canonicalisation is the epilogue's.  sigma(c0) of element g joins the same pair: the
// row of output prime i is parked in the plane (free behind evk_digits' last barrier), gathered through src_g as in
// k_ct_galois, and added to acc0 -- a canonical word d < q_i on an accumulator in [0, 2 q_i) is below 3 q_i < 2^32, and
// min(s, s - 2 q_i) brings it back.  The sum is modular and every step exact, so the result has the bits of the modular sum
// of G k_ct_galois outputs in any order.  Element 1 is the identity: no key switch, both rows are added as they lie.
// Addresses: as in k_ct_galois (formed from the checked elements only, masked to [0, n)).
// grid evk_grid(B, L).
// ------------------------------------------------------------------------------------------
template <int LOGN>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_galois_accum(const DevParams P, const DevTables T,
                                                                           const GaloisSetArgs A)
{
    using G         = XformGeom<LOGN>;
    constexpr int N = G::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lds      = reinterpret_cast<uint32_t *>(smem);
    const int t        = threadIdx.x;
    const uint32_t i   = blockIdx.y;
    const uint32_t qi  = P.q[i], two_qi = qi << 1;
    const uint32_t *rw = T.ntt_rw + 2 * xform_table_len(N) * i;

    for (size_t b = blockIdx.x; b < A.B; b += gridDim.x)
    {
        uint32_t acc0[16], acc1[16];
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = acc1[e] = 0;
#pragma unroll 1
        for (uint32_t s = 0; s < A.G; s++)
        {
            const uint32_t g = A.elt[s];
            const size_t rec = ((size_t)s * A.B + b) * A.primes * N;
            if (g != 1)
            {
                const uint32_t *k0 = A.key[s] + (size_t)i * 2 * N;
                for (uint32_t j = 0; j < A.primes; j++)
                {
                    const int tj      = opaque_index(t);
                    const uint32_t qj = P.q[j];
                    uint32_t x[16];
                    evk_row_coeffs<LOGN>(x, A.c1 + rec + (size_t)j * N, j, P, T, lds, tj);
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
                    evk_digits<LOGN>(x, acc0, acc1, A, k0, j, rw, qi, lds, t);
                }
            }
            const int te   = opaque_index(t);
            const size_t o = rec + (size_t)i * N;
            uint32_t c[16];
            load_quads(c, A.c0 + o, te);
            if (g != 1)
            {
                const int k4 = quad_index(te, 0);
                park_row_quads(c, lds, k4);   // sigma(c0) row i
                __syncthreads();
                gather_row<LOGN>(c, lds, k4, g);
            }
#pragma unroll
            for (int e = 0; e < 16; e++)
            {
                const uint32_t u = acc0[e] + c[e];
                acc0[e]          = min(u, u - two_qi);
            }
            if (g != 1)
                __syncthreads();   // the next transpose writes the plane the gather reads
            else
            {
                load_quads(c, A.c1 + o, te);
#pragma unroll
                for (int e = 0; e < 16; e++)
                {
                    const uint32_t u = acc1[e] + c[e];
                    acc1[e]          = min(u, u - two_qi);
                }
            }
        }
        const int te   = opaque_index(t);
        const size_t o = b * A.primes * N + (size_t)i * N;
#pragma unroll
        for (int e = 0; e < 16; e++)
        {
            acc0[e] = csub(acc0[e], qi);
            acc1[e] = csub(acc1[e], qi);
        }
        store_quads(A.out0 + o, acc0, te);
        store_quads(A.out1 + o, acc1, te);
    }
}

hipError_t launch_ct_galois_accum(const DevParams &P, const DevTables &T, const GaloisSetArgs &A, hipStream_t st)
{
    if (A.B == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        using G         = XformGeom<L>;
        return launch(k_ct_galois_accum<L>, evk_grid(A.B, A.primes), dim3(G::THREADS),
                      (size_t)G::SLOTS * sizeof(uint32_t), st, P, T, A);
    });
}

// Plan set-up of se_amd_bsgs_create: out[r][k] = in[r][src_elt(k)], one thread per word.
template <int LOGN>
__global__ __launch_bounds__(kLcThreads) void k_bsgs_permute(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                          uint32_t elt, size_t words)
{
    const size_t w = (size_t)blockIdx.x * kLcThreads + threadIdx.x;
    if (w >= words) return;
    const uint32_t k = (uint32_t)(w & ((1u << LOGN) - 1));
    out[w]           = in[w - k + galois_src<LOGN>(k, elt)];
}

hipError_t launch_bsgs_permute(const DevParams &P, const uint32_t *in, uint32_t *out, size_t rows, uint32_t elt,
                               hipStream_t st)
{
    const size_t words = rows << P.logn;
    if (words == 0) return hipSuccess;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        return launch(k_bsgs_permute<L>, dim3((unsigned)(words / kLcThreads)), dim3(kLcThreads), 0, st, in, out, elt,
                      words);
    });
}

// Plan set-up: one thread per key word of an installed block [2][R][np][2][n] (R = 2 np rows of a digit key, np - 1 of a
// special-prime key), or per diagonal word when there is no block (the weight of the record itself).  d = the diagonal word of the thread's column and position reduced mod q_i
// (any 32-bit word is valid input; columns i >= pt have no diagonal and get 0); the thread of half 0, row 0 also writes
// the (d, Shoup) pair of its position.
__global__ __launch_bounds__(kLcThreads) void k_lintrans_fold(const DevParams P, const uint32_t *__restrict__ key_in,
                                                           uint32_t *__restrict__ key_out,
                                                           const uint32_t *__restrict__ diag_in,
                                                           uint32_t *__restrict__ pair_out, uint32_t pt, size_t words)
{
    const size_t k = (size_t)blockIdx.x * kLcThreads + threadIdx.x;
    if (k >= words) return;
    const size_t col   = k >> P.logn, c = k & (P.n - 1);   // col = (half R + row) np + i
    const uint32_t i   = (uint32_t)(col % P.nprimes);
    const uint32_t q   = P.q[i];
    const uint32_t d   = i < pt ? diag_in[((size_t)i << P.logn) + c] % q : 0;
    if (col < P.nprimes)
    {
        pair_out[((2 * col) << P.logn) + c]     = d;
        pair_out[((2 * col + 1) << P.logn) + c] = (uint32_t)(((uint64_t)d << 32) / q);
    }
    if (!key_in) return;
    const uint32_t w = barrett64((uint64_t)key_in[((2 * col) << P.logn) + c] * d, q, P.cr_hi[i], P.cr_lo[i]);
    key_out[((2 * col) << P.logn) + c]     = w;
    key_out[((2 * col + 1) << P.logn) + c] = (uint32_t)(((uint64_t)w << 32) / q);
}

hipError_t launch_lintrans_fold(const DevParams &P, const uint32_t *key_in, uint32_t *key_out, size_t rows,
                                const uint32_t *diag_in, uint32_t *pair_out, uint32_t pt, hipStream_t st)
{
    // 2 halves of `rows` rows (2 np of a digit block, np - 1 of a special-prime block: at least one row of np columns)
    const size_t words = ((size_t)(key_in ? 2 * rows : 1) * P.nprimes) << P.logn;
    return launch(k_lintrans_fold, dim3((unsigned)(words / kLcThreads)), dim3(kLcThreads), 0, st, P, key_in, key_out,
                  diag_in, pair_out, pt, words);
}

// The diagonal term of an evaluation key on the [R][np][n] slab the public-key chain wrote:
//   key0[2j + t][j][k] += 2^(15 t) . d[k]  mod q_j,  t = 0, 1   (2^15 < q_j: the factor is its own residue),
// d = s_hat^2 for the relinearisation key (SIGMA false; g unused), d[k] = s_hat[src_g(k)] -- sigma_g(s) in NTT form --
// for the Galois key of element g (SIGMA true; g is odd and below 2n, checked by the host).  The third target, d = the
// row as it is, is a switching key's (special-prime rows only; g unused): the caller passes the canonical NTT form of
// the OTHER secret key, the one the key hides.
// d < q_j < 2^30 lives in a register only; d 2^15 + key0 < 2^46.  grid n / 256.
enum DiagTarget { kDiagSquare, kDiagSigma, kDiagOther };
template <bool SIGMA>
constexpr DiagTarget kDiagOf = SIGMA ? kDiagSigma : kDiagSquare;
template <int LOGN, DiagTarget TARGET>
__device__ __forceinline__ uint64_t evk_diag_target(const DevParams &P, uint32_t j, uint32_t g, uint32_t c,
                                                    const uint32_t *__restrict__ s_hat)
{
    if constexpr (TARGET == kDiagSigma)
        return s_hat[galois_src<LOGN>(c, g)];
    else if constexpr (TARGET == kDiagOther)
        return s_hat[c];
    else
        return barrett64((uint64_t)s_hat[c] * s_hat[c], P.q[j], P.cr_hi[j], P.cr_lo[j]);
}

template <int LOGN, bool SIGMA>
__global__ __launch_bounds__(kLcThreads) void k_evk_diag(const DevParams P, uint32_t j, uint32_t g,
                                                      const uint32_t *__restrict__ s_hat, uint32_t *__restrict__ key0)
{
    const uint32_t c = blockIdx.x * kLcThreads + threadIdx.x;
    const uint32_t q = P.q[j], cr_hi = P.cr_hi[j], cr_lo = P.cr_lo[j];
    const uint64_t d = evk_diag_target<LOGN, kDiagOf<SIGMA>>(P, j, g, c, s_hat);
#pragma unroll
    for (uint32_t dg = 0; dg < 2; dg++)
    {
        uint32_t *p = key0 + ((((size_t)(2 * j + dg)) * P.nprimes + j) << LOGN) + c;
        *p          = barrett64((d << (kRelinDigitBits * dg)) + *p, q, cr_hi, cr_lo);
    }
}

// The special-prime key's diagonal on its [np - 1][np][n] slab: key0[j][j][k] += (P mod q_j) . d[k] mod q_j for a data
// prime j < np - 1, P = q_{np-1} and d as above.  (P mod q_j) d + key0 < 2^60 + 2^30.
template <int LOGN, DiagTarget TARGET>
__device__ __forceinline__ void evk_diag_sp(const DevParams &P, uint32_t j, uint32_t g,
                                            const uint32_t *__restrict__ s_hat, uint32_t *__restrict__ key0)
{
    const uint32_t c = blockIdx.x * kLcThreads + threadIdx.x;
    const uint32_t q = P.q[j], cr_hi = P.cr_hi[j], cr_lo = P.cr_lo[j];
    const uint64_t d = evk_diag_target<LOGN, TARGET>(P, j, g, c, s_hat);
    uint32_t *p      = key0 + (((size_t)j * P.nprimes + j) << LOGN) + c;
    *p               = barrett64(d * (P.q[P.nprimes - 1] % q) + *p, q, cr_hi, cr_lo);
}

template <int LOGN, bool SIGMA>
__global__ __launch_bounds__(kLcThreads) void k_evk_diag_sp(const DevParams P, uint32_t j, uint32_t g,
                                                         const uint32_t *__restrict__ s_hat, uint32_t *__restrict__ key0)
{
    evk_diag_sp<LOGN, kDiagOf<SIGMA>>(P, j, g, s_hat, key0);
}

// a switching key's diagonal: key0[j][j][k] += (P mod q_j) . s_from_hat[k], s_from_hat the NTT form mod q_j of the key it hides
template <int LOGN>
__global__ __launch_bounds__(kLcThreads) void k_evk_diag_switch_sp(const DevParams P, uint32_t j,
                                                                const uint32_t *__restrict__ s_from_hat,
                                                                uint32_t *__restrict__ key0)
{
    evk_diag_sp<LOGN, kDiagOther>(P, j, 0, s_from_hat, key0);
}

// elt 0: the relinearisation key's diagonal; else the Galois key's of that element.  sp: the special-prime key's rows.
// other: a switching key's diagonal (special-prime rows only), s_hat = the NTT form of the key it hides.
hipError_t launch_evk_diag(const DevParams &P, uint32_t j, uint32_t elt, bool sp, const uint32_t *s_hat, uint32_t *key0,
                           hipStream_t st, bool other)
{
    if (other && !sp) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value;
        const dim3 grid(P.n / kLcThreads), block(kLcThreads);
        if (other) return launch(k_evk_diag_switch_sp<L>, grid, block, 0, st, P, j, s_hat, key0);
        if (sp)
            return elt ? launch(k_evk_diag_sp<L, true>, grid, block, 0, st, P, j, elt, s_hat, key0)
                       : launch(k_evk_diag_sp<L, false>, grid, block, 0, st, P, j, elt, s_hat, key0);
        return elt ? launch(k_evk_diag<L, true>, grid, block, 0, st, P, j, elt, s_hat, key0)
                   : launch(k_evk_diag<L, false>, grid, block, 0, st, P, j, elt, s_hat, key0);
    });
}

}  // namespace seamd
