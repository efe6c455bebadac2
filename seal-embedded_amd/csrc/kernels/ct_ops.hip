// ct_ops.hip -- key-free operations on resident ciphertext slabs: weighted sums of records (se_amd_ct_lincomb_device).
//
// A slab is uint32 [record][prime][coeff] in NTT form, so a linear combination of records is element-wise arithmetic
// mod q_j: no transform, no key, no table.  Unlike the rest of the tree these kernels are bound by HBM, not by VALU
// issue: every input row is read once per use and every output row written once.
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

}  // namespace seamd
