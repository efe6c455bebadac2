// ct_pack.hip -- slot packing: se_amd_ct_pack_sp_device (PackSpArgs).  Many records become one, each rotated by its own
// element, under the installed special-prime Galois keys:
//   out[g] = sum_{k in row g} rot_{elt[eidx[k]]}(record idx[k]),
// with the motif of the switch-key ring (ct_switch_sp, ct_ops.hip): the undivided key-switch terms of a whole CSR row are
// accumulated and divided by P ONCE.  The body is ct_switch_sp<LOGN, SUM> in its geometry -- one workgroup of n/16 threads
// per (output row, output prime i < L), LDS the exchange plane alone, no scratch, no global temporary, one launch -- with
// three changes:
//   the element: sp_row_digit<LOGN, true> and load_row_sigma<LOGN, true> are driven by the ENTRY's element elt[eidx[k]];
//   the key:     the block of that element, A.key[eidx[k]] (resolved on the host, in the argument block), not a ring slot;
//   identity:    an entry whose element is 1 needs no key and no key switch: it is skipped in both passes and both of its
//                rows join the divided sums as they lie.
//   row:    the entries [lo, hi) and their validity, decided before anything of the row is written: every record index is
//           compared with B and every element index with E before either forms an address (the record's rows, A.elt[.] and
//           A.key[.]).  All of these depend on blockIdx and the loop counters alone: they are wave-uniform, and so is the
//           choice between a rotated and an identity entry.  An invalid row (status 2) and an empty one (status 1) are all
//           zero.
//   pass 0: per rotated entry and input row j: sp_row_digit mod P (sigma of the entry's element in the coefficient domain)
//           -> evk_mac against row j, column p of THAT element's key;   then sp_delta once for the row;
//   pass 1: the entries again against column i (row i of an entry enters through load_row_sigma, without a transform);
//   epilogue: . P^-1; the c1 rows of the identity entries join acc1 and out1 is stored, then the rows sigma_k(c0[b_k])[i]
//           (as they lie for an identity entry) are added into the divided acc0 one at a time -- exact, canonical after
//           every step, and no third accumulator tile.
// Transforms per workgroup for a row of m rotated entries: (2 L - 1) m INTTs and as many NTTs, and 4 for the two deltas:
// (4 L - 2) m + 4, against (4 L + 2) m for m single rotations and a sum; the rotated records never touch memory.
// Lazy ranges: evk_mac's range argument (ct_ops.hip, above k_ct_relin) does not depend on the number of terms, so it
// covers a row of any length; pass 1 enters in (0, 2 q_i] as in ct_key_switch_sp.  A row of one rotated entry runs the
// operations of k_ct_galois_sp in their order: the same bits.  A row of identity entries only leaves the accumulators 0:
// delta = 0, ks = 0, the plain modular sum.  A long row is not sliced: it runs on L workgroups (pack in groups, then
// se_amd_ct_lincomb_device over the group results).
// Addresses: as in k_ct_galois (LDS addresses formed from elements the host has checked -- odd, below 2n -- and masked to
// [0, n)); no word of a slab or of a key is used as an address.
// grid evk_grid(rows, L).
#include "ct_keyswitch.cuh"

namespace seamd {

template <int LOGN, bool SUM>
__global__ __launch_bounds__(XformGeom<LOGN>::THREADS) void k_ct_pack_sp(const DevParams P, const DevTables T,
                                                                      const RescaleParams R, const PackSpArgs A)
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
    const uint32_t *__restrict__ idx  = A.idx;
    const uint32_t *__restrict__ eidx = A.eidx;
    auto record_of = [&](uint32_t e) -> uint32_t {
        if constexpr (SUM)
            return idx[e];
        else
            return e;
    };
    // the element index of a validated entry: the same word in every lane, so it indexes the argument block as a scalar
    auto element_of = [&](uint32_t e) -> uint32_t { return __builtin_amdgcn_readfirstlane(eidx[e]); };

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
        for (uint32_t e = lo; e < hi && !bad; e++) bad = record_of(e) >= A.B || eidx[e] >= A.G;
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
#pragma unroll 1
            for (uint32_t e = lo; e < hi; e++)
            {
                const uint32_t s   = element_of(e);
                const uint32_t elt = A.elt[s];
                if (elt == 1) continue;   // the identity: no key, no key switch
                const uint32_t *sw = A.c1 + record_of(e) * words;
                const uint32_t *kc = A.key[s] + (size_t)col * 2 * N;   // column col of key row 0
                for (uint32_t j = 0; j < A.primes; j++)
                {
                    uint32_t y[16];
                    if (pass && j == i)
                        load_row_sigma<LOGN, true>(y, sw + (size_t)i * N, elt, lds, opaque_index(t));
                    else
                        sp_row_digit<LOGN, true>(y, sw + (size_t)j * N, j, elt, q, rw, P, T, lds, t);
                    const uint32_t *key = kc + (size_t)j * A.np * 2 * N + quad_index(opaque_index(t), 0);
                    evk_mac<LOGN>(acc0, acc1, y, key, A.half, q);
                    __syncthreads();
                }
            }
            if (pass == 0) sp_delta<LOGN>(acc0, acc1, i, sp, P, T, lds, t);
        }
        // ks_k = acc_k . P^-1; out1 leaves first, with the c1 rows of the identity entries, then the c0 rows join the
        // divided acc0
        const uint32_t w = R.inv[i], wp = R.inv_sh[i];
#pragma unroll
        for (int e = 0; e < 16; e++) acc1[e] = csub(mul_shoup_lazy(acc1[e], w, wp, qi), qi);
#pragma unroll 1
        for (uint32_t e = lo; e < hi; e++)
        {
            if (A.elt[element_of(e)] != 1) continue;
            uint32_t c[16];
            load_quads(c, A.c1 + record_of(e) * words + (size_t)i * N, te);
#pragma unroll
            for (int k = 0; k < 16; k++) acc1[k] = csub(acc1[k] + c[k], qi);
        }
        store_quads(A.out1 + o, acc1, te);
#pragma unroll
        for (int e = 0; e < 16; e++) acc0[e] = csub(mul_shoup_lazy(acc0[e], w, wp, qi), qi);
#pragma unroll 1
        for (uint32_t e = lo; e < hi; e++)
        {
            const uint32_t elt  = A.elt[element_of(e)];
            const uint32_t *row = A.c0 + record_of(e) * words + (size_t)i * N;
            uint32_t c[16];
            if (elt != 1)
            {
                load_row_sigma<LOGN, true>(c, row, elt, lds, te);
#pragma unroll
                for (int k = 0; k < 16; k++) acc0[k] = csub(acc0[k] + c[k], qi);
                __syncthreads();   // the next park, or the next row's first transpose, writes the plane the gather reads
            }
            else
            {
                load_quads(c, row, te);
#pragma unroll
                for (int k = 0; k < 16; k++) acc0[k] = csub(acc0[k] + c[k], qi);
            }
        }
        store_quads(A.out0 + o, acc0, te);
        if (A.status && i == 0 && t == 0) A.status[g] = 1;
    }
}

// row_ptr set: the CSR form.  LOGN 12 .. 14, as launch_ct_key_switch_sp.
hipError_t launch_ct_pack_sp(const DevParams &P, const DevTables &T, const RescaleParams &R, const PackSpArgs &A,
                             hipStream_t st)
{
    if (A.rows == 0) return hipSuccess;
    if (P.logn < 12) return hipErrorInvalidValue;
    return for_logn(P.logn, [&](auto l) {
        constexpr int L = decltype(l)::value < 12 ? 12 : decltype(l)::value;
        using G         = XformGeom<L>;
        const dim3 grid    = evk_grid(A.rows, A.primes);
        const size_t plane = (size_t)G::SLOTS * sizeof(uint32_t);
        return A.row_ptr ? launch(k_ct_pack_sp<L, true>, grid, dim3(G::THREADS), plane, st, P, T, R, A)
                         : launch(k_ct_pack_sp<L, false>, grid, dim3(G::THREADS), plane, st, P, T, R, A);
    });
}

}  // namespace seamd
