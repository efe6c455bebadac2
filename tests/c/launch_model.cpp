// launch_model.cpp -- the 55 launch wrappers of seal-embedded_amd/csrc/kernels/kernel_args.h against the model runtime
// (hip_model.h).  A wrapper launches nothing: it records its name, the stream, the current device and every pointer
// field of its argument block, and -- where kernel_args.h states a slab's shape in fields the block carries -- the byte
// extent, which the model holds against the allocation.  Device memory stays all zero, except for the status bytes that
// the three encode launches set (mark_encoded): no other host path needs a kernel's result to finish.
#include <string.h>

#include <vector>

#include "hip_model.h"
#include "kernels/kernel_args.h"

namespace seamd {
namespace {

using hipmodel::PtrArg;

constexpr size_t kW = sizeof(uint32_t);

struct Rec
{
    const char *name;
    std::vector<PtrArg> v;
    explicit Rec(const char *n) : name(n) {}
    Rec &ptr(const char *field, const void *p, size_t bytes = 0)
    {
        v.push_back(PtrArg{field, p, bytes});
        return *this;
    }
    Rec &tables(const DevTables &T)
    {
        return ptr("dt.inv_map", T.inv_map)
            .ptr("dt.ifft_w", T.ifft_w)
            .ptr("dt.ntt_rw", T.ntt_rw)
            .ptr("dt.s_hat", T.s_hat)
            .ptr("dt.pk0", T.pk0)
            .ptr("dt.pk1", T.pk1)
            .ptr("dt.intt_rw", T.intt_rw)
            .ptr("dt.index_map", T.index_map)
            .ptr("dt.gather_map", T.gather_map);
    }
    Rec &ring(const KeyRing *r, size_t B)
    {
        if (!r) return *this;
        return ptr("ring.k0", r->k0).ptr("ring.k1", r->k1).ptr("ring.idx", r->idx, B * kW);
    }
    Rec &enc(const EncArgs &A, size_t B, size_t n)
    {
        return ptr("values", A.values, B * (n / 2) * sizeof(float))
            .ptr("err", A.err)
            .ptr("ucodes", A.ucodes)
            .ptr("c0", A.c0)
            .ptr("c1", A.c1)
            .ptr("ntt_pte", A.ntt_pte)
            .ptr("pte", A.pte, B * n * sizeof(int64_t))
            .ptr("status", A.status, B)
            .ptr("general", A.general)
            .ptr("compact", A.compact);
    }
    Rec &uniform(const UniformArgs &A)
    {
        return ptr("seeds", A.seeds, (size_t)A.B * kSeedBytes)
            .ptr("ctr_in", A.ctr_in)
            .ptr("ctr_out", A.ctr_out)
            .ptr("out", A.out)
            .ptr("rej_list", A.rej_list)
            .ptr("spec", A.spec)
            .ptr("only_from", A.only_from)
            .ptr("prime_of", A.prime_of)
            .ptr("nrej", A.nrej)
            .ptr("flagged", A.flagged);
    }
    // the element-set block: slabs without extents (they differ per kernel), the key block of every listed element
    Rec &set(const GaloisSetArgs &A, size_t in_rec, size_t out_rec, size_t n)
    {
        ptr("c0", A.c0, in_rec * A.primes * n * kW).ptr("c1", A.c1, in_rec * A.primes * n * kW);
        ptr("out0", A.out0, out_rec * n * kW).ptr("out1", A.out1, out_rec * n * kW);
        for (uint32_t e = 0; e < A.G && e < kMaxGaloisKeys; e++) ptr("key[e]", A.key[e], A.key[e] ? 2 * A.half * kW : 0);
        return *this;
    }
    hipError_t on(hipStream_t s) { return hipmodel::record_launch(name, s, v.data(), v.size()); }
};

// The one value a host path needs from a kernel: the host-pointer entries count the status bytes that are 0 (encode
// overflow) into their return code, so an all-zero status would make every good batch return B.  1 = encoded.
void mark_encoded(const EncArgs &A, size_t B)
{
    if (A.status) memset(A.status, 1, B);
}

}  // namespace

hipError_t launch_encode_encrypt(const DevParams &P, const DevTables &T, const EncArgs &A, int, size_t B, hipStream_t s,
                                 const KeyRing *ring)
{
    const size_t slab = B * P.nprimes * P.n * kW;
    const hipError_t e =
        Rec("launch_encode_encrypt").tables(T).enc(A, B, P.n).ptr("c0[B][np][n]", A.c0, slab).ptr("c1[B][np][n]", A.c1, slab)
            .ptr("ntt_pte[B][np][n]", A.ntt_pte, slab).ring(ring, B).on(s);
    mark_encoded(A, B);
    return e;
}
hipError_t launch_encode_rns(const DevParams &P, const DevTables &T, const EncArgs &A, bool, size_t B, hipStream_t s)
{
    mark_encoded(A, B);
    return Rec("launch_encode_rns").tables(T).enc(A, B, P.n).on(s);
}
hipError_t launch_ntt_fuse(const DevParams &P, const DevTables &T, const EncArgs &A, int, int, size_t B, hipStream_t s,
                           const KeyRing *ring)
{
    mark_encoded(A, B);
    return Rec("launch_ntt_fuse").tables(T).enc(A, B, P.n).ring(ring, B).on(s);
}
hipError_t launch_decrypt_decode(const DevParams &P, const DevTables &T, const uint32_t *c0, const uint32_t *c1,
                                 uint32_t in_primes, int, uint32_t *dec_ntt, uint32_t *pt, float *values, size_t B,
                                 hipStream_t s, const KeyRing *ring)
{
    const size_t row = P.n * kW;
    return Rec("launch_decrypt_decode").tables(T).ptr("c0", c0, B * in_primes * row).ptr("c1", c1, B * in_primes * row)
        .ptr("dec_ntt", dec_ntt, B * row).ptr("pt", pt, B * row).ptr("values", values, B * (P.n / 2) * sizeof(float))
        .ring(ring, B).on(s);
}
hipError_t launch_decrypt_full(const DevParams &P, const DevTables &T, const CrtParams &, const FullArgs &A, size_t B,
                               hipStream_t s, const KeyRing *ring)
{
    const size_t slab = B * P.nprimes * P.n * kW;
    return Rec("launch_decrypt_full").tables(T).ptr("c0", A.c0, slab).ptr("c1", A.c1, slab).ptr("c2", A.c2, slab)
        .ptr("pte", A.pte, B * P.n * sizeof(int64_t)).ptr("values", A.values, B * (P.n / 2) * sizeof(float))
        .ptr("values_f64", A.values_f64, B * (P.n / 2) * sizeof(double)).ptr("status", A.status, B).ring(ring, B).on(s);
}
hipError_t launch_ct_lincomb(const DevParams &P, const LincombArgs &A, uint32_t, hipStream_t s)
{
    const size_t row = (size_t)P.nprimes * P.n * kW;
    return Rec("launch_ct_lincomb").ptr("in0", A.in0, A.B * row).ptr("in1", A.in1, A.B * row).ptr("out0", A.out0, A.G * row)
        .ptr("out1", A.out1, A.G * row).ptr("row_ptr", A.row_ptr, (A.G + 1) * kW).ptr("idx", A.idx, A.nnz * kW)
        .ptr("w", A.w, A.nnz * sizeof(int32_t)).ptr("status", A.status, A.G).ptr("part", A.part).ptr("flag", A.flag).on(s);
}
static hipError_t rescale_like(const char *name, const DevParams &P, const DevTables &T, const RescaleArgs &A, size_t B,
                               hipStream_t s)
{
    const size_t row = P.n * kW;
    return Rec(name).tables(T).ptr("in0", A.in0, B * A.primes * row).ptr("in1", A.in1, B * A.primes * row)
        .ptr("out0", A.out0, B * (A.primes - 1) * row).ptr("out1", A.out1, B * (A.primes - 1) * row).on(s);
}
hipError_t launch_ct_rescale(const DevParams &P, const DevTables &T, const RescaleParams &, const RescaleArgs &A, size_t B,
                             hipStream_t s)
{
    return rescale_like("launch_ct_rescale", P, T, A, B, s);
}
hipError_t launch_ct_mod_down_sp(const DevParams &P, const DevTables &T, const RescaleParams &, const RescaleArgs &A,
                                 size_t B, hipStream_t s)
{
    return rescale_like("launch_ct_mod_down_sp", P, T, A, B, s);
}
hipError_t launch_ct_mul_plain(const DevParams &P, const MulPlainArgs &A, hipStream_t s)
{
    const size_t slab = (size_t)A.B * A.primes * P.n * kW;
    return Rec("launch_ct_mul_plain").ptr("in0", A.in0, slab).ptr("in1", A.in1, slab).ptr("out0", A.out0, slab)
        .ptr("out1", A.out1, slab).ptr("pt", A.pt, (size_t)A.P * A.pt_primes * P.n * kW).ptr("pt_idx", A.pt_idx, A.B * kW)
        .ptr("status", A.status, A.B).on(s);
}
hipError_t launch_ct_mul(const DevParams &P, const MulArgs &A, hipStream_t s)
{
    const size_t rec = (size_t)A.primes * P.n * kW;
    return Rec("launch_ct_mul").ptr("a0", A.a0, A.Ba * rec).ptr("a1", A.a1, A.Ba * rec).ptr("b0", A.b0, A.Bb * rec)
        .ptr("b1", A.b1, A.Bb * rec).ptr("ia", A.ia, A.P * kW).ptr("ib", A.ib, A.P * kW).ptr("out0", A.out0, A.P * rec)
        .ptr("out1", A.out1, A.P * rec).ptr("out2", A.out2, A.P * rec).ptr("status", A.status, A.P).on(s);
}
static Rec mul_sum(const char *name, const DevParams &P, const MulSumArgs &A)
{
    const size_t rec = (size_t)A.primes * P.n * kW;
    Rec r(name);
    r.ptr("a0", A.a0, A.Ba * rec).ptr("a1", A.a1, A.Ba * rec).ptr("b0", A.b0, A.Bb * rec).ptr("b1", A.b1, A.Bb * rec)
        .ptr("row_ptr", A.row_ptr, ((size_t)A.G + 1) * kW).ptr("ia", A.ia, A.nnz * kW).ptr("ib", A.ib, A.nnz * kW)
        .ptr("out0", A.out0, A.G * rec).ptr("out1", A.out1, A.G * rec).ptr("out2", A.out2, A.G * rec)
        .ptr("status", A.status, A.G).ptr("key", A.key, A.key ? 2 * A.half * kW : 0);
    return r;
}
hipError_t launch_ct_mul_sum(const DevParams &P, const MulSumArgs &A, hipStream_t s)
{
    return mul_sum("launch_ct_mul_sum", P, A).on(s);
}
hipError_t launch_ct_dot_sp(const DevParams &P, const DevTables &T, const RescaleParams &, const MulSumArgs &A, hipStream_t s)
{
    return mul_sum("launch_ct_dot_sp", P, A).tables(T).on(s);
}
hipError_t launch_ct_relin(const DevParams &P, const DevTables &T, const RelinArgs &A, hipStream_t s)
{
    const size_t slab = A.B * A.primes * P.n * kW;
    return Rec("launch_ct_relin").tables(T).ptr("d0", A.d0, slab).ptr("d1", A.d1, slab).ptr("d2", A.d2, slab)
        .ptr("out0", A.out0, slab).ptr("out1", A.out1, slab).ptr("key", A.key, 2 * A.half * kW).on(s);
}
hipError_t launch_ct_galois(const DevParams &P, const DevTables &T, const GaloisArgs &A, hipStream_t s)
{
    const size_t slab = A.B * A.primes * P.n * kW;
    return Rec("launch_ct_galois").tables(T).ptr("c0", A.c0, slab).ptr("c1", A.c1, slab).ptr("out0", A.out0, slab)
        .ptr("out1", A.out1, slab).ptr("key", A.key, 2 * A.half * kW).on(s);
}
hipError_t launch_ct_key_switch_sp(const DevParams &P, const DevTables &T, const RescaleParams &, const KeySwitchSpArgs &A,
                                   hipStream_t s)
{
    const size_t slab = A.B * A.primes * P.n * kW;
    return Rec("launch_ct_key_switch_sp").tables(T).ptr("a0", A.a0, slab).ptr("a1", A.a1, A.a1 ? slab : 0).ptr("sw", A.sw, slab)
        .ptr("out0", A.out0, slab).ptr("out1", A.out1, slab).ptr("key", A.key, 2 * A.half * kW).on(s);
}
hipError_t launch_ct_switch_sp(const DevParams &P, const DevTables &T, const RescaleParams &, const SwitchSpArgs &A,
                               hipStream_t s)
{
    const size_t rec = (size_t)A.primes * P.n * kW;
    return Rec("launch_ct_switch_sp").tables(T).ptr("c0", A.c0, A.B * rec).ptr("c1", A.c1, A.B * rec)
        .ptr("out0", A.out0, A.rows * rec).ptr("out1", A.out1, A.rows * rec).ptr("ring", A.ring, A.K * A.stride * kW)
        .ptr("key_idx", A.key_idx, A.B * kW).ptr("row_ptr", A.row_ptr, (A.rows + 1) * kW).ptr("idx", A.idx, A.nnz * kW)
        .ptr("status", A.status, A.rows).on(s);
}
hipError_t launch_ct_galois_hoist(const DevParams &P, const DevTables &T, const GaloisHoistArgs &A, hipStream_t s)
{
    return Rec("launch_ct_galois_hoist").tables(T).set(A, A.B, (A.sum ? 1 : A.G) * A.B * A.primes, P.n).on(s);
}
hipError_t launch_ct_lintrans(const DevParams &P, const DevTables &T, const LintransArgs &A, hipStream_t s)
{
    const size_t pair = (size_t)A.np * 2 * P.n * kW;
    return Rec("launch_ct_lintrans").tables(T).set(A, A.B, A.B * A.primes, P.n).ptr("diag", A.diag, A.G * pair)
        .ptr("diag0", A.diag0, pair).on(s);
}
hipError_t launch_ct_hoist_sp(const DevParams &P, const DevTables &T, const RescaleParams &, const HoistSpArgs &A,
                              hipStream_t s)
{
    const size_t pair = (size_t)A.np * 2 * P.n * kW;
    return Rec("launch_ct_hoist_sp").tables(T).set(A, A.B, A.B * A.primes, P.n).ptr("diag", A.diag, A.weighted ? A.G * pair : 0)
        .ptr("diag0", A.diag0, pair).on(s);
}
hipError_t launch_lintrans_fold(const DevParams &P, const uint32_t *key_in, uint32_t *key_out, size_t rows,
                                const uint32_t *diag_in, uint32_t *pair_out, uint32_t pt, hipStream_t s)
{
    const size_t block = 2 * rows * P.nprimes * 2 * P.n * kW;
    return Rec("launch_lintrans_fold").ptr("key_in", key_in, block).ptr("key_out", key_out, key_in ? block : 0)
        .ptr("diag_in", diag_in, (size_t)pt * P.n * kW).ptr("pair_out", pair_out, (size_t)P.nprimes * 2 * P.n * kW).on(s);
}
hipError_t launch_ct_mul_plain_sum(const DevParams &P, const MulPlainSumArgs &A, hipStream_t s)
{
    const size_t rec = (size_t)A.B * A.primes * P.n * kW;
    return Rec("launch_ct_mul_plain_sum").ptr("in0", A.in0, A.E * rec).ptr("in1", A.in1, A.E * rec)
        .ptr("pt", A.pt, (size_t)A.Gout * A.E * A.pt_primes * P.n * kW).ptr("out0", A.out0, A.Gout * rec)
        .ptr("out1", A.out1, A.Gout * rec).on(s);
}
hipError_t launch_ct_galois_accum(const DevParams &P, const DevTables &T, const GaloisSetArgs &A, hipStream_t s)
{
    return Rec("launch_ct_galois_accum").tables(T).set(A, A.G * A.B, A.B * A.primes, P.n).on(s);
}
hipError_t launch_ct_galois_many_ext_sp(const DevParams &P, const DevTables &T, const GaloisSetArgs &A, hipStream_t s)
{
    return Rec("launch_ct_galois_many_ext_sp").tables(T).set(A, A.B, A.G * A.B * (A.primes + 1), P.n).on(s);
}
hipError_t launch_ct_galois_accum_sp(const DevParams &P, const DevTables &T, const RescaleParams &, const GaloisSetArgs &A,
                                     hipStream_t s)
{
    return Rec("launch_ct_galois_accum_sp").tables(T).set(A, A.G * A.B, A.B * A.primes, P.n).on(s);
}
hipError_t launch_ct_pack_sp(const DevParams &P, const DevTables &T, const RescaleParams &, const PackSpArgs &A,
                             hipStream_t s)
{
    return Rec("launch_ct_pack_sp").tables(T).set(A, A.B, A.rows * A.primes, P.n).ptr("row_ptr", A.row_ptr, (A.rows + 1) * kW)
        .ptr("idx", A.idx, A.nnz * kW).ptr("eidx", A.eidx, A.nnz * kW).ptr("status", A.status, A.rows).on(s);
}
hipError_t launch_ct_affine_rescale(const DevParams &P, const DevTables &T, const RescaleParams &,
                                    const AffineRescaleArgs &A, size_t B, hipStream_t s)
{
    Rec r("launch_ct_affine_rescale");
    r.tables(T);
    for (uint32_t t = 0; t < A.T && t < kAffineMaxTerms; t++)
    {
        const size_t slab = B * A.term_primes[t] * P.n * kW;
        r.ptr("term0[t]", A.term0[t], slab).ptr("term1[t]", A.term1[t], slab);
    }
    const size_t out = B * (A.primes - 1) * P.n * kW;
    return r.ptr("out0", A.out0, out).ptr("out1", A.out1, out).on(s);
}
hipError_t launch_row_iota(uint32_t *out, size_t count, hipStream_t s)
{
    return Rec("launch_row_iota").ptr("out", out, count * kW).on(s);
}
hipError_t launch_bsgs_permute(const DevParams &P, const uint32_t *in, uint32_t *out, size_t rows, uint32_t, hipStream_t s)
{
    return Rec("launch_bsgs_permute").ptr("in", in, rows * P.n * kW).ptr("out", out, rows * P.n * kW).on(s);
}
hipError_t launch_relin_key_rows(const DevParams &P, const uint32_t *in, uint32_t *out, size_t rows, hipStream_t s)
{
    const size_t words = rows * P.nprimes * P.n;
    return Rec("launch_relin_key_rows").ptr("in", in, words * kW).ptr("out", out, 2 * words * kW).on(s);
}
hipError_t launch_evk_diag(const DevParams &P, uint32_t, uint32_t, bool, const uint32_t *s_hat, uint32_t *key0,
                           hipStream_t s, bool)
{
    return Rec("launch_evk_diag").ptr("s_hat", s_hat, P.n * kW).ptr("key0", key0).on(s);
}
hipError_t launch_ring_secret_ntt(const DevParams &P, const DevTables &T, int, const uint8_t *packed, uint32_t *ring,
                                  size_t K, hipStream_t s)
{
    return Rec("launch_ring_secret_ntt").tables(T).ptr("packed", packed, K * (P.n / 4)).ptr("ring", ring).on(s);
}
hipError_t launch_ring_pairs(const DevParams &P, const uint32_t *vals, uint32_t *pairs, size_t K, hipStream_t s)
{
    const size_t words = K * P.nprimes * P.n;
    return Rec("launch_ring_pairs").ptr("vals", vals, words * kW).ptr("pairs", pairs, 2 * words * kW).on(s);
}
hipError_t launch_key_sanitize(const uint32_t *raw, uint32_t *idx, uint32_t *bad, size_t, size_t B, hipStream_t s)
{
    return Rec("launch_key_sanitize").ptr("raw", raw, B * kW).ptr("idx", idx, B * kW).ptr("bad", bad, (B + 1) * kW).on(s);
}
hipError_t launch_key_reject(const DevParams &, const KeyRejectArgs &A, size_t B, hipStream_t s)
{
    Rec r("launch_key_reject");
    r.ptr("bad", A.bad, (B + 1) * kW).ptr("status", A.status, B);
    for (int i = 0; i < 3; i++) r.ptr("rows[i]", A.rows[i], B * A.words[i] * kW);
    return r.on(s);
}
hipError_t launch_reduce_small(const DevParams &, const int8_t *e, uint32_t *out, size_t count, hipStream_t s)
{
    return Rec("launch_reduce_small").ptr("e", e, count).ptr("out", out, count * kW).on(s);
}
hipError_t launch_ntt_polys(const DevParams &P, const DevTables &T, int, uint32_t *polys, uint32_t *pairs, size_t count,
                            hipStream_t s)
{
    return Rec("launch_ntt_polys").tables(T).ptr("polys", polys, count * P.n * kW).ptr("pairs", pairs, 2 * count * P.n * kW).on(s);
}
hipError_t launch_make_pairs(const uint32_t *vals, uint32_t *pairs, uint32_t, size_t count, hipStream_t s)
{
    return Rec("launch_make_pairs").ptr("vals", vals, count * kW).ptr("pairs", pairs, 2 * count * kW).on(s);
}
hipError_t launch_sample_uniform(const DevParams &, const UniformArgs &A, hipStream_t s)
{
    return Rec("launch_sample_uniform").uniform(A).on(s);
}
hipError_t launch_uniform_bulk_pair(const DevParams &, const UniformArgs &A, hipStream_t s)
{
    return Rec("launch_uniform_bulk_pair").uniform(A).on(s);
}
hipError_t launch_uniform_candidates(const UniformArgs &A, hipStream_t s)
{
    return Rec("launch_uniform_candidates").uniform(A).on(s);
}
hipError_t launch_uniform_resolve(const DevParams &, const UniformArgs &A, hipStream_t s)
{
    return Rec("launch_uniform_resolve").uniform(A).on(s);
}
hipError_t launch_spec_setup(const SpecPlan &plan, const uint8_t *seeds, uint8_t *seeds_v, uint64_t *ctr_v,
                             uint8_t *prime_v, hipStream_t s)
{
    return Rec("launch_spec_setup").ptr("seeds", seeds, (size_t)plan.B * kSeedBytes)
        .ptr("seeds_v", seeds_v, (size_t)plan.total * kSeedBytes).ptr("ctr_v", ctr_v, plan.total * sizeof(uint64_t))
        .ptr("prime_v", prime_v, plan.total).on(s);
}
hipError_t launch_spec_select(const SpecPlan &plan, uint32_t n, uint64_t *ctr0, const uint64_t *ctrout_v,
                              const uint32_t *rows, uint32_t *c1, uint32_t *fail, hipStream_t s)
{
    return Rec("launch_spec_select").ptr("ctr0", ctr0, plan.B * sizeof(uint64_t))
        .ptr("ctrout_v", ctrout_v, plan.total * sizeof(uint64_t)).ptr("rows", rows, (size_t)plan.total * n * kW)
        .ptr("c1", c1, (size_t)plan.B * plan.nprimes * n * kW).ptr("fail", fail).on(s);
}
hipError_t launch_fft_polys(const DevParams &P, const DevTables &T, const FftArgs &A, size_t count, hipStream_t s)
{
    const size_t cplx = count * P.n * 2 * sizeof(double);
    return Rec("launch_fft_polys").tables(T).ptr("in", A.in, cplx).ptr("out_cplx", A.out_cplx, cplx)
        .ptr("out_int", A.out_int, count * P.n * sizeof(int64_t)).ptr("fail_idx", A.fail_idx, count * kW).on(s);
}
hipError_t launch_reduce_poly(const DevParams &, int, const int64_t *pte, const int8_t *e, uint32_t *out, bool, size_t total,
                              hipStream_t s)
{
    return Rec("launch_reduce_poly").ptr("pte", pte, pte ? total * sizeof(int64_t) : 0).ptr("e", e, e ? total : 0)
        .ptr("out", out, total * kW).on(s);
}
hipError_t launch_word_ops(const DevParams &, int, int, const uint64_t *a, const uint64_t *b, const uint64_t *c,
                           uint32_t *out, size_t count, hipStream_t s)
{
    return Rec("launch_word_ops").ptr("a", a, count * 8).ptr("b", b, count * 8).ptr("c", c, count * 8)
        .ptr("out", out, count * kW).on(s);
}
hipError_t launch_add_small(int64_t *m, const int8_t *e, size_t total, hipStream_t s)
{
    return Rec("launch_add_small").ptr("m", m, total * sizeof(int64_t)).ptr("e", e, total).on(s);
}
hipError_t launch_pack_ternary(const int8_t *codes, uint8_t *packed, size_t total_bytes, hipStream_t s)
{
    return Rec("launch_pack_ternary").ptr("codes", codes, 4 * total_bytes).ptr("packed", packed, total_bytes).on(s);
}
hipError_t launch_ternary_words(const uint32_t *in, uint32_t *out, uint32_t *nrej, uint32_t, uint32_t, int, hipStream_t s)
{
    return Rec("launch_ternary_words").ptr("in", in).ptr("out", out).ptr("nrej", nrej).on(s);
}
hipError_t launch_expand_ternary(const uint8_t *packed, uint32_t *out, uint32_t, uint32_t n, hipStream_t s)
{
    return Rec("launch_expand_ternary").ptr("packed", packed, n / 4).ptr("out", out, n * kW).on(s);
}
hipError_t launch_lower_sym_prime(const DevParams &, const DevTables &T, const LowerSymArgs &A, size_t, hipStream_t s)
{
    return Rec("launch_lower_sym_prime").tables(T).ptr("s_small", A.s_small).ptr("pte", A.pte).ptr("ep", A.ep).ptr("a", A.a)
        .ptr("c0", A.c0).ptr("ntt_pte", A.ntt_pte).ptr("s_save", A.s_save).on(s);
}
hipError_t launch_lower_asym_prime(const DevParams &P, const DevTables &T, const LowerAsymArgs &A, size_t count,
                                   hipStream_t s)
{
    const size_t row = count * P.n * kW;
    return Rec("launch_lower_asym_prime").tables(T).ptr("u_small", A.u_small, count * (P.n / 4)).ptr("e1", A.e1, count * P.n)
        .ptr("pte", A.pte, count * P.n * sizeof(int64_t)).ptr("pk0", A.pk0, row).ptr("pk1", A.pk1, row).ptr("c0", A.c0, row)
        .ptr("c1", A.c1, row).ptr("ntt_pte", A.ntt_pte, row).ptr("ntt_u_save", A.ntt_u_save, row)
        .ptr("ntt_e1_save", A.ntt_e1_save, row).on(s);
}
hipError_t launch_sample_cbd(const CbdArgs &A, hipStream_t s)
{
    return Rec("launch_sample_cbd").ptr("seeds", A.seeds, (size_t)A.B * kSeedBytes).ptr("ctr_base", A.ctr_base)
        .ptr("out", A.out).on(s);
}
hipError_t launch_sample_ternary(const TernaryArgs &A, hipStream_t s)
{
    return Rec("launch_sample_ternary").ptr("seeds", A.seeds, (size_t)A.B * kSeedBytes).ptr("codes", A.codes, (size_t)A.B * A.n)
        .ptr("ctr_out", A.ctr_out, A.B * sizeof(uint64_t)).ptr("ctr_in", A.ctr_in, A.B * sizeof(uint64_t)).on(s);
}
hipError_t launch_prng_blocks(const uint8_t *seeds, const uint64_t *ctrs, uint8_t *out, uint32_t outlen, uint32_t count,
                              hipStream_t s)
{
    return Rec("launch_prng_blocks").ptr("seeds", seeds, (size_t)count * kSeedBytes).ptr("ctrs", ctrs, count * sizeof(uint64_t))
        .ptr("out", out, (size_t)count * outlen).on(s);
}

}  // namespace seamd
