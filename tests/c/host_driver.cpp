// Host-only driver for tests/test_host_model.py: the library's host half (the seven .cpp files between the C ABI and the
// kernels) linked against a model of the HIP runtime (hip_model.cpp) and recording launch wrappers (launch_model.cpp),
// built with plain g++ under a sanitizer.  It calls the C ABI only.  Every scenario prints "== <name>" and then one line
// per fact or finding; tests/test_host_model.py judges the lines.  The exit code is non-zero on a sanitizer report only.
//   host_driver [scenario ...]      no argument: every scenario
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "hip_model.h"
#include "seal_embedded_amd.h"

namespace hm = hipmodel;

namespace {

constexpr size_t kN = 4096, kNp = 3, kB = 3, kL = 2;   // the context of most scenarios; kL: the special-prime level
constexpr size_t kRow = kN * sizeof(uint32_t);

void scenario(const char *name) { printf("== %s\n", name); }

int g_setup_failures = 0;
#define SETUP(call)                                                                                \
    do                                                                                             \
    {                                                                                              \
        const int rc_ = (int)(call);                                                               \
        if (rc_ != 0)                                                                              \
        {                                                                                          \
            printf("setup-failure %s -> %d (%s)\n", #call, rc_, se_amd_last_error());              \
            g_setup_failures++;                                                                    \
        }                                                                                          \
    } while (0)

// ---- device memory of the driver: exact allocations on the current device, released together ---------------------------
struct Pool
{
    std::vector<void *> owned;
    void *bytes(size_t b)
    {
        void *p = nullptr;
        if (hipMalloc(&p, b) != hipSuccess) printf("setup-failure hipMalloc %zu\n", b), g_setup_failures++;
        owned.push_back(p);
        return p;
    }
    uint32_t *words(size_t w) { return (uint32_t *)bytes(w * sizeof(uint32_t)); }
    uint32_t *slab(size_t records, size_t primes) { return words(records * primes * kN); }
    uint32_t *upload(std::initializer_list<uint32_t> v)
    {
        uint32_t *p = words(v.size());
        (void)hipMemcpy(p, v.begin(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        return p;
    }
    void release()
    {
        for (void *p : owned) (void)hipFree(p);
        owned.clear();
    }
};

// ---- one window of the log, judged against the caller's stream -----------------------------------------------------------
struct Counts
{
    size_t launches = 0, copies = 0, memsets = 0, blocking = 0, calls = 0, findings = 0;
};

std::string describe(const hm::Op &op) { return op.kind + "@" + hm::stream_name(op.stream); }

// S: the caller's stream (id), entry: its position when the window began, dev: the context's device.  Prints one
// "finding <name> <category> <operation>" line per defect; host-blocking calls are counted, not printed (the caller
// decides whether they are findings).
Counts judge(const char *name, size_t a, size_t b, int S, uint64_t entry, int dev, bool print_blocking = false)
{
    Counts c;
    c.calls = b - a;
    auto finding = [&](const char *category, const std::string &what) {
        printf("finding %s %s %s\n", name, category, what.c_str());
        c.findings++;
    };
    for (size_t i = a; i < b; i++)
    {
        const hm::Op op = hm::log_op(i);
        for (const std::string &v : op.violations) finding("violation", v);
        if (op.blocking)
        {
            c.blocking++;
            if (print_blocking) finding("host_blocking", describe(op));
        }
        if (!op.work) continue;
        c.launches += op.launch;
        c.copies += op.kind.find("Memcpy") != std::string::npos;
        c.memsets += op.kind.find("Memset") != std::string::npos;
        const bool null_stream = hm::is_null_stream(op.stream);
        if (null_stream) finding("null_stream", describe(op));
        if (op.stream != S && (null_stream || hm::stream_device(op.stream) != dev)) finding("off_stream", describe(op));
        if (!hm::ordered_after_entry(i, S, entry)) finding("not_after_entry", describe(op));
        if (!hm::joined(i, S)) finding("not_joined", describe(op));
        if (op.launch && op.device != dev) finding("wrong_device_launch", describe(op) + " under device " + std::to_string(op.device));
    }
    return c;
}

// ---- a context with every key, ring and plan installed (all key material zero: valid residues, valid 2-bit codes) --------
struct Fixture
{
    se_amd_ctx *ctx = nullptr;
    int dev         = 0;
    se_amd_lintrans *lt = nullptr, *lt_sp = nullptr;
    se_amd_bsgs *bs = nullptr, *bs_sp = nullptr;
    uint32_t elts[2] = {0, 0};
    Pool pool;
};

const std::vector<uint32_t> &zeros()
{
    static const std::vector<uint32_t> z((size_t)2 * 2 * 2 * kNp * kNp * kN + 64, 0u);   // the largest host key: [K=2][R=2np][np][n]
    return z;
}

void make_fixture(Fixture &f, int dev)
{
    f.dev = dev;
    SETUP(hipSetDevice(dev));
    SETUP(se_amd_create(&f.ctx, kN, kNp, dev));
    if (!f.ctx) return;
    const uint32_t *z = zeros().data();
    const uint8_t *zb = (const uint8_t *)z;
    SETUP(se_amd_galois_element(kN, 1, &f.elts[0]));
    SETUP(se_amd_galois_element(kN, 2, &f.elts[1]));
    SETUP(se_amd_set_secret_key(f.ctx, zb));
    SETUP(se_amd_set_public_key(f.ctx, z, z));
    SETUP(se_amd_set_secret_keyring(f.ctx, 2, zb));
    SETUP(se_amd_set_public_keyring(f.ctx, 2, z, z));
    SETUP(se_amd_set_relin_key(f.ctx, z, z));
    SETUP(se_amd_set_galois_keys(f.ctx, f.elts, 2, z, z));
    SETUP(se_amd_set_relin_key_sp(f.ctx, z, z));
    SETUP(se_amd_set_galois_keys_sp(f.ctx, f.elts, 2, z, z));
    SETUP(se_amd_set_switch_keyring_sp(f.ctx, 2, z, z));
    uint32_t *diag = f.pool.words(2 * 2 * kNp * kN), *diag0 = f.pool.words(kNp * kN);
    SETUP(se_amd_lintrans_create(f.ctx, f.elts, 2, diag, diag0, kNp, &f.lt));
    SETUP(se_amd_lintrans_create_sp(f.ctx, f.elts, 2, diag, diag0, kNp, &f.lt_sp));
    SETUP(se_amd_bsgs_create(f.ctx, f.elts, 2, f.elts, 2, diag, kNp, &f.bs));
    SETUP(se_amd_bsgs_create_sp(f.ctx, f.elts, 2, f.elts, 2, diag, kNp, &f.bs_sp));
}

void drop_fixture(Fixture &f)
{
    (void)hipSetDevice(f.dev);
    se_amd_lintrans_destroy(f.lt);
    se_amd_lintrans_destroy(f.lt_sp);
    se_amd_bsgs_destroy(f.bs);
    se_amd_bsgs_destroy(f.bs_sp);
    se_amd_destroy(f.ctx);
    f.pool.release();
    f = Fixture();
}

// ---- the table of stream entries -------------------------------------------------------------------------------------
// An entry is called as fn(stream, ctx, p0, primes, plan): p0 is a pointer the entry requires (its first output where it has a
// required one, else its first input), primes its level argument and plan its plan, so that the refusals scenario can
// replace each of them (and the context: every entry refuses a NULL one).  flags: N the entry refuses p0 == NULL, A it refuses p0 at 4 modulo 16, P it has a level argument
// and refuses 0 and np + 1, L it takes a plan and refuses one of another context.
struct Entry
{
    const char *name;
    const char *flags;
    se_amd_ctx *ctx;
    void *p0;
    size_t primes;
    const void *plan;
    std::function<int(void *, se_amd_ctx *, void *, size_t, const void *)> fn;
};

#define ENTRY(fname, flags, p0, primes, plan, ...)                                                                      \
    out.push_back(Entry{#fname, flags, ctx, (void *)(p0), (size_t)(primes), (const void *)(plan),                       \
                        [=](void *s, se_amd_ctx *ctx, void *p0_, size_t primes_, const void *plan_) -> int {            \
                            (void)p0_, (void)primes_, (void)plan_;                                                      \
                            return fname(__VA_ARGS__);                                                                  \
                        }})

void build_entries(Fixture &f, se_amd_poly *poly, Fixture *poly_fix, std::vector<Entry> &out)
{
    (void)hipSetDevice(f.dev);
    Pool &m         = f.pool;
    se_amd_ctx *ctx = f.ctx;
    const size_t B = kB, n = kN, np = kNp;
    float *values   = (float *)m.bytes(B * (n / 2) * sizeof(float));
    uint8_t *seeds  = (uint8_t *)m.bytes(B * 64), *share = (uint8_t *)m.bytes(B * 64), *status = (uint8_t *)m.bytes(B);
    int64_t *pte    = (int64_t *)m.bytes(B * n * sizeof(int64_t));
    float *dec_vals = (float *)m.bytes(B * (n / 2) * sizeof(float));
    double *dec_f64 = (double *)m.bytes(B * (n / 2) * sizeof(double));
    uint32_t *kidx  = m.upload({0, 1, 0});
    uint32_t *rowp  = m.upload({0, 1, 2, 3}), *idx = m.upload({0, 1, 2}), *eidx = m.upload({0, 1, 0});
    // full-level slabs [B][np][n], special-prime-level slabs [B][L][n], rows [B][n]
    uint32_t *a3 = m.slab(B, np), *b3 = m.slab(B, np), *c3 = m.slab(B, np), *o3 = m.slab(B, np), *p3 = m.slab(B, np),
             *q3 = m.slab(B, np);
    uint32_t *a2 = m.slab(B, kL), *b2 = m.slab(B, kL), *c2 = m.slab(B, kL), *o2 = m.slab(B, kL), *p2 = m.slab(B, kL);
    uint32_t *r1 = m.slab(B, 1), *r1b = m.slab(B, 1);
    uint32_t *pt1 = m.slab(1, np);
    uint32_t *stack3a = m.slab(2 * B, np), *stack3b = m.slab(2 * B, np), *many3a = m.slab(2 * B, np), *many3b = m.slab(2 * B, np);
    uint32_t *stack2a = m.slab(2 * B, kL), *stack2b = m.slab(2 * B, kL);
    uint32_t *ext_a = m.slab(2 * B, kL + 1), *ext_b = m.slab(2 * B, kL + 1), *ext_oa = m.slab(2 * B, kL + 1),
             *ext_ob = m.slab(2 * B, kL + 1);
    uint32_t *pt_sum = m.slab(2 * 2, np);   // [Gout = 2][E = 2][np][n]
    uint32_t *sum_oa = m.slab(2 * B, np), *sum_ob = m.slab(2 * B, np);
    uint64_t *ctr = (uint64_t *)m.bytes(B * 8), *ctr_out = (uint64_t *)m.bytes(B * 8);
    uint64_t *wa = (uint64_t *)m.bytes(64 * 8), *wb = (uint64_t *)m.bytes(64 * 8), *wc = (uint64_t *)m.bytes(64 * 8);
    uint32_t *wout = m.words(64);
    int8_t *codes  = (int8_t *)m.bytes(B * n), *cbd = (int8_t *)m.bytes(B * 2 * n);
    uint8_t *blocks = (uint8_t *)m.bytes(B * 136);
    const uint32_t *elts = f.elts;
    const double scale   = se_amd_scale(ctx);
    const size_t ws_bytes = se_amd_bsgs_workspace_bytes(f.bs, B, 2), ws_sp_bytes = se_amd_bsgs_workspace_bytes(f.bs_sp, B, kL);
    void *ws = m.bytes(ws_bytes), *ws_sp = m.bytes(ws_sp_bytes);
    // the affine entry's host arrays must outlive the table: static
    static const uint32_t *term0[2], *term1[2];
    static const uint32_t term_primes[2] = {3, 3};
    static const int64_t weights[2]      = {5, -7};
    term0[0] = a3, term0[1] = b3, term1[0] = c3, term1[1] = p3;

    ENTRY(se_amd_encrypt_sym_device, "N", a3, 0, 0, ctx, values, B, share, seeds, (uint32_t *)p0_, b3, c3, pte, status, s);
    ENTRY(se_amd_encrypt_sym_seeded_device, "N", a3, 0, 0, ctx, values, B, share, seeds, (uint32_t *)p0_, status, s);
    ENTRY(se_amd_expand_c1_device, "N", a3, 0, 0, ctx, share, B, (uint32_t *)p0_, s);
    ENTRY(se_amd_encrypt_asym_device, "N", a3, 0, 0, ctx, values, B, seeds, (uint32_t *)p0_, b3, c3, pte, status, s);
    ENTRY(se_amd_encrypt_sym_keyed_device, "N", a3, 0, 0, ctx, values, B, kidx, share, seeds, (uint32_t *)p0_, b3, c3, pte,
          status, s);
    ENTRY(se_amd_encrypt_asym_keyed_device, "N", a3, 0, 0, ctx, values, B, kidx, seeds, (uint32_t *)p0_, b3, c3, pte, status, s);
    ENTRY(se_amd_decrypt_decode_keyed_device, "N", a3, 0, 0, ctx, (const uint32_t *)p0_, b3, B, kidx, 1, r1, r1b, dec_vals, s);
    ENTRY(se_amd_encode_ntt_device, "N", a3, 0, 0, ctx, values, B, (uint32_t *)p0_, pte, status, s);
    ENTRY(se_amd_encode_device, "N", pte, 0, 0, ctx, values, B, (int64_t *)p0_, status, s);
    ENTRY(se_amd_ntt_device, "N", r1, 0, 0, ctx, 1, (uint32_t *)p0_, B, s);
    ENTRY(se_amd_intt_device, "N", r1, 0, 0, ctx, 1, (uint32_t *)p0_, B, s);
    ENTRY(se_amd_decrypt_decode_device, "N", a3, 0, 0, ctx, (const uint32_t *)p0_, b3, B, 1, r1, r1b, dec_vals, s);
    ENTRY(se_amd_decrypt_full_device, "N", a3, 0, 0, ctx, (const uint32_t *)p0_, b3, B, pte, dec_vals, dec_f64, status, s);
    ENTRY(se_amd_decrypt_full_keyed_device, "N", a3, 0, 0, ctx, (const uint32_t *)p0_, b3, B, kidx, pte, dec_vals, dec_f64,
          status, s);
    ENTRY(se_amd_ct_lincomb_device, "NA", o3, 0, 0, ctx, a3, b3, B, 1, nullptr, nullptr, nullptr, B, (uint32_t *)p0_, p3,
          status, s);
    ENTRY(se_amd_ct_rescale_device, "NAP", o2, 3, 0, ctx, a3, b3, B, primes_, (uint32_t *)p0_, p2, s);
    ENTRY(se_amd_ct_mul_plain_device, "NAP", o3, 3, 0, ctx, a3, b3, B, primes_, pt1, 1, np, nullptr, (uint32_t *)p0_, p3,
          status, s);
    ENTRY(se_amd_decrypt_level_device, "NP", a2, 2, 0, ctx, (const uint32_t *)p0_, b2, B, primes_, scale, pte, dec_vals, dec_f64,
          status, s);
    ENTRY(se_amd_decrypt_level_keyed_device, "NP", a2, 2, 0, ctx, (const uint32_t *)p0_, b2, B, primes_, scale, kidx, pte,
          dec_vals, dec_f64, status, s);
    ENTRY(se_amd_ct_mul_device, "NAP", o3, 3, 0, ctx, a3, b3, B, a3, b3, B, primes_, B, nullptr, nullptr, (uint32_t *)p0_, p3,
          q3, status, s);
    ENTRY(se_amd_decrypt3_level_device, "NP", a2, 2, 0, ctx, (const uint32_t *)p0_, b2, c2, B, primes_, scale, pte, dec_vals,
          dec_f64, status, s);
    ENTRY(se_amd_decrypt3_level_keyed_device, "NP", a2, 2, 0, ctx, (const uint32_t *)p0_, b2, c2, B, primes_, scale, kidx, pte,
          dec_vals, dec_f64, status, s);
    ENTRY(se_amd_ct_relin_device, "NAP", o3, 3, 0, ctx, a3, b3, c3, B, primes_, (uint32_t *)p0_, p3, s);
    ENTRY(se_amd_ct_galois_device, "NAP", o3, 3, 0, ctx, a3, b3, B, primes_, elts[0], (uint32_t *)p0_, p3, s);
    ENTRY(se_amd_ct_galois_many_device, "NAP", many3a, 3, 0, ctx, a3, b3, B, primes_, elts, 2, (uint32_t *)p0_, many3b, s);
    ENTRY(se_amd_ct_galois_sum_device, "NAP", o3, 3, 0, ctx, a3, b3, B, primes_, elts, 2, 1, (uint32_t *)p0_, p3, s);
    ENTRY(se_amd_ct_lintrans_device, "NAPL", o3, 3, f.lt, ctx, (const se_amd_lintrans *)plan_, a3, b3, B, primes_,
          (uint32_t *)p0_, p3, s);
    ENTRY(se_amd_ct_relin_sp_device, "NAP", o2, 2, 0, ctx, a2, b2, c2, B, primes_, (uint32_t *)p0_, p2, s);
    ENTRY(se_amd_ct_galois_sp_device, "NAP", o2, 2, 0, ctx, a2, b2, B, primes_, elts[0], (uint32_t *)p0_, p2, s);
    ENTRY(se_amd_ct_drop_primes_device, "NAP", o2, 3, 0, ctx, a3, b3, B, primes_, 2, (uint32_t *)p0_, p2, s);
    ENTRY(se_amd_ct_galois_sum_sp_device, "NAP", o2, 2, 0, ctx, a2, b2, B, primes_, elts, 2, 1, (uint32_t *)p0_, p2, s);
    ENTRY(se_amd_ct_lintrans_sp_device, "NAPL", o2, 2, f.lt_sp, ctx, (const se_amd_lintrans *)plan_, a2, b2, B, primes_,
          (uint32_t *)p0_, p2, s);
    ENTRY(se_amd_ct_mul_plain_sum_device, "NAP", sum_oa, 3, 0, ctx, stack3a, stack3b, 2, B, primes_, pt_sum, 2, np,
          (uint32_t *)p0_, sum_ob, s);
    ENTRY(se_amd_ct_galois_accum_device, "NAP", o3, 3, 0, ctx, stack3a, stack3b, B, primes_, elts, 2, (uint32_t *)p0_, p3, s);
    ENTRY(se_amd_ct_bsgs_device, "NAPL", o2, 2, f.bs, ctx, (const se_amd_bsgs *)plan_, a2, b2, B, primes_, (uint32_t *)p0_, p2,
          ws, ws_bytes, s);
    ENTRY(se_amd_ct_galois_many_ext_sp_device, "NAP", ext_oa, 2, 0, ctx, a2, b2, B, primes_, elts, 2, (uint32_t *)p0_, ext_ob, s);
    ENTRY(se_amd_ct_mul_plain_sum_ext_sp_device, "NAP", ext_oa, 2, 0, ctx, ext_a, ext_b, 2, B, primes_, pt_sum, 2,
          (uint32_t *)p0_, ext_ob, s);
    ENTRY(se_amd_ct_mod_down_sp_device, "NAP", o2, 2, 0, ctx, ext_a, ext_b, B, primes_, (uint32_t *)p0_, p2, s);
    ENTRY(se_amd_ct_galois_accum_sp_device, "NAP", o2, 2, 0, ctx, stack2a, stack2b, B, primes_, elts, 2, (uint32_t *)p0_, p2, s);
    ENTRY(se_amd_ct_bsgs_sp_device, "NAPL", o2, 2, f.bs_sp, ctx, (const se_amd_bsgs *)plan_, a2, b2, B, primes_,
          (uint32_t *)p0_, p2, ws_sp, ws_sp_bytes, s);
    ENTRY(se_amd_ct_switch_keyed_sp_device, "NAP", o2, 2, 0, ctx, a2, b2, B, primes_, kidx, (uint32_t *)p0_, p2, status, s);
    ENTRY(se_amd_ct_switch_sum_keyed_sp_device, "NAP", o2, 2, 0, ctx, a2, b2, B, primes_, kidx, B, rowp, idx, B,
          (uint32_t *)p0_, p2, status, s);
    ENTRY(se_amd_ct_pack_sp_device, "NAP", o2, 2, 0, ctx, a2, b2, B, primes_, elts, 2, B, rowp, idx, eidx, B, (uint32_t *)p0_,
          p2, status, s);
    ENTRY(se_amd_ct_mul_sum_device, "NAP", o3, 3, 0, ctx, a3, b3, B, a3, b3, B, primes_, B, rowp, idx, idx, B, (uint32_t *)p0_,
          p3, q3, status, s);
    ENTRY(se_amd_ct_dot_sp_device, "NAP", o2, 2, 0, ctx, a2, b2, B, a2, b2, B, primes_, B, rowp, idx, idx, B, (uint32_t *)p0_, p2,
          status, s);
    ENTRY(se_amd_ct_affine_rescale_device, "NAP", o2, 3, 0, ctx, term0, term1, term_primes, weights, 2, 9, B, primes_,
          (uint32_t *)p0_, p2, s);
    if (poly && poly_fix)
    {
        // slot-wise polynomials need np - 1 >= depth + 2 levels: a context of its own (8192 x 6, degree 3)
        (void)hipSetDevice(poly_fix->dev);
        Pool &pm         = poly_fix->pool;
        se_amd_ctx *ctx  = poly_fix->ctx;
        const size_t pn = 8192, in_primes = 5;
        size_t out_primes = 0;
        int64_t c_after   = 0;
        (void)se_amd_poly_result(poly, &out_primes, &c_after);
        uint32_t *pa = pm.words(B * in_primes * pn), *pb = pm.words(B * in_primes * pn);
        uint32_t *po = pm.words(B * out_primes * pn), *pq = pm.words(B * out_primes * pn);
        const size_t work_bytes = se_amd_poly_workspace_bytes(poly, B);
        void *work              = pm.bytes(work_bytes);
        ENTRY(se_amd_ct_poly_sp_device, "NAL", po, 0, poly, ctx, (const se_amd_poly *)plan_, pa, pb, B, work, work_bytes,
              (uint32_t *)p0_, pq, s);
        (void)hipSetDevice(f.dev);
    }
    ENTRY(se_amd_prng_blocks_device, "N", blocks, 0, 0, ctx, seeds, ctr, (uint8_t *)p0_, 136, B, s);
    ENTRY(se_amd_sample_uniform_device, "N", a3, 0, 0, ctx, seeds, ctr, B, (uint32_t *)p0_, ctr_out, s);
    ENTRY(se_amd_sample_ternary_device, "N", codes, 0, 0, ctx, seeds, B, (int8_t *)p0_, ctr_out, s);
    ENTRY(se_amd_sample_cbd_device, "N", cbd, 0, 0, ctx, seeds, ctr, B, 2, (int8_t *)p0_, s);
    ENTRY(se_amd_word_ops_device, "N", wout, 0, 0, ctx, 1, 0, wa, wb, wc, (uint32_t *)p0_, 64, s);
}

// the polynomial fixture: 8192 x 6 with the special-prime relinearisation key, and a plan of degree 3 at level 5
void make_poly_fixture(Fixture &pf, se_amd_poly **poly, int dev)
{
    pf.dev = dev;
    SETUP(hipSetDevice(dev));
    SETUP(se_amd_create(&pf.ctx, 8192, 6, dev));
    static const std::vector<uint32_t> z((size_t)5 * 6 * 8192, 0u);   // [R' = np - 1][np][n]
    if (pf.ctx) SETUP(se_amd_set_relin_key_sp(pf.ctx, z.data(), z.data()));
    const double coeff[4] = {0.5, 1.0, 0.0, -0.25};
    SETUP(se_amd_poly_create(8192, 6, 5, coeff, 3, 1073741824.0, 1073741824.0, poly));
}

hipStream_t make_stream(int dev)
{
    hipStream_t s = nullptr;
    (void)hipSetDevice(dev);
    (void)hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    return s;
}

// ---- a. streams --------------------------------------------------------------------------------------------------------
void run_streams()
{
    scenario("streams");
    const int dev = 2;
    Fixture f, pf;
    se_amd_poly *poly = nullptr;
    make_fixture(f, dev);
    make_poly_fixture(pf, &poly, dev);
    std::vector<Entry> entries;
    build_entries(f, poly, &pf, entries);
    hipStream_t S = make_stream(dev);
    const int sid = hm::stream_id(S, dev);
    void *prior   = f.pool.bytes(64);
    auto run_one = [&](const char *kind, const std::string &name, const Entry &e) {
        Counts c[2];
        int rc[2] = {0, 0};
        for (int pass = 0; pass < 2; pass++)
        {
            // the caller's own earlier work on S: what the entry must come after
            (void)hipSetDevice(dev);
            (void)hipMemsetAsync(prior, 0, 64, S);
            const uint64_t entry = hm::stream_position(sid);
            const size_t a       = hm::log_size();
            // a fresh thread: its current device is 0, not the context's
            std::thread t([&] { rc[pass] = e.fn(S, e.ctx, e.p0, e.primes, e.plan); });
            t.join();
            c[pass] = judge(name.c_str(), a, hm::log_size(), sid, entry, dev);
        }
        printf("%s %s rc=%d,%d launches=%zu copies=%zu memsets=%zu blocking_first=%zu blocking=%zu\n", kind, name.c_str(), rc[0],
               rc[1], c[1].launches, c[1].copies, c[1].memsets, c[0].blocking, c[1].blocking);
    };
    for (const Entry &e : entries) run_one("entry", e.name, e);
    // The whole-path entries choose among several launch shapes (se_amd_set_pipeline, se_amd_set_debug_flags); at this
    // batch size the default is the small-batch form.  Every other shape forks and joins the library's streams in its
    // own way, so each runs here too: fused chain, per-prime pipeline without and with the staged sampler, and both
    // without the auxiliary stream.
    struct
    {
        const char *name;
        int overlap, split;
        uint32_t flags;
    } shapes[] = {{"fused", 1, 0, 0}, {"pipeline", 1, 1, 1024}, {"staged", 1, 1, 512}, {"fused_serial", 0, 0, 0},
                  {"pipeline_serial", 0, 1, 0}};
    for (const auto &shape : shapes)
    {
        SETUP(se_amd_set_pipeline(f.ctx, shape.overlap, shape.split));
        SETUP(se_amd_set_debug_flags(f.ctx, shape.flags));
        for (const Entry &e : entries)
            if (strstr(e.name, "se_amd_encrypt_") == e.name || !strcmp(e.name, "se_amd_encode_ntt_device"))
                run_one("variant", std::string(e.name) + "/" + shape.name, e);
    }
    SETUP(se_amd_set_pipeline(f.ctx, 1, 2));
    SETUP(se_amd_set_debug_flags(f.ctx, 0));
    (void)hipSetDevice(dev);
    (void)hipStreamSynchronize(S);
    (void)hipStreamDestroy(S);
    se_amd_poly_destroy(poly);
    drop_fixture(pf);
    drop_fixture(f);
    printf("setup_failures %d\n", g_setup_failures);
    printf("live %zu %zu %zu\n", hm::live_allocations(), hm::live_streams(), hm::live_events());
}

// ---- b. refusals ---------------------------------------------------------------------------------------------------------
void run_refusals()
{
    scenario("refusals");
    const int dev = 2;
    Fixture f, other, pf;
    se_amd_poly *poly = nullptr, *other_poly = nullptr;
    make_fixture(f, dev);
    make_fixture(other, dev);   // its plans are "a plan of another context"
    make_poly_fixture(pf, &poly, dev);
    const double coeff[2] = {0.0, 1.0};
    SETUP(se_amd_poly_create(kN, kNp, 2, coeff, 1, 1073741824.0, 1073741824.0, &other_poly));   // a plan of another (n, np)
    std::vector<Entry> entries;
    build_entries(f, poly, &pf, entries);
    hipStream_t S = make_stream(dev);
    for (const Entry &e : entries)
    {
        auto refuse = [&](const char *what, void *p0, size_t primes, const void *plan, se_amd_ctx *ctx = nullptr) {
            const size_t a = hm::log_size();
            const int rc   = e.fn(S, ctx ? ctx : e.ctx, p0, primes, plan);
            printf("refusal %s %s rc=%d calls=%zu\n", e.name, what, rc, hm::log_size() - a);
        };
        const bool is_sp = strstr(e.name, "_sp_") != nullptr;
        {
            const size_t a = hm::log_size();
            const int rc   = e.fn(S, nullptr, e.p0, e.primes, e.plan);
            printf("refusal %s null_ctx rc=%d calls=%zu\n", e.name, rc, hm::log_size() - a);
        }
        if (strchr(e.flags, 'N')) refuse("null", nullptr, e.primes, e.plan);
        if (strchr(e.flags, 'A')) refuse("misaligned", (char *)e.p0 + 4, e.primes, e.plan);
        if (strchr(e.flags, 'P')) refuse("primes=0", e.p0, 0, e.plan);
        if (strchr(e.flags, 'P')) refuse("primes=np+1", e.p0, kNp + 1, e.plan);
        if (strchr(e.flags, 'P') && is_sp) refuse("primes=np", e.p0, kNp, e.plan);
        if (strchr(e.flags, 'L'))
        {
            const void *foreign = e.plan == f.lt      ? (const void *)other.lt
                                  : e.plan == f.lt_sp ? (const void *)other.lt_sp
                                  : e.plan == f.bs    ? (const void *)other.bs
                                  : e.plan == f.bs_sp ? (const void *)other.bs_sp
                                                      : (const void *)other_poly;
            refuse("foreign_plan", e.p0, e.primes, foreign);
            refuse("null_plan", e.p0, e.primes, nullptr);
        }
    }
    (void)hipSetDevice(dev);
    (void)hipStreamDestroy(S);
    se_amd_poly_destroy(poly);
    se_amd_poly_destroy(other_poly);
    drop_fixture(pf);
    drop_fixture(other);
    drop_fixture(f);
    printf("setup_failures %d\n", g_setup_failures);
}

// ---- c. lifetimes --------------------------------------------------------------------------------------------------------
struct Live
{
    size_t a, s, e;
    bool operator==(const Live &o) const { return a == o.a && s == o.s && e == o.e; }
};
Live live() { return Live{hm::live_allocations(), hm::live_streams(), hm::live_events()}; }

// create(&handle) -> rc; destroy(handle).  A good run counts the allocations; then allocation k + 1 of the create fails
// for every k, and each failed create must return an error, leave the handle NULL, bring the live counts back and be
// followed by a good create.
void lifetime(const char *name, const std::function<int(void **)> &create, const std::function<void(void *)> &destroy)
{
    const Live before = live();
    void *h           = nullptr;
    const uint64_t a0 = hm::allocations_made();
    const int rc      = create(&h);
    const uint64_t k_good = hm::allocations_made() - a0;
    destroy(h);
    printf("lifetime %s rc=%d allocations=%llu restored=%d\n", name, rc, (unsigned long long)k_good, (int)(live() == before));
    for (uint64_t k = 0; k < k_good; k++)
    {
        void *bad = (void *)0x10;   // a failed create must overwrite it with NULL
        hip_model_fail_alloc_after((long)k);
        const int frc = create(&bad);
        hip_model_fail_alloc_after(-1);
        const bool null_out = bad == nullptr;
        if (frc == 0 && bad && bad != (void *)0x10) destroy(bad);
        const bool restored = live() == before;
        void *again         = nullptr;
        const int grc       = create(&again);
        destroy(again);
        printf("failed-create %s k=%llu rc=%d null=%d restored=%d retry_rc=%d\n", name, (unsigned long long)k, frc, (int)null_out,
               (int)restored, grc);
    }
}

// A key install has no handle: on a fresh context per k, allocation k + 1 of the install fails; the install must return an
// error, a good install must follow, and destroying the context must bring the live counts back.
void install_lifetime(const char *name, size_t n, size_t np, const std::function<int(se_amd_ctx *)> &install)
{
    const Live before = live();
    auto fresh = [&]() {
        se_amd_ctx *c = nullptr;
        (void)se_amd_create(&c, n, np, 1);
        return c;
    };
    se_amd_ctx *c     = fresh();
    const uint64_t a0 = hm::allocations_made();
    const int rc      = c ? install(c) : -1;
    const uint64_t k_good = hm::allocations_made() - a0;
    const int rc2         = c ? install(c) : -1;   // a second install replaces the first
    se_amd_destroy(c);
    printf("lifetime %s rc=%d,%d allocations=%llu restored=%d\n", name, rc, rc2, (unsigned long long)k_good, (int)(live() == before));
    for (uint64_t k = 0; k < k_good; k++)
    {
        c = fresh();
        hip_model_fail_alloc_after((long)k);
        const int frc = c ? install(c) : 0;
        hip_model_fail_alloc_after(-1);
        const int grc = c ? install(c) : -1;
        se_amd_destroy(c);
        printf("failed-install %s k=%llu rc=%d retry_rc=%d restored=%d\n", name, (unsigned long long)k, frc, grc,
               (int)(live() == before));
    }
}

void run_lifetimes()
{
    scenario("lifetimes");
    const size_t log_begin = hm::log_size();
    const uint32_t *z = zeros().data();
    const uint8_t *zb = (const uint8_t *)z;
    (void)hipSetDevice(1);
    lifetime("se_amd_create", [](void **h) { return se_amd_create((se_amd_ctx **)h, 1024, 1, 1); },
             [](void *h) { se_amd_destroy((se_amd_ctx *)h); });
    lifetime("se_amd_create_4096x3", [](void **h) { return se_amd_create((se_amd_ctx **)h, kN, kNp, 3); },
             [](void *h) { se_amd_destroy((se_amd_ctx *)h); });
    {
        const int devices[4] = {0, 1, 2, 3};
        lifetime("se_amd_group_create", [&](void **h) { return se_amd_group_create((se_amd_group **)h, 1024, 1, devices, 4); },
                 [](void *h) { se_amd_group_destroy((se_amd_group *)h); });
    }
    install_lifetime("se_amd_set_secret_key", 1024, 1, [&](se_amd_ctx *c) { return se_amd_set_secret_key(c, zb); });
    install_lifetime("se_amd_set_public_key", 1024, 1, [&](se_amd_ctx *c) { return se_amd_set_public_key(c, z, z); });
    install_lifetime("se_amd_set_secret_keyring", 1024, 1, [&](se_amd_ctx *c) { return se_amd_set_secret_keyring(c, 2, zb); });
    install_lifetime("se_amd_set_public_keyring", 1024, 1, [&](se_amd_ctx *c) { return se_amd_set_public_keyring(c, 2, z, z); });
    uint32_t elts[2];
    (void)se_amd_galois_element(kN, 1, &elts[0]);
    (void)se_amd_galois_element(kN, 2, &elts[1]);
    install_lifetime("se_amd_set_relin_key", kN, kNp, [&](se_amd_ctx *c) { return se_amd_set_relin_key(c, z, z); });
    install_lifetime("se_amd_set_galois_keys", kN, kNp, [&](se_amd_ctx *c) { return se_amd_set_galois_keys(c, elts, 2, z, z); });
    install_lifetime("se_amd_set_relin_key_sp", kN, kNp, [&](se_amd_ctx *c) { return se_amd_set_relin_key_sp(c, z, z); });
    install_lifetime("se_amd_set_galois_keys_sp", kN, kNp,
                     [&](se_amd_ctx *c) { return se_amd_set_galois_keys_sp(c, elts, 2, z, z); });
    install_lifetime("se_amd_set_switch_keyring_sp", kN, kNp,
                     [&](se_amd_ctx *c) { return se_amd_set_switch_keyring_sp(c, 2, z, z); });
    {
        // plans on one context that holds the Galois keys; create -> use -> destroy
        Fixture f;
        make_fixture(f, 1);
        Pool &m        = f.pool;
        uint32_t *diag = m.words(2 * 2 * kNp * kN), *diag0 = m.words(kNp * kN);
        uint32_t *a = m.slab(kB, kL), *b = m.slab(kB, kL), *o = m.slab(kB, kL), *p = m.slab(kB, kL);
        hipStream_t S = make_stream(1);
        se_amd_ctx *ctx = f.ctx;
        const uint32_t *e = f.elts;
        lifetime("se_amd_lintrans_create",
                 [&](void **h) {
                     const int rc = se_amd_lintrans_create(ctx, e, 2, diag, diag0, kNp, (se_amd_lintrans **)h);
                     if (rc == 0) (void)se_amd_ct_lintrans_device(ctx, (se_amd_lintrans *)*h, a, b, kB, kL, o, p, S);
                     return rc;
                 },
                 [](void *h) { se_amd_lintrans_destroy((se_amd_lintrans *)h); });
        lifetime("se_amd_lintrans_create_sp",
                 [&](void **h) {
                     const int rc = se_amd_lintrans_create_sp(ctx, e, 2, diag, diag0, kNp, (se_amd_lintrans **)h);
                     if (rc == 0) (void)se_amd_ct_lintrans_sp_device(ctx, (se_amd_lintrans *)*h, a, b, kB, kL, o, p, S);
                     return rc;
                 },
                 [](void *h) { se_amd_lintrans_destroy((se_amd_lintrans *)h); });
        lifetime("se_amd_bsgs_create",
                 [&](void **h) { return se_amd_bsgs_create(ctx, e, 2, e, 2, diag, kNp, (se_amd_bsgs **)h); },
                 [](void *h) { se_amd_bsgs_destroy((se_amd_bsgs *)h); });
        lifetime("se_amd_bsgs_create_sp",
                 [&](void **h) { return se_amd_bsgs_create_sp(ctx, e, 2, e, 2, diag, kNp, (se_amd_bsgs **)h); },
                 [](void *h) { se_amd_bsgs_destroy((se_amd_bsgs *)h); });
        (void)hipStreamSynchronize(S);
        (void)hipStreamDestroy(S);
        drop_fixture(f);
    }
    {
        const double coeff[4] = {0.5, 1.0, 0.0, -0.25};
        lifetime("se_amd_poly_create",
                 [&](void **h) { return se_amd_poly_create(8192, 6, 5, coeff, 3, 1073741824.0, 1073741824.0, (se_amd_poly **)h); },
                 [](void *h) { se_amd_poly_destroy((se_amd_poly *)h); });
    }
    printf("setup_failures %d\n", g_setup_failures);
    printf("live %zu %zu %zu\n", hm::live_allocations(), hm::live_streams(), hm::live_events());
    printf("violations %zu\n", hm::violations(log_begin, hm::log_size()).size());
}

// ---- d. workspace --------------------------------------------------------------------------------------------------------
// Every pointer and extent of the window that falls into allocation `serial` must stay inside its `bytes`.
void workspace_uses(const char *name, size_t a, size_t b, const void *ws, size_t bytes)
{
    size_t uses = 0, reach = 0, outside = 0;
    for (size_t i = a; i < b; i++)
    {
        const hm::Op op = hm::log_op(i);
        if (!op.work) continue;
        for (const hm::PtrUse &u : op.ptrs)
        {
            const uintptr_t p = (uintptr_t)u.p, w = (uintptr_t)ws;
            if (!u.p || p + u.bytes <= w || p >= w + bytes + 4096) continue;   // not near the workspace
            uses++;
            if (p < w || p + u.bytes > w + bytes)
            {
                outside++;
                printf("finding %s outside_workspace %s %s offset %zd bytes %zu of %zu\n", name, op.kind.c_str(), u.name.c_str(),
                       (ssize_t)(p - w), u.bytes, bytes);
            }
            else if (p + u.bytes - w > reach)
                reach = p + u.bytes - w;
        }
    }
    printf("workspace %s bytes=%zu uses=%zu reach=%zu outside=%zu\n", name, bytes, uses, reach, outside);
}

void run_workspace()
{
    scenario("workspace");
    const int dev = 2;
    Fixture f, pf;
    se_amd_poly *poly = nullptr;
    make_fixture(f, dev);
    make_poly_fixture(pf, &poly, dev);
    hipStream_t S = make_stream(dev);
    const int sid = hm::stream_id(S, dev);
    Pool &m       = f.pool;
    uint32_t *a = m.slab(kB, kL), *b = m.slab(kB, kL), *o = m.slab(kB, kL), *p = m.slab(kB, kL);
    auto run = [&](const char *name, size_t bytes, int expect_refusal, const std::function<int(void *, size_t)> &call) {
        (void)hipSetDevice(dev);
        void *ws = nullptr;
        (void)hipMalloc(&ws, bytes);
        const uint64_t entry = hm::stream_position(sid);
        const size_t a0      = hm::log_size();
        const int rc         = call(ws, bytes);
        const size_t b0      = hm::log_size();
        if (expect_refusal)
            printf("refusal %s rc=%d calls=%zu\n", name, rc, b0 - a0);
        else
        {
            const Counts c = judge(name, a0, b0, sid, entry, dev);
            printf("call %s rc=%d launches=%zu copies=%zu\n", name, rc, c.launches, c.copies);
            workspace_uses(name, a0, b0, ws, bytes);
        }
        (void)hipStreamSynchronize(S);
        (void)hipFree(ws);
    };
    (void)hipMemsetAsync(a, 0, 64, S);
    auto bsgs    = [&](void *ws, size_t bytes) { return se_amd_ct_bsgs_device(f.ctx, f.bs, a, b, kB, kL, o, p, ws, bytes, S); };
    auto bsgs_sp = [&](void *ws, size_t bytes) { return se_amd_ct_bsgs_sp_device(f.ctx, f.bs_sp, a, b, kB, kL, o, p, ws, bytes, S); };
    // the whole batch at once, then one record at a time (the header: chunks of workspace_bytes / per-record records), then
    // 16 bytes less than one record, which the header refuses
    run("se_amd_ct_bsgs_device", se_amd_bsgs_workspace_bytes(f.bs, kB, kL), 0, bsgs);
    run("se_amd_ct_bsgs_device/one_record", se_amd_bsgs_workspace_bytes(f.bs, 1, kL), 0, bsgs);
    run("se_amd_ct_bsgs_device/short", se_amd_bsgs_workspace_bytes(f.bs, 1, kL) - 16, 1, bsgs);
    run("se_amd_ct_bsgs_sp_device", se_amd_bsgs_workspace_bytes(f.bs_sp, kB, kL), 0, bsgs_sp);
    run("se_amd_ct_bsgs_sp_device/one_record", se_amd_bsgs_workspace_bytes(f.bs_sp, 1, kL), 0, bsgs_sp);
    run("se_amd_ct_bsgs_sp_device/short", se_amd_bsgs_workspace_bytes(f.bs_sp, 1, kL) - 16, 1, bsgs_sp);
    if (poly && pf.ctx)
    {
        size_t out_primes = 0;
        int64_t c_after   = 0;
        (void)se_amd_poly_result(poly, &out_primes, &c_after);
        Pool &pm     = pf.pool;
        uint32_t *pa = pm.words(kB * 5 * 8192), *pb = pm.words(kB * 5 * 8192);
        uint32_t *po = pm.words(kB * out_primes * 8192), *pq = pm.words(kB * out_primes * 8192);
        auto polyc = [&](void *ws, size_t bytes) { return se_amd_ct_poly_sp_device(pf.ctx, poly, pa, pb, kB, ws, bytes, po, pq, S); };
        run("se_amd_ct_poly_sp_device", se_amd_poly_workspace_bytes(poly, kB), 0, polyc);
        run("se_amd_ct_poly_sp_device/short", se_amd_poly_workspace_bytes(poly, kB) - 16, 1, polyc);
    }
    (void)hipStreamDestroy(S);
    se_amd_poly_destroy(poly);
    drop_fixture(pf);
    drop_fixture(f);
    printf("setup_failures %d\n", g_setup_failures);
}

// ---- e. group ------------------------------------------------------------------------------------------------------------
void run_group()
{
    scenario("group");
    const int devices[4] = {0, 1, 2, 3};
    se_amd_group *g      = nullptr;
    SETUP(se_amd_group_create(&g, kN, kNp, devices, 4));
    if (!g) return;
    const uint32_t *z = zeros().data();
    SETUP(se_amd_group_set_secret_key(g, (const uint8_t *)z));
    SETUP(se_amd_group_set_public_key(g, z, z));
    const size_t rec = kNp * kN;
    for (int mode = 0; mode < 3; mode++)
        for (size_t B : {(size_t)10, (size_t)3})
            for (int root : {-1, 1})
            {
                const char *names[3] = {"se_amd_encrypt_sym_multi_device", "se_amd_encrypt_asym_multi_device",
                                        "se_amd_encode_ntt_multi_device"};
                char name[96];
                snprintf(name, sizeof(name), "%s/B=%zu/root=%d", names[mode], B, root);
                size_t first[4], count[4];
                SETUP(se_amd_group_partition(g, B, first, count));
                Pool pools[4];
                const float *values[4]   = {};
                const uint8_t *seeds[4]  = {}, *share[4] = {};
                uint32_t *c0[4] = {}, *c1[4] = {};
                uint8_t *status[4] = {};
                uint32_t *all0 = nullptr, *all1 = nullptr;
                if (root >= 0)
                {
                    (void)hipSetDevice(devices[root]);
                    all0 = pools[root].words(B * rec), all1 = pools[root].words(B * rec);
                }
                for (int i = 0; i < 4; i++)
                {
                    if (!count[i]) continue;   // a member without units gets no buffers at all
                    (void)hipSetDevice(devices[i]);
                    values[i] = (const float *)pools[i].bytes(count[i] * (kN / 2) * sizeof(float));
                    seeds[i]  = (const uint8_t *)pools[i].bytes(count[i] * 64);
                    share[i]  = (const uint8_t *)pools[i].bytes(count[i] * 64);
                    status[i] = (uint8_t *)pools[i].bytes(count[i]);
                    // the root produces in place in its slice of the slab; the others in buffers of their own
                    c0[i] = i == root ? all0 + first[i] * rec : pools[i].words(count[i] * rec);
                    c1[i] = i == root ? all1 + first[i] * rec : pools[i].words(count[i] * rec);
                }
                (void)hipSetDevice(0);
                const size_t a = hm::log_size();
                int rc;
                if (mode == 0)
                    rc = se_amd_encrypt_sym_multi_device(g, B, values, share, seeds, c0, c1, status, root, all0, all1);
                else if (mode == 1)
                    rc = se_amd_encrypt_asym_multi_device(g, B, values, seeds, c0, c1, status, root, all0, all1);
                else
                    rc = se_amd_encode_ntt_multi_device(g, B, values, c0, status, root, all0);
                const size_t b = hm::log_size();
                size_t launches[4] = {}, peers = 0, findings = 0;
                auto finding = [&](const char *category, const std::string &what) {
                    printf("finding %s %s %s\n", name, category, what.c_str());
                    findings++;
                };
                for (size_t i = a; i < b; i++)
                {
                    const hm::Op op = hm::log_op(i);
                    for (const std::string &v : op.violations) finding("violation", v);
                    if (!op.work) continue;
                    const int member = op.device;   // the devices are distinct: the current device names the member
                    launches[member] += op.launch;
                    if (hm::is_null_stream(op.stream)) finding("null_stream", describe(op));
                    if (hm::stream_device(op.stream) != op.device) finding("off_stream", describe(op));
                    if (!hm::joined_host(i)) finding("in_flight_at_return", describe(op));
                    if (op.peer_dst < 0)
                    {
                        for (const hm::PtrUse &u : op.ptrs)
                            if (u.alloc_dev >= 0 && u.alloc_dev != op.device) finding("foreign_pointer", describe(op) + " " + u.name);
                        continue;
                    }
                    peers++;
                    const hm::PtrUse &dst = op.ptrs[0];
                    const bool in_all1    = all1 && (uintptr_t)dst.p >= (uintptr_t)all1 && (uintptr_t)dst.p < (uintptr_t)(all1 + B * rec);
                    const uint32_t *slab  = in_all1 ? all1 : all0;
                    if (root < 0 || op.peer_dst != devices[root] || op.peer_src != op.device)
                        finding("peer_devices", describe(op) + " names " + std::to_string(op.peer_src) + "->" + std::to_string(op.peer_dst));
                    if ((const uint32_t *)dst.p != slab + first[member] * rec || dst.bytes != count[member] * rec * sizeof(uint32_t))
                        finding("peer_slice", describe(op) + " of member " + std::to_string(member));
                }
                for (int i = 0; i < 4; i++)
                    if ((launches[i] > 0) != (count[i] > 0)) finding("member_launches", "member " + std::to_string(i));
                const size_t expect_peers = root < 0 ? 0 : (mode == 2 ? 1 : 2) * ((B < 4 ? B : 4) - 1);
                printf("group %s rc=%d launches=%zu,%zu,%zu,%zu peer_copies=%zu expected_peer_copies=%zu findings=%zu\n", name, rc,
                       launches[0], launches[1], launches[2], launches[3], peers, expect_peers, findings);
                for (int i = 0; i < 4; i++)
                {
                    (void)hipSetDevice(devices[i]);
                    pools[i].release();
                }
            }
    se_amd_group_destroy(g);
    printf("setup_failures %d\n", g_setup_failures);
    printf("live %zu %zu %zu\n", hm::live_allocations(), hm::live_streams(), hm::live_events());
}

// ---- f. batch --------------------------------------------------------------------------------------------------------
// se_encrypt_batch on host pointers over $SE_AMD_DEVICES = 0,1,2 (one thread per device).  With the test-hooks build of
// se_api.cpp and $SE_AMD_INJECT_SHARD_FAILURE the shard of that device is lost and re-run on another.
void run_batch()
{
    scenario("batch");
    const char *dir = getenv("SE_AMD_DATA_PATH");
    if (!dir)
    {
        printf("setup-failure SE_AMD_DATA_PATH is not set\n");
        return;
    }
    setenv("SE_AMD_DEVICES", "0,1,2", 1);
    const std::vector<uint8_t> sk(kN / 4, 0);
    SETUP(se_amd_save_secret_key_file(dir, kN, sk.data()));
    SE_PARMS *parms = se_setup(kN, kNp, 33554432.0, SE_SYM_ENCR);
    const size_t B  = 7;
    std::vector<float> values(B * (kN / 2), 1.0f);
    std::vector<uint8_t> seeds(B * 64, 1), share(B * 64, 2);
    std::vector<uint32_t> c0(B * kNp * kN, 0xFFFFFFFFu), c1(B * kNp * kN, 0xFFFFFFFFu);
    const size_t a = hm::log_size();
    const int rc   = se_encrypt_batch(parms, values.data(), B, share.data(), seeds.data(), c0.data(), c1.data());
    const size_t b = hm::log_size();
    size_t launches[8] = {}, findings = 0, untouched = 0;
    for (size_t i = a; i < b; i++)
    {
        const hm::Op op = hm::log_op(i);
        for (const std::string &v : op.violations) printf("finding se_encrypt_batch violation %s\n", v.c_str()), findings++;
        if (!op.work) continue;
        launches[op.device] += op.launch;
        if (hm::is_null_stream(op.stream) && !op.blocking) printf("finding se_encrypt_batch null_stream %s\n", describe(op).c_str()), findings++;
        if (hm::stream_device(op.stream) != op.device) printf("finding se_encrypt_batch off_stream %s\n", describe(op).c_str()), findings++;
        if (!hm::joined_host(i)) printf("finding se_encrypt_batch in_flight_at_return %s\n", describe(op).c_str()), findings++;
    }
    // the model's device memory is all zero, so every record a device delivered is all zero: a sentinel word left is a
    // record nobody delivered
    for (uint32_t w : c0) untouched += w == 0xFFFFFFFFu;
    for (uint32_t w : c1) untouched += w == 0xFFFFFFFFu;
    printf("batch rc=%d launches=%zu,%zu,%zu,%zu undelivered_words=%zu findings=%zu\n", rc, launches[0], launches[1], launches[2],
           launches[3], untouched, findings);
    se_cleanup(parms);
    printf("setup_failures %d\n", g_setup_failures);
    printf("live %zu %zu %zu\n", hm::live_allocations(), hm::live_streams(), hm::live_events());
}

// ---- two threads, two entries, one context (the thread sanitizer's scenario) -----------------------------------------------
void run_threads()
{
    scenario("threads");
    const int dev = 2;
    Fixture f;
    make_fixture(f, dev);
    Pool &m = f.pool;
    hipStream_t S[2] = {make_stream(dev), make_stream(dev)};
    float *values  = (float *)m.bytes(kB * (kN / 2) * sizeof(float));
    uint8_t *seeds = (uint8_t *)m.bytes(kB * 64), *share = (uint8_t *)m.bytes(kB * 64);
    uint32_t *c0 = m.slab(kB, kNp), *c1 = m.slab(kB, kNp), *in0 = m.slab(kB, kNp), *out0 = m.slab(kB, kNp - 1);
    uint32_t *l0 = m.slab(kB, kNp), *lo = m.slab(1, kNp);
    const size_t a = hm::log_size();
    int rcs[2]     = {0, 0};
    std::thread t0([&] {
        for (int k = 0; k < 3 && !rcs[0]; k++)
            rcs[0] = se_amd_encrypt_sym_device(f.ctx, values, kB, share, seeds, c0, c1, nullptr, nullptr, nullptr, S[0]);
    });
    std::thread t1([&] {
        for (int k = 0; k < 3 && !rcs[1]; k++)
        {
            rcs[1] = se_amd_ct_rescale_device(f.ctx, in0, nullptr, kB, kNp, out0, nullptr, S[1]);
            if (!rcs[1]) rcs[1] = se_amd_ct_lincomb_device(f.ctx, l0, nullptr, kB, 1, nullptr, nullptr, nullptr, kB, lo, nullptr, nullptr, S[1]);
        }
    });
    t0.join();
    t1.join();
    size_t findings = 0;
    for (const std::string &v : hm::violations(a, hm::log_size())) printf("finding threads violation %s\n", v.c_str()), findings++;
    (void)hipSetDevice(dev);
    for (hipStream_t s : S) (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s);
    printf("threads rc=%d,%d findings=%zu\n", rcs[0], rcs[1], findings);
    drop_fixture(f);
    printf("setup_failures %d\n", g_setup_failures);
}

// ---- g. selftest: wrong sequences straight at the model ------------------------------------------------------------------
void run_selftest()
{
    scenario("selftest");
    const int dev = 2;
    (void)hipSetDevice(dev);
    hipStream_t S = make_stream(dev), aux = make_stream(dev);
    const int sid = hm::stream_id(S, dev);
    hipEvent_t fork = nullptr, join = nullptr;
    (void)hipEventCreateWithFlags(&fork, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&join, hipEventDisableTiming);
    void *buf = nullptr, *other = nullptr;
    (void)hipMalloc(&buf, 256);
    (void)hipSetDevice(1);
    (void)hipMalloc(&other, 256);
    (void)hipSetDevice(dev);
    auto window = [&](const char *name, const std::function<void()> &body) {
        (void)hipMemsetAsync(buf, 0, 16, S);   // the caller's earlier work
        const uint64_t entry = hm::stream_position(sid);
        const size_t a       = hm::log_size();
        body();
        const Counts c = judge(name, a, hm::log_size(), sid, entry, dev, true);
        printf("selftest %s findings=%zu\n", name, c.findings);
    };
    window("good_fork_join", [&] {
        (void)hipEventRecord(fork, S);
        (void)hipStreamWaitEvent(aux, fork, 0);
        (void)hm::record_launch("launch_selftest", aux, {hm::ptr("buf", buf, 256)});
        (void)hipEventRecord(join, aux);
        (void)hipStreamWaitEvent(S, join, 0);
        (void)hm::record_launch("launch_selftest", S, {hm::ptr("buf", buf, 256)});
    });
    window("launch_on_null_stream", [&] { (void)hm::record_launch("launch_selftest", nullptr, {hm::ptr("buf", buf, 256)}); });
    window("aux_never_joined", [&] {
        (void)hipEventRecord(fork, S);
        (void)hipStreamWaitEvent(aux, fork, 0);
        (void)hm::record_launch("launch_selftest", aux, {hm::ptr("buf", buf, 256)});
    });
    window("launch_before_fork", [&] {
        (void)hm::record_launch("launch_selftest", aux, {hm::ptr("buf", buf, 256)});
        (void)hipEventRecord(fork, S);
        (void)hipStreamWaitEvent(aux, fork, 0);
        (void)hipEventRecord(join, aux);
        (void)hipStreamWaitEvent(S, join, 0);
    });
    window("pointer_of_other_device", [&] { (void)hm::record_launch("launch_selftest", S, {hm::ptr("other", other, 256)}); });
    window("copy_past_allocation", [&] { (void)hipMemcpyAsync(buf, (char *)buf + 128, 192, hipMemcpyDeviceToDevice, S); });
    window("free_of_unknown_pointer", [&] { (void)hipFree((char *)buf + 64); });
    window("launch_under_wrong_device", [&] {
        std::thread t([&] { (void)hm::record_launch("launch_selftest", S, {hm::ptr("buf", buf, 256)}); });   // device 0
        t.join();
    });
    window("host_blocking_call", [&] { (void)hipStreamSynchronize(S); });
    (void)hipStreamSynchronize(aux);
    (void)hipFree(buf);
    (void)hipEventDestroy(fork);
    (void)hipEventDestroy(join);
    (void)hipStreamDestroy(S);
    (void)hipStreamDestroy(aux);
    // `other` is left alive on purpose: the live count must show it
    printf("live %zu %zu %zu\n", hm::live_allocations(), hm::live_streams(), hm::live_events());
    (void)hipSetDevice(1);
    (void)hipFree(other);
    printf("live %zu %zu %zu\n", hm::live_allocations(), hm::live_streams(), hm::live_events());
}

}  // namespace

int main(int argc, char **argv)
{
    setvbuf(stdout, nullptr, _IOLBF, 0);
    struct
    {
        const char *name;
        void (*run)();
    } all[] = {{"selftest", run_selftest}, {"streams", run_streams},     {"refusals", run_refusals}, {"lifetimes", run_lifetimes},
               {"workspace", run_workspace}, {"group", run_group},       {"batch", run_batch},       {"threads", run_threads}};
    for (auto &s : all)
    {
        bool wanted = argc < 2;
        for (int i = 1; i < argc; i++) wanted = wanted || strcmp(argv[i], s.name) == 0;
        if (wanted) s.run();
    }
    scenario("end");
    printf("done\n");
    return 0;
}
