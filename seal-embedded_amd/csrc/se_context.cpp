// se_context.cpp -- GPU context: table upload, key preparation, scratch, and the kernel chains of
// the whole-path entry points.
//
// Kernel chains (no host synchronisation inside; an auxiliary stream of the context runs the kernels
// that do not depend on each other side by side and is joined back into the caller's stream):
//   symmetric  (ckks_sym.c:181-301):  [k_sample_cbd || k_sample_uniform(a -> c1)] -> k_encode_encrypt,
//                                      or the per-prime software pipeline k_encode_rns / k_ntt_fuse
//                                      beside the per-prime uniform sampler (encrypt_sym below)
//   asymmetric (ckks_asym.c:173-286): k_sample_ternary(u, counter) -> k_sample_cbd(e0|e1 at
//                                      counter base) -> k_encode_encrypt
//   encode-only (BASELINE config 5):  k_encode_encrypt<EncodeOnly>
#include "se_context.h"
#include "se_hostpipe.h"

#include <algorithm>
#include <math.h>
#include <stdio.h>
#include <string.h>

namespace seamd {

static thread_local std::string g_last_error;

void set_last_error(const std::string &msg) { g_last_error = msg; }
const std::string &last_error() { return g_last_error; }

int hip_fail(hipError_t e, const char *what)
{
    char buf[512];
    snprintf(buf, sizeof(buf), "HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    set_last_error(buf);
    return kErrHip;
}

// ---- checks the key setters and the ct_* entries share --------------------------------------------------------------
// Two [rows][np][n] slabs of residues, column i of a row modulo q_i: the first row of either that holds a word >= its
// prime, or `rows` when every word is reduced.
static size_t first_unreduced_row(const HostParams &hp, const uint32_t *s0, const uint32_t *s1, size_t rows)
{
    const size_t n = hp.n, np = hp.nprimes;
    for (size_t r = 0; r < rows; r++)
        for (size_t i = 0; i < np; i++)
        {
            const uint32_t q   = hp.q[i];
            const uint32_t *r0 = s0 + (r * np + i) * n, *r1 = s1 + (r * np + i) * n;
            uint32_t bad       = 0;
            for (size_t c = 0; c < n; c++) bad |= (uint32_t)(r0[c] >= q) | (uint32_t)(r1[c] >= q);
            if (bad) return r;
        }
    return rows;
}

// 2-bit packed secret keys: the first byte with both bits of some field set (code 3), or `bytes` when there is none.
static size_t first_code3(const uint8_t *packed, size_t bytes)
{
    size_t i = 0;
    while (i < bytes && !(packed[i] & (packed[i] >> 1) & 0x55u)) i++;
    return i;
}

// every pointer 16-byte aligned (NULL is): the quad loads and stores of the ct_* kernels
static bool aligned16(std::initializer_list<const void *> ptrs)
{
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= (uintptr_t)p;
    return !(bits & 15);
}

Context::~Context()
{
    // nothing may still use the scratch when the members wipe and free it (the auxiliary streams are non-blocking)
    (void)hipSetDevice(device);
    host_pipe.reset();
    (void)hipDeviceSynchronize();
}

int Context::init(size_t n, size_t nprimes, int dev)
{
    int rc = host_params_init(hp, n, nprimes);
    if (rc != 0)
    {
        set_last_error("unsupported parameter set (degree, nprimes)");
        return kErrInvalid;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    {
        set_last_error("no HIP device available: this library has no CPU path");
        return kErrNoDevice;
    }
    if (dev < 0 || dev >= count)
    {
        set_last_error("device index out of range");
        return kErrInvalid;
    }
    device = dev;
    SEAMD_HIP(hipSetDevice(device));
    if (hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        num_cus <= 0)
        num_cus = 256;
    // SE_AMD_NUM_CUS=<k>: plan launches as if the device had k CUs (a CPX / partial partition seen from the
    // dispatch logic; tests of the small-device limits).  Never more than the device has.
    if (const char *e = getenv("SE_AMD_NUM_CUS"))
    {
        const int k = atoi(e);
        if (k > 0 && k < num_cus) num_cus = k;
    }
    // SE_AMD_STAGED=0|1 / SE_AMD_SPECULATION=0|1: override the form the dispatch would pick (the thresholds were
    // measured on one 256-CU MI355X and are scaled by the CU count; results are bit-identical either way)
    // (kept in members of their own: se_amd_set_debug_flags assigns the whole debug_flags field)
    if (const char *e = getenv("SE_AMD_STAGED")) staged_mode = atoi(e) ? 1 : 0;
    if (const char *e = getenv("SE_AMD_SPECULATION")) spec_mode = atoi(e) ? 1 : 0;
    dp         = to_dev_params(hp);
    dp.num_cus = (uint32_t)num_cus;
    crt        = host_crt_params(hp);
    rej_cap = (uint32_t)(n / 16 > 256 ? n / 16 : 256);
    // rej_cap >= 3x the expected rejections per polynomial; spec_cap ~ mean + >5 sigma of the draws
    // speculation capacity: the helper waves compute this many candidates per polynomial WHILE the
    // chains squeeze n*4/136 blocks, and the chains wait for them -- more than the chains need is
    // pure critical path.  mean + 4 sigma of the draws per polynomial (30-bit primes: reject
    // probability 0.0186; draws beyond the capacity go through the pooled loop), multiple of 16.
    {
        const double mean = (double)n * 0.0186 * 1.02;
        uint32_t cap      = (uint32_t)(mean + 4.0 * sqrt((double)n * 0.0186) + 15.0) & ~15u;
        spec_cap          = n <= 2048 ? 32u : cap;
    }

    std::vector<uint16_t> inv;
    host_index_map(hp, index_map, inv);
    std::vector<double> w;
    host_ifft_twiddles(hp, w);
    // every table is followed by the thread-major copy of its window-0 entries (se_types.h)
    const size_t tl = xform_table_len(n), th = n / 16;
    auto append_thread_major = [&](auto *tab) {   // tab: [tl][2], first n pairs filled
        for (int b = 0; b < 4; b++)
            for (size_t g = 0; g < ((size_t)1 << (3 - b)); g++)
                for (size_t t = 0; t < th; t++)
                {
                    const size_t src = (n >> (b + 1)) + (t << (3 - b)) + g;
                    const size_t dst = n + ((8u >> b) - 1 + g) * th + t;
                    tab[2 * dst] = tab[2 * src], tab[2 * dst + 1] = tab[2 * src + 1];
                }
    };
    w.resize(2 * tl);
    append_thread_major(w.data());
    std::vector<uint32_t> rw_all(2 * tl * nprimes), rw;
    for (size_t j = 0; j < nprimes; j++)
    {
        host_ntt_root_pairs(hp, j, rw);
        // the device table holds (-root mod 2^32, shoup(root)): the forward butterfly then needs no
        // separate negation (ct_butterfly, modarith.cuh)
        for (size_t i = 0; i < n; i++) rw[2 * i] = 0u - rw[2 * i];
        memcpy(rw_all.data() + 2 * tl * j, rw.data(), 2 * n * sizeof(uint32_t));
        append_thread_major(rw_all.data() + 2 * tl * j);
    }
    SEAMD_HIP(d_inv_map.grow(n));
    SEAMD_HIP(d_ifft_w.grow(w.size()));
    SEAMD_HIP(d_ntt_rw.grow(rw_all.size()));
    SEAMD_HIP(hipMemcpy(d_inv_map, inv.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice));
    SEAMD_HIP(hipMemcpy(d_ifft_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    SEAMD_HIP(hipMemcpy(d_ntt_rw, rw_all.data(), rw_all.size() * sizeof(uint32_t),
                        hipMemcpyHostToDevice));
    SEAMD_HIP(aux_stream.create(hipStreamNonBlocking));
    for (Event *e : {&ev_fork, &ev_join, &ev_cbd, &ev_enc, &ev_done}) SEAMD_HIP(e->create(hipEventDisableTiming));
    for (Event &e : ev_prime) SEAMD_HIP(e.create(hipEventDisableTiming));
    {
        std::vector<uint32_t> irw_all(2 * n * nprimes), irw;
        for (size_t j = 0; j < nprimes; j++)
        {
            host_intt_root_pairs(hp, j, irw);
            memcpy(irw_all.data() + 2 * n * j, irw.data(), 2 * n * sizeof(uint32_t));
        }
        SEAMD_HIP(d_intt_rw.grow(irw_all.size()));
        SEAMD_HIP(hipMemcpy(d_intt_rw, irw_all.data(), irw_all.size() * sizeof(uint32_t),
                            hipMemcpyHostToDevice));
        SEAMD_HIP(d_map.grow(n));
        SEAMD_HIP(hipMemcpy(d_map, index_map.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice));
        dt.intt_rw   = d_intt_rw;
        dt.index_map = d_map;
    }
    {
        std::vector<uint16_t> gather(n);
        // point k = 16 t + e is entry e % 8 of the uint4 at [e / 8][t]
        for (size_t k = 0; k < n; k++)
        {
            const size_t t = k >> 4, e = k & 15;
            gather[((e >> 3) * (n / 16) + t) * 8 + (e & 7)] =
                (uint16_t)sv_slot((uint32_t)(inv[k] & (n / 2 - 1)), (uint32_t)hp.logn);
        }
        SEAMD_HIP(d_gather.grow(n));
        SEAMD_HIP(hipMemcpy(d_gather, gather.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice));
        dt.gather_map = d_gather;
    }
    dt.inv_map = d_inv_map;
    dt.ifft_w  = d_ifft_w;
    dt.ntt_rw  = d_ntt_rw;
    return 0;
}

// The fused kernel's list of declined plaintexts (kernel_args.h, EncArgs::general): 4 bytes per plaintext.
int Context::ensure_general(size_t B)
{
    if (B < d_general.size()) return 0;
    SEAMD_HIP(hipSetDevice(device));
    SEAMD_HIP(hipDeviceSynchronize());
    SEAMD_HIP(d_general.grow(B + 1));
    return 0;
}

// The keyed calls' clamped indices and list of out-of-range records: 8 bytes per record.
int Context::ensure_keyed(size_t B)
{
    if (B <= d_kidx.size() && B < d_kbad.size()) return 0;
    SEAMD_HIP(hipSetDevice(device));
    SEAMD_HIP(hipDeviceSynchronize());
    SEAMD_HIP(d_kidx.grow(B));
    SEAMD_HIP(d_kbad.grow(B + 1));
    return 0;
}

int Context::ensure_scratch(size_t B, size_t rows)
{
    if (int rc = ensure_general(B)) return rc;
    // d_err / d_ucodes / d_ctr are per real ciphertext; the reject lists and speculation rows are
    // also needed by the virtual ciphertexts of the small-batch path, which need nothing else
    if (rows < B) rows = B;
    const size_t n = hp.n, rej = rows * (rej_cap ? rej_cap : 1), spec = rows * spec_cap;
    if (d_err.size() >= B * 2 * n && d_ucodes.size() >= B * n && d_ctr.size() >= B && d_compact.size() >= B &&
        d_nrej.size() >= B && d_flagged.size() > B && d_rej.size() >= rej && d_spec.size() >= spec)
        return 0;
    SEAMD_HIP(hipSetDevice(device));
    SEAMD_HIP(hipDeviceSynchronize());
    SEAMD_HIP(d_err.grow(B * 2 * n));
    SEAMD_HIP(d_ucodes.grow(B * n));
    SEAMD_HIP(d_ctr.grow(B));
    SEAMD_HIP(d_compact.grow(B));
    SEAMD_HIP(d_nrej.grow(B));
    SEAMD_HIP(d_flagged.grow(B + 1));
    SEAMD_HIP(d_rej.grow(rej));
    SEAMD_HIP(d_spec.grow(spec));
    return 0;
}

// Successive calls share the context's scratch and auxiliary streams: order them.  The caller
// holds `mu`.
int Context::begin_call(hipStream_t st)
{
    SEAMD_HIP(hipSetDevice(device));
    if (have_done) SEAMD_HIP(hipStreamWaitEvent(st, ev_done, 0));
    return 0;
}

int Context::end_call(hipStream_t st, int rc)
{
    if (rc != 0)
    {
        // a launch failed part-way: auxiliary streams may be forked and un-joined; drain the device
        // so nothing still refers to the scratch, keep the first error
        const std::string first = last_error();
        (void)hipDeviceSynchronize();
        set_last_error(first);
        return rc;
    }
    SEAMD_HIP(hipEventRecord(ev_done, st));
    have_done = true;
    return 0;
}

// body() between begin_call and end_call; the caller holds `mu`.  body returns 0 or an error code and may leave early
// (SEAMD_HIP): end_call runs either way.
template <class Body>
int Context::call_scope(hipStream_t st, Body &&body)
{
    if (int rc = begin_call(st)) return rc;
    return end_call(st, body());
}

// A keyed call inside a call scope: sanitise the caller's indices (key_prologue), run body(ring) with the clamped ones
// over the K keys at k0 / k1, then give the out-of-range records the status and zero rows of `ra` (ra.bad is set here).
template <class Body>
int Context::keyed_call(const uint32_t *d_key_idx, size_t K, const uint32_t *k0, const uint32_t *k1, KeyRejectArgs ra,
                        size_t B, hipStream_t st, Body &&body)
{
    return call_scope(st, [&]() -> int {
        if (int rc = key_prologue(d_key_idx, K, B, st)) return rc;
        KeyRing ring{};
        ring.k0     = k0;
        ring.k1     = k1;
        ring.idx    = d_kidx;
        ring.stride = (size_t)2 * hp.nprimes * hp.n;
        if (int rc = body(ring)) return rc;
        ra.bad = d_kbad;
        SEAMD_HIP(launch_key_reject(dp, ra, B, st));
        return 0;
    });
}

// What every launch of the uniform sampler takes from the context; the caller adds seeds, counters, output, B and the
// prime range.
UniformArgs Context::uniform_args() const
{
    UniformArgs ua{};
    ua.rej_list    = d_rej;
    ua.rej_cap     = rej_cap;
    ua.spec        = d_spec;
    ua.spec_cap    = spec_cap;
    ua.debug_flags = debug_flags;
    return ua;
}

int Context::fetch_asym_randomness(int8_t *ucodes, int8_t *e1)
{
    std::lock_guard<std::mutex> lk(mu);
    if (!d_ucodes || !d_err) return kErrInvalid;
    SEAMD_HIP(hipSetDevice(device));
    SEAMD_HIP(hipDeviceSynchronize());
    const size_t n = hp.n;
    SEAMD_HIP(hipMemcpy(ucodes, d_ucodes, n, hipMemcpyDeviceToHost));
    SEAMD_HIP(hipMemcpy(e1, d_err + n, n, hipMemcpyDeviceToHost));
    return 0;
}

// sk arrives 2-bit packed (sk_<n>.dat, fileops.c:140-170).  Expand per prime (sample.c:98-129),
// NTT on the device, keep (NTT(s), shoup) pairs -- ckks_sym.c:255-266 hoisted out of the
// per-ciphertext path.
int Context::set_secret_key(const uint8_t *sk_packed)
{
    std::lock_guard<std::mutex> lk(mu);
    return set_secret_key_impl(sk_packed);
}

// the caller holds `mu`
int Context::set_secret_key_impl(const uint8_t *sk_packed)
{
    const size_t n = hp.n, np = hp.nprimes;
    SEAMD_HIP(hipSetDevice(device));
    std::vector<uint32_t> expanded(np * n);
    // the expanded key never outlives this call, on either side of the bus
    struct Wipe
    {
        std::vector<uint32_t> &v;
        ~Wipe() { explicit_bzero(v.data(), v.size() * sizeof(uint32_t)); }
    } wipe{expanded};
    for (size_t j = 0; j < np; j++)
        for (size_t i = 0; i < n; i++)
        {
            uint32_t code = (sk_packed[i / 4] >> (6 - 2 * (i % 4))) & 3u;
            if (code > 2)
            {
                set_last_error("secret key holds an invalid 2-bit code (3)");
                return kErrInvalid;
            }
            expanded[j * n + i] = code + (code == 0 ? hp.q[j] : 0u) - 1u;
        }
    DevBuf<uint32_t> d_tmp{Secret::yes};
    SEAMD_HIP(d_tmp.grow(np * n));
    SEAMD_HIP(d_s_hat.grow(2 * np * n));
    SEAMD_HIP(hipMemcpy(d_tmp, expanded.data(), np * n * sizeof(uint32_t), hipMemcpyHostToDevice));
    for (size_t j = 0; j < np; j++)
        SEAMD_HIP(launch_ntt_polys(dp, dt, (int)j, d_tmp + j * n, d_s_hat + 2 * j * n, 1, nullptr));
    SEAMD_HIP(hipDeviceSynchronize());
    dt.s_hat = d_s_hat;
    have_sk  = true;
    return 0;
}

// pk slabs are already NTT-form residues (pk{0,1}_ntt_<n>_<q>.dat, fileops.c:172-204); add the
// Shoup companions once.
int Context::set_public_key(const uint32_t *pk0, const uint32_t *pk1)
{
    const size_t n = hp.n, np = hp.nprimes;
    SEAMD_HIP(hipSetDevice(device));
    if (first_unreduced_row(hp, pk0, pk1, 1) != 1)
    {
        set_last_error("public key coefficient not reduced modulo its prime");
        return kErrInvalid;
    }
    std::lock_guard<std::mutex> lk(mu);
    DevBuf<uint32_t> d_tmp;
    SEAMD_HIP(d_tmp.grow(2 * np * n));
    SEAMD_HIP(d_pk0.grow(2 * np * n));
    SEAMD_HIP(d_pk1.grow(2 * np * n));
    SEAMD_HIP(hipMemcpy(d_tmp, pk0, np * n * sizeof(uint32_t), hipMemcpyHostToDevice));
    SEAMD_HIP(hipMemcpy(d_tmp + np * n, pk1, np * n * sizeof(uint32_t), hipMemcpyHostToDevice));
    for (size_t j = 0; j < np; j++)
    {
        SEAMD_HIP(launch_make_pairs(d_tmp + j * n, d_pk0 + 2 * j * n, hp.q[j], n, nullptr));
        SEAMD_HIP(launch_make_pairs(d_tmp + np * n + j * n, d_pk1 + 2 * j * n, hp.q[j], n, nullptr));
    }
    SEAMD_HIP(hipDeviceSynchronize());
    dt.pk0  = d_pk0;
    dt.pk1  = d_pk1;
    have_pk = true;
    return 0;
}

// Key rings: K keys validated as the single-key setters validate one, installed with O(np) launches whatever K.
// A ring is replaced only after every call already enqueued on the context has finished (they may read the old one).
int Context::set_secret_keyring(size_t K, const uint8_t *sk_packed)
{
    const size_t n = hp.n, np = hp.nprimes, bytes = K * (n / 4);
    if (K == 0 || K > 0xFFFFFFFFull)
    {
        set_last_error("set_secret_keyring: K must be between 1 and 2^32 - 1");
        return kErrInvalid;
    }
    if (const size_t i = first_code3(sk_packed, bytes); i != bytes)
    {
        set_last_error("secret key ring: key " + std::to_string(i / (n / 4)) + " holds an invalid 2-bit code (3)");
        return kErrInvalid;
    }
    std::lock_guard<std::mutex> lk(mu);
    SEAMD_HIP(hipSetDevice(device));
    SEAMD_HIP(hipDeviceSynchronize());   // calls in flight may still read the old ring
    ring_sk = 0;
    d_ring_sk.release();                 // wiped (secret)
    // the packed keys cross the bus as they are and are expanded on the device: no host copy to wipe, and the
    // device staging buffer is secret (wiped when it is freed below)
    DevBuf<uint8_t> d_packed{Secret::yes};
    SEAMD_HIP(d_packed.grow(bytes));
    SEAMD_HIP(d_ring_sk.grow(2 * K * np * n));
    SEAMD_HIP(hipMemcpy(d_packed, sk_packed, bytes, hipMemcpyHostToDevice));
    for (size_t j = 0; j < np; j++)
        SEAMD_HIP(launch_ring_secret_ntt(dp, dt, (int)j, d_packed, d_ring_sk, K, nullptr));
    SEAMD_HIP(hipDeviceSynchronize());
    ring_sk = K;
    return 0;
}

int Context::set_public_keyring(size_t K, const uint32_t *pk0, const uint32_t *pk1)
{
    const size_t n = hp.n, np = hp.nprimes;
    if (K == 0 || K > 0xFFFFFFFFull)
    {
        set_last_error("set_public_keyring: K must be between 1 and 2^32 - 1");
        return kErrInvalid;
    }
    if (const size_t k = first_unreduced_row(hp, pk0, pk1, K); k != K)
    {
        set_last_error("public key ring: key " + std::to_string(k) + " holds a coefficient not reduced modulo its prime");
        return kErrInvalid;
    }
    std::lock_guard<std::mutex> lk(mu);
    SEAMD_HIP(hipSetDevice(device));
    SEAMD_HIP(hipDeviceSynchronize());   // calls in flight may still read the old ring
    ring_pk = 0;
    d_ring_pk0.release();
    d_ring_pk1.release();
    const size_t slab = K * np * n;
    DevBuf<uint32_t> d_tmp;
    SEAMD_HIP(d_tmp.grow(slab));
    SEAMD_HIP(d_ring_pk0.grow(2 * slab));
    SEAMD_HIP(d_ring_pk1.grow(2 * slab));
    SEAMD_HIP(hipMemcpy(d_tmp, pk0, slab * sizeof(uint32_t), hipMemcpyHostToDevice));
    SEAMD_HIP(launch_ring_pairs(dp, d_tmp, d_ring_pk0, K, nullptr));
    SEAMD_HIP(hipDeviceSynchronize());
    SEAMD_HIP(hipMemcpy(d_tmp, pk1, slab * sizeof(uint32_t), hipMemcpyHostToDevice));
    SEAMD_HIP(launch_ring_pairs(dp, d_tmp, d_ring_pk1, K, nullptr));
    SEAMD_HIP(hipDeviceSynchronize());
    ring_pk = K;
    return 0;
}

// gen_pk (ckks_asym.c:159-171, driven as device/test/ckks_tests_asym.c:174-208 does): the public
// key is a symmetric encryption of zero with a small error:  pk1_j = a_j (shareable PRNG re-seeded
// with pk_seed at counter 0 for EVERY prime), pk0_j = -(a_j . NTT(s)) + NTT(ep mod q_j), ep = n CBD
// samples from PRNG(ep_seed).  Built from the path's own kernels.
int Context::gen_public_key(const uint8_t *sk_packed, const uint8_t *pk_seed, const uint8_t *ep_seed,
                            uint32_t *pk0_out, uint32_t *pk1_out)
{
    // one critical section: the key the public key is derived from is the key that stays installed
    std::lock_guard<std::mutex> lk(mu);
    int rc = set_secret_key_impl(sk_packed);
    if (rc) return rc;
    rc = ensure_scratch(1);
    if (rc) return rc;
    const uint32_t n = (uint32_t)hp.n, np = (uint32_t)hp.nprimes;
    DevBuf<uint8_t> d_seeds{Secret::yes};
    DevBuf<uint32_t> d_c;  // [2][np][n]: residues/pk0 then a/pk1
    SEAMD_HIP(d_seeds.grow(128));
    SEAMD_HIP(d_c.grow((size_t)2 * np * n));
    SEAMD_HIP(hipMemcpy(d_seeds, ep_seed, 64, hipMemcpyHostToDevice));
    SEAMD_HIP(hipMemcpy(d_seeds + 64, pk_seed, 64, hipMemcpyHostToDevice));
    uint32_t *d_p0 = d_c, *d_p1 = d_c + (size_t)np * n;
    CbdArgs ca{};
    ca.seeds         = d_seeds;
    ca.out           = d_err;
    ca.blocks_per_ct = n / 16;
    ca.B             = 1;
    SEAMD_HIP(launch_sample_cbd(ca, nullptr));
    SEAMD_HIP(launch_reduce_small(dp, d_err, d_p0, 1, nullptr));
    EncArgs ea{};
    ea.c0 = d_p0;
    ea.c1 = d_p1;
    UniformArgs ua = uniform_args();
    ua.seeds       = d_seeds + 64;
    ua.out         = d_p1;
    ua.B           = 1;
    ua.out_primes  = np;
    ua.debug_flags = 0;   // the default forms, whatever the context's test flags
    for (uint32_t j = 0; j < np; j++)
    {
        ua.prime_lo = j;
        ua.prime_hi = j + 1;
        SEAMD_HIP(launch_sample_uniform(dp, ua, nullptr));
        SEAMD_HIP(launch_ntt_fuse(dp, dt, ea, kModeSym, (int)j, 1, nullptr));
    }
    SEAMD_HIP(hipDeviceSynchronize());
    SEAMD_HIP(hipMemcpy(pk0_out, d_p0, (size_t)np * n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SEAMD_HIP(hipMemcpy(pk1_out, d_p1, (size_t)np * n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SEAMD_HIP(hipMemset(d_err, 0, n));  // the key-generation error is secret too
    return 0;
}

// Batched key generation: K independent key pairs in one launch chain.
//   secret key k : ckks_setup_s's sample branch (ckks_sym.c:162-179) = sample_small_poly_ternary_prng_96
//                  from PRNG(sk_seeds[k]) at counter 0 (sample.c:218-242), 2-bit packed; or sk_in[k]
//   public key k : gen_pk per prime as device/test/ckks_tests_asym.c:174-208 drives it: ep = n CBD samples
//                  from PRNG(ep_seeds[k]); per prime the shareable PRNG restarts from pk_seeds[k] at
//                  counter 0: pk1_j = a_j, pk0_j = -(a_j . NTT(s)) + NTT(ep mod q_j)
// Launches: 1 ternary sampler + 1 pack + 1 CBD + per prime {uniform sampler, sym-prime kernel} for all K.
int Context::gen_keys_batch(size_t K, const uint8_t *sk_in, const uint8_t *sk_seeds, const uint8_t *pk_seeds,
                            const uint8_t *ep_seeds, uint8_t *sk_out, uint32_t *pk0_out, uint32_t *pk1_out)
{
    if (K == 0) return 0;
    if ((!sk_in && !sk_seeds) || !pk_seeds || !ep_seeds || !pk0_out || !pk1_out)
    {
        set_last_error("gen_keys_batch: sk_in or sk_seeds, pk_seeds, ep_seeds and both output slabs are required");
        return kErrInvalid;
    }
    std::lock_guard<std::mutex> lk(mu);
    return gen_keys_chain({KeyChain::kPairs}, K, sk_in, sk_seeds, pk_seeds, ep_seeds, sk_out, pk0_out, pk1_out);
}

// Relinearisation key: the chain above with K = R = 2 np rows under ONE secret key, pk_seeds = a_seeds and ep_seeds =
// e_seeds -- row r is public key r, (evk0[r], evk1[r]) = (-a_r s_hat + NTT(e_r), a_r) -- plus the diagonal term
// 2^(15 t) s_hat^2 on column j of the rows r = 2j + t (kernels/ct_ops.hip, k_evk_diag).
// The special-prime key (sp): K = R' = np - 1 rows, the diagonal (q_{np-1} mod q_j) s_hat^2 on column j of row j.
int Context::gen_relin_key(const uint8_t *sk_packed, const uint8_t *a_seeds, const uint8_t *e_seeds, uint32_t *evk0_out,
                           uint32_t *evk1_out, bool sp)
{
    if (sp && !special_prime_ok()) return kErrInvalid;
    if (!evk_secret_ok(sk_packed)) return kErrInvalid;
    std::lock_guard<std::mutex> lk(mu);
    return gen_keys_chain({KeyChain::kRelin, 0, sp}, evk_rows(sp), sk_packed, nullptr, a_seeds, e_seeds, nullptr,
                          evk0_out, evk1_out);
}

// the special-prime entries need a prime to reserve: np >= 2 (the default chains of n = 1024 and 2048 have one prime)
bool Context::special_prime_ok() const
{
    if (hp.nprimes >= 2) return true;
    set_last_error("the special-prime key switch needs a context of at least two primes");
    return false;
}

// the secret key of gen_relin_key / gen_galois_keys: n/4 bytes without code 3
bool Context::evk_secret_ok(const uint8_t *sk_packed) const
{
    if (first_code3(sk_packed, hp.n / 4) == hp.n / 4) return true;
    set_last_error("secret key holds an invalid 2-bit code (3)");
    return false;
}

int Context::gen_keys_chain(KeyChain chain, size_t K, const uint8_t *sk_in, const uint8_t *sk_seeds,
                            const uint8_t *pk_seeds, const uint8_t *ep_seeds, uint8_t *sk_out, uint32_t *pk0_out,
                            uint32_t *pk1_out)
{
    const bool relin = chain.kind != KeyChain::kPairs;   // evaluation-key rows: one secret key, a diagonal term
    SEAMD_HIP(hipSetDevice(device));
    int rc = ensure_scratch(K);
    if (rc) return rc;
    const uint32_t n = (uint32_t)hp.n, np = (uint32_t)hp.nprimes;
    const size_t slab = (size_t)K * np * n;
    DevBuf<uint8_t> seeds{Secret::yes}, keys{Secret::yes};
    DevBuf<int8_t> codes{Secret::yes}, ep{Secret::yes};
    DevBuf<uint32_t> pk0, pk1, tmp{Secret::yes};   // tmp: NTT(ep), secret as well
    DevBuf<uint32_t> s_hat{Secret::yes};           // evaluation key: NTT(s) mod the current prime, [K][n] (every row the same)
    const size_t nkeys = relin ? 1 : K;            // secret keys behind the K rows
    if (relin) SEAMD_HIP(s_hat.grow((size_t)K * n));
    // switching key: the packed key it hides, its NTT form mod the current prime [n] and the two rows the chain step that
    // makes it writes beside (a public-key row under that key: secret as well)
    const bool other = chain.kind == KeyChain::kSwitch;
    DevBuf<uint8_t> other_key{Secret::yes};
    DevBuf<uint32_t> other_hat{Secret::yes};
    if (other)
    {
        SEAMD_HIP(other_key.grow(n / 4));
        SEAMD_HIP(other_hat.grow((size_t)3 * n));
        SEAMD_HIP(hipMemcpy(other_key, chain.other, n / 4, hipMemcpyHostToDevice));
    }
    SEAMD_HIP(seeds.grow(K * 192));
    SEAMD_HIP(keys.grow(nkeys * (n / 4)));
    SEAMD_HIP(codes.grow((size_t)K * n));
    SEAMD_HIP(ep.grow((size_t)K * n));
    SEAMD_HIP(pk0.grow(slab));
    SEAMD_HIP(pk1.grow(slab));
    SEAMD_HIP(tmp.grow((size_t)K * n));
    uint8_t *d_sk_seeds = seeds, *d_pk_seeds = d_sk_seeds + K * 64, *d_ep_seeds = d_sk_seeds + K * 128;
    if (sk_seeds) SEAMD_HIP(hipMemcpy(d_sk_seeds, sk_seeds, K * 64, hipMemcpyHostToDevice));
    SEAMD_HIP(hipMemcpy(d_pk_seeds, pk_seeds, K * 64, hipMemcpyHostToDevice));
    SEAMD_HIP(hipMemcpy(d_ep_seeds, ep_seeds, K * 64, hipMemcpyHostToDevice));
    if (sk_in)
        SEAMD_HIP(hipMemcpy(keys, sk_in, nkeys * (n / 4), hipMemcpyHostToDevice));
    else
    {
        TernaryArgs ta{};
        ta.seeds   = d_sk_seeds;
        ta.codes   = codes;
        ta.n       = n;
        ta.B       = (uint32_t)K;
        ta.num_cus = (uint32_t)num_cus;
        SEAMD_HIP(launch_sample_ternary(ta, nullptr));
        SEAMD_HIP(launch_pack_ternary(codes, keys, K * (n / 4), nullptr));
    }
    CbdArgs ca{};
    ca.seeds         = d_ep_seeds;
    ca.out           = ep;
    ca.blocks_per_ct = n / 16;
    ca.B             = (uint32_t)K;
    SEAMD_HIP(launch_sample_cbd(ca, nullptr));
    UniformArgs ua = uniform_args();
    ua.seeds       = d_pk_seeds;
    ua.out         = pk1;
    ua.B           = (uint32_t)K;
    ua.out_primes  = np;
    LowerSymArgs sa{};
    sa.s_small   = keys;
    sa.ep        = ep;
    sa.ntt_pte   = tmp;
    sa.s_stride  = relin ? 0 : n / 4;
    sa.s_save    = relin ? s_hat.get() : nullptr;
    sa.a_stride  = np * n;
    sa.c0_stride = np * n;
    for (uint32_t j = 0; j < np; j++)
    {
        // a_j for every key, counter 0 (gen_pk re-seeds per prime, ckks_asym.c:163), into pk1[:, j]
        ua.prime_lo = j;
        ua.prime_hi = j + 1;
        SEAMD_HIP(launch_sample_uniform(dp, ua, nullptr));
        sa.a  = pk1 + (size_t)j * n;
        sa.c0 = pk0 + (size_t)j * n;
        sa.j  = (int)j;
        SEAMD_HIP(launch_lower_sym_prime(dp, dt, sa, K, nullptr));
        if (!relin || (chain.sp && j + 1 == np)) continue;   // the special prime's own column has no diagonal
        if (other)
        {
            // NTT_j of the hidden key, made the way s_save makes s_hat: the same step on one polynomial
            LowerSymArgs oa = sa;
            oa.s_small   = other_key;
            oa.s_stride  = 0;
            oa.s_save    = other_hat;
            oa.c0        = other_hat + n;
            oa.ntt_pte   = other_hat + (size_t)2 * n;
            oa.c0_stride = 0;
            SEAMD_HIP(launch_lower_sym_prime(dp, dt, oa, 1, nullptr));
        }
        SEAMD_HIP(launch_evk_diag(dp, j, chain.kind == KeyChain::kGalois ? chain.elt : 0, chain.sp,
                                  other ? other_hat.get() : s_hat.get(), pk0, nullptr, other));
    }
    SEAMD_HIP(hipDeviceSynchronize());
    if (sk_out) SEAMD_HIP(hipMemcpy(sk_out, keys, K * (n / 4), hipMemcpyDeviceToHost));
    SEAMD_HIP(hipMemcpy(pk0_out, pk0, slab * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SEAMD_HIP(hipMemcpy(pk1_out, pk1, slab * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

void Context::stage_begin(int stage, hipStream_t st)
{
    if (!profiling) return;
    StageEvent ev;
    ev.stage = stage;
    (void)ev.start.create(hipEventDefault);
    (void)ev.stop.create(hipEventDefault);
    (void)hipEventRecord(ev.start, st);
    events.push_back(std::move(ev));
}

void Context::stage_end(hipStream_t st)
{
    if (!profiling || events.empty()) return;
    (void)hipEventRecord(events.back().stop, st);
}

void Context::collect_events()
{
    for (auto &ev : events)
    {
        float ms = 0;
        if (hipEventSynchronize(ev.stop) == hipSuccess &&
            hipEventElapsedTime(&ms, ev.start, ev.stop) == hipSuccess)
        {
            stage_ms[ev.stage] += ms;
            stage_launches[ev.stage]++;
        }
    }
    events.clear();
}

// The refusals of the whole-path entries: no key, then (for a batch that is not empty) a missing pointer.  The unkeyed
// entries ask before they open a call scope, so that a refused call makes no runtime call at all (the scope's error path
// drains the device); the *_impl functions ask again for the keyed entries, which arrive with a ring.
static int refuse_sym(bool have_key, size_t B, const void *d_values, const void *d_share_seeds, const void *d_seeds,
                      const void *d_c0, const void *d_c1)
{
    if (!have_key)
    {
        set_last_error("symmetric encryption needs a secret key (se_amd_set_secret_key)");
        return kErrNoKey;
    }
    return B != 0 && (!d_values || !d_share_seeds || !d_seeds || !d_c0 || !d_c1) ? kErrInvalid : 0;
}

static int refuse_asym(bool have_key, size_t B, const void *d_values, const void *d_seeds, const void *d_c0,
                       const void *d_c1)
{
    if (!have_key)
    {
        set_last_error("asymmetric encryption needs a public key (se_amd_set_public_key)");
        return kErrNoKey;
    }
    return B != 0 && (!d_values || !d_seeds || !d_c0 || !d_c1) ? kErrInvalid : 0;
}

int Context::encrypt_sym(const float *d_values, size_t B, const uint8_t *d_share_seeds,
                         const uint8_t *d_seeds, uint32_t *d_c0, uint32_t *d_c1,
                         uint32_t *d_ntt_pte, int64_t *d_pte, uint8_t *d_status, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(mu);
    if (int rc = refuse_sym(have_sk, B, d_values, d_share_seeds, d_seeds, d_c0, d_c1)) return rc;
    return call_scope(st, [&] {
        return encrypt_sym_impl(d_values, B, d_share_seeds, d_seeds, d_c0, d_c1, d_ntt_pte, d_pte, d_status, st);
    });
}

// Seed-compressed form: `a` goes to context scratch instead of a caller slab.  The scratch is grown, and
// its pointer handed to the kernels, inside ONE critical section -- a concurrent call with a larger batch
// cannot free it under a call that is still being launched (and the launched work is ordered behind
// ev_done like every other use of the context's scratch).
int Context::encrypt_sym_seeded(const float *d_values, size_t B, const uint8_t *d_share_seeds,
                                const uint8_t *d_seeds, uint32_t *d_c0, uint8_t *d_status, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(mu);
    if (int rc = refuse_sym(have_sk, B, d_values, d_share_seeds, d_seeds, d_c0, d_c0)) return rc;
    SEAMD_HIP(hipSetDevice(device));
    if (B * hp.nprimes * hp.n > d_a.size())
    {
        SEAMD_HIP(hipDeviceSynchronize());   // earlier calls may still read the old slab
        SEAMD_HIP(d_a.grow(B * hp.nprimes * hp.n));
    }
    return call_scope(st, [&] {
        return encrypt_sym_impl(d_values, B, d_share_seeds, d_seeds, d_c0, d_a, nullptr, nullptr, d_status, st);
    });
}

int Context::encrypt_asym(const float *d_values, size_t B, const uint8_t *d_seeds, uint32_t *d_c0,
                          uint32_t *d_c1, uint32_t *d_ntt_pte, int64_t *d_pte, uint8_t *d_status,
                          hipStream_t st)
{
    std::lock_guard<std::mutex> lk(mu);
    if (int rc = refuse_asym(have_pk, B, d_values, d_seeds, d_c0, d_c1)) return rc;
    return call_scope(st, [&] {
        return encrypt_asym_impl(d_values, B, d_seeds, d_c0, d_c1, d_ntt_pte, d_pte, d_status, st);
    });
}

int Context::sample_uniform(const uint8_t *d_seeds, const uint64_t *d_ctr_in, size_t B, uint32_t *d_out,
                            uint64_t *d_ctr_out, hipStream_t st)
{
    if (B == 0) return 0;
    std::lock_guard<std::mutex> lk(mu);
    return call_scope(st, [&]() -> int {
        if (int rc = ensure_scratch(B)) return rc;
        UniformArgs ua = uniform_args();
        ua.seeds       = d_seeds;
        ua.ctr_in      = d_ctr_in;
        ua.ctr_out     = d_ctr_out;
        ua.out         = d_out;
        ua.B           = (uint32_t)B;
        ua.prime_hi    = (uint32_t)hp.nprimes;
        ua.out_primes  = (uint32_t)hp.nprimes;
        SEAMD_HIP(launch_sample_uniform(dp, ua, st));
        return 0;
    });
}

int Context::encrypt_sym_impl(const float *d_values, size_t B, const uint8_t *d_share_seeds,
                              const uint8_t *d_seeds, uint32_t *d_c0, uint32_t *d_c1,
                              uint32_t *d_ntt_pte, int64_t *d_pte, uint8_t *d_status, hipStream_t st,
                              const KeyRing *ring)
{
    if (int rc = refuse_sym(have_sk || ring, B, d_values, d_share_seeds, d_seeds, d_c0, d_c1)) return rc;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    // a handful of ciphertexts: latency path (all primes' samplers at once, prime speculation)
    SpecPlan plan;
    const bool small = split_mode == 2 && small_batch_plan(B, plan, ring != nullptr) && speculation_pays(B, plan);
    // ... whose virtual ciphertexts need reject lists / candidates too
    int rc = ensure_scratch(B, small ? B + plan.total : 0);
    if (rc) return rc;
    const uint32_t n = (uint32_t)hp.n, np = (uint32_t)hp.nprimes;

    CbdArgs ca{};
    ca.seeds         = d_seeds;
    ca.out           = d_err;
    ca.blocks_per_ct = n / 16;
    ca.B             = (uint32_t)B;
    EncArgs ea{};
    ea.values  = d_values;
    ea.err     = d_err;
    ea.c0      = d_c0;
    ea.c1      = d_c1;
    ea.ntt_pte = d_ntt_pte;
    ea.pte     = d_pte;
    ea.status  = d_status;
    ea.general = d_general;
    ea.compact = d_compact;
    ea.debug_flags = debug_flags;
    // a from the shareable seed, written straight into c1 (ckks_sym.c:220)
    UniformArgs ua = uniform_args();
    ua.seeds       = d_share_seeds;
    ua.out         = d_c1;
    ua.B           = (uint32_t)B;
    ua.out_primes  = np;
    if (small) return encrypt_sym_small(plan, ca, ea, ua, st, ring);

    const size_t chain_waves_per_cu = ((B + 63) / 64 + (size_t)num_cus - 1) / (size_t)num_cus;
    const bool split = split_mode == 1 || (split_mode == 2 && (hp.n >= 8192 || chain_waves_per_cu < 4));
    if (!split)
    {
        // Simple chain: [cbd on the aux stream || uniform] -> fused encode+encrypt.
        hipStream_t cbd_stream = overlap ? aux_stream : st;
        if (overlap)
        {
            SEAMD_HIP(hipEventRecord(ev_fork, st));
            SEAMD_HIP(hipStreamWaitEvent(aux_stream, ev_fork, 0));
        }
        stage_begin(0, cbd_stream);
        SEAMD_HIP(launch_sample_cbd(ca, cbd_stream));
        stage_end(cbd_stream);
        if (overlap) SEAMD_HIP(hipEventRecord(ev_join, aux_stream));
        ua.prime_hi = np;   // all primes in one launch
        stage_begin(1, st);
        SEAMD_HIP(launch_sample_uniform(dp, ua, st));
        stage_end(st);
        if (overlap) SEAMD_HIP(hipStreamWaitEvent(st, ev_join, 0));
        stage_begin(3, st);
        SEAMD_HIP(launch_encode_encrypt(dp, dt, ea, kModeSym, B, st, ring));
        stage_end(st);
        return 0;
    }

    // Software pipeline over the primes.  The uniform sampler is one long sequential chain per
    // ciphertext that keeps ONE wave per SIMD busy; everything that does not need a_j runs beside
    // it on the auxiliary stream:
    //   S : U_0 ──► U_1 ──► ... ──► U_{np-1} ─────────────► N_{np-1}
    //   A : cbd ► encode_rns ► (wait U_0) N_0 ► (wait U_1) N_1 ► ... ┘(join)
    // U_j = k_sample_uniform for prime j (counter carried in d_ctr), N_j = k_ntt_fuse for prime j.
    hipStream_t ax = overlap ? aux_stream : st;
    if (overlap)
    {
        SEAMD_HIP(hipEventRecord(ev_fork, st));
        SEAMD_HIP(hipStreamWaitEvent(ax, ev_fork, 0));
    }
    // n = 16384 (`late_encode`): the encode workgroup (136 KiB of LDS, 128 VGPRs x 16 waves) cannot
    // share a CU with a chain workgroup, so on the auxiliary stream it would sit behind every U_j
    // and drag all N_j with it (measured: no overlap at all).  There it runs on the main stream
    // between U_0 and U_1, the chain workgroups carry 2 helper waves instead of 6 (one wave per SIMD,
    // 128 VGPRs) and k_ntt_fuse<14> is held to 80 VGPRs, so an N_j workgroup fits beside U_{j+1}:
    //   S : U_0 ► (wait cbd) encode_rns ► U_1 ──► U_2 ──► ... ► U_{np-1} ──────► N_{np-1}
    //   A : cbd ─────────────────────────► N_0 ► (wait U_1) N_1 ► ...        ┘(join)
    const bool late_encode   = overlap && hp.n >= 16384 && !(debug_flags & 128);
    const uint32_t fill      = late_encode ? 4 : 0;  // leave VGPRs for the co-resident N_j workgroup
    stage_begin(0, ax);
    SEAMD_HIP(launch_sample_cbd(ca, ax));  // e, counters 0.. (ckks_sym.c:196)
    stage_end(ax);
    if (late_encode)
        SEAMD_HIP(hipEventRecord(ev_cbd, ax));
    else
    {
        stage_begin(4, ax);
        SEAMD_HIP(launch_encode_rns(dp, dt, ea, true, B, ax));
        stage_end(ax);
    }
    // Staged sampler (kernels/samplers.hip: k_bulk_pair / k_candidates / k_resolve_wave) for batches between
    // the wave form's limit and one PAIR wave per SIMD (B <= 128 per CU): the chain launches are the critical
    // path of this pipeline, and a ciphertext per lane pair shortens each by ~1.5x; the candidates, which the
    // helper waves of k_sample_uniform compute inside the chain workgroups, become a throughput kernel on a
    // stream of its own.  debug_flags 512 forces it, 1024 forbids it.
    const bool staged = overlap && !(debug_flags & (32 | 1024)) && staged_mode != 0 &&
                        ((B > uniform_wave_limit((unsigned)num_cus) && B <= (size_t)128 * (size_t)num_cus) ||
                         (debug_flags & 512) || staged_mode == 1);
    if (staged && !cand_stream)
    {
        SEAMD_HIP(cand_stream.create(hipStreamNonBlocking));
        for (Event &e : ev_cand) SEAMD_HIP(e.create(hipEventDisableTiming));
    }
    for (uint32_t j = 0; j < np; j++)
    {
        UniformArgs uj = ua;   // a_j; the counter is carried from prime to prime in d_ctr
        uj.ctr_in      = j ? d_ctr.get() : nullptr;
        uj.ctr_out     = d_ctr;
        uj.prime_lo    = j;
        uj.prime_hi    = j + 1;
        uj.helper_fill = fill;
        uj.nrej        = d_nrej;
        uj.flagged     = staged ? d_flagged.get() : nullptr;
        if (staged)
        {
            // Candidates per ciphertext: here they are pure throughput work beside the chains, and a
            // ciphertext that needs more gets them from the resolving wave itself -- so mean + 1.5 sigma of the
            // draws instead of the helper waves' mean + 4 sigma (every unused candidate is a wasted permutation:
            // 384 -> 336 at n = 16384 is 4 % of the phase's instructions).
            {
                const double p_rej = (double)(0u - dp.bound[j]) / 4294967296.0;
                const double mean  = (double)hp.n * p_rej / (1.0 - p_rej);
                const uint32_t cap = ((uint32_t)(mean + 1.5 * sqrt((double)hp.n * p_rej) + 15.0)) & ~15u;
                if (cap < uj.spec_cap) uj.spec_cap = cap ? cap : 16u;
            }
            //   C : (start counters of prime j known) k_candidates_j ───────────┐
            //   S : k_bulk_pair_j ─────────────────────────────────── (wait C) k_resolve_wave_j
            SEAMD_HIP(hipStreamWaitEvent(cand_stream, j ? ev_prime[j - 1] : ev_fork, 0));
            SEAMD_HIP(launch_uniform_candidates(uj, cand_stream));
            SEAMD_HIP(hipEventRecord(ev_cand[j], cand_stream));
            stage_begin(1, st);
            SEAMD_HIP(launch_uniform_bulk_pair(dp, uj, st));
            SEAMD_HIP(hipStreamWaitEvent(st, ev_cand[j], 0));
            SEAMD_HIP(launch_uniform_resolve(dp, uj, st));
            stage_end(st);
        }
        else
        {
            stage_begin(1, st);
            SEAMD_HIP(launch_sample_uniform(dp, uj, st));
            stage_end(st);
        }
        if (late_encode && j == 0)
        {
            SEAMD_HIP(hipStreamWaitEvent(st, ev_cbd, 0));
            stage_begin(4, st);
            SEAMD_HIP(launch_encode_rns(dp, dt, ea, true, B, st));
            stage_end(st);
        }
        if (j + 1 < np)
        {
            if (overlap)
            {
                SEAMD_HIP(hipEventRecord(ev_prime[j], st));
                SEAMD_HIP(hipStreamWaitEvent(ax, ev_prime[j], 0));
            }
            stage_begin(5, ax);
            SEAMD_HIP(launch_ntt_fuse(dp, dt, ea, kModeSym, (int)j, B, ax, ring));
            stage_end(ax);
        }
    }
    if (overlap)
    {
        SEAMD_HIP(hipEventRecord(ev_join, ax));
        SEAMD_HIP(hipStreamWaitEvent(st, ev_join, 0));
    }
    stage_begin(5, st);
    SEAMD_HIP(launch_ntt_fuse(dp, dt, ea, kModeSym, (int)np - 1, B, st, ring));
    stage_end(st);
    return 0;
}

// ---- small-batch prime speculation -----------------------------------------------------------
bool Context::small_batch_plan(size_t B, SpecPlan &plan, bool keyed) const
{
    const uint32_t np = (uint32_t)hp.nprimes;
    if (!overlap || !(have_sk || keyed) || np < 2 || B == 0 || B > 1024) return false;
    plan         = SpecPlan{};
    plan.nprimes = np;
    plan.B       = (uint32_t)B;
    const double n     = (double)hp.n;
    const double width = (debug_flags & 256) ? 0.0 : 5.5;  // 256: windows of one guess (forces the fallback)
    double mu = 0.0, var = 0.0;
    uint64_t off = 0;
    for (uint32_t j = 1; j < np; j++)
    {
        // prime j-1 consumed 1 block + (draws) counters; draws ~ Binomial(n, p)/(1 - p)
        const double p = (double)(0u - dp.bound[j - 1]) / 4294967296.0;
        mu += 1.0 + n * p / (1.0 - p);
        var += n * p * 1.06;
        const uint64_t h = (debug_flags & 256) ? 0 : (uint64_t)(width * sqrt(var)) + 2;
        const uint64_t c = (uint64_t)(mu + 0.5);
        plan.base[j]     = c > h ? c - h : 0;
        plan.count[j]    = (uint32_t)(2 * h + 1);
        plan.offset[j]   = (uint32_t)off;
        off += (uint64_t)B * plan.count[j];
        if (off > (uint64_t)small_limit) return false;  // beyond this it stops paying
        if (off * hp.n * sizeof(uint32_t) > small_bytes) return false;  // scratch rows bounded in bytes
    }
    plan.total = (uint32_t)off;
    // All guesses are ONE launch (UniformArgs::prime_of).  Beyond the wave form's limit that launch takes the
    // lane form, whose per-lane-prime instantiation exists for workgroups of up to 8 waves = 512 ciphertexts per
    // CU: a fan-out wider than that (small devices / partitions: fewer than 128 CUs at the default small_limit)
    // is not planned at all and the call takes the ordinary per-prime chain.
    if ((uint64_t)B + off > (uint64_t)512 * (uint64_t)num_cus) return false;
    return true;
}

// Which form serves a small batch faster?  The uniform sampler is a chain of `steps` sequential permutations
// per polynomial; what it costs depends on the kernel form the launch takes (kernels/samplers.hip,
// launch_sample_uniform; per-permutation times measured with tools/ubench5 and tools/chain_step_probe.py):
//   wave per ciphertext : 3.3 us up to 256 waves, + 1.2 us per further 1 024 waves (4.2 us at one wave per
//                         SIMD, 7.8 us at four)
//   lane per ciphertext : 10.7 us whatever the batch (up to one wave per SIMD)
// Speculation runs the guesses of every prime at once: one chain deep, but B + plan.total ciphertexts wide;
// the plain form runs np chains in sequence, B wide.
bool Context::speculation_pays(size_t B, const SpecPlan &plan) const
{
    if (spec_mode >= 0) return spec_mode != 0;          // SE_AMD_SPECULATION
    const double steps = (double)((hp.n * 4 + 135) / 136);
    // measured on 256 CUs: flat up to one wave per CU, then + 1.2 us per further wave per SIMD (4 per CU)
    const double cus = (double)num_cus;
    auto perm_us = [&](size_t cts) {
        if (cts > uniform_wave_limit((unsigned)num_cus) || (debug_flags & 32)) return 10.7;
        return 3.3 + 1.2 * ((double)cts > cus ? ((double)cts - cus) / (4.0 * cus) : 0.0);
    };
    const double spec  = steps * perm_us(B + plan.total);
    const double plain = (double)hp.nprimes * steps * perm_us(B);
    return spec < 0.9 * plain;
}

int Context::encrypt_sym_small(const SpecPlan &plan, const CbdArgs &ca, const EncArgs &ea, const UniformArgs &ua,
                               hipStream_t st, const KeyRing *ring)
{
    const size_t B     = plan.B;
    const uint32_t n   = (uint32_t)hp.n, np = (uint32_t)hp.nprimes;
    const size_t total = plan.total;
    if (d_sp_seeds.size() < total * 64 || d_sp_ctr.size() < total || d_sp_ctrout.size() < total ||
        d_sp_rows.size() < total * n || d_sp_prime.size() < total)
    {
        SEAMD_HIP(hipDeviceSynchronize());
        SEAMD_HIP(d_sp_seeds.grow(total * 64));
        SEAMD_HIP(d_sp_ctr.grow(total));
        SEAMD_HIP(d_sp_ctrout.grow(total));
        SEAMD_HIP(d_sp_rows.grow(total * n));
        SEAMD_HIP(d_sp_prime.grow(total));
    }
    SEAMD_HIP(d_sp_fail.grow(1024));   // small_batch_plan: B <= 1024
    // Three streams whatever the length of the prime chain (the runtime's default of 4 hardware queues is
    // enough): the guesses of ALL primes are ONE launch (UniformArgs::prime_of).
    SEAMD_HIP(spec_stream.create(hipStreamNonBlocking));

    //   S : U_0 (real ciphertexts) ─────────────────────┐ (wait P) select ► redo (masked) ► (wait A) N_0 .. N_{np-1}
    //   A : cbd ► k_encode_rns ─────────────────────────┤
    //   P : setup ► U_{1..np-1} (all guesses, one launch)┘
    SEAMD_HIP(hipEventRecord(ev_fork, st));
    SEAMD_HIP(hipStreamWaitEvent(aux_stream, ev_fork, 0));
    SEAMD_HIP(hipStreamWaitEvent(spec_stream, ev_fork, 0));

    SEAMD_HIP(launch_spec_setup(plan, ua.seeds, d_sp_seeds, d_sp_ctr, d_sp_prime, spec_stream));
    {
        // one output row per virtual ciphertext; its prime comes from d_sp_prime
        UniformArgs ug = uniform_args();
        ug.seeds       = d_sp_seeds;
        ug.ctr_in      = d_sp_ctr;
        ug.ctr_out     = d_sp_ctrout;
        ug.out         = d_sp_rows;
        ug.rej_list    = d_rej + B * rej_cap;     // behind the rows of the real ciphertexts
        ug.spec        = d_spec + B * spec_cap;
        ug.B           = (uint32_t)total;
        ug.out_primes  = 1;
        ug.prime_of    = d_sp_prime;
        SEAMD_HIP(launch_sample_uniform(dp, ug, spec_stream));
        SEAMD_HIP(hipEventRecord(ev_enc, spec_stream));
    }

    stage_begin(0, aux_stream);
    SEAMD_HIP(launch_sample_cbd(ca, aux_stream));
    stage_end(aux_stream);
    stage_begin(4, aux_stream);
    SEAMD_HIP(launch_encode_rns(dp, dt, ea, true, B, aux_stream));
    stage_end(aux_stream);
    SEAMD_HIP(hipEventRecord(ev_join, aux_stream));

    UniformArgs u0 = ua;   // prime 0 of the real ciphertexts
    u0.ctr_out     = d_ctr;
    u0.prime_hi    = 1;
    stage_begin(1, st);
    SEAMD_HIP(launch_sample_uniform(dp, u0, st));
    stage_end(st);
    SEAMD_HIP(hipStreamWaitEvent(st, ev_enc, 0));
    SEAMD_HIP(launch_spec_select(plan, n, d_ctr, d_sp_ctrout, d_sp_rows, ea.c1, d_sp_fail, st));
    // misses (~1e-7 per prime): the ordinary per-prime chain, masked to the ciphertexts that missed;
    // without a miss every workgroup of these launches returns at once
    UniformArgs ur = u0;
    ur.ctr_in      = d_ctr;
    ur.only_from   = d_sp_fail;
    for (uint32_t j = 1; j < np; j++)
    {
        ur.prime_lo = j;
        ur.prime_hi = j + 1;
        SEAMD_HIP(launch_sample_uniform(dp, ur, st));
    }
    SEAMD_HIP(hipStreamWaitEvent(st, ev_join, 0));
    for (uint32_t j = 0; j < np; j++)
    {
        stage_begin(5, st);
        SEAMD_HIP(launch_ntt_fuse(dp, dt, ea, kModeSym, (int)j, B, st, ring));
        stage_end(st);
    }
    return 0;
}

int Context::encrypt_asym_impl(const float *d_values, size_t B, const uint8_t *d_seeds, uint32_t *d_c0,
                               uint32_t *d_c1, uint32_t *d_ntt_pte, int64_t *d_pte, uint8_t *d_status,
                               hipStream_t st, const KeyRing *ring)
{
    if (int rc = refuse_asym(have_pk || ring, B, d_values, d_seeds, d_c0, d_c1)) return rc;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    int rc = ensure_scratch(B);
    if (rc) return rc;
    const uint32_t n = (uint32_t)hp.n;

    // u first for the whole batch (its redraws decide where each ciphertext's CBD counters start,
    // ckks_asym.c:188-201): the ternary sampler is a per-ciphertext chain, so its duration does not
    // shrink with a chunk and it is launched once.  Then the batch is cut into chunks: the CBD sampler
    // of chunk k+1 (e0 | e1 contiguous per ciphertext; VALU-throughput-bound) runs on the auxiliary
    // stream beside the fused kernel of chunk k (latency-bound at 2 waves per SIMD), which leaves the
    // CBD sampler's time mostly hidden.
    //   S : ternary(all) ──fork──────► (wait C_0) E_0 ► (wait C_1) E_1 ► ...
    //   A :                 └► C_0 ► C_1 ► C_2 ► ...
    const size_t np = hp.nprimes;
    size_t nchunks  = overlap ? asym_chunks : 1;
    if (nchunks > (size_t)kMaxPrimes) nchunks = kMaxPrimes;   // one join event per chunk
    if (nchunks < 1 || B < 4096 * nchunks) nchunks = 1;        // small batches: one chunk
    TernaryArgs ta{};
    ta.seeds       = d_seeds;
    ta.codes       = d_ucodes;
    ta.ctr_out     = d_ctr;
    ta.n           = n;
    ta.B           = (uint32_t)B;
    ta.num_cus     = (uint32_t)num_cus;
    ta.debug_flags = debug_flags;
    stage_begin(2, st);
    SEAMD_HIP(launch_sample_ternary(ta, st));
    stage_end(st);
    hipStream_t ax = nchunks > 1 ? aux_stream : st;
    if (nchunks > 1)
    {
        SEAMD_HIP(hipEventRecord(ev_fork, st));
        SEAMD_HIP(hipStreamWaitEvent(ax, ev_fork, 0));
    }
    for (size_t c = 0; c < nchunks; c++)
    {
        const size_t lo = B * c / nchunks, hi = B * (c + 1) / nchunks, cb = hi - lo;
        if (cb == 0) continue;
        CbdArgs ca{};
        ca.seeds         = d_seeds + lo * 64;
        ca.ctr_base      = d_ctr + lo;
        ca.out           = d_err + lo * 2 * n;
        ca.blocks_per_ct = 2 * (n / 16);
        ca.B             = (uint32_t)cb;
        stage_begin(0, ax);
        SEAMD_HIP(launch_sample_cbd(ca, ax));
        stage_end(ax);
        if (nchunks > 1) SEAMD_HIP(hipEventRecord(ev_prime[c], ax));
    }
    for (size_t c = 0; c < nchunks; c++)
    {
        const size_t lo = B * c / nchunks, hi = B * (c + 1) / nchunks, cb = hi - lo;
        if (cb == 0) continue;
        if (nchunks > 1) SEAMD_HIP(hipStreamWaitEvent(st, ev_prime[c], 0));
        EncArgs ea{};
        ea.values  = d_values + lo * (n / 2);
        ea.err     = d_err + lo * 2 * n;
        ea.ucodes  = d_ucodes + lo * n;
        ea.c0      = d_c0 + lo * np * n;
        ea.c1      = d_c1 + lo * np * n;
        ea.ntt_pte = d_ntt_pte ? d_ntt_pte + lo * np * n : nullptr;
        ea.pte     = d_pte ? d_pte + lo * n : nullptr;
        ea.status  = d_status ? d_status + lo : nullptr;
        ea.general = d_general;
        KeyRing rc_chunk{};
        if (ring)
        {
            rc_chunk = *ring;
            rc_chunk.idx += lo;   // the chunk's records
        }
        stage_begin(3, st);
        SEAMD_HIP(launch_encode_encrypt(dp, dt, ea, kModeAsym, cb, st, ring ? &rc_chunk : nullptr));
        stage_end(st);
    }
    return 0;
}

// ---- keyed entries ---------------------------------------------------------------------------
// Every call first writes a clamped copy of the caller's indices (d_kidx: the kernels never see an index >= K) and the
// list of records whose index was out of range (d_kbad); the unkeyed dispatch then runs with the keyed kernels
// (KeyRing), and a last pass gives the listed records status 2 and zero c0 (and c1 in public-key mode).
int Context::key_prologue(const uint32_t *d_key_idx, size_t K, size_t B, hipStream_t st)
{
    int rc = ensure_keyed(B);
    if (rc) return rc;
    SEAMD_HIP(launch_key_sanitize(d_key_idx, d_kidx, d_kbad, K, B, st));
    return 0;
}

int Context::encrypt_sym_keyed(const float *d_values, size_t B, const uint32_t *d_key_idx,
                               const uint8_t *d_share_seeds, const uint8_t *d_seeds, uint32_t *d_c0, uint32_t *d_c1,
                               uint32_t *d_ntt_pte, int64_t *d_pte, uint8_t *d_status, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(mu);
    if (!ring_sk)
    {
        set_last_error("keyed symmetric encryption needs a secret key ring (se_amd_set_secret_keyring)");
        return kErrNoKey;
    }
    if (B == 0) return 0;
    if (!d_values || !d_key_idx || !d_share_seeds || !d_seeds || !d_c0) return kErrInvalid;
    SEAMD_HIP(hipSetDevice(device));
    // d_c1 NULL: the seed-compressed form, `a` into context scratch (as encrypt_sym_seeded)
    if (!d_c1 && B * hp.nprimes * hp.n > d_a.size())
    {
        SEAMD_HIP(hipDeviceSynchronize());   // earlier calls may still read the old slab
        SEAMD_HIP(d_a.grow(B * hp.nprimes * hp.n));
    }
    KeyRejectArgs ra{};
    ra.status   = d_status;
    ra.rows[0]  = d_c0;
    ra.words[0] = hp.nprimes * hp.n;
    return keyed_call(d_key_idx, ring_sk, d_ring_sk, d_ring_sk, ra, B, st, [&](const KeyRing &ring) {
        return encrypt_sym_impl(d_values, B, d_share_seeds, d_seeds, d_c0, d_c1 ? d_c1 : d_a.get(), d_ntt_pte, d_pte,
                                d_status, st, &ring);
    });
}

int Context::encrypt_asym_keyed(const float *d_values, size_t B, const uint32_t *d_key_idx, const uint8_t *d_seeds,
                                uint32_t *d_c0, uint32_t *d_c1, uint32_t *d_ntt_pte, int64_t *d_pte,
                                uint8_t *d_status, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(mu);
    if (!ring_pk)
    {
        set_last_error("keyed public-key encryption needs a public key ring (se_amd_set_public_keyring)");
        return kErrNoKey;
    }
    if (B == 0) return 0;
    if (!d_values || !d_key_idx || !d_seeds || !d_c0 || !d_c1) return kErrInvalid;
    KeyRejectArgs ra{};
    ra.status   = d_status;
    ra.rows[0]  = d_c0;
    ra.rows[1]  = d_c1;
    ra.words[0] = hp.nprimes * hp.n;
    ra.words[1] = hp.nprimes * hp.n;
    return keyed_call(d_key_idx, ring_pk, d_ring_pk0, d_ring_pk1, ra, B, st, [&](const KeyRing &ring) {
        return encrypt_asym_impl(d_values, B, d_seeds, d_c0, d_c1, d_ntt_pte, d_pte, d_status, st, &ring);
    });
}

// An out-of-range index: the record is decrypted under the clamped index and its outputs are then zeroed.
int Context::decrypt_decode_keyed(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, const uint32_t *d_key_idx,
                                  size_t prime, uint32_t *d_dec_ntt, uint32_t *d_pt, float *d_values, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(mu);
    if (!ring_sk)
    {
        set_last_error("keyed decrypt needs a secret key ring (se_amd_set_secret_keyring)");
        return kErrNoKey;
    }
    if (B == 0) return 0;
    if (!d_c0 || !d_c1 || !d_key_idx || prime >= hp.nprimes) return kErrInvalid;
    KeyRejectArgs ra{};
    ra.rows[0]  = d_dec_ntt;
    ra.rows[1]  = d_pt;
    ra.rows[2]  = reinterpret_cast<uint32_t *>(d_values);
    ra.words[0] = hp.n;
    ra.words[1] = hp.n;
    ra.words[2] = hp.n / 2;
    return keyed_call(d_key_idx, ring_sk, d_ring_sk, d_ring_sk, ra, B, st, [&](const KeyRing &ring) -> int {
        SEAMD_HIP(launch_decrypt_decode(dp, dt, d_c0, d_c1, (uint32_t)hp.nprimes, (int)prime, d_dec_ntt, d_pt, d_values,
                                        B, st, &ring));
        return 0;
    });
}

// Full-modulus decrypt: one launch, no scratch (nothing of the context is written, so no begin_call / end_call).
int Context::decrypt_full(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, int64_t *d_pte, float *d_values,
                          double *d_values_f64, uint8_t *d_status, hipStream_t st)
{
    return decrypt_level(d_c0, d_c1, B, hp.nprimes, hp.scale, d_pte, d_values, d_values_f64, d_status, st);
}

// The kernel takes its record stride and its scale from the by-value DevParams; the chain, the key rows and the Garner
// constants of the first `primes` primes are those of the parameter set (n, primes).
static bool level_params(const DevParams &dp, size_t np, size_t primes, double scale, DevParams &out)
{
    if (primes < 1 || primes > np || !(scale > 0) || scale == HUGE_VAL) return false;   // NaN fails scale > 0
    out         = dp;
    out.nprimes = (uint32_t)primes;
    out.scale   = scale;
    return true;
}

int Context::decrypt_level(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, double scale,
                           int64_t *d_pte, float *d_values, double *d_values_f64, uint8_t *d_status, hipStream_t st)
{
    return decrypt_level_impl(d_c0, d_c1, nullptr, false, B, primes, scale, nullptr, false, d_pte, d_values,
                              d_values_f64, d_status, st);
}

int Context::decrypt3_level(const uint32_t *d_c0, const uint32_t *d_c1, const uint32_t *d_c2, size_t B, size_t primes,
                            double scale, int64_t *d_pte, float *d_values, double *d_values_f64, uint8_t *d_status,
                            hipStream_t st)
{
    return decrypt_level_impl(d_c0, d_c1, d_c2, true, B, primes, scale, nullptr, false, d_pte, d_values, d_values_f64,
                              d_status, st);
}

// An out-of-range index: the record is decrypted under the clamped index; its status then becomes 2 and its other
// outputs zero.
int Context::decrypt_full_keyed(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, const uint32_t *d_key_idx,
                                int64_t *d_pte, float *d_values, double *d_values_f64, uint8_t *d_status,
                                hipStream_t st)
{
    return decrypt_level_keyed(d_c0, d_c1, B, hp.nprimes, hp.scale, d_key_idx, d_pte, d_values, d_values_f64, d_status,
                               st);
}

int Context::decrypt_level_keyed(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, double scale,
                                 const uint32_t *d_key_idx, int64_t *d_pte, float *d_values, double *d_values_f64,
                                 uint8_t *d_status, hipStream_t st)
{
    return decrypt_level_impl(d_c0, d_c1, nullptr, false, B, primes, scale, d_key_idx, true, d_pte, d_values,
                              d_values_f64, d_status, st);
}

int Context::decrypt3_level_keyed(const uint32_t *d_c0, const uint32_t *d_c1, const uint32_t *d_c2, size_t B,
                                  size_t primes, double scale, const uint32_t *d_key_idx, int64_t *d_pte,
                                  float *d_values, double *d_values_f64, uint8_t *d_status, hipStream_t st)
{
    return decrypt_level_impl(d_c0, d_c1, d_c2, true, B, primes, scale, d_key_idx, true, d_pte, d_values, d_values_f64,
                              d_status, st);
}

// deg2: the third slab d_c2 is mandatory and the degree-2 kernels run (FullArgs::c2).  keyed: under the secret ring,
// inside a call scope (the sanitised indices are context scratch); else one launch that writes nothing of the context.
int Context::decrypt_level_impl(const uint32_t *d_c0, const uint32_t *d_c1, const uint32_t *d_c2, bool deg2, size_t B,
                                size_t primes, double scale, const uint32_t *d_key_idx, bool keyed, int64_t *d_pte,
                                float *d_values, double *d_values_f64, uint8_t *d_status, hipStream_t st)
{
    std::unique_lock<std::mutex> lk(mu, std::defer_lock);
    if (keyed) lk.lock();
    if (keyed ? !ring_sk : !have_sk)
    {
        set_last_error(keyed ? "keyed decrypt needs a secret key ring (se_amd_set_secret_keyring)"
                             : "decrypt needs the secret key (se_amd_set_secret_key)");
        return kErrNoKey;
    }
    DevParams lp;
    if (!d_c0 || !d_c1 || (deg2 && !d_c2) || (keyed && !d_key_idx) ||
        (!d_pte && !d_values && !d_values_f64 && !d_status))
        return kErrInvalid;
    if (!level_params(dp, hp.nprimes, primes, scale, lp)) return kErrInvalid;
    if (B == 0) return 0;
    FullArgs fa{};
    fa.c0         = d_c0;
    fa.c1         = d_c1;
    fa.c2         = deg2 ? d_c2 : nullptr;
    fa.pte        = d_pte;
    fa.values     = d_values;
    fa.values_f64 = d_values_f64;
    fa.status     = d_status;
    if (!keyed)
    {
        SEAMD_HIP(hipSetDevice(device));
        SEAMD_HIP(launch_decrypt_full(lp, dt, crt, fa, B, st));
        return 0;
    }
    KeyRejectArgs ra{};
    ra.status   = d_status;
    ra.rows[0]  = reinterpret_cast<uint32_t *>(d_pte);
    ra.rows[1]  = reinterpret_cast<uint32_t *>(d_values);
    ra.rows[2]  = reinterpret_cast<uint32_t *>(d_values_f64);
    ra.words[0] = 2 * hp.n;
    ra.words[1] = hp.n / 2;
    ra.words[2] = hp.n;
    return keyed_call(d_key_idx, ring_sk, d_ring_sk, d_ring_sk, ra, B, st, [&](const KeyRing &ring) -> int {
        SEAMD_HIP(launch_decrypt_full(lp, dt, crt, fa, B, st, &ring));
        return 0;
    });
}

// Key-free, one launch, nothing of the context is written: level `primes` -> `primes` - 1 on one or two slabs.
int Context::ct_rescale(const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t primes, uint32_t *d_out0,
                        uint32_t *d_out1, hipStream_t st)
{
    if (!d_in0 || !d_out0 || !d_in1 != !d_out1) return kErrInvalid;
    if (primes < 2 || primes > hp.nprimes || B > 0x7fffffffu) return kErrInvalid;
    if (!aligned16({d_in0, d_in1, d_out0, d_out1})) return kErrInvalid;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    RescaleArgs ra{};
    ra.in0    = d_in0;
    ra.in1    = d_in1;
    ra.out0   = d_out0;
    ra.out1   = d_out1;
    ra.primes = (uint32_t)primes;
    SEAMD_HIP(launch_ct_rescale(dp, dt, host_rescale_params(hp, primes), ra, B, st));
    return 0;
}

// Key-free, one launch, nothing of the context is written and nothing is uploaded: the residues of the weights and of the
// constant travel in the argument block.
int Context::ct_affine_rescale(const uint32_t *const *d_term0, const uint32_t *const *d_term1, const uint32_t *term_primes,
                               const int64_t *w, size_t T, int64_t c_after, size_t B, size_t primes, uint32_t *d_out0,
                               uint32_t *d_out1, hipStream_t st)
{
    if (!d_term0 || !d_term1 || !term_primes || !w || !d_out0 || !d_out1) return kErrInvalid;
    if (T < 1 || T > kAffineMaxTerms || primes < 2 || primes > hp.nprimes || B > 0x7fffffffu) return kErrInvalid;
    if (!aligned16({d_out0, d_out1})) return kErrInvalid;
    // the non-negative residue of any int64 (the remainder of a negative value is in (-q, 0])
    auto residue = [](int64_t v, uint32_t q) { return (uint32_t)((v % (int64_t)q + (int64_t)q) % (int64_t)q); };
    AffineRescaleArgs aa{};
    for (size_t t = 0; t < T; t++)
    {
        if (!d_term0[t] || !d_term1[t] || !aligned16({d_term0[t], d_term1[t]})) return kErrInvalid;
        if (term_primes[t] < primes || term_primes[t] > hp.nprimes) return kErrInvalid;
        aa.term0[t]       = d_term0[t];
        aa.term1[t]       = d_term1[t];
        aa.term_primes[t] = term_primes[t];
        for (size_t j = 0; j < primes; j++) aa.w[t][j] = residue(w[t], hp.q[j]);
    }
    if (B == 0) return 0;
    for (size_t i = 0; i + 1 < primes; i++) aa.c[i] = residue(c_after, hp.q[i]);
    aa.out0   = d_out0;
    aa.out1   = d_out1;
    aa.T      = (uint32_t)T;
    aa.primes = (uint32_t)primes;
    SEAMD_HIP(hipSetDevice(device));
    SEAMD_HIP(launch_ct_affine_rescale(dp, dt, host_rescale_params(hp, primes), aa, B, st));
    return 0;
}

// The schedule of a polynomial plan, every step an entry of this file on `st` in the caller's workspace (PolyPlan::
// workspace_words is its layout): row pointers | per power above 1 its two slabs | a product | a dropped operand.
int Context::ct_poly_sp(const PolyPlan *plan, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, void *d_work,
                        size_t work_bytes, uint32_t *d_out0, uint32_t *d_out1, hipStream_t st)
{
    if (!plan || !d_c0 || !d_c1 || !d_out0 || !d_out1 || !aligned16({d_c0, d_c1, d_out0, d_out1, d_work}))
        return kErrInvalid;
    if (plan->n != hp.n || plan->np != hp.nprimes || B > 0x7fffffffu) return kErrInvalid;
    const size_t need = plan->workspace_words(B) * sizeof(uint32_t);
    if (work_bytes < need || (need && !d_work)) return kErrInvalid;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!(const uint32_t *)evk[1].relin)
        {
            set_last_error("no special-prime relinearisation key is installed (se_amd_set_relin_key_sp)");
            return kErrNoKey;
        }
    }
    if (B == 0) return 0;
    const size_t n = hp.n, L = plan->L;
    const std::vector<PolyPower> &pw = plan->powers;
    // where x^d lives: the input, or its slabs in the workspace
    const uint32_t *s0[16] = {}, *s1[16] = {};
    uint32_t lv[16]        = {};
    s0[1] = d_c0, s1[1] = d_c1, lv[1] = (uint32_t)L;
    uint32_t *row_ptr = (uint32_t *)d_work, *slab[16][2] = {}, *prod0 = nullptr, *prod1 = nullptr, *drop0 = nullptr,
             *drop1 = nullptr;
    if (pw.size() > 1)
    {
        uint32_t *at = row_ptr + ((B + 1 + 3) & ~(size_t)3);
        for (size_t k = 1; k < pw.size(); k++)
            for (int h = 0; h < 2; h++, at += B * pw[k].level * n) slab[pw[k].d][h] = at;
        prod0 = at, prod1 = prod0 + B * L * n, drop0 = prod1 + B * L * n, drop1 = drop0 + B * (L - 1) * n;
        SEAMD_HIP(hipSetDevice(device));
        SEAMD_HIP(launch_row_iota(row_ptr, B + 1, st));
    }
    for (size_t k = 1; k < pw.size(); k++)
    {
        const uint32_t d = pw[k].d, m = pw[k].level + 1;
        uint32_t h = 1;
        while (2 * h < d) h *= 2;   // 2^(depth(d) - 1)
        const uint32_t *b0 = s0[d - h], *b1 = s1[d - h];
        if (lv[d - h] > m)
        {
            const int rc = ct_drop_primes(b0, b1, B, lv[d - h], m, drop0, drop1, st);
            if (rc != 0) return rc;
            b0 = drop0, b1 = drop1;
        }
        int rc = ct_mul_sum(s0[h], s1[h], B, b0, b1, B, m, B, row_ptr, nullptr, nullptr, B, true, prod0, prod1, nullptr,
                            nullptr, st);
        if (rc != 0) return rc;
        rc = ct_rescale(prod0, prod1, B, m, slab[d][0], slab[d][1], st);
        if (rc != 0) return rc;
        s0[d] = slab[d][0], s1[d] = slab[d][1], lv[d] = pw[k].level;
    }
    const uint32_t *t0[kAffineMaxTerms], *t1[kAffineMaxTerms];
    uint32_t tp[kAffineMaxTerms];
    int64_t tw[kAffineMaxTerms];
    size_t T = 0;
    for (const PolyPower &p : pw)
        if (p.term) t0[T] = s0[p.d], t1[T] = s1[p.d], tp[T] = p.level, tw[T] = p.w, T++;
    return ct_affine_rescale(t0, t1, tp, tw, T, plan->c_after, B, plan->comb_level, d_out0, d_out1, st);
}

// Key-free, one launch, nothing of the context is written.
int Context::ct_mul_plain(const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t primes, const uint32_t *d_pt,
                          size_t P, size_t pt_primes, const uint32_t *d_pt_idx, uint32_t *d_out0, uint32_t *d_out1,
                          uint8_t *d_status, hipStream_t st)
{
    constexpr size_t k32 = (size_t)1 << 32;
    if (!d_in0 || !d_out0 || !d_pt || !d_in1 != !d_out1) return kErrInvalid;
    if (primes < 1 || primes > hp.nprimes || pt_primes < primes || pt_primes >= k32) return kErrInvalid;
    if (B >= k32 || P >= k32) return kErrInvalid;
    if (!d_pt_idx && P != 1 && P != B) return kErrInvalid;
    if (!aligned16({d_in0, d_in1, d_out0, d_out1, d_pt})) return kErrInvalid;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    MulPlainArgs ma{};
    ma.in0       = d_in0;
    ma.in1       = d_in1;
    ma.out0      = d_out0;
    ma.out1      = d_out1;
    ma.pt        = d_pt;
    ma.pt_idx    = d_pt_idx;
    ma.status    = d_status;
    ma.B         = (uint32_t)B;
    ma.P         = (uint32_t)P;
    ma.primes    = (uint32_t)primes;
    ma.pt_primes = (uint32_t)pt_primes;
    SEAMD_HIP(launch_ct_mul_plain(dp, ma, st));
    return 0;
}

// Key-free, one launch, nothing of the context is written.
int Context::ct_mul(const uint32_t *d_a0, const uint32_t *d_a1, size_t Ba, const uint32_t *d_b0, const uint32_t *d_b1,
                    size_t Bb, size_t primes, size_t P, const uint32_t *d_ia, const uint32_t *d_ib, uint32_t *d_out0,
                    uint32_t *d_out1, uint32_t *d_out2, uint8_t *d_status, hipStream_t st)
{
    constexpr size_t k32 = (size_t)1 << 32;
    if (!d_a0 || !d_a1 || !d_b0 || !d_b1 || !d_out0 || !d_out1 || !d_out2 || !d_ia != !d_ib) return kErrInvalid;
    if (primes < 1 || primes > hp.nprimes || P >= k32 || Ba >= k32 || Bb >= k32) return kErrInvalid;
    if (!d_ia && (P != Ba || P != Bb)) return kErrInvalid;
    if (!aligned16({d_a0, d_a1, d_b0, d_b1, d_out0, d_out1, d_out2})) return kErrInvalid;
    if (P == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    MulArgs ma{};
    ma.a0     = d_a0;
    ma.a1     = d_a1;
    ma.b0     = d_b0;
    ma.b1     = d_b1;
    ma.ia     = d_ia;
    ma.ib     = d_ib;
    ma.out0   = d_out0;
    ma.out1   = d_out1;
    ma.out2   = d_out2;
    ma.status = d_status;
    ma.P      = (uint32_t)P;
    ma.Ba     = (uint32_t)Ba;
    ma.Bb     = (uint32_t)Bb;
    ma.primes = (uint32_t)primes;
    SEAMD_HIP(launch_ct_mul(dp, ma, st));
    return 0;
}

// The tensor summed over CSR rows of pairs (MulSumArgs).  dot false: key-free, (T0, T1, T2) to three slabs, nothing of
// the context is written.  dot true: T2 of every row key-switched under the installed special-prime relinearisation
// key inside the same launch (the digit key, Galois keys and a switch ring do not serve), d_out2 unused.  One launch, no
// scratch, no host synchronisation; the pair indices are compared with Ba / Bb inside the kernel (status 2).
int Context::ct_mul_sum(const uint32_t *d_a0, const uint32_t *d_a1, size_t Ba, const uint32_t *d_b0, const uint32_t *d_b1,
                        size_t Bb, size_t primes, size_t G, const uint32_t *d_row_ptr, const uint32_t *d_ia,
                        const uint32_t *d_ib, size_t nnz, bool dot, uint32_t *d_out0, uint32_t *d_out1, uint32_t *d_out2,
                        uint8_t *d_status, hipStream_t st)
{
    if (dot && !special_prime_ok()) return kErrInvalid;
    constexpr size_t k32 = (size_t)1 << 32;
    if (!d_a0 || !d_a1 || !d_b0 || !d_b1 || !d_out0 || !d_out1 || (!dot && !d_out2) || !d_row_ptr || !d_ia != !d_ib)
        return kErrInvalid;
    if (primes < 1 || primes > hp.nprimes - dot || G >= k32 || nnz >= k32 || Ba >= k32 || Bb >= k32) return kErrInvalid;
    if (!d_ia && (nnz != Ba || nnz != Bb)) return kErrInvalid;
    if (!aligned16({d_a0, d_a1, d_b0, d_b1, d_out0, d_out1, d_out2})) return kErrInvalid;
    MulSumArgs ma{};
    ma.a0      = d_a0;
    ma.a1      = d_a1;
    ma.b0      = d_b0;
    ma.b1      = d_b1;
    ma.row_ptr = d_row_ptr;
    ma.ia      = d_ia;
    ma.ib      = d_ib;
    ma.out0    = d_out0;
    ma.out1    = d_out1;
    ma.out2    = d_out2;
    ma.status  = d_status;
    ma.G       = (uint32_t)G;
    ma.nnz     = (uint32_t)nnz;
    ma.Ba      = (uint32_t)Ba;
    ma.Bb      = (uint32_t)Bb;
    ma.np      = (uint32_t)hp.nprimes;
    ma.primes  = (uint32_t)primes;
    if (!dot)
    {
        if (G == 0) return 0;
        SEAMD_HIP(hipSetDevice(device));
        SEAMD_HIP(launch_ct_mul_sum(dp, ma, st));
        return 0;
    }
    std::lock_guard<std::mutex> lk(mu);
    const uint32_t *key = (const uint32_t *)evk[1].relin;
    if (!key)
    {
        set_last_error("no special-prime relinearisation key is installed (se_amd_set_relin_key_sp)");
        return kErrNoKey;
    }
    if (G == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    ma.key  = key;
    ma.half = evk_rows(true) * hp.nprimes * 2 * hp.n;
    SEAMD_HIP(launch_ct_dot_sp(dp, dt, host_rescale_params(hp, hp.nprimes), ma, st));
    return 0;
}

// One device evaluation-key block [2][R][np][2][n] (kernels/kernel_args.h) from the host's halves k0, k1 [R][np][n],
// R = 2 np rows of a digit key or np - 1 of a special-prime key:
// staged through `stage`, every column given its Shoup companions on the device (launch_relin_key_rows), and
// synchronised -- `stage` may be reused, and every call enqueued before has finished.  The caller holds `mu`, has the
// device current and has checked the words.
int Context::build_evk(const uint32_t *k0, const uint32_t *k1, size_t R, DevBuf<uint32_t> &stage,
                       DevBuf<uint32_t> &block)
{
    SEAMD_HIP(block.grow(4 * R * hp.nprimes * hp.n));
    return build_evk_at(k0, k1, R, stage, block);
}

// the same into 4 R np n words the caller owns: one block of a ring
int Context::build_evk_at(const uint32_t *k0, const uint32_t *k1, size_t R, DevBuf<uint32_t> &stage, uint32_t *block)
{
    const size_t slab = R * hp.nprimes * hp.n;
    SEAMD_HIP(stage.grow(2 * slab));
    SEAMD_HIP(hipMemcpy(stage, k0, slab * sizeof(uint32_t), hipMemcpyHostToDevice));
    SEAMD_HIP(hipMemcpy(stage + slab, k1, slab * sizeof(uint32_t), hipMemcpyHostToDevice));
    SEAMD_HIP(launch_relin_key_rows(dp, stage, block, 2 * R, nullptr));
    SEAMD_HIP(hipDeviceSynchronize());
    return 0;
}

// What every key-switch call checks and fills alike: every slab pointer present and 16-byte aligned, the level and the
// batch in range; then the fields of the argument block that describe the batch and the key layout.  sp: a
// special-prime key, whose records have at most np - 1 primes and whose halves have np - 1 rows.
template <class Args>
bool Context::evk_call_args(Args &a, std::initializer_list<const void *> slabs, size_t B, size_t primes, bool sp) const
{
    for (const void *p : slabs)
        if (!p) return false;
    if (primes < 1 || primes > hp.nprimes - sp || B >= ((size_t)1 << 32) || !aligned16(slabs)) return false;
    a.half   = evk_rows(sp) * hp.nprimes * 2 * hp.n;
    a.B      = B;
    a.np     = (uint32_t)hp.nprimes;
    a.primes = (uint32_t)primes;
    return true;
}

const uint32_t *EvalKeys::find(uint32_t elt) const
{
    for (size_t g = 0; g < elts.size(); g++)
        if (elts[g] == elt) return galois[g];
    return nullptr;
}

// The elements of a call: 1 .. kMaxGaloisKeys of them (else the last error is `count_msg`), each one a Galois element;
// distinct: and none listed twice (an installed set).
bool Context::galois_elts_ok(const uint32_t *elts, size_t G, const char *count_msg, bool distinct) const
{
    if (!elts || G == 0 || G > kMaxGaloisKeys)
    {
        set_last_error(count_msg);
        return false;
    }
    for (size_t g = 0; g < G; g++)
    {
        bool bad = !galois_elt_ok(elts[g]);
        for (size_t h = 0; distinct && h < g; h++) bad |= elts[h] == elts[g];
        if (bad)
        {
            set_last_error("Galois element " + std::to_string(elts[g]) +
                           (distinct ? " is even, not below 2n, or listed twice" : " is not odd and below 2n"));
            return false;
        }
    }
    return true;
}

// The installed block of `elt` in a family; without one NULL and the last error set: the caller returns kErrNoKey.  The
// caller holds `mu`.
const uint32_t *Context::galois_key(bool sp, uint32_t elt) const
{
    const uint32_t *key = evk[sp].find(elt);
    if (!key)
        set_last_error(std::string("no ") + (sp ? "special-prime " : "") + "Galois key is installed for element " +
                       std::to_string(elt) + (sp ? " (se_amd_set_galois_keys_sp)" : " (se_amd_set_galois_keys)"));
    return key;
}

// evk_call_args on an element-set block, whose four slabs it fills too (a composite replaces them per chunk).
bool Context::set_call_args(GaloisSetArgs &a, const uint32_t *c0, const uint32_t *c1, uint32_t *out0, uint32_t *out1,
                            size_t B, size_t primes, bool sp) const
{
    if (!evk_call_args(a, {c0, c1, out0, out1}, B, primes, sp)) return false;
    a.c0   = c0;
    a.c1   = c1;
    a.out0 = out0;
    a.out1 = out1;
    return true;
}

// The elements of a call and the installed block of each in a family, into the block.  one_keyless: element 1 is the
// identity and needs no key (NULL).  kErrNoKey, with galois_key's last error, at the first element without its key.  The
// caller holds `mu` and has checked the elements (galois_elts_ok).
int Context::resolve_keys(GaloisSetArgs &a, const uint32_t *elts, size_t G, bool sp, bool one_keyless) const
{
    a.G = (uint32_t)G;
    for (size_t e = 0; e < G; e++)
    {
        const bool keyless = one_keyless && elts[e] == 1;
        a.elt[e] = elts[e];
        a.key[e] = keyless ? nullptr : galois_key(sp, elts[e]);
        if (!keyless && !a.key[e]) return kErrNoKey;
    }
    return 0;
}

// A plan serves the context that made it, the entry of its kind and the levels up to its own; else the last error is
// set.  `what` names the transform, `create` the digit-key creator, `level_msg` what a level above the plan's means.
template <class Plan>
bool Context::plan_ok(const Plan *plan, bool sp, size_t primes, const char *what, const char *create,
                      const char *level_msg) const
{
    if (plan && plan->owner == this && plan->sp == sp && primes <= plan->levels) return true;
    const std::string w = std::string(what) + ": ", c = create;
    set_last_error(w + (!plan ? "no plan"
                        : plan->owner != this ? "the plan belongs to another context"
                        : plan->sp != sp ? (sp ? "a digit-key plan (" + c + ") does not serve the special-prime entry"
                                               : "a special-prime plan (" + c + "_sp) does not serve the digit-key entry")
                                         : std::string(level_msg)));
    return false;
}

// Evaluation keys are public material: validated like a public key (a word >= q_i is refused), then built beside the
// installed key and swapped in once every call already enqueued has finished (build_evk ends in a synchronisation).
// Anything refused, or a HIP call that fails, leaves the previous key installed and usable.
int Context::set_relin_key(const uint32_t *evk0, const uint32_t *evk1, bool sp)
{
    if (sp && !special_prime_ok()) return kErrInvalid;
    const size_t R = evk_rows(sp);
    if (const size_t r = first_unreduced_row(hp, evk0, evk1, R); r != R)
    {
        set_last_error("relinearisation key: row " + std::to_string(r) + " holds a word not reduced modulo its prime");
        return kErrInvalid;
    }
    std::lock_guard<std::mutex> lk(mu);
    SEAMD_HIP(hipSetDevice(device));
    DevBuf<uint32_t> stage, block;
    if (int rc = build_evk(evk0, evk1, R, stage, block)) return rc;
    evk[sp].relin = std::move(block);
    return 0;
}

// One launch, no scratch, no secret key; reads the installed relinearisation key.
int Context::ct_relin(const uint32_t *d_d0, const uint32_t *d_d1, const uint32_t *d_d2, size_t B, size_t primes,
                      uint32_t *d_out0, uint32_t *d_out1, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(mu);
    if (!evk[0].relin)
    {
        set_last_error("relinearisation needs an evaluation key (se_amd_set_relin_key)");
        return kErrNoKey;
    }
    RelinArgs ra{};
    if (!evk_call_args(ra, {d_d0, d_d1, d_d2, d_out0, d_out1}, B, primes)) return kErrInvalid;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    ra.d0   = d_d0;
    ra.d1   = d_d1;
    ra.d2   = d_d2;
    ra.out0 = d_out0;
    ra.out1 = d_out1;
    ra.key  = evk[0].relin;
    SEAMD_HIP(launch_ct_relin(dp, dt, ra, st));
    return 0;
}

// Galois keys: per element the chain of gen_relin_key on that element's block of seeds, with the diagonal term
// 2^(15 t) sigma(s_hat) instead of 2^(15 t) s_hat^2 (kernels/ct_ops.hip, k_evk_diag).
int Context::gen_galois_keys(const uint8_t *sk_packed, const uint32_t *elts, size_t G, const uint8_t *a_seeds,
                             const uint8_t *e_seeds, uint32_t *gk0_out, uint32_t *gk1_out, bool sp)
{
    if (sp && !special_prime_ok()) return kErrInvalid;
    if (!galois_elts_ok(elts, G, "Galois keys: between 1 and 64 elements")) return kErrInvalid;
    if (!evk_secret_ok(sk_packed)) return kErrInvalid;
    std::lock_guard<std::mutex> lk(mu);
    const size_t R = evk_rows(sp), slab = R * hp.nprimes * hp.n;
    for (size_t g = 0; g < G; g++)
    {
        const int rc = gen_keys_chain({KeyChain::kGalois, elts[g], sp}, R, sk_packed, nullptr, a_seeds + g * R * 64,
                                      e_seeds + g * R * 64, nullptr, gk0_out + g * slab, gk1_out + g * slab);
        if (rc) return rc;
    }
    return 0;
}

// The whole installed set is replaced, by the rule of set_relin_key: one block per element, swapped in together.
int Context::set_galois_keys(const uint32_t *elts, size_t G, const uint32_t *gk0, const uint32_t *gk1, bool sp)
{
    if (sp && !special_prime_ok()) return kErrInvalid;
    const size_t n = hp.n, np = hp.nprimes, R = evk_rows(sp), slab = R * np * n;
    if (!galois_elts_ok(elts, G, "Galois keys: between 1 and 64 elements", true)) return kErrInvalid;
    if (const size_t r = first_unreduced_row(hp, gk0, gk1, G * R); r != G * R)
    {
        set_last_error("Galois key of element " + std::to_string(elts[r / R]) + ": row " + std::to_string(r % R) +
                       " holds a word not reduced modulo its prime");
        return kErrInvalid;
    }
    std::lock_guard<std::mutex> lk(mu);
    SEAMD_HIP(hipSetDevice(device));
    DevBuf<uint32_t> stage;
    std::vector<DevBuf<uint32_t>> blocks(G);
    for (size_t g = 0; g < G; g++)
        if (int rc = build_evk(gk0 + g * slab, gk1 + g * slab, R, stage, blocks[g])) return rc;
    evk[sp].elts.assign(elts, elts + G);
    evk[sp].galois = std::move(blocks);
    return 0;
}

// One launch, no scratch, no secret key; reads the installed special-prime key: the relinearisation key (elt 0) or the
// Galois key of `elt`.  The digit keys do not serve it.  The checks of ct_galois in their order, with the level in
// [1, np - 1].
int Context::ct_key_switch_sp(const uint32_t *d_a0, const uint32_t *d_a1, const uint32_t *d_sw, size_t B, size_t primes,
                              uint32_t elt, uint32_t *d_out0, uint32_t *d_out1, hipStream_t st)
{
    if (!special_prime_ok()) return kErrInvalid;
    const bool rot = elt != 0;
    KeySwitchSpArgs ka{};
    // a rotation has no a1: a0 stands in its place
    if (!evk_call_args(ka, {d_a0, rot ? d_a0 : d_a1, d_sw, d_out0, d_out1}, B, primes, true)) return kErrInvalid;
    if (rot && !galois_elt_ok(elt)) return kErrInvalid;
    std::lock_guard<std::mutex> lk(mu);
    const uint32_t *key = rot ? galois_key(true, elt) : (const uint32_t *)evk[1].relin;
    if (!key)
    {
        if (!rot) set_last_error("no special-prime relinearisation key is installed (se_amd_set_relin_key_sp)");
        return kErrNoKey;
    }
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    ka.a0   = d_a0;
    ka.a1   = d_a1;
    ka.sw   = d_sw;
    ka.out0 = d_out0;
    ka.out1 = d_out1;
    ka.key  = key;
    ka.elt  = elt;
    SEAMD_HIP(launch_ct_key_switch_sp(dp, dt, host_rescale_params(hp, hp.nprimes), ka, st));
    return 0;
}

// Switching keys: per key k the chain of gen_relin_key's special-prime form under sk_to on that key's block of seeds,
// with the diagonal (q_{np-1} mod q_j) . NTT_j(s_from_k) instead of s_hat^2: row j hides P . s_from_k under s_to.  Needs
// BOTH secrets -- it belongs to whoever issued the device keys -- and installs nothing.
int Context::gen_switch_keys(size_t K, const uint8_t *sk_from, const uint8_t *sk_to, const uint8_t *a_seeds,
                             const uint8_t *e_seeds, uint32_t *wk0_out, uint32_t *wk1_out)
{
    if (!special_prime_ok()) return kErrInvalid;
    if (K == 0)
    {
        set_last_error("switching keys: at least one source key");
        return kErrInvalid;
    }
    if (!evk_secret_ok(sk_to)) return kErrInvalid;
    for (size_t k = 0; k < K; k++)
        if (!evk_secret_ok(sk_from + k * (hp.n / 4))) return kErrInvalid;
    std::lock_guard<std::mutex> lk(mu);
    const size_t R = evk_rows(true), slab = R * hp.nprimes * hp.n;
    for (size_t k = 0; k < K; k++)
    {
        const int rc = gen_keys_chain({KeyChain::kSwitch, 0, true, sk_from + k * (hp.n / 4)}, R, sk_to, nullptr,
                                      a_seeds + k * R * 64, e_seeds + k * R * 64, nullptr, wk0_out + k * slab,
                                      wk1_out + k * slab);
        if (rc) return rc;
    }
    return 0;
}

// The ring is public material, validated and built by the rule of set_relin_key: beside the installed ring, every
// block by build_evk_at (which ends in a synchronisation: calls already enqueued have finished on the old ring), and
// swapped in at the end.  Anything refused, or a HIP call that fails, leaves the previous ring installed and usable.
int Context::set_switch_keyring(size_t K, const uint32_t *wk0, const uint32_t *wk1)
{
    if (!special_prime_ok()) return kErrInvalid;
    if (K == 0 || K >= ((size_t)1 << 32))
    {
        set_last_error("switch-key ring: between 1 and 2^32 - 1 keys");
        return kErrInvalid;
    }
    const size_t R = evk_rows(true), slab = R * hp.nprimes * hp.n;
    if (const size_t r = first_unreduced_row(hp, wk0, wk1, K * R); r != K * R)
    {
        set_last_error("switch-key ring: key " + std::to_string(r / R) + ", row " + std::to_string(r % R) +
                       " holds a word not reduced modulo its prime");
        return kErrInvalid;
    }
    std::lock_guard<std::mutex> lk(mu);
    SEAMD_HIP(hipSetDevice(device));
    DevBuf<uint32_t> stage, ring;
    SEAMD_HIP(ring.grow(K * 4 * slab));
    for (size_t k = 0; k < K; k++)
        if (int rc = build_evk_at(wk0 + k * slab, wk1 + k * slab, R, stage, ring + k * 4 * slab)) return rc;
    d_switch_ring = std::move(ring);
    switch_keys   = K;
    return 0;
}

// One launch, no scratch, no secret key, no host synchronisation; reads the installed switch-key ring.  The key indices
// are compared with K inside the kernel (status 2), never sanitised on the way.  sum: the CSR rows of ct_lincomb.
int Context::ct_switch_keyed_sp(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                                const uint32_t *d_key_idx, bool sum, size_t G, const uint32_t *d_row_ptr,
                                const uint32_t *d_idx, size_t nnz, uint32_t *d_out0, uint32_t *d_out1,
                                uint8_t *d_status, hipStream_t st)
{
    if (!special_prime_ok()) return kErrInvalid;
    constexpr size_t k32 = (size_t)1 << 32;
    SwitchSpArgs sa{};
    if (!evk_call_args(sa, {d_c0, d_c1, d_out0, d_out1}, B, primes, true) || !d_key_idx) return kErrInvalid;
    if (sum &&(!d_row_ptr || (!d_idx && nnz) || G >= k32 || nnz >= k32)) return kErrInvalid;
    std::lock_guard<std::mutex> lk(mu);
    if (!switch_keys)
    {
        set_last_error("no switch-key ring is installed (se_amd_set_switch_keyring_sp)");
        return kErrNoKey;
    }
    const size_t rows = sum ? G : B;
    if (rows == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    sa.c0      = d_c0;
    sa.c1      = d_c1;
    sa.out0    = d_out0;
    sa.out1    = d_out1;
    sa.ring    = d_switch_ring;
    sa.key_idx = d_key_idx;
    sa.row_ptr = sum ? d_row_ptr : nullptr;
    sa.idx     = sum ? d_idx : nullptr;
    sa.status  = d_status;
    sa.stride  = 2 * sa.half;
    sa.rows    = rows;
    sa.nnz     = nnz;
    sa.K       = (uint32_t)switch_keys;
    SEAMD_HIP(launch_ct_switch_sp(dp, dt, host_rescale_params(hp, hp.nprimes), sa, st));
    return 0;
}

// Slot packing.  The checks of ct_key_switch_sp in their order (a context of one prime, the slabs, the level in
// [1, np - 1], alignment), then the entry tables and the elements; under `mu` the special-prime Galois key of every
// listed element other than 1, read NOW (the digit keys, the relinearisation key and the switch ring do not serve);
// nothing is launched unless every such element has one.  One launch, no scratch, no host synchronisation: the record
// and element indices are compared inside the kernel (status 2), never sanitised on the way.
int Context::ct_pack_sp(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, const uint32_t *elts,
                        size_t E, size_t G, const uint32_t *d_row_ptr, const uint32_t *d_idx, const uint32_t *d_eidx,
                        size_t nnz, uint32_t *d_out0, uint32_t *d_out1, uint8_t *d_status, hipStream_t st)
{
    if (!special_prime_ok()) return kErrInvalid;
    constexpr size_t k32 = (size_t)1 << 32;
    PackSpArgs pa{};
    if (!set_call_args(pa, d_c0, d_c1, d_out0, d_out1, B, primes, true) || !d_eidx) return kErrInvalid;
    const bool single = !d_row_ptr && !d_idx;
    if (!single && (!d_row_ptr || !d_idx))
    {
        set_last_error("slot packing: d_row_ptr and d_idx are given together, or both NULL (the single form)");
        return kErrInvalid;
    }
    if (single && (G != B || nnz != B))
    {
        set_last_error("slot packing: the single form takes one entry per record, G = B = nnz");
        return kErrInvalid;
    }
    if (G >= k32 || nnz >= k32) return kErrInvalid;
    if (!galois_elts_ok(elts, E, "slot packing: between 1 and 64 elements")) return kErrInvalid;
    std::lock_guard<std::mutex> lk(mu);
    if (int rc = resolve_keys(pa, elts, E, true, true)) return rc;
    if (G == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    pa.row_ptr = d_row_ptr;
    pa.idx     = d_idx;
    pa.eidx    = d_eidx;
    pa.status  = d_status;
    pa.rows    = G;
    pa.nnz     = nnz;
    SEAMD_HIP(launch_ct_pack_sp(dp, dt, host_rescale_params(hp, hp.nprimes), pa, st));
    return 0;
}

// Rows 0 .. primes_out-1 of every record: [B][primes_in][n] -> [B][primes_out][n], one pitched asynchronous device copy
// per slab, no kernel.  Dropping primes changes neither message nor scale.
int Context::ct_drop_primes(const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t primes_in, size_t primes_out,
                            uint32_t *d_out0, uint32_t *d_out1, hipStream_t st)
{
    if (!d_in0 || !d_out0 || !d_in1 != !d_out1) return kErrInvalid;
    if (primes_out < 1 || primes_out > primes_in || primes_in > hp.nprimes || B >= ((size_t)1 << 32)) return kErrInvalid;
    if (!aligned16({d_in0, d_in1, d_out0, d_out1})) return kErrInvalid;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    const size_t in_row = primes_in * hp.n * sizeof(uint32_t), out_row = primes_out * hp.n * sizeof(uint32_t);
    SEAMD_HIP(hipMemcpy2DAsync(d_out0, out_row, d_in0, in_row, out_row, B, hipMemcpyDeviceToDevice, st));
    if (d_in1) SEAMD_HIP(hipMemcpy2DAsync(d_out1, out_row, d_in1, in_row, out_row, B, hipMemcpyDeviceToDevice, st));
    return 0;
}

// One launch, no scratch, no secret key; reads the installed Galois key of `elt`.
int Context::ct_galois(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, uint32_t elt,
                       uint32_t *d_out0, uint32_t *d_out1, hipStream_t st)
{
    GaloisArgs ga{};
    if (!evk_call_args(ga, {d_c0, d_c1, d_out0, d_out1}, B, primes)) return kErrInvalid;
    if (!galois_elt_ok(elt)) return kErrInvalid;
    std::lock_guard<std::mutex> lk(mu);
    const uint32_t *key = galois_key(false, elt);
    if (!key) return kErrNoKey;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    ga.c0   = d_c0;
    ga.c1   = d_c1;
    ga.out0 = d_out0;
    ga.out1 = d_out1;
    ga.key  = key;
    ga.elt  = elt;
    SEAMD_HIP(launch_ct_galois(dp, dt, ga, st));
    return 0;
}

// One launch, no scratch, no secret key, no host synchronisation; reads the installed Galois keys of elts[0 .. G).  The
// checks of ct_galois in its order, the element check once per element; nothing is launched unless every element has a
// key.  The key-block pointers travel in the argument block, so a call already enqueued keeps the blocks it was given.
// sp (the sum form only): on the special-prime keys, the digit keys do not serve it -- the checks of ct_key_switch_sp (a
// context of one prime, the level in [1, np - 1]) in front; one decomposition and one division by P whatever G is.
int Context::ct_galois_hoist(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, const uint32_t *elts,
                             size_t G, bool sum, bool add_input, uint32_t *d_out0, uint32_t *d_out1, hipStream_t st,
                             bool sp)
{
    if (sp && !special_prime_ok()) return kErrInvalid;
    GaloisSetArgs a{};
    if (!set_call_args(a, d_c0, d_c1, d_out0, d_out1, B, primes, sp)) return kErrInvalid;
    if (!galois_elts_ok(elts, G, "hoisted rotations: between 1 and 64 elements")) return kErrInvalid;
    std::lock_guard<std::mutex> lk(mu);
    if (int rc = resolve_keys(a, elts, G, sp, false)) return rc;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    if (sp)
    {
        HoistSpArgs hs{a};
        hs.add_input = add_input;
        SEAMD_HIP(launch_ct_hoist_sp(dp, dt, host_rescale_params(hp, hp.nprimes), hs, st));
        return 0;
    }
    GaloisHoistArgs ha{a};
    ha.sum       = sum;
    ha.add_input = sum && add_input;
    SEAMD_HIP(launch_ct_galois_hoist(dp, dt, ha, st));
    return 0;
}

// The plan of a linear transform.  Argument checks first, then under `mu`: every element needs an installed key (the
// blocks are read, not kept); one fold launch per entry and one for d0, then a synchronisation, so the caller's
// diagonals and the installed blocks may go once this returns.  Anything refused leaves `plan` empty.
// sp: on the special-prime keys.  The diagonals must have all np rows -- the row at the special prime is folded into key
// column np - 1 -- and the plan serves the levels 1 .. np - 1.
int Context::lintrans_create(const uint32_t *elts, size_t G, const uint32_t *d_diag, const uint32_t *d_diag0,
                             size_t pt_primes, LintransPlan &plan, bool sp)
{
    if (sp && !special_prime_ok()) return kErrInvalid;
    const size_t n = hp.n, np = hp.nprimes;
    const char *args_msg = sp ? "special-prime linear transform: between 1 and 64 elements, pt_primes = the context's "
                                "primes, 16-byte aligned diagonals"
                              : "linear transform: between 1 and 64 elements, pt_primes >= 1, 16-byte aligned diagonals";
    if (!d_diag || pt_primes == 0 || (sp && pt_primes != np) || !aligned16({d_diag, d_diag0}))
    {
        set_last_error(args_msg);
        return kErrInvalid;
    }
    if (!galois_elts_ok(elts, G, args_msg)) return kErrInvalid;
    std::lock_guard<std::mutex> lk(mu);
    GaloisSetArgs from{};
    if (int rc = resolve_keys(from, elts, G, sp, false)) return rc;
    SEAMD_HIP(hipSetDevice(device));
    // the diagonal columns that are folded: all of a special-prime plan's, the first pt_primes of a digit plan's
    const size_t cols = pt_primes < np ? pt_primes : np, pairs = np * 2 * n, R = evk_rows(sp), block = 2 * R * pairs;
    LintransPlan built;
    built.keys.resize(G);
    SEAMD_HIP(built.diag.grow((G + 1) * pairs));
    for (size_t e = 0; e < G; e++)
    {
        SEAMD_HIP(built.keys[e].grow(block));
        SEAMD_HIP(launch_lintrans_fold(dp, from.key[e], built.keys[e], R, d_diag + e * pt_primes * n,
                                       built.diag + e * pairs, (uint32_t)cols, nullptr));
    }
    if (d_diag0)
        SEAMD_HIP(launch_lintrans_fold(dp, nullptr, nullptr, R, d_diag0, built.diag + G * pairs, (uint32_t)cols, nullptr));
    SEAMD_HIP(hipDeviceSynchronize());
    built.owner  = this;
    built.device = device;
    built.levels = sp ? np - 1 : cols;
    built.sp     = sp;
    built.diag0  = d_diag0 != nullptr;
    built.elts.assign(elts, elts + G);
    plan = std::move(built);
    return 0;
}

// One launch, no scratch, no host synchronisation, nothing of the context but its tables: the plan owns what the kernel
// reads.  The checks of ct_galois first (sp: of ct_key_switch_sp), then the plan's: a plan serves the entry of its kind.
int Context::ct_lintrans(const LintransPlan *plan, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                         uint32_t *d_out0, uint32_t *d_out1, hipStream_t st, bool sp)
{
    if (sp && !special_prime_ok()) return kErrInvalid;
    GaloisSetArgs a{};
    if (!set_call_args(a, d_c0, d_c1, d_out0, d_out1, B, primes, sp)) return kErrInvalid;
    if (!plan_ok(plan, sp, primes, "linear transform", "se_amd_lintrans_create",
                 "the plan's diagonals have fewer primes than the call"))
        return kErrInvalid;
    if (B == 0) return 0;
    std::lock_guard<std::mutex> lk(mu);
    SEAMD_HIP(hipSetDevice(device));
    const size_t G = plan->elts.size(), pairs = hp.nprimes * 2 * hp.n;
    const uint32_t *diag0 = plan->diag0 ? plan->diag + G * pairs : nullptr;
    a.G = (uint32_t)G;
    for (size_t e = 0; e < G; e++)
    {
        a.elt[e] = plan->elts[e];
        a.key[e] = plan->keys[e];
    }
    if (sp)
    {
        HoistSpArgs hs{a};
        hs.weighted = 1;
        hs.diag     = plan->diag;
        hs.diag0    = diag0;
        SEAMD_HIP(launch_ct_hoist_sp(dp, dt, host_rescale_params(hp, hp.nprimes), hs, st));
        return 0;
    }
    LintransArgs la{a};
    la.diag  = plan->diag;
    la.diag0 = diag0;
    SEAMD_HIP(launch_ct_lintrans(dp, dt, la, st));
    return 0;
}

// The unchecked halves of the step entries below, which the composites (ct_bsgs, ct_bsgs_sp) call too: fill the argument
// block and launch.  The caller has made the entry's checks and has the device current.  `primes` is the LEVEL of the
// records; sp: extended records of primes + 1 rows, the last one modulo the special prime against row np - 1 of
// plaintexts that have all np rows.  These alone know that convention.
int Context::mul_plain_sum_step(const uint32_t *d_in0, const uint32_t *d_in1, size_t E, size_t B, size_t primes,
                                const uint32_t *d_pt, size_t Gout, size_t pt_primes, uint32_t *d_out0, uint32_t *d_out1,
                                bool sp, hipStream_t st)
{
    MulPlainSumArgs ma{};
    ma.in0        = d_in0;
    ma.in1        = d_in1;
    ma.pt         = d_pt;
    ma.out0       = d_out0;
    ma.out1       = d_out1;
    ma.B          = (uint32_t)B;
    ma.E          = (uint32_t)E;
    ma.Gout       = (uint32_t)Gout;
    ma.primes     = (uint32_t)(primes + sp);
    ma.pt_primes  = (uint32_t)(sp ? hp.nprimes : pt_primes);
    ma.last_prime = (uint32_t)(sp ? hp.nprimes : primes) - 1;
    SEAMD_HIP(launch_ct_mul_plain_sum(dp, ma, st));
    return 0;
}

int Context::mod_down_sp_step(const uint32_t *d_in0, const uint32_t *d_in1, size_t count, size_t primes,
                              uint32_t *d_out0, uint32_t *d_out1, hipStream_t st)
{
    RescaleArgs ra{};
    ra.in0    = d_in0;
    ra.in1    = d_in1;
    ra.out0   = d_out0;
    ra.out1   = d_out1;
    ra.primes = (uint32_t)primes + 1;
    ra.drop   = (uint32_t)hp.nprimes - 1;
    SEAMD_HIP(launch_ct_mod_down_sp(dp, dt, host_rescale_params(hp, hp.nprimes), ra, count, st));
    return 0;
}

int Context::galois_accum_step(const GaloisSetArgs &aa, bool sp, hipStream_t st)
{
    if (sp)
        SEAMD_HIP(launch_ct_galois_accum_sp(dp, dt, host_rescale_params(hp, hp.nprimes), aa, st));
    else
        SEAMD_HIP(launch_ct_galois_accum(dp, dt, aa, st));
    return 0;
}

// Key-free, one launch, nothing of the context is written.  The checks of ct_mul_plain, then the stack's.
// sp: on stacks of extended records, behind the check of ct_key_switch_sp for a context of one prime; the level is in
// [1, np - 1] and pt_primes is not read.
int Context::ct_mul_plain_sum(const uint32_t *d_in0, const uint32_t *d_in1, size_t E, size_t B, size_t primes,
                              const uint32_t *d_pt, size_t Gout, size_t pt_primes, uint32_t *d_out0, uint32_t *d_out1,
                              hipStream_t st, bool sp)
{
    constexpr size_t k32 = (size_t)1 << 32;
    if (sp && !special_prime_ok()) return kErrInvalid;
    if (!d_in0 || !d_out0 || !d_pt || !d_in1 != !d_out1) return kErrInvalid;
    if (primes < 1 || primes > hp.nprimes - sp || (!sp && (pt_primes < primes || pt_primes >= k32))) return kErrInvalid;
    if (B >= k32 || !aligned16({d_in0, d_in1, d_out0, d_out1, d_pt})) return kErrInvalid;
    if (E < 1 || E > kMaxGaloisKeys || Gout < 1 || Gout > kMaxGaloisKeys || E * B >= k32 || Gout * B >= k32)
    {
        set_last_error("weighted sum over a stack: E and Gout between 1 and 64, E B and Gout B below 2^32");
        return kErrInvalid;
    }
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    return mul_plain_sum_step(d_in0, d_in1, E, B, primes, d_pt, Gout, pt_primes, d_out0, d_out1, sp, st);
}

// One launch, no scratch, no secret key, no host synchronisation; reads the installed Galois keys of the elements other
// than 1.  The checks of ct_galois_hoist in its order, then G B; nothing is launched unless every such element has a key.
// sp: on the special-prime keys with ONE division by P, the checks of ct_key_switch_sp in front.
int Context::ct_galois_accum(const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t primes, const uint32_t *elts,
                             size_t G, uint32_t *d_out0, uint32_t *d_out1, hipStream_t st, bool sp)
{
    if (sp && !special_prime_ok()) return kErrInvalid;
    GaloisSetArgs aa{};
    if (!set_call_args(aa, d_in0, d_in1, d_out0, d_out1, B, primes, sp)) return kErrInvalid;
    if (!galois_elts_ok(elts, G, "rotate and accumulate: between 1 and 64 elements")) return kErrInvalid;
    if (G * B >= ((size_t)1 << 32))
    {
        set_last_error("rotate and accumulate: G B must stay below 2^32");
        return kErrInvalid;
    }
    std::lock_guard<std::mutex> lk(mu);
    if (int rc = resolve_keys(aa, elts, G, sp, true)) return rc;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    return galois_accum_step(aa, sp, st);
}

// The plan of a baby-step / giant-step transform: argument checks, then one permutation launch per giant step -- row
// (g, b) of the caller's diagonals by giant[g]^-1, written to the slot of baby[b] with element 1 moved to the front --
// and a synchronisation, so the caller's diagonals may go once this returns.  No key is read.  Anything refused leaves
// `plan` empty.
// sp: the plan of ct_bsgs_sp.  The diagonals must have all np rows -- the row at the special prime meets row L of the
// extended records -- and the plan serves the levels 1 .. np - 1.
int Context::bsgs_create(const uint32_t *baby, size_t n1, const uint32_t *giant, size_t n2, const uint32_t *d_diag,
                         size_t pt_primes, BsgsPlan &plan, bool sp)
{
    if (sp && !special_prime_ok()) return kErrInvalid;
    const char *args_msg = sp ? "special-prime baby-step / giant-step plan: between 1 and 64 distinct elements in each "
                                "list, pt_primes = the context's primes, 16-byte aligned diagonals"
                              : "baby-step / giant-step plan: between 1 and 64 distinct elements in each list, pt_primes "
                                ">= 1, 16-byte aligned diagonals";
    if (!d_diag || pt_primes == 0 || pt_primes >= ((size_t)1 << 32) || (sp && pt_primes != hp.nprimes) ||
        !aligned16({d_diag}))
    {
        set_last_error(args_msg);
        return kErrInvalid;
    }
    if (!galois_elts_ok(baby, n1, args_msg, true) || !galois_elts_ok(giant, n2, args_msg, true)) return kErrInvalid;
    const size_t n = hp.n, np = hp.nprimes, rows = n1 * pt_primes;
    BsgsPlan built;
    // the slot of every baby step: element 1 first, the others in their order behind it
    std::vector<size_t> slot(n1);
    const size_t one = std::find(baby, baby + n1, 1u) - baby;
    for (size_t b = 0, next = one < n1 ? 1 : 0; b < n1; b++) slot[b] = b == one ? 0 : next++;
    built.baby.resize(n1);
    for (size_t b = 0; b < n1; b++) built.baby[slot[b]] = baby[b];
    built.giant.assign(giant, giant + n2);
    std::lock_guard<std::mutex> lk(mu);
    SEAMD_HIP(hipSetDevice(device));
    SEAMD_HIP(built.diag.grow(n2 * rows * n));
    for (size_t g = 0; g < n2; g++)
    {
        // giant[g]^-1 mod 2n by Newton's iteration: x = a is the inverse mod 8 of an odd a, every step doubles the bits
        uint32_t inv = giant[g];
        for (int it = 0; it < 4; it++) inv *= 2 - giant[g] * inv;
        inv &= (uint32_t)(2 * n - 1);
        for (size_t b = 0; b < n1; b++)
            SEAMD_HIP(launch_bsgs_permute(dp, d_diag + (g * n1 + b) * pt_primes * n,
                                          built.diag + (g * n1 + slot[b]) * pt_primes * n, pt_primes, inv, nullptr));
    }
    SEAMD_HIP(hipDeviceSynchronize());
    built.owner     = this;
    built.device    = device;
    built.n         = n;
    built.levels    = sp ? np - 1 : pt_primes < np ? pt_primes : np;
    built.pt_primes = pt_primes;
    built.sp        = sp;
    plan            = std::move(built);
    return 0;
}

// The checks of ct_galois first, then the plan's and the workspace's, then under `mu` the keys of every element other
// than 1 (read from the context NOW: a plan holds none).  The batch is walked in chunks of Bc = min(B, workspace records);
// a chunk of c records uses the workspace as rot0 | rot1 | inner0 | inner1, stacks [n1][c] resp. [n2][c] of level-`primes`
// rows at offsets fixed by Bc.  Everything is enqueued on `st`: no context scratch, no allocation, no synchronisation.
int Context::ct_bsgs(const BsgsPlan *plan, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                     uint32_t *d_out0, uint32_t *d_out1, void *d_workspace, size_t workspace_bytes, hipStream_t st)
{
    GaloisHoistArgs ha{};
    if (!set_call_args(ha, d_c0, d_c1, d_out0, d_out1, B, primes, false)) return kErrInvalid;
    if (!plan_ok(plan, false, primes, "baby-step / giant-step transform", "se_amd_bsgs_create",
                 "the plan's diagonals have fewer primes than the call"))
        return kErrInvalid;
    const size_t n1 = plan->baby.size(), n2 = plan->giant.size(), row = primes * hp.n;
    const size_t per = bsgs_record_bytes(false, n1, n2, primes, hp.n);
    if (!d_workspace || !aligned16({d_workspace}) || workspace_bytes < per)
    {
        set_last_error("baby-step / giant-step transform: the workspace must be 16-byte aligned and hold at least one "
                       "record (se_amd_bsgs_workspace_bytes)");
        return kErrInvalid;
    }
    GaloisSetArgs aa = ha;   // the giant steps: the same batch and key layout
    std::lock_guard<std::mutex> lk(mu);
    const bool own   = plan->baby[0] == 1;   // the record itself is baby step 0
    const size_t many = n1 - own;
    if (int rc = resolve_keys(ha, plan->baby.data() + own, many, false, false)) return rc;
    if (int rc = resolve_keys(aa, plan->giant.data(), n2, false, true)) return rc;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    const size_t Bc = std::min(B, workspace_bytes / per);
    uint32_t *rot0 = static_cast<uint32_t *>(d_workspace), *rot1 = rot0 + n1 * Bc * row;
    uint32_t *inner0 = rot1 + n1 * Bc * row, *inner1 = inner0 + n2 * Bc * row;
    aa.c0 = inner0;
    aa.c1 = inner1;
    for (size_t b0 = 0; b0 < B; b0 += Bc)
    {
        const size_t c = std::min(Bc, B - b0), bytes = c * row * sizeof(uint32_t);
        const uint32_t *c0 = d_c0 + b0 * row, *c1 = d_c1 + b0 * row;
        if (own)
        {
            SEAMD_HIP(hipMemcpyAsync(rot0, c0, bytes, hipMemcpyDeviceToDevice, st));
            SEAMD_HIP(hipMemcpyAsync(rot1, c1, bytes, hipMemcpyDeviceToDevice, st));
        }
        if (many)
        {
            ha.c0   = c0;
            ha.c1   = c1;
            ha.out0 = rot0 + own * c * row;
            ha.out1 = rot1 + own * c * row;
            ha.B    = c;
            SEAMD_HIP(launch_ct_galois_hoist(dp, dt, ha, st));
        }
        if (int rc = mul_plain_sum_step(rot0, rot1, n1, c, primes, plan->diag, n2, plan->pt_primes, inner0, inner1, false,
                                        st))
            return rc;
        aa.B    = c;
        aa.out0 = d_out0 + b0 * row;
        aa.out1 = d_out1 + b0 * row;
        if (int rc = galois_accum_step(aa, false, st)) return rc;
    }
    return 0;
}

// The steps of the special-prime baby-step / giant-step transform that have no digit-key twin (the other two are
// ct_mul_plain_sum and ct_galois_accum with sp).  Each: the checks of ct_key_switch_sp in their order (a context of one
// prime, the slabs, the level in [1, np - 1], alignment), then its own; one launch, no scratch, no host synchronisation.
// The keyed one reads the installed special-prime Galois keys of the elements other than 1 (the digit keys do not serve
// it) and launches nothing unless every such element has one.
int Context::ct_galois_many_ext_sp(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                                   const uint32_t *elts, size_t G, uint32_t *d_out0, uint32_t *d_out1, hipStream_t st)
{
    if (!special_prime_ok()) return kErrInvalid;
    GaloisSetArgs ma{};
    if (!set_call_args(ma, d_c0, d_c1, d_out0, d_out1, B, primes, true)) return kErrInvalid;
    if (!galois_elts_ok(elts, G, "undivided rotations: between 1 and 64 elements")) return kErrInvalid;
    if (G * B >= ((size_t)1 << 32))
    {
        set_last_error("undivided rotations: G B must stay below 2^32");
        return kErrInvalid;
    }
    std::lock_guard<std::mutex> lk(mu);
    if (int rc = resolve_keys(ma, elts, G, true, true)) return rc;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    SEAMD_HIP(launch_ct_galois_many_ext_sp(dp, dt, ma, st));
    return 0;
}

// The division by the special prime: `count` extended records of primes + 1 rows -> records of `primes` rows.
int Context::ct_mod_down_sp(const uint32_t *d_in0, const uint32_t *d_in1, size_t count, size_t primes, uint32_t *d_out0,
                            uint32_t *d_out1, hipStream_t st)
{
    if (!special_prime_ok()) return kErrInvalid;
    if (!d_in0 || !d_out0 || !d_in1 != !d_out1) return kErrInvalid;
    if (primes < 1 || primes > hp.nprimes - 1 || count > 0x7fffffffu) return kErrInvalid;
    if (!aligned16({d_in0, d_in1, d_out0, d_out1})) return kErrInvalid;
    if (count == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    return mod_down_sp_step(d_in0, d_in1, count, primes, d_out0, d_out1, st);
}

// ct_bsgs on the special-prime keys.  The checks of ct_key_switch_sp first, then the plan's and the workspace's, then
// under `mu` the special-prime keys of every element other than 1, read NOW.  The batch is walked in chunks of Bc =
// min(B, workspace records); a chunk of c records uses the workspace as U0 | U1 | V0 | V1 | W0 | W1 -- stacks [n1][c] and
// [n2][c] of extended records (primes + 1 rows) and [n2][c] of level-`primes` records -- at offsets fixed by Bc:
//   U = many_ext(c; baby),  V[g] = sum_b d'[g][b] . U[b] on all primes + 1 rows,  W = mod_down(V),  out = accum_sp(W; giant).
// Everything is enqueued on `st`: no context scratch, no allocation, no synchronisation.
int Context::ct_bsgs_sp(const BsgsPlan *plan, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                        uint32_t *d_out0, uint32_t *d_out1, void *d_workspace, size_t workspace_bytes, hipStream_t st)
{
    if (!special_prime_ok()) return kErrInvalid;
    GaloisSetArgs ua{};
    if (!set_call_args(ua, d_c0, d_c1, d_out0, d_out1, B, primes, true)) return kErrInvalid;
    if (!plan_ok(plan, true, primes, "baby-step / giant-step transform", "se_amd_bsgs_create",
                 "the level is above the plan's"))
        return kErrInvalid;
    const size_t n1 = plan->baby.size(), n2 = plan->giant.size(), n = hp.n;
    const size_t row = primes * n, xrow = (primes + 1) * n;
    const size_t per = bsgs_record_bytes(true, n1, n2, primes, n);
    if (!d_workspace || !aligned16({d_workspace}) || workspace_bytes < per)
    {
        set_last_error("baby-step / giant-step transform: the workspace must be 16-byte aligned and hold at least one "
                       "record (se_amd_bsgs_workspace_bytes)");
        return kErrInvalid;
    }
    GaloisSetArgs aa = ua;   // the giant steps: the same batch and key layout
    std::lock_guard<std::mutex> lk(mu);
    if (int rc = resolve_keys(ua, plan->baby.data(), n1, true, true)) return rc;
    if (int rc = resolve_keys(aa, plan->giant.data(), n2, true, true)) return rc;
    if (B == 0) return 0;
    SEAMD_HIP(hipSetDevice(device));
    // a chunk's stacks are launch grids too: n1 c and n2 c stay below 2^31
    const size_t Bc = std::min({B, workspace_bytes / per, (size_t)0x7fffffffu / std::max(n1, n2)});
    uint32_t *u0 = static_cast<uint32_t *>(d_workspace), *u1 = u0 + n1 * Bc * xrow;
    uint32_t *v0 = u1 + n1 * Bc * xrow, *v1 = v0 + n2 * Bc * xrow;
    uint32_t *w0 = v1 + n2 * Bc * xrow, *w1 = w0 + n2 * Bc * row;
    ua.out0 = u0;
    ua.out1 = u1;
    aa.c0   = w0;
    aa.c1   = w1;
    for (size_t b0 = 0; b0 < B; b0 += Bc)
    {
        const size_t c = std::min(Bc, B - b0);
        ua.c0 = d_c0 + b0 * row;
        ua.c1 = d_c1 + b0 * row;
        ua.B  = c;
        SEAMD_HIP(launch_ct_galois_many_ext_sp(dp, dt, ua, st));
        if (int rc = mul_plain_sum_step(u0, u1, n1, c, primes, plan->diag, n2, 0, v0, v1, true, st)) return rc;
        if (int rc = mod_down_sp_step(v0, v1, n2 * c, primes, w0, w1, st)) return rc;
        aa.B    = c;
        aa.out0 = d_out0 + b0 * row;
        aa.out1 = d_out1 + b0 * row;
        if (int rc = galois_accum_step(aa, true, st)) return rc;
    }
    return 0;
}

// Slices per output row of ct_lincomb.  A workgroup owns 1024 residues of one output row, so G rows give
// G * slabs * row / 1024 workgroups: 24 for the whole-batch sum at 4096 x 3, on 256 compute units.  Rows are cut until
// there are 8 workgroups (32 waves) per compute unit -- all resident at once, twice the 16 waves per CU at which a row
// gather reaches the HBM rate -- but a slice keeps at least 32 entries: it costs one partial row written and read back.
uint32_t Context::lincomb_slices(size_t G, size_t nnz, size_t slabs) const
{
    const size_t wgs = G * slabs * ((hp.nprimes * hp.n) >> 10), want = (size_t)8 * (size_t)num_cus;
    if (wgs >= want) return 1;
    size_t S = (want + wgs - 1) / wgs;
    const size_t longest = nnz / G / 32;   // by the mean row: no device read-back
    if (S > longest) S = longest;
    return (uint32_t)(S < 1 ? 1 : S > 65535 ? 65535 : S);
}

int Context::ensure_lincomb(size_t part_words, size_t flags)
{
    if (part_words <= d_lc_part.size() && flags <= d_lc_flag.size()) return 0;
    SEAMD_HIP(hipDeviceSynchronize());
    SEAMD_HIP(d_lc_part.grow(part_words));
    SEAMD_HIP(d_lc_flag.grow(flags));
    return 0;
}

// Key-free.  S = 1 is one launch that touches nothing of the context; S > 1 goes through the context's partial rows and
// is ordered on them like every other call with scratch.
int Context::ct_lincomb(const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t G, const uint32_t *d_row_ptr,
                        const uint32_t *d_idx, const int32_t *d_w, size_t nnz, uint32_t *d_out0, uint32_t *d_out1,
                        uint8_t *d_status, hipStream_t st)
{
    constexpr size_t k32 = (size_t)1 << 32;
    if (!d_in0 || !d_out0 || !d_in1 != !d_out1 || !d_row_ptr != !d_idx) return kErrInvalid;
    if (B >= k32 || G >= k32 || nnz >= k32) return kErrInvalid;
    if (!d_row_ptr && nnz != G * B) return kErrInvalid;
    if (!aligned16({d_in0, d_in1, d_out0, d_out1})) return kErrInvalid;
    if (G == 0) return 0;
    std::lock_guard<std::mutex> lk(mu);
    SEAMD_HIP(hipSetDevice(device));
    const size_t slabs = d_in1 ? 2 : 1;
    uint32_t S         = lincomb_split ? lincomb_split : lincomb_slices(G, nnz, slabs);
    if (S > 65535) S = 65535;
    LincombArgs la{};
    la.in0     = d_in0;
    la.in1     = d_in1;
    la.out0    = d_out0;
    la.out1    = d_out1;
    la.row_ptr = d_row_ptr;
    la.idx     = d_idx;
    la.w       = d_w;
    la.status  = d_status;
    la.B       = (uint32_t)B;
    la.nnz     = (uint32_t)nnz;
    la.G       = G;
    if (S == 1)
    {
        SEAMD_HIP(launch_ct_lincomb(dp, la, 1, st));
        return 0;
    }
    return call_scope(st, [&]() -> int {
        if (int rc = ensure_lincomb(slabs * G * S * hp.nprimes * hp.n, G * S)) return rc;
        la.part = d_lc_part;
        la.flag = d_lc_flag;
        SEAMD_HIP(launch_ct_lincomb(dp, la, S, st));
        return 0;
    });
}

// d_out NULL: plain ckks_encode_base (only the int64 plaintexts are written)
int Context::encode_ntt(const float *d_values, size_t B, uint32_t *d_out, int64_t *d_pte,
                        uint8_t *d_status, hipStream_t st)
{
    if (B == 0) return 0;
    if (!d_values || (!d_out && !d_pte)) return kErrInvalid;
    std::lock_guard<std::mutex> lk(mu);   // the list of declined plaintexts is context scratch
    return call_scope(st, [&]() -> int {
        if (int rc = ensure_general(B)) return rc;
        EncArgs ea{};
        ea.values  = d_values;
        ea.c0      = d_out;
        ea.pte     = d_pte;
        ea.status  = d_status;
        ea.general = d_general;
        ea.debug_flags = debug_flags;
        stage_begin(3, st);
        SEAMD_HIP(launch_encode_encrypt(dp, dt, ea, kModeEncodeOnly, B, st));
        stage_end(st);
        return 0;
    });
}

}  // namespace seamd
