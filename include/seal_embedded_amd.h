/*
 * seal_embedded_amd.h -- C ABI of the MI355X-native CKKS encode+encrypt library
 *                        (libseal_embedded_amd.so).
 *
 * Two layers, both plain C (pointers and sizes only, no torch / C++ types):
 *
 *  1. The reference's own API surface for this path, same names / argument meaning / error
 *     behaviour, so existing SEAL-Embedded callers link unchanged:
 *        se_setup_custom, se_setup, se_setup_default, se_encrypt_seeded, se_encrypt, se_cleanup
 *        (replaces /root/reference/device/lib/seal_embedded.h:91-130, seal_embedded.c:24-235)
 *     Each call runs a batch of ONE through the GPU kernels.
 *
 *  2. Batched entry points (new): whole batches of independent plaintexts, host-pointer and
 *     device-pointer flavours, plus stage-level batched operators that mirror the lower surface
 *     the reference's tests/bench call directly (ckks_encode_base, ntt_inpl, prng_fill_buffer,
 *     sample_poly_uniform, sample_small_poly_ternary_prng_96, sample_poly_cbd_generic_prng_16).
 *
 * Ciphertext layout everywhere: uint32 [ct][prime][coeff] -- per ciphertext the polynomials of
 * prime 0..np-1, each n little-endian uint32 residues in [0,q_j), NTT form, bit-reversed order
 * (ntt.h:19-24).  c0 and c1 are separate slabs of that shape; record b of c0 followed by record b
 * of c1 per prime is exactly the byte stream the reference hands to its SEND_FNCT_PTR
 * (seal_embedded.c:196-203).
 *
 * All functions return SE_SUCCESS (0) or a negative SE_ERR_* code unless stated otherwise.
 * The library needs a HIP device: there is no CPU fallback; without one se_amd_create fails.
 */
#ifndef SEAL_EMBEDDED_AMD_H
#define SEAL_EMBEDDED_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>

/* complex128 as the reference spells it (`double complex`, ckks_common.h:38); C++ translation
 * units see the same type through the GNU `_Complex` keyword */
#ifdef __cplusplus
typedef double _Complex se_complex;
#else
#include <complex.h>
typedef double complex se_complex;
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes: seal_embedded.h:35-40 --------------------------------------------------- */
#define SE_SUCCESS 0
#define SE_ERR_NO_MEMORY -12
#define SE_ERR_INVALD_ARGUMENT -22
#define SE_ERR_UNKNOWN -1000
#define SE_ERR_MINIMUM -9999
/* additions (inside the reserved range) */
#define SE_ERR_NO_DEVICE -19
#define SE_ERR_HIP -1001
#define SE_ERR_NO_KEY -1002

/* ---- reference types, same layout (defines.h:366-379, modulus.h:22-30, parameters.h:43-67,
 *      ckks_common.h:36-52, seal_embedded.h:52-65; default config: SE_USE_MALLOC, 32-bit ZZ) ---- */
typedef uint32_t ZZ;
typedef float flpt;
#define SE_PRNG_SEED_BYTE_COUNT 64 /* defines.h:67 */

typedef struct Modulus
{
    ZZ value;
    ZZ const_ratio[2]; /* floor(2^64/q): low word, high word */
} Modulus;

typedef struct
{
    size_t coeff_count;
    size_t logn;
    Modulus *moduli;
    Modulus *curr_modulus;
    size_t curr_modulus_idx;
    size_t nprimes;
    double scale;
    bool is_asymmetric;
    bool pk_from_file;
    bool sample_s;
    bool small_s;
    bool small_u;
} Parms;

typedef struct SE_PTRS
{
    se_complex *conj_vals;  /* n complex128; first 8n bytes hold the int64 plaintext after encode */
    se_complex *ifft_roots; /* 0, as in the reference's default SE_IFFT_OTF (ckks_sym.c:91) */
    flpt *values;           /* n/2 floats */
    ZZ *ternary;            /* 2-bit packed s (sym) / u of the last call (asym), n/4 bytes */
    int64_t *conj_vals_int_ptr;
    ZZ *c0_ptr; /* n residues of the current prime */
    ZZ *c1_ptr;
    uint16_t *index_map_ptr;
    ZZ *ntt_roots_ptr; /* one-shot NTT roots of the last prime processed (ntt.c:40-52) */
    ZZ *ntt_pte_ptr;
    int8_t *e1_ptr; /* e1 of the last asymmetric call */
} SE_PTRS;

typedef struct
{
    Parms *parms;
    SE_PTRS *se_ptrs;
} SE_PARMS;

typedef enum { SE_SYM_ENCR, SE_ASYM_ENCR } EncryptType;
typedef size_t (*SEND_FNCT_PTR)(void *, size_t);
typedef ssize_t (*RND_FNCT_PTR)(void *, size_t, unsigned int flags); /* seal_embedded.h:73 */

/* ---- layer 1: the reference API (seal_embedded.h:91-130) ----------------------------------
 * Behaviour kept: default parameter sets only (custom moduli are unreachable in the reference,
 * ckks_common.c:90); `scale` is overridden by the parameter set (parameters.c:190-226); one
 * parameter set per process (static singletons, seal_embedded.c:18-22); the secret key is read
 * from <SE_DATA_PATH>/sk_<n>.dat and the public key from pk{0,1}_ntt_<n>_<q>.dat relative to the
 * CWD (fileops.c:140-204; SE_DATA_PATH = "adapter_output_data", overridable through the
 * SE_AMD_DATA_PATH environment variable); NULL seeds draw from getrandom (rng.h:45-53); the
 * callback receives c0 then c1 of each prime, n*4 bytes each, from library-owned buffers.
 * Divergence (documented in DESIGN.md): in symmetric mode the reference's default build hands
 * the callback ntt(m+e) in place of c1 because the two buffers alias (ckks_sym.c:86-88).  We
 * deliver the correct c1 = a unless SE_AMD_REFERENCE_C1_ALIAS=1 is set in the environment, in
 * which case the reference's byte stream is reproduced bit for bit. */
SE_PARMS *se_setup_custom(size_t degree, size_t nprimes, const ZZ *modulus_vals, const ZZ *ratios,
                          double scale, EncryptType encrypt_type);
SE_PARMS *se_setup(size_t degree, size_t nprimes, double scale, EncryptType encrypt_type);
SE_PARMS *se_setup_default(EncryptType encrypt_type);
bool se_encrypt_seeded(uint8_t *shareable_seed, uint8_t *seed, SEND_FNCT_PTR network_send_function,
                       void *v, size_t vlen_bytes, bool print, SE_PARMS *se_parms);
bool se_encrypt(SEND_FNCT_PTR network_send_function, void *v, size_t vlen_bytes, bool print,
                SE_PARMS *se_parms);
void se_cleanup(SE_PARMS *se_parms);

/* New beside them: batched host-pointer entry on the handle se_setup returned.
 * values [B][n/2] float; share_seeds [B][64] (ignored for asymmetric; may be NULL then);
 * seeds [B][64]; c0, c1 [B][np][n] uint32 out.  Symmetric only: c1 may be NULL -- seed-compressed
 * form, the receiver re-expands c1 = a from share_seeds (se_amd_expand_c1_device), which halves
 * the bytes crossing PCIe.  With $SE_AMD_DEVICES = "all" or a comma list at se_setup time the
 * batch is sharded over those devices in contiguous blocks (one host thread per device).  Returns SE_SUCCESS, or the number (>0) of
 * plaintexts whose encoding overflowed int64 (their records are unspecified), or SE_ERR_*. */
int se_encrypt_batch(const SE_PARMS *se_parms, const float *values, size_t B,
                     const uint8_t *share_seeds, const uint8_t *seeds, uint32_t *c0, uint32_t *c1);

/* ---- layer 2: explicit context, batched, device pointers ---------------------------------- */
typedef struct se_amd_ctx se_amd_ctx;

/* Builds the parameter set (parameters.c:176-230), the index map (ckks_common.c:32-68), the IFFT
 * root table with the HOST libm (fft.c:39-45) and the per-prime NTT root tables (ntt.c:24-60)
 * and uploads them to HIP device `device`. */
int se_amd_create(se_amd_ctx **out, size_t degree, size_t nprimes, int device);
void se_amd_destroy(se_amd_ctx *ctx);

/* parameter read-back */
size_t se_amd_degree(const se_amd_ctx *ctx);
size_t se_amd_nprimes(const se_amd_ctx *ctx);
double se_amd_scale(const se_amd_ctx *ctx);
int se_amd_moduli(const se_amd_ctx *ctx, uint32_t *q /*[np]*/);
int se_amd_index_map(const se_amd_ctx *ctx, uint16_t *map /*[n], host*/);

/* keys (host pointers).  sk: 2-bit packed, n/4 bytes, sk_<n>.dat format.  pk: [np][n] uint32,
 * NTT form, the pk{0,1}_ntt_<n>_<q>.dat payloads concatenated over primes. */
int se_amd_set_secret_key(se_amd_ctx *ctx, const uint8_t *sk_packed);
int se_amd_set_public_key(se_amd_ctx *ctx, const uint32_t *pk0, const uint32_t *pk1);
int se_amd_load_keys_from_dir(se_amd_ctx *ctx, const char *dir, int want_pk);
/* gen_pk (ckks_asym.c:159-171 as driven by device/test/ckks_tests_asym.c:174-208) on the GPU: ep =
 * n CBD samples from PRNG(ep_seed); per prime the shareable PRNG restarts from pk_seed at counter 0;
 * pk1_j = a_j, pk0_j = -(a_j . NTT(s)) + NTT(ep mod q_j).  Also installs sk in the context.
 * Outputs [np][n] uint32 (host), the payloads of pk{0,1}_ntt_<n>_<q>.dat. */
int se_amd_gen_public_key(se_amd_ctx *ctx, const uint8_t *sk_packed, const uint8_t *pk_seed,
                          const uint8_t *ep_seed, uint32_t *pk0, uint32_t *pk1);

/* K key pairs in one launch chain (host pointers).  Secret key k: the sample branch
 * of ckks_setup_s (ckks_sym.c:162-179) = sample_small_poly_ternary_prng_96 from PRNG(sk_seeds[k]) at
 * counter 0, 2-bit packed (sk_<n>.dat format) -- or sk_in[k] when sk_in != NULL (sk_seeds may then be
 * NULL).  Public key k: gen_pk per prime exactly as se_amd_gen_public_key, from pk_seeds[k] / ep_seeds[k].
 * Seeds [K][64]; sk_in / sk_out [K][n/4] (sk_out may be NULL); pk0, pk1 [K][np][n] uint32 out.  The keys
 * installed in the context are not touched. */
int se_amd_gen_keys_batch(se_amd_ctx *ctx, size_t K, const uint8_t *sk_in, const uint8_t *sk_seeds,
                          const uint8_t *pk_seeds, const uint8_t *ep_seeds, uint8_t *sk_out, uint32_t *pk0,
                          uint32_t *pk1);

/* Whole path, device pointers, asynchronous on `stream` (a hipStream_t, NULL = default stream).
 * Optional outputs may be NULL: ntt_pte [B][np][n] = NTT(m+e mod q_j); pte [B][n] int64;
 * status [B] bytes (1 ok / 0 encode overflow).  Internal scratch is grown on demand (not
 * stream-ordered: call once with the largest B before timing). */
int se_amd_encrypt_sym_device(se_amd_ctx *ctx, const float *d_values, size_t B,
                              const uint8_t *d_share_seeds, const uint8_t *d_seeds, uint32_t *d_c0,
                              uint32_t *d_c1, uint32_t *d_ntt_pte, int64_t *d_pte,
                              uint8_t *d_status, void *stream);
/* Seed-compressed symmetric ciphertext (the reference has only a stub, seal_embedded.c:184-194):
 * c1 = a is the expansion of the 64-byte shareable seed from counter 0 (sample.c:39-57 over the
 * prime chain), so only (share_seed, c0) need to travel; se_amd_expand_c1_device regenerates c1 on
 * the receiving side, bit-identical to what se_amd_encrypt_sym_device would have returned. */
int se_amd_encrypt_sym_seeded_device(se_amd_ctx *ctx, const float *d_values, size_t B,
                                     const uint8_t *d_share_seeds, const uint8_t *d_seeds,
                                     uint32_t *d_c0, uint8_t *d_status, void *stream);
int se_amd_expand_c1_device(se_amd_ctx *ctx, const uint8_t *d_share_seeds, size_t B, uint32_t *d_c1,
                            void *stream);
int se_amd_encrypt_asym_device(se_amd_ctx *ctx, const float *d_values, size_t B,
                               const uint8_t *d_seeds, uint32_t *d_c0, uint32_t *d_c1,
                               uint32_t *d_ntt_pte, int64_t *d_pte, uint8_t *d_status,
                               void *stream);
/* ---- key rings: one batch under many keys, chosen per ciphertext ----------------------------------
 * A context holds at most one secret ring and one public ring of K keys each, independent of the key installed by
 * se_amd_set_{secret,public}_key.  Host pointers, the layouts se_amd_gen_keys_batch writes: sk [K][n/4] 2-bit packed;
 * pk0, pk1 [K][np][n] uint32 in NTT form.  Keys are validated as the single-key setters do (2-bit code 3, or a pk
 * coefficient >= q_j, is refused); installing replaces the ring of that kind after the calls in flight finish.
 * Device memory: 2 np n 4 bytes per secret key, twice that per public key. */
int se_amd_set_secret_keyring(se_amd_ctx *ctx, size_t K, const uint8_t *sk_packed);
int se_amd_set_public_keyring(se_amd_ctx *ctx, size_t K, const uint32_t *pk0, const uint32_t *pk1);
/* Keyed entries: ciphertext b is encrypted under ring key d_key_idx[b] (d_key_idx: [B] uint32 on the device),
 * bit-identical to the unkeyed entry with that key installed.  Other arguments as in the unkeyed entries; symmetric:
 * d_c1 may be NULL, which gives the seed-compressed form of se_amd_encrypt_sym_seeded_device.  SE_ERR_NO_KEY without
 * a ring of the kind.  A record whose index is >= K gets status 2 and an all-zero c0 (public key: and c1); status 2
 * takes precedence over 0 (encode overflow). */
int se_amd_encrypt_sym_keyed_device(se_amd_ctx *ctx, const float *d_values, size_t B, const uint32_t *d_key_idx,
                                    const uint8_t *d_share_seeds, const uint8_t *d_seeds, uint32_t *d_c0,
                                    uint32_t *d_c1, uint32_t *d_ntt_pte, int64_t *d_pte, uint8_t *d_status,
                                    void *stream);
int se_amd_encrypt_asym_keyed_device(se_amd_ctx *ctx, const float *d_values, size_t B, const uint32_t *d_key_idx,
                                     const uint8_t *d_seeds, uint32_t *d_c0, uint32_t *d_c1, uint32_t *d_ntt_pte,
                                     int64_t *d_pte, uint8_t *d_status, void *stream);
/* se_amd_decrypt_decode_device with ciphertext b decrypted under secret-ring key d_key_idx[b]; the outputs of a
 * record whose index is >= K are zero. */
int se_amd_decrypt_decode_keyed_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B,
                                       const uint32_t *d_key_idx, size_t prime, uint32_t *d_dec_ntt,
                                       uint32_t *d_pt, float *d_values, void *stream);
/* BASELINE config 5: encode + RNS reduce + NTT only; out [B][np][n] = NTT(m mod q_j). */
int se_amd_encode_ntt_device(se_amd_ctx *ctx, const float *d_values, size_t B, uint32_t *d_out,
                             int64_t *d_pte, uint8_t *d_status, void *stream);

/* ---- device-resident multi-GPU ----------------------------------------------
 * The path shards embarrassingly (independent plaintexts, own seeds, replicated keys / tables): a GROUP
 * holds one context per HIP device of one node; a batch of B units is cut into contiguous blocks
 * (se_amd_group_partition: the first B % ndev members take one more unit) and block i lives on member i's
 * device -- d_values[i], d_seeds[i], d_c0[i] ... are device pointers ON THAT DEVICE holding count[i]
 * records.  Every member runs the ordinary batched call on its block, driven by a host thread of its
 * own on the group's stream for that device; no collective on the data path.  The calls block until
 * every member has finished.
 *   gather_root < 0 : outputs stay resident on their devices.
 *   gather_root = r : additionally every member writes its finished block into its slice of member r's
 *                     slabs d_c0_all / d_c1_all ([B][np][n] on member r's device, record order = batch
 *                     order) by peer-to-peer copy on its own stream: on an 8-GPU node 7 concurrent
 *                     writers over 7 different xGMI links.  A member whose d_c0[i] already points at
 *                     its slice of the slab (typically the root) is not copied.  d_c1_all may be NULL:
 *                     only c0 is gathered -- with d_c1 == NULL as well this is the seed-compressed
 *                     symmetric form (the caller holds the 64-byte shareable seeds; se_amd_expand_c1_device
 *                     regenerates c1 where it is needed).
 * devices == NULL / ndev == 0: all visible devices.  The same ordinal may be listed more than once (two
 * contexts on one GPU) -- used by the single-GPU tests.  The reference has no counterpart: its boundary
 * is one ciphertext per call (seal_embedded.h:118-124). */
typedef struct se_amd_group se_amd_group;
int se_amd_group_create(se_amd_group **out, size_t degree, size_t nprimes, const int *devices, size_t ndev);
void se_amd_group_destroy(se_amd_group *g);
size_t se_amd_group_size(const se_amd_group *g);
se_amd_ctx *se_amd_group_ctx(se_amd_group *g, size_t i); /* member i's context (keys, stage-level calls) */
int se_amd_group_device(const se_amd_group *g, size_t i);
int se_amd_group_partition(const se_amd_group *g, size_t B, size_t *first /*[ndev]*/, size_t *count /*[ndev]*/);
int se_amd_group_set_secret_key(se_amd_group *g, const uint8_t *sk_packed);
int se_amd_group_set_public_key(se_amd_group *g, const uint32_t *pk0, const uint32_t *pk1);
int se_amd_group_reserve(se_amd_group *g, size_t B); /* scratch for batches of up to B units in total */
int se_amd_encrypt_sym_multi_device(se_amd_group *g, size_t B, const float *const *d_values,
                                    const uint8_t *const *d_share_seeds, const uint8_t *const *d_seeds,
                                    uint32_t *const *d_c0, uint32_t *const *d_c1 /* NULL: seed-compressed */,
                                    uint8_t *const *d_status /* NULL or [ndev] */, int gather_root,
                                    uint32_t *d_c0_all, uint32_t *d_c1_all);
int se_amd_encrypt_asym_multi_device(se_amd_group *g, size_t B, const float *const *d_values,
                                     const uint8_t *const *d_seeds, uint32_t *const *d_c0, uint32_t *const *d_c1,
                                     uint8_t *const *d_status, int gather_root, uint32_t *d_c0_all,
                                     uint32_t *d_c1_all);
int se_amd_encode_ntt_multi_device(se_amd_group *g, size_t B, const float *const *d_values, uint32_t *const *d_out,
                                   uint8_t *const *d_status, int gather_root, uint32_t *d_out_all);

/* Host-pointer entries: synchronous; a chunked pipeline (compute || D2H through a pinned staging
 * ring, or DMA straight into pinned/registered caller memory) that runs at the PCIe link rate.
 * c1 may be NULL for the symmetric form (seed-compressed: only c0 is returned). */
int se_amd_encrypt_sym_host(se_amd_ctx *ctx, const float *values, size_t B,
                            const uint8_t *share_seeds, const uint8_t *seeds, uint32_t *c0,
                            uint32_t *c1, uint32_t *ntt_pte, int64_t *pte, uint8_t *status);
int se_amd_encrypt_asym_host(se_amd_ctx *ctx, const float *values, size_t B, const uint8_t *seeds,
                             uint32_t *c0, uint32_t *c1, uint32_t *ntt_pte, int64_t *pte,
                             uint8_t *status);

/* ---- stage-level batched operators (device pointers) -------------------------------------- */
/* ckks_encode_base (ckks_common.c:105-215): values [B][n/2] -> int64 [B][n]; status [B]. */
int se_amd_encode_device(se_amd_ctx *ctx, const float *d_values, size_t B, int64_t *d_out,
                         uint8_t *d_status, void *stream);
/* ntt_inpl (ntt.c:168-189) for prime j on `count` polynomials [count][n], in place. */
int se_amd_ntt_device(se_amd_ctx *ctx, size_t prime, uint32_t *d_polys, size_t count, void *stream);
/* intt_inpl (intt.c:144-222, test-side in the reference) for prime j on `count` polynomials
 * [count][n], in place: NTT-form bit-reversed in, natural-order canonical out. */
int se_amd_intt_device(se_amd_ctx *ctx, size_t prime, uint32_t *d_polys, size_t count, void *stream);
/* The reference's round-trip check, batched (device/test/ckks_tests_common.c:59-231): for prime j
 * of every ciphertext d = c0 + c1 . NTT(s) (ckks_decrypt), pt = INTT(d), values = ckks_decode(pt).
 * Optional outputs (NULL to skip): d_dec_ntt [B][n], d_pt [B][n] uint32, d_values [B][n/2] float.
 * For a symmetric ciphertext d_dec_ntt equals NTT(m+e mod q_j) exactly. */
int se_amd_decrypt_decode_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1,
                                 size_t B, size_t prime, uint32_t *d_dec_ntt, uint32_t *d_pt,
                                 float *d_values, void *stream);
/* Full-modulus decrypt and decode: the receiving side for plaintexts of any size the encoder accepts.  One launch
 * over ALL primes of every ciphertext: pt_j = INTT(c0_j + c1_j . NTT(s)_j) for j = 0 .. np-1 as above, then the
 * residues are recombined (incremental Garner / CRT) to the one integer y per coefficient with y = pt_j (mod q_j) for
 * every j and y in (-Q/2, Q/2], Q = q_0 ... q_{np-1}; for a symmetric ciphertext that is the int64 m + e the
 * encryption entry reports in d_pte.  Decode is ckks_decode (ckks_tests_common.c:72-115) on y instead of the
 * single-prime lift: y / scale, fft_inpl, slot pick through the index map.
 * Range: exact while every |m + e| < min(2^63, Q/2).  d_status[b] = 1 if every recombined coefficient of record b lies
 * in [-2^63, 2^63), else 0 (a plaintext beyond the range, a wrong key or a corrupted record); the other outputs of a
 * status-0 record are unspecified.  With one prime this is the single-prime lift (status always 1).
 * Outputs, each optional (NULL to skip), at least one required: d_pte [B][n] int64, natural order; d_values [B][n/2]
 * float; d_values_f64 [B][n/2] double, the same slots before the float conversion; d_status [B].  With neither
 * d_values nor d_values_f64 the FFT is skipped.  Asynchronous on `stream`; no scratch memory is allocated.
 * SE_ERR_NO_KEY without a secret key (keyed: without a secret ring); SE_ERR_INVALD_ARGUMENT for a NULL d_c0 / d_c1
 * (/ d_key_idx) or when no output is requested.
 * Keyed: ciphertext b under secret-ring key d_key_idx[b]; a record whose index is >= K gets status 2 and all-zero
 * outputs. */
int se_amd_decrypt_full_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B,
                               int64_t *d_pte, float *d_values, double *d_values_f64,
                               uint8_t *d_status, void *stream);
int se_amd_decrypt_full_keyed_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B,
                                     const uint32_t *d_key_idx, int64_t *d_pte, float *d_values,
                                     double *d_values_f64, uint8_t *d_status, void *stream);
/* Weighted sums of records, for the machine in the middle: a gateway or aggregator that holds NO key, receives
 * ciphertexts and forwards one per group, window or model output.  The entry needs no key, installed or in a ring.
 * With row = np . n, d_in0 / d_in1 are slabs [B][row] of residues (element (b, j, i) in [0, q_j), NTT form as every
 * encryption entry writes them) and d_out0 / d_out1 are [G][row]:
 *     out[g][j][i] = ( sum_k (w_k mod q_j) . in[idx_k][j][i] ) mod q_j,   canonical in [0, q_j),
 * over the entries k of output row g.  w_k is a signed int32 and w mod q_j its non-negative residue (negative weights
 * and INT32_MIN are valid).  The map is defined on arbitrary residue slabs and is applied identically to both; the
 * second pair is optional (d_in1 = d_out1 = NULL).
 * Entries, CSR form: d_row_ptr [G+1] uint32, non-decreasing, row_ptr[G] <= nnz; d_idx [nnz] uint32; d_w [nnz] int32 or
 * NULL for all ones.  Row g takes k in [row_ptr[g], row_ptr[g+1]); an empty row is all zero with status 1.
 * Dense form (d_row_ptr = d_idx = NULL, nnz = G . B): row g takes every record b with weight d_w[g . B + b]; d_w = NULL
 * with G = 1 is the plain sum of the batch.
 * d_status [G], optional: 1, or 2 (the key ring's convention) for a row with an index >= B or a row_ptr pair that
 * decreases or reaches beyond nnz; a status-2 row is all zero in both slabs, other rows are unaffected and nothing is
 * read out of bounds.  B = 0 with non-empty rows gives those rows status 2; G = 0 is a successful no-op.
 * SE_ERR_INVALD_ARGUMENT: NULL d_in0 or d_out0; d_in1 and d_out1 not both set or both NULL; only one of d_row_ptr and
 * d_idx NULL; dense form with nnz != G . B; B, G or nnz at or above 2^32; a slab pointer that is not 16-byte aligned.
 * Outputs must not overlap inputs (not checked).
 * Decryption: se_amd_decrypt_full_device on the result gives exactly sum_k w_k (m_b + e_b), the weighted sum of what
 * the encryption entries report in d_pte, while every coefficient of that sum stays within min(2^63, Q/2); beyond that
 * range it reports status 0.  Integer weights keep the CKKS scale; noise and range growth are the caller's business.
 * All records of a row must be under the same key.  Seed-compressed records need se_amd_expand_c1_device first.
 * Asynchronous on `stream`.  A long row is cut into S slices of its entry list so that a sum with few output rows
 * still uses the whole chip; S is chosen on the host from G, nnz / G and the number of compute units.  S = 1 is one
 * launch without scratch; S > 1 writes S partial rows per output row into context scratch (grown on demand, which
 * synchronises the device; not stream-ordered: calls on one context are serialised on it) and sums them in a second
 * launch.  Every S gives the same bits. */
int se_amd_ct_lincomb_device(se_amd_ctx *ctx,
        const uint32_t *d_in0, const uint32_t *d_in1 /* NULL: one slab */, size_t B,
        size_t G, const uint32_t *d_row_ptr, const uint32_t *d_idx, const int32_t *d_w, size_t nnz,
        uint32_t *d_out0, uint32_t *d_out1 /* NULL iff d_in1 NULL */,
        uint8_t *d_status /* [G], optional */, void *stream);
/* test hook: partial sums a long row is split into (0 = automatic) */
int se_amd_set_lincomb_split(se_amd_ctx *ctx, uint32_t splits);
/* ---- real-valued weights: rescale, plaintext products, level-aware decrypt ----------------------
 * "Level L" is a slab [B][L][n] of uint32 residues under the primes q_0 .. q_{L-1}, NTT form and bit-reversed order
 * as every encryption entry writes it, 1 <= L <= np of the context.  The default chains are prefixes of one another,
 * so a level-L record is an ordinary ciphertext of the parameter set (n, L).  The three device entries below take
 * device pointers, are asynchronous on `stream`, allocate no scratch and -- except the decrypt -- need no key.
 *
 * Rescale: level L = primes (2 <= L <= np) in, level L - 1 out ([B][L-1][n]); divides the CKKS scale by q_{L-1}.
 * With delta = INTT_{L-1}(in[b][L-1]), coefficients lifted to the centred representative in (-q_{L-1}/2, q_{L-1}/2],
 *     out[b][j] = ( in[b][j] - NTT_j(delta mod q_j) ) . q_{L-1}^-1  mod q_j,   canonical,   j < L - 1:
 * the exact quotient (c - delta) / q_{L-1}, i.e. c / q_{L-1} rounded to nearest (the moduli are odd: no ties) -- SEAL's
 * rescale_to_next on NTT-form data.  The map is defined on arbitrary residue slabs and is applied identically to each
 * slab; the second pair is optional (d_in1 = d_out1 = NULL).  Outputs must not overlap inputs (not checked).
 * SE_ERR_INVALD_ARGUMENT: NULL d_in0 or d_out0; d_in1 and d_out1 not both set or both NULL; primes outside [2, np]; a
 * slab pointer that is not 16-byte aligned; B at or above 2^31.  B = 0 is a successful no-op. */
int se_amd_ct_rescale_device(se_amd_ctx *ctx, const uint32_t *d_in0, const uint32_t *d_in1 /* NULL: one slab */,
                             size_t B, size_t primes, uint32_t *d_out0, uint32_t *d_out1 /* NULL iff d_in1 NULL */,
                             void *stream);
/* Slot-wise product with encoded plaintexts, on level-`primes` slabs (1 <= primes <= np), both slabs alike:
 *     out[b][j][i] = in[b][j][i] . pt[p(b)][j][i]  mod q_j,   canonical,   j < primes.
 * d_pt is [P][pt_primes][n], the layout se_amd_encode_ntt_device writes (NTT(m mod q_j)); pt_primes >= primes and only
 * the first `primes` rows of a plaintext are read.  d_pt_idx [B] uint32 gives p(b); with d_pt_idx = NULL, P = 1 means
 * one plaintext for every record and P = B means p(b) = b.  A record with p(b) >= P gets status 2 and all-zero rows;
 * nothing is read out of bounds and other records are unaffected.  d_status [B] is optional (1, or 2).
 * The scales of plaintext and ciphertext multiply: the result is at scale^2 until it is rescaled.
 * d_out0 == d_in0 (and d_out1 == d_in1) exactly is allowed: the map is element-wise.  Any other overlap is not.
 * SE_ERR_INVALD_ARGUMENT: NULL d_in0, d_out0 or d_pt; d_in1 and d_out1 not both set or both NULL; primes outside
 * [1, np]; pt_primes < primes; d_pt_idx NULL with P neither 1 nor B; B or P at or above 2^32; a slab or plaintext
 * pointer that is not 16-byte aligned.  B = 0 is a successful no-op. */
int se_amd_ct_mul_plain_device(se_amd_ctx *ctx, const uint32_t *d_in0, const uint32_t *d_in1 /* NULL: one slab */,
                               size_t B, size_t primes, const uint32_t *d_pt, size_t P, size_t pt_primes,
                               const uint32_t *d_pt_idx /* [B] or NULL */, uint32_t *d_out0,
                               uint32_t *d_out1 /* NULL iff d_in1 NULL */, uint8_t *d_status /* [B], optional */,
                               void *stream);
/* se_amd_decrypt_full[_keyed]_device on level-`primes` records (d_c0 / d_c1 [B][primes][n], 1 <= primes <= np),
 * decoded with the caller's `scale` (finite, > 0) in place of the context's: the recombination runs over
 * Q_primes = q_0 ... q_{primes-1}.  Range: exact while every |y| < min(2^63, Q_primes / 2).  Outputs, status values,
 * SE_ERR_NO_KEY and the other argument errors are those of the full entries; additionally SE_ERR_INVALD_ARGUMENT for
 * primes outside [1, np] and for a scale that is not finite and positive.  With primes = np and scale =
 * se_amd_scale(ctx) this IS the full entry.
 * Scale bookkeeping: after a weighted sum with weights round(w . 2^s) the scale is scale . 2^s, after a plaintext
 * product scale^2, and a rescale from level L divides it by q_{L-1}. */
int se_amd_decrypt_level_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                                double scale, int64_t *d_pte, float *d_values, double *d_values_f64,
                                uint8_t *d_status, void *stream);
int se_amd_decrypt_level_keyed_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B,
                                      size_t primes, double scale, const uint32_t *d_key_idx, int64_t *d_pte,
                                      float *d_values, double *d_values_f64, uint8_t *d_status, void *stream);
/* ---- ciphertext products: tensor, relinearisation key, degree-2 decrypt ------------------------------
 * Conventions are those of the level entries above: a level-L slab is uint32 [records][L][n], NTT form, bit-reversed
 * order, residues in [0, q_j), 1 <= L <= np; device pointers are 16-byte aligned; the device entries are asynchronous on
 * `stream`, allocate no scratch, and their outputs must not overlap their inputs (not checked).  A product of two
 * ciphertexts at scale D is at scale D^2; relinearisation changes neither scale nor level; a rescale afterwards divides
 * the scale by the prime it drops.
 *
 * Tensor product, key-free.  For pair p with x = record ia[p] of (d_a0, d_a1) [Ba][primes][n] and y = record ib[p] of
 * (d_b0, d_b1) [Bb][primes][n], per prime j < primes and element, mod q_j and canonical:
 *     out0 = x0 . y0,     out1 = x0 . y1 + x1 . y0,     out2 = x1 . y1          (each [P][primes][n]).
 * (out0, out1, out2) decrypts as out0 + out1 s + out2 s^2 (se_amd_decrypt3_level_device) or is brought back to two slabs
 * by se_amd_ct_relin_device.  d_ia / d_ib [P] uint32 on the device; with d_ia = d_ib = NULL, P must equal Ba and Bb and
 * pair p is (p, p).  The a and b slabs may be the same pointers (squares, all pairs within one batch).  A pair with
 * ia[p] >= Ba or ib[p] >= Bb gets status 2 and all-zero rows; nothing is read out of bounds and other pairs are
 * unaffected.  d_status [P] is optional (1, or 2).
 * SE_ERR_INVALD_ARGUMENT: a NULL slab pointer; only one of d_ia / d_ib NULL; both NULL with P != Ba or P != Bb; primes
 * outside [1, np]; P, Ba or Bb at or above 2^32; a slab pointer that is not 16-byte aligned.  P = 0 is a successful
 * no-op.  Nothing is written on an argument error. */
int se_amd_ct_mul_device(se_amd_ctx *ctx, const uint32_t *d_a0, const uint32_t *d_a1, size_t Ba, const uint32_t *d_b0,
                         const uint32_t *d_b1, size_t Bb, size_t primes, size_t P,
                         const uint32_t *d_ia /* [P] or NULL */, const uint32_t *d_ib /* [P] or NULL */,
                         uint32_t *d_out0, uint32_t *d_out1, uint32_t *d_out2, uint8_t *d_status /* [P], optional */,
                         void *stream);
/* se_amd_decrypt_level[_keyed]_device on the degree-2 form: a third slab d_c2 after d_c1 and, per prime,
 * d = c0 + s_hat . (c1 + s_hat . c2).  Everything after that is the level entry unchanged: INTT and recombination over
 * Q_primes, status 0 or 1, decode with the caller's `scale`, the same optional outputs, SE_ERR_NO_KEY, the ring's status
 * 2, the same argument errors (and a NULL d_c2).  With d_c2 pointing at an all-zero slab every output equals
 * se_amd_decrypt_level_device byte for byte. */
int se_amd_decrypt3_level_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, const uint32_t *d_c2,
                                 size_t B, size_t primes, double scale, int64_t *d_pte, float *d_values,
                                 double *d_values_f64, uint8_t *d_status, void *stream);
int se_amd_decrypt3_level_keyed_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1,
                                       const uint32_t *d_c2, size_t B, size_t primes, double scale,
                                       const uint32_t *d_key_idx, int64_t *d_pte, float *d_values,
                                       double *d_values_f64, uint8_t *d_status, void *stream);
/* Relinearisation key.  Digits are SE_AMD_RELIN_DIGIT_BITS = 15 bits, two per prime (30-bit digits would put the
 * key-switch noise near the reference's 0.1 acceptance at the large parameter sets).  The key
 * has R = 2 np rows; evk0 and evk1 are uint32 [R][np][n] each, NTT form.  Row r = 2j + t (j < np, t in {0, 1}) at prime
 * i, mod q_i and canonical:
 *     evk1[r][i] = a_{r,i}
 *     evk0[r][i] = -a_{r,i} . s_hat_i + NTT_i(e_r mod q_i) + [i == j] . (2^(15 t) mod q_i) . s_hat_i^2.
 * The diagonal term uses the CRT basis element of q_j (1 mod q_j, 0 mod the others), so ONE key serves every level L:
 * the rows r < 2L and the columns i < L.
 * se_amd_gen_relin_key (host pointers; a_seeds, e_seeds [R][64]): (evk0[r], evk1[r]) minus the diagonal term is exactly
 * public key r of se_amd_gen_keys_batch with K = R, sk_in = this key replicated, pk_seeds = a_seeds and ep_seeds =
 * e_seeds.  Keys installed in the context are not touched; a 2-bit code 3 in sk_packed is refused.
 * se_amd_set_relin_key (host pointers): installs the key for se_amd_ct_relin_device; a word >= q_i is refused; replaces
 * the previous key after the calls in flight finish.  The key is public material.  Device memory: 16 R np n bytes. */
#define SE_AMD_RELIN_DIGIT_BITS 15
int se_amd_gen_relin_key(se_amd_ctx *ctx, const uint8_t *sk_packed, const uint8_t *a_seeds /*[R][64]*/,
                         const uint8_t *e_seeds /*[R][64]*/, uint32_t *evk0, uint32_t *evk1 /*[R][np][n], host out*/);
int se_amd_set_relin_key(se_amd_ctx *ctx, const uint32_t *evk0, const uint32_t *evk1);
/* Relinearisation: level-`primes` slabs (d_d0, d_d1, d_d2) [B][primes][n] -> (d_out0, d_out1) of the same level.  Let
 * D_{j,t} be the t-th 15-bit digit of each coefficient of the canonical natural-order INTT_j(d2[b][j]) (the n^-1 factor
 * included), so that D_{j,0} + 2^15 D_{j,1} is that coefficient and every digit is already a residue of every prime.
 * For i < primes, mod q_i and canonical:
 *     out0[b][i] = d0[b][i] + sum_{j < primes, t} NTT_i(D_{j,t}) . evk0[2j + t][i]
 *     out1[b][i] = d1[b][i] + sum_{j < primes, t} NTT_i(D_{j,t}) . evk1[2j + t][i].
 * The map is defined on arbitrary residue slabs and arbitrary installed key words below q_i; it needs no secret key.
 * SE_ERR_NO_KEY without an installed relinearisation key; SE_ERR_INVALD_ARGUMENT for a NULL slab pointer, primes
 * outside [1, np], a slab pointer that is not 16-byte aligned, B at or above 2^32.  B = 0 is a successful no-op. */
int se_amd_ct_relin_device(se_amd_ctx *ctx, const uint32_t *d_d0, const uint32_t *d_d1, const uint32_t *d_d2, size_t B,
                           size_t primes, uint32_t *d_out0, uint32_t *d_out1, void *stream);
/* ---- slot rotations: Galois elements, Galois keys, the automorphism fused with its key switch --------
 * Conventions are those of the ciphertext products above (level-L slabs, 16-byte aligned device pointers, asynchronous
 * device entry without scratch, outputs that do not overlap inputs).  A Galois element is an odd g, 1 <= g < 2n; sigma_g
 * is the ring automorphism x(X) -> x(X^g).  On an NTT-form row in bit-reversed order it is a pure permutation,
 *     sigma_g(x)[k] = x[src_g(k)],   src_g(k) = brev((((2 brev(k) + 1) g mod 2n) - 1) / 2),   brev over log2 n bits.
 * With the encoder's index map (the orbit of 3), g = 3^s mod 2n rotates the slot vector LEFT by s:
 * out_slot[k] = in_slot[(k + s) mod n/2]; a negative step rotates right; g = 2n - 1 conjugates (the real-valued slots
 * of this encoder are unchanged by it).  A rotation changes neither scale nor level.
 * Scale bookkeeping.  This entry's digit key has no special prime, so the key-switch term is the size of the
 * relinearisation's (about 2.5e7 per coefficient at 4096 x 3): rotate at a raised scale and rescale afterwards.  A
 * product before its rescale is already at scale^2; a fresh record is first lifted by se_amd_ct_lincomb_device with
 * weight 2^30, which costs one level -- or rotated at its own scale by the special-prime
 * entry further down, se_amd_ct_galois_sp_device, which reserves the last prime for the key instead.
 * Out of scope: plaintext-weighted sums of rotations (the diagonal method), multi-GPU group entries.  (A per-record
 * element list is the single form of se_amd_ct_pack_sp_device, on the special-prime keys.)
 *
 * se_amd_galois_element (host only, no context): *elt = 3^(step mod n/2) mod 2n, the step reduced into [0, n/2); step 0
 * gives 1.  se_amd_galois_table (host only): src [n] uint16 with sigma_elt(x)[k] = x[src[k]]; element 1 gives the
 * identity.  SE_ERR_INVALD_ARGUMENT for a degree that is not a power of two in [1024, 16384], a NULL output, an even
 * element or one >= 2n. */
int se_amd_galois_element(size_t degree, int64_t step, uint32_t *elt);
int se_amd_galois_table(size_t degree, uint32_t elt, uint16_t *src /*[n]*/);
/* Galois keys of G elements, 1 <= G <= SE_AMD_MAX_GALOIS_KEYS.  Each key has the shape of the relinearisation key: R =
 * 2 np rows, the same 15-bit digits, gk0 and gk1 uint32 [G][R][np][n], NTT form.  For element elts[g], row r = 2j + t at
 * prime i, mod q_i and canonical:
 *     gk1[g][r][i] = a_{g,r,i}
 *     gk0[g][r][i] = -a_{g,r,i} . s_hat_i + NTT_i(e_{g,r} mod q_i) + [i == j] . (2^(15 t) mod q_i) . sigma(s_hat)_i,
 * sigma(s_hat)_i[k] = s_hat_i[src(k)].  As for the relinearisation key, one key serves every level L: rows r < 2L and
 * columns i < L.
 * se_amd_gen_galois_keys (host pointers; a_seeds, e_seeds [G][R][64]): (gk0[g][r], gk1[g][r]) minus the diagonal term is
 * exactly public key r of se_amd_gen_keys_batch with K = R, sk_in = this key replicated, pk_seeds = the g-th block of
 * a_seeds and ep_seeds = the g-th block of e_seeds.  Keys installed in the context are not touched.  Refused
 * (SE_ERR_INVALD_ARGUMENT): a 2-bit code 3 in sk_packed, an even element, an element >= 2n, G = 0, G > 64, a NULL pointer.
 * se_amd_set_galois_keys (host pointers): installs the keys of exactly these G elements for se_amd_ct_galois_device,
 * replacing the whole installed set after the calls in flight finish.  Refused: a word >= q_i, an even element, an
 * element >= 2n, an element listed twice, G = 0, G > 64; a refused install leaves the previous set in place.  The keys
 * are public material.  Device memory: 16 R np n bytes per element, 16 G R np n = 32 G np^2 n bytes in all (4096 x 3:
 * 1.1 MiB per element; 16384 x 13: 84.5 MiB per element). */
#define SE_AMD_MAX_GALOIS_KEYS 64
int se_amd_gen_galois_keys(se_amd_ctx *ctx, const uint8_t *sk_packed, const uint32_t *elts, size_t G,
                           const uint8_t *a_seeds /*[G][R][64]*/, const uint8_t *e_seeds /*[G][R][64]*/,
                           uint32_t *gk0, uint32_t *gk1 /*[G][R][np][n], host out*/);
int se_amd_set_galois_keys(se_amd_ctx *ctx, const uint32_t *elts, size_t G, const uint32_t *gk0, const uint32_t *gk1);
/* Rotation / conjugation: level-`primes` slabs (d_c0, d_c1) [B][primes][n] -> (d_out0, d_out1) of the same level under
 * the same secret key.  Let p0 = sigma(c0) and p1 = sigma(c1), row-wise through src, and D_{j,t} the t-th 15-bit digit
 * of each coefficient of the canonical natural-order INTT_j(p1[b][j]).  For i < primes, mod q_i and canonical:
 *     out0[b][i] = p0[b][i] + sum_{j < primes, t} NTT_i(D_{j,t}) . gk0[g][2j + t][i]
 *     out1[b][i] =            sum_{j < primes, t} NTT_i(D_{j,t}) . gk1[g][2j + t][i],
 * g the installed key of `elt`: se_amd_ct_relin_device applied to (sigma(c0), 0, sigma(c1)) with gk[g] installed as the
 * relinearisation key.  The map is defined on arbitrary residue slabs and arbitrary installed key words below q_i; it
 * needs no secret key.
 * SE_ERR_INVALD_ARGUMENT for a NULL slab pointer, primes outside [1, np], a slab pointer that is not 16-byte aligned, B
 * at or above 2^32, an even `elt` or one >= 2n; SE_ERR_NO_KEY when no key is installed for `elt`.  B = 0 is a successful
 * no-op.  Nothing is written on an error. */
int se_amd_ct_galois_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                            uint32_t elt, uint32_t *d_out0, uint32_t *d_out1, void *stream);
/* Hoisted rotations: G rotations of every record from ONE digit decomposition of c1, under the Galois keys installed
 * for se_amd_ct_galois_device as they are.  elts is a HOST pointer to G elements, 1 <= G <= SE_AMD_MAX_GALOIS_KEYS; an
 * element may be listed twice.  Let D_{j,t} be the t-th 15-bit digit of each coefficient of the canonical natural-order
 * INTT_j(c1[b][j]) -- of c1 itself, not of sigma(c1).  For element g (its installed key gk[g]), record b and i < primes,
 * mod q_i and canonical:
 *     rot0[g][b][i][k] = c0[b][i][src_g(k)] + sum_{j < primes, t} NTT_i(D_{j,t})[src_g(k)] . gk0[g][2j + t][i][k]
 *     rot1[g][b][i][k] =                      sum_{j < primes, t} NTT_i(D_{j,t})[src_g(k)] . gk1[g][2j + t][i][k].
 * sum_t 2^(15 t) sigma(D_{j,t}) = sigma(c1_j) mod q_j and sigma(D) has coefficients of magnitude below 2^15, so rot[g]
 * decrypts to sigma_g of the input plus a key-switch term of the same bound as se_amd_ct_galois_device's.  It is NOT
 * bit-identical to that entry: there the digits are those of sigma(c1), and a negated coefficient q - c has other digits
 * than c.  The transforms (the dominant cost) are shared by the elements: an element costs a permutation and a
 * multiply-accumulate.
 * se_amd_ct_galois_many_device: d_out0, d_out1 are [G][B][primes][n], out[e] = rot[elts[e]].
 * se_amd_ct_galois_sum_device: d_out0, d_out1 are [B][primes][n], out = add_input . (c0, c1) + sum_e rot[elts[e]] mod
 * q_i; an element listed twice counts twice; add_input (0 or not) adds the record itself, the rotation by 0, which needs
 * no key.  The transforms per record are those of ONE rotation whatever G is.
 * Outputs must not overlap the inputs.  One asynchronous call each, no scratch, no host synchronisation.
 * SE_ERR_INVALD_ARGUMENT for a NULL slab pointer, primes outside [1, np], a slab pointer that is not 16-byte aligned, B
 * at or above 2^32 (the checks of se_amd_ct_galois_device), then for elts NULL, G = 0, G > 64, an even element or one
 * >= 2n; SE_ERR_NO_KEY when an element has no installed key (the last-error text names it).  Nothing is launched or
 * written on an error.  B = 0 is a successful no-op. */
int se_amd_ct_galois_many_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                                 const uint32_t *elts /*host, [G]*/, size_t G, uint32_t *d_out0, uint32_t *d_out1,
                                 void *stream);
int se_amd_ct_galois_sum_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                                const uint32_t *elts /*host, [G]*/, size_t G, int add_input, uint32_t *d_out0,
                                uint32_t *d_out1, void *stream);
/* Linear transforms: plaintext-weighted sums of hoisted rotations (the diagonal method),
 *     y = d0 . x + sum_e d_e . rot_{elts[e]}(x)      slot-wise,
 * an encrypted matrix-vector product by generalised diagonals, a convolution with arbitrary taps, the baby steps of a
 * baby-step / giant-step product (the plan for that product, which reaches beyond 64 diagonals, is se_amd_bsgs_create
 * further down).  rot0 / rot1 are exactly those of the hoisted rotations above -- the digits of c1
 * itself, the Galois keys installed when the plan was created, src_e = se_amd_galois_table(elts[e]) -- and the
 * diagonals are plaintexts in the layout se_amd_encode_ntt_device writes.  For record b, i < primes, mod q_i, canonical:
 *     out0[b][i][k] = d0[i][k] . c0[b][i][k] + sum_e d_e[i][k] . rot0[e][b][i][k]
 *     out1[b][i][k] = d0[i][k] . c1[b][i][k] + sum_e d_e[i][k] . rot1[e][b][i][k]     (no d0 terms when d_diag0 is NULL)
 * which fixes every bit: the result equals se_amd_ct_galois_many_device, then se_amd_ct_mul_plain_device per element,
 * then the modular sum.  The scale is multiplied by the diagonals' scale, the level is unchanged; the key-switch term of
 * element e is multiplied slot-wise by d_e, so relative to the result it is that of a rotation at the input's scale.
 * The weight does not depend on the key row, so se_amd_lintrans_create folds d_e into a copy of the key block of
 * elts[e] (words gk . d_e mod q_i with their Shoup companions) and a call costs ONE pass of the sum form, whatever G is,
 * plus an epilogue: no [G][B][primes][n] scratch, no further passes over memory.
 * se_amd_lintrans_create: elts is a HOST pointer to G odd elements below 2n, 1 <= G <= SE_AMD_MAX_GALOIS_KEYS, repeats
 * allowed (each with its own diagonal); d_diag is DEVICE memory [G][pt_primes][n], d_diag0 DEVICE [pt_primes][n] or NULL
 * (the weight of the record itself, the rotation by 0, which needs no key); pt_primes >= 1.  The plan serves the levels
 * primes <= min(pt_primes, np).  Diagonal words are reduced mod q_i, so any 32-bit word is valid.  The call takes the
 * context's lock, reads the diagonals and the installed key blocks and returns with everything complete (it
 * synchronises): the plan is a SNAPSHOT, a later se_amd_set_galois_keys does not change it and the diagonals may be
 * freed.  Device memory per plan: (G . 16 R np + (G + 1) . 8 np) n bytes, R = 2 np (4096 x 3, G = 7: 8.6 MiB;
 * 16384 x 13, G = 7: 604.5 MiB -- 1.1 MiB resp. 84.5 MiB per element for the folded block, 96 KiB resp. 1.6 MiB per
 * diagonal).  SE_ERR_INVALD_ARGUMENT for NULL elts / d_diag / out, G outside [1, 64], pt_primes = 0, an even element
 * or one >= 2n, a diagonal pointer that is not 16-byte aligned; SE_ERR_NO_KEY when an element has no installed key
 * (the last-error text names it).  A failed create leaves *out NULL and frees what it built.
 * se_amd_lintrans_destroy: waits for the device, then frees; NULL is a no-op.  Destroy plans before their context.
 * se_amd_ct_lintrans_device: d_out0, d_out1 are [B][primes][n].  One asynchronous launch, no scratch, no host
 * synchronisation; outputs must not overlap the inputs.  SE_ERR_INVALD_ARGUMENT for the pointer, alignment, level and B
 * checks of se_amd_ct_galois_device, then for a NULL plan, a plan of another context, a special-prime plan
 * (se_amd_lintrans_create_sp), or primes above the plan's levels.  Nothing is launched or written on an error.  B = 0
 * is a successful no-op. */
typedef struct se_amd_lintrans se_amd_lintrans;
int se_amd_lintrans_create(se_amd_ctx *ctx, const uint32_t *elts /*host, [G]*/, size_t G, const uint32_t *d_diag,
                           const uint32_t *d_diag0, size_t pt_primes, se_amd_lintrans **out);
void se_amd_lintrans_destroy(se_amd_lintrans *plan);
int se_amd_ct_lintrans_device(se_amd_ctx *ctx, const se_amd_lintrans *plan, const uint32_t *d_c0, const uint32_t *d_c1,
                              size_t B, size_t primes, uint32_t *d_out0, uint32_t *d_out1, void *stream);
/* ---- special-prime (hybrid) key switch: relinearise and rotate at the record's own scale ------------
 * The digit keys above add a term of about 2.5e7 per coefficient (4096 x 3), the size of a fresh message at scale 2^25,
 * so every caller lifts, switches and rescales: one level per rotation.  These entries reserve the LAST prime of the
 * context for the key instead, P = q_p with p = np - 1 (the largest prime of every default chain), as SEAL's key
 * switching does.  Data levels are 1 <= L <= np - 1; np >= 2 is required (the n = 1024 and 2048 contexts have one prime:
 * SE_ERR_INVALD_ARGUMENT from every entry of this block but se_amd_ct_drop_primes_device).  The key-switch term is
 * divided by P on the way out: a few hundred per coefficient, 6e-4 in the slots at 4096 x 3 with scale 2^25
 * (tools/ct_keyswitch_sp_noise_sim.py).  A key switch changes neither scale nor level, and needs no lift and no rescale.
 * Conventions are those of the digit twins: level-L slabs, 16-byte aligned device pointers, one asynchronous launch
 * without scratch, outputs that do not overlap inputs, nothing written on an error.  centred(x, q) is the representative
 * in (-q/2, q/2], the convention of the rescale's delta.
 * Key (the relinearisation key and a Galois key share one shape): R' = np - 1 rows, one per data prime, np columns; k0
 * and k1 are uint32 [R'][np][n], NTT form.  Row j at prime i, mod q_i and canonical:
 *     k1[j][i] = a_{j,i}
 *     k0[j][i] = -a_{j,i} . s_hat_i + NTT_i(e_j mod q_i) + [i == j] . (P mod q_j) . target_j,
 * target_j = s_hat_j^2 (relinearisation) or sigma(s_hat)_j (Galois key of an element).  The diagonal is P times the CRT
 * basis element of q_j over Q P, which is 0 mod P: column p has no diagonal, and ONE key serves every level L <= np - 1
 * (rows j < L, columns i < L and column p).  Minus its diagonal, row j is exactly public key j of se_amd_gen_keys_batch
 * with K = R', sk_in = this key replicated, pk_seeds = a_seeds and ep_seeds = e_seeds ([R'][64]; Galois: [G][R'][64]).
 * The gen / set entries take host pointers and refuse what their digit twins refuse (a 2-bit code 3, a word >= q_i, an
 * even, too large or repeated element, G = 0, G > SE_AMD_MAX_GALOIS_KEYS); an install is built beside the previous
 * one, swapped in at the end, and the previous block is freed after the calls in flight; a refused install leaves the
 * previous one usable.  The special-prime keys are installed sets of their own: neither install touches the digit
 * keys, and an installed digit key does not serve the entries of this block.  Device memory per key: 16 R' np n =
 * 16 (np - 1) np n bytes, half of a digit key (4096 x 3: 384 KiB; 16384 x 13: 39 MiB).
 * Key switch of a level-L row polynomial d:
 *     D_j     = centred(INTT_j(d[j]), q_j), j < L               natural order, n^-1 included: |D_j| < q_j / 2 < P / 2
 *     acc_k[i] = sum_{j < L} NTT_i(D_j mod q_i) . k_k[j][i]     k in {0, 1}, i in {0 .. L-1, p}; for i = j the factor is d[j]
 *     delta_k = centred(INTT_p(acc_k[p]), P)
 *     ks_k[i] = (acc_k[i] - NTT_i(delta_k mod q_i)) . P^-1      mod q_i, i < L: the rescale's map with P dropped, the
 *                                                               constants of se_amd_rescale_constants(degree, np, ...)
 * se_amd_ct_relin_sp_device: (d0, d1, d2) -> out0 = d0 + ks_0, out1 = d1 + ks_1 with d = d2.
 * se_amd_ct_galois_sp_device: (c0, c1), element elt -> out0 = sigma(c0) + ks_0, out1 = ks_1 with d = sigma(c1): the
 * relinearisation entry on (sigma(c0), 0, sigma(c1)) with the Galois key installed as the relinearisation key.
 * Both maps are defined on arbitrary residue slabs and arbitrary installed key words below q_i; no secret key is needed.
 * SE_ERR_INVALD_ARGUMENT for the digit twins' argument errors, np = 1, primes outside [1, np - 1]; SE_ERR_NO_KEY when no
 * special-prime key is installed, or none for elt.  B = 0 is a successful no-op.
 * se_amd_ct_drop_primes_device: rows 0 .. primes_out - 1 of every record, [B][primes_in][n] -> [B][primes_out][n], 1 <=
 * primes_out <= primes_in <= np; d_in1 and d_out1 both NULL: one slab.  A pitched asynchronous device copy, no kernel.
 * A fresh record is at level np and the entries above need level np - 1 at most; dropping a prime changes neither
 * message nor scale.  SE_ERR_INVALD_ARGUMENT for a NULL or misaligned slab, one of d_in1 / d_out1 alone, levels out of
 * range, B at or above 2^32.
 * The sum and linear-transform forms on this key are the next block.  Out of scope: the hoisted many form on the
 * special-prime key, several special primes, custom chains, host-pointer and multi-device forms. */
int se_amd_gen_relin_key_sp(se_amd_ctx *ctx, const uint8_t *sk_packed, const uint8_t *a_seeds /*[R'][64]*/,
                            const uint8_t *e_seeds /*[R'][64]*/, uint32_t *evk0, uint32_t *evk1 /*[R'][np][n], host out*/);
int se_amd_set_relin_key_sp(se_amd_ctx *ctx, const uint32_t *evk0, const uint32_t *evk1);
int se_amd_gen_galois_keys_sp(se_amd_ctx *ctx, const uint8_t *sk_packed, const uint32_t *elts, size_t G,
                              const uint8_t *a_seeds /*[G][R'][64]*/, const uint8_t *e_seeds /*[G][R'][64]*/,
                              uint32_t *gk0, uint32_t *gk1 /*[G][R'][np][n], host out*/);
int se_amd_set_galois_keys_sp(se_amd_ctx *ctx, const uint32_t *elts, size_t G, const uint32_t *gk0, const uint32_t *gk1);
int se_amd_ct_relin_sp_device(se_amd_ctx *ctx, const uint32_t *d_d0, const uint32_t *d_d1, const uint32_t *d_d2, size_t B,
                              size_t primes, uint32_t *d_out0, uint32_t *d_out1, void *stream);
int se_amd_ct_galois_sp_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                               uint32_t elt, uint32_t *d_out0, uint32_t *d_out1, void *stream);
int se_amd_ct_drop_primes_device(se_amd_ctx *ctx, const uint32_t *d_in0, const uint32_t *d_in1 /* NULL: one slab */,
                                 size_t B, size_t primes_in, size_t primes_out, uint32_t *d_out0,
                                 uint32_t *d_out1 /* NULL with d_in1 */, void *stream);
/* ---- special-prime hoisted rotations: the sum form and linear transforms at the record's own scale ----
 * The sum of G rotations (se_amd_ct_galois_sum_sp_device) and the plaintext-weighted sum of G rotations
 * (se_amd_ct_lintrans_sp_device) on the special-prime Galois keys, with ONE decomposition of c1 and ONE division by P per
 * record whatever G is ("double hoisting"): a moving sum or a diagonal-method matrix-vector product on FRESH records, with
 * no lift and no level spent on the key switch.  Notation is that of the block above: p = np - 1, P = q_p, records at
 * level 1 <= L <= np - 1, E = {0 .. L-1, p}, centred(x, q) in (-q/2, q/2], src_e = se_amd_galois_table(elts[e]), (k0^e,
 * k1^e) the installed special-prime Galois key of elts[e].  The digits are taken from c1 ITSELF, once, and sigma is
 * applied to the transformed digit as a permutation:
 *     D_j         = centred(INTT_j(c1[b][j]), q_j)                     j < L, natural order
 *     F_{j,i}     = NTT_i(D_j mod q_i)                                 i in E   (F_{j,j} is c1[b][j] as it lies)
 *     ACC_k[i][x] = sum_e w_e[i][x] . sum_{j<L} F_{j,i}[src_e(x)] . k_k^e[j][i][x]     mod q_i, i in E, k in {0, 1}
 *     delta_k     = centred(INTT_p(ACC_k[p]), P)
 *     ks_k[i]     = (ACC_k[i] - NTT_i(delta_k mod q_i)) . P^-1         mod q_i, i < L (se_amd_rescale_constants(degree, np, ..))
 *     out0[i][x]  = ks_0[i][x] + w_0[i][x] . c0[b][i][x] + sum_e w_e[i][x] . c0[b][i][src_e(x)]
 *     out1[i][x]  = ks_1[i][x] + w_0[i][x] . c1[b][i][x]
 * all canonical; an element listed twice counts twice.  Sum form: w_e = 1 and w_0 = add_input ? 1 : 0.  Linear transform:
 * w_e = d_e mod q_i, the e-th diagonal INCLUDING its row at prime p, which enters ACC_k[p]; w_0 = d_0, no w_0 terms when
 * d_diag0 is NULL.  The record's own term and the c0 terms are added after the division by P: they are exact.
 * Two facts.  (1) Centring commutes with sigma -- a negated coefficient q - c centres to -centred(c) -- so sigma(D_j) is
 * the digit of sigma(c1), and the sum form with G = 1, add_input = 0 is BIT-IDENTICAL to se_amd_ct_galois_sp_device (the
 * digit twin se_amd_ct_galois_sum_device has no such property: see there).  (2) G >= 2 does NOT equal the sum of G single
 * calls: that sum carries G roundings delta^e, this form carries centred(sum_e delta^e mod P), and the two differ
 * wherever |sum_e delta^e| > P/2 -- about a quarter of the coefficients at G = 2 on random data.  One rounding instead of
 * G; a workgroup's transforms stay at 4 L + 2 whatever G is.
 * Conventions are those of the digit twins and of se_amd_ct_galois_sp_device: level-`primes` slabs [B][primes][n], 16-byte
 * aligned; one asynchronous launch, no scratch, no host synchronisation in the device entries; outputs do not overlap
 * inputs; nothing is written on an error; B = 0 is a successful no-op.  SE_ERR_INVALD_ARGUMENT for the argument errors of
 * se_amd_ct_galois_sum_device / se_amd_ct_lintrans_device, np = 1, primes outside [1, np - 1]; SE_ERR_NO_KEY when an
 * element has no installed SPECIAL-PRIME key (installed digit keys do not serve these entries; the last-error text names
 * the element).
 * se_amd_lintrans_create_sp: as se_amd_lintrans_create, on the installed special-prime blocks.  pt_primes MUST equal np:
 * the diagonals' row at the special prime is folded into key column p (anything else: SE_ERR_INVALD_ARGUMENT).  The plan
 * serves the levels 1 .. np - 1.  It is a snapshot: the words k . d_e mod q_c with their Shoup companions for every column
 * c, p included, and the (word, Shoup) rows of the diagonals; (G . 16 (np - 1) np + (G + 1) . 8 np) n bytes of device
 * memory (4096 x 3, G = 7: 3.4 MiB; 16384 x 13, G = 7: 286 MiB).  se_amd_lintrans_destroy serves both kinds of plan.
 * A plan has a kind: se_amd_ct_lintrans_device refuses a special-prime plan and se_amd_ct_lintrans_sp_device refuses a
 * digit plan, both with SE_ERR_INVALD_ARGUMENT and nothing written.
 * Beyond 64 diagonals: the baby-step / giant-step plans on this key (se_amd_bsgs_create_sp below), whose baby steps are
 * the UNDIVIDED many form.  Out of scope: several special primes, custom chains, host-pointer and multi-device forms. */
int se_amd_ct_galois_sum_sp_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                                   const uint32_t *elts /*host, [G]*/, size_t G, int add_input, uint32_t *d_out0,
                                   uint32_t *d_out1, void *stream);
int se_amd_lintrans_create_sp(se_amd_ctx *ctx, const uint32_t *elts /*host, [G]*/, size_t G, const uint32_t *d_diag,
                              const uint32_t *d_diag0, size_t pt_primes, se_amd_lintrans **out);
int se_amd_ct_lintrans_sp_device(se_amd_ctx *ctx, const se_amd_lintrans *plan, const uint32_t *d_c0, const uint32_t *d_c1,
                                 size_t B, size_t primes, uint32_t *d_out0, uint32_t *d_out1, void *stream);
/* ---- baby-step / giant-step linear transforms on the digit Galois keys ----------------------------------
 * A linear-transform plan above costs one Galois key and one folded key block per diagonal, so it ends at
 * SE_AMD_MAX_GALOIS_KEYS = 64 diagonals.  With the diagonals indexed by a product of elements,
 *     y = sum_{g < n2, b < n1} d[g][b] . rot_{giant[g] . baby[b] mod 2n}(x)       slot-wise,
 * n1 + n2 - 2 keys serve n1 . n2 diagonals (64 as 8 x 8: 14 keys instead of 63; 2048 as 32 x 64: 94 keys), and a plan
 * holds diagonals only.  The digit-key family only (se_amd_set_galois_keys, 15-bit digits), every degree and level its
 * entries serve.  Conventions are theirs: level-`primes` slabs [records][primes][n] in NTT form, bit-reversed order,
 * canonical residues; 16-byte aligned device pointers; asynchronous on `stream`; outputs do not overlap inputs; nothing
 * is launched or written on an error; B = 0 is a successful no-op; errors through se_amd_last_error.
 * se_amd_ct_mul_plain_sum_device: a plaintext-weighted sum over a stack of E batches, key-free, one launch.
 *     in  (d_in0, d_in1)   [E][B][primes][n]          d_in1 and d_out1 both NULL: one slab
 *     pt  d_pt             [Gout][E][pt_primes][n]    the layout se_amd_encode_ntt_device writes; pt_primes >= primes
 *     out (d_out0, d_out1) [Gout][B][primes][n]
 *     out[g][b][i][k] = sum_{e < E} (pt[g][e][i][k] mod q_i) . in[e][b][i][k]     mod q_i, canonical.
 * 1 <= E <= 64 and 1 <= Gout <= 64.  Any 32-bit plaintext word stands for its residue, as in
 * se_amd_ct_mul_plain_device; every bit is fixed: the result equals se_amd_ct_mul_plain_device per (g, e) followed by the
 * modular sum, and is exact for every input (E = 64 with all words at q_i - 1 included).  SE_ERR_INVALD_ARGUMENT for the
 * argument errors of se_amd_ct_mul_plain_device (a NULL d_in0 / d_out0 / d_pt, one of d_in1 / d_out1 alone, primes outside
 * [1, np], pt_primes < primes, B at or above 2^32, a pointer that is not 16-byte aligned), E or Gout outside [1, 64],
 * E . B or Gout . B at or above 2^32.
 * se_amd_ct_galois_accum_device: rotate G DIFFERENT ciphertexts and add, one launch, no scratch.
 *     in (d_in0, d_in1) [G][B][primes][n];  elts HOST [G], 1 <= G <= 64, odd, below 2n, repeats allowed
 *     out[b] = sum_{g < G} rho_g(in[g][b])     mod q_i, canonical, [B][primes][n]
 * rho_g is the map of se_amd_ct_galois_device with elts[g] (the digits of sigma(c1), the installed digit key), and the
 * identity when elts[g] == 1, which needs no key.  The output equals, bit for bit, the modular sum of G
 * se_amd_ct_galois_device outputs.  SE_ERR_INVALD_ARGUMENT for the argument errors of se_amd_ct_galois_many_device, and
 * for G . B at or above 2^32; SE_ERR_NO_KEY when an element other than 1 has no installed key (the last-error text names
 * it).
 * The plan.  se_amd_bsgs_create: baby HOST [n1], giant HOST [n2], 1 <= n1, n2 <= 64, elements odd and below 2n, no
 * element twice within a list (SE_ERR_INVALD_ARGUMENT); element 1 may appear once in each list and needs no key.  d_diag
 * is DEVICE memory [n2][n1][pt_primes][n], pt_primes >= 1: d[g][b] is the diagonal of the COMPOSITE element giant[g] .
 * baby[b] mod 2n, unrotated, as a flat plan would take it.  The plan serves primes <= min(pt_primes, np).  Create stores
 *     d'[g][b][i][k] = d[g][b][i][src_{giant[g]^-1 mod 2n}(k)],      src from se_amd_galois_table:
 * on an NTT-form row a plaintext rotation is that permutation and src_a o src_{a^-1} is the identity, so
 * sigma_gamma(d' . z) = d . sigma_gamma(z).  The plan is a snapshot of the diagonals ONLY: create synchronises, the
 * diagonals may be freed afterwards, and no key is read.  Plan memory: n1 . n2 . pt_primes . n words (no Shoup
 * companions: the step that reads them is bound by memory traffic, which they would double).  A failed create leaves
 * *out NULL.  se_amd_bsgs_destroy waits for the device, then frees; NULL is a no-op; destroy plans before their context.
 * se_amd_ct_bsgs_device is fixed bit for bit as
 *     rot[b]   = (c0, c1) if baby[b] == 1, else the se_amd_ct_galois_many_device output for baby[b]  (digits of c1 itself)
 *     inner[g] = sum_b d'[g][b] . rot[b]                          se_amd_ct_mul_plain_sum_device
 *     out      = sum_g rho_g(inner[g])                            se_amd_ct_galois_accum_device, elements giant[g]
 * Keys are read from the context at CALL time: SE_ERR_NO_KEY names the element without a key, and a later
 * se_amd_set_galois_keys takes effect on the next call.  The scale is multiplied by the diagonals' scale, the level is
 * unchanged; the result carries the key-switch term of a baby step weighted by a diagonal and that of a giant step on top.
 * Workspace: the caller's, used in stream order; no context scratch, no hidden allocation, no host synchronisation.  One
 * record needs 2 . (n1 + n2) . primes . n . 4 bytes (both halves of the rot and of the inner stack);
 * se_amd_bsgs_workspace_bytes returns records times that (0 for a NULL plan).  The call takes Bc = min(B, workspace_bytes
 * / per-record) and walks the batch in chunks of Bc records: the chunk is copied into the identity slot of rot (if 1 is
 * listed), the many form fills the other slots, then the two steps above, the second straight into the chunk's output
 * rows.  Every chunk size gives the same bits.  SE_ERR_INVALD_ARGUMENT for the pointer, alignment, level and B checks of
 * se_amd_ct_galois_device, a NULL plan, a plan of another context, primes above the plan's levels, a NULL workspace, one
 * that is not 16-byte aligned or one below one record.
 * The special-prime family has its own plan kind (se_amd_bsgs_create_sp below); se_amd_ct_bsgs_device refuses such a
 * plan with SE_ERR_INVALD_ARGUMENT and nothing written.  Out of scope: sparse diagonal masks, multi-device and
 * host-pointer forms. */
int se_amd_ct_mul_plain_sum_device(se_amd_ctx *ctx, const uint32_t *d_in0, const uint32_t *d_in1 /* NULL: one slab */,
                                   size_t E, size_t B, size_t primes, const uint32_t *d_pt, size_t Gout, size_t pt_primes,
                                   uint32_t *d_out0, uint32_t *d_out1 /* NULL with d_in1 */, void *stream);
int se_amd_ct_galois_accum_device(se_amd_ctx *ctx, const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t primes,
                                  const uint32_t *elts /*host, [G]*/, size_t G, uint32_t *d_out0, uint32_t *d_out1,
                                  void *stream);
typedef struct se_amd_bsgs se_amd_bsgs;
int se_amd_bsgs_create(se_amd_ctx *ctx, const uint32_t *baby /*host, [n1]*/, size_t n1, const uint32_t *giant /*host, [n2]*/,
                       size_t n2, const uint32_t *d_diag /*device, [n2][n1][pt_primes][n]*/, size_t pt_primes,
                       se_amd_bsgs **out);
void se_amd_bsgs_destroy(se_amd_bsgs *plan);
size_t se_amd_bsgs_workspace_bytes(const se_amd_bsgs *plan, size_t records, size_t primes);
int se_amd_ct_bsgs_device(se_amd_ctx *ctx, const se_amd_bsgs *plan, const uint32_t *d_c0, const uint32_t *d_c1, size_t B,
                          size_t primes, uint32_t *d_out0, uint32_t *d_out1, void *d_workspace, size_t workspace_bytes,
                          void *stream);
/* ---- baby-step / giant-step linear transforms on the special-prime keys, division by P deferred ----------
 * The plans above meet fresh records only after a lift; the special-prime linear transform ends at 64 diagonals.  Here
 * the baby steps stay UNDIVIDED, as residues modulo q_0 .. q_{L-1}, P: the diagonals are multiplied in there, their row at
 * P included, every giant step's inner sum is divided by P once and the giant steps share ONE more division: n2 + 1
 * roundings for n1 . n2 diagonals, at the record's own scale, no lift, no level spent.  Notation of the special-prime
 * block: p = np - 1, P = q_p, L = primes in [1, np - 1], E = {0 .. L-1, p}, centred(x, q) in (-q/2, q/2], src_e =
 * se_amd_galois_table(elts[e]), (k0^e, k1^e) the installed SPECIAL-PRIME Galois key of elts[e] (an installed digit key
 * does not serve).  An EXTENDED record is [L + 1][n] words per half: rows r < L modulo q_r, row L modulo P, NTT form,
 * bit-reversed, canonical: "P times a ciphertext plus a key-switch sum", not decryptable until it is brought down.
 * Conventions are those above: 16-byte aligned device pointers; asynchronous on `stream`; outputs do not overlap inputs;
 * nothing is launched or written on an error; B = 0 (count = 0) is a successful no-op.  Every step is exact modular
 * arithmetic or a centred rounding: every bit is fixed.  Every entry returns SE_ERR_INVALD_ARGUMENT on a one-prime
 * context, for a NULL slab, primes outside [1, np - 1], a pointer that is not 16-byte aligned, B at or above 2^32.
 * se_amd_ct_galois_many_ext_sp_device: (d_c0, d_c1) [B][L][n], elts HOST [G], 1 <= G <= 64, odd, below 2n -> (d_out0,
 * d_out1) [G][B][L+1][n].  The digits are those of c1 itself, taken once:
 *     D_j = centred(INTT_j(c1[b][j]), q_j), j < L;   F_{j,i} = NTT_i(D_j mod q_i), i in E   (F_{j,j} is c1[b][j] as it lies)
 *     U^e_k[i][x] = sum_{j<L} F_{j,i}[src_e(x)] . k_k^e[j][i][x]   mod q_i
 *     out0[e][b][r] = U^e_0[i_r] + [r < L] (P mod q_r) . c0[b][r][src_e(x)];   out1[e][b][r] = U^e_1[i_r]   (i_r = r, or p for r = L)
 *     elts[e] == 1: out_k[e][b][r] = (P mod q_r) . c_k[b][r] for r < L, row L all zero; no key needed.
 * G . B below 2^32.  SE_ERR_NO_KEY names the element other than 1 without a special-prime key.
 * se_amd_ct_mul_plain_sum_ext_sp_device: se_amd_ct_mul_plain_sum_device on stacks of extended records, in [E][B][L+1][n],
 * out [Gout][B][L+1][n]; row r < L uses q_r and plaintext row r, row L uses P and plaintext row p; plaintexts
 * [Gout][E][np][n], ALL np rows, any 32-bit words.  At L = np - 1 it is bit for bit the plain entry with primes = np.
 * se_amd_ct_mod_down_sp_device: [count][L+1][n] -> [count][L][n] on one slab (d_in1 = d_out1 = NULL) or two,
 *     delta = centred(INTT_p(in[L]), P);   out[i] = (in[i] - NTT_i(delta mod q_i)) . P^-1 mod q_i,
 * the rescale's map with P as the dropped prime and the constants of se_amd_rescale_constants(degree, np, ..).  At L =
 * np - 1 it is bit for bit se_amd_ct_rescale_device with primes = np.  count at most 2^31 - 1.
 * se_amd_ct_galois_accum_sp_device: the one-division giant sum of G DIFFERENT level-L ciphertexts (a^g, b^g) = in[g][b],
 * in [G][B][L][n], out [B][L][n]:
 *     keyed g (elts[g] != 1):  D^g_j = centred(INTT_j(sigma_g(b^g[j])), q_j)          (the digits of se_amd_ct_galois_sp_device)
 *     ACC_k[i] = sum_{keyed g} sum_{j<L} NTT_i(D^g_j mod q_i) . k_k^g[j][i],  i in E
 *     delta_k = centred(INTT_p(ACC_k[p]), P);   ks_k[i] = (ACC_k[i] - NTT_i(delta_k mod q_i)) . P^-1
 *     out0[i] = ks_0[i] + sum_{keyed g} sigma_g(a^g)[i] + sum_{elts[g]==1} a^g[i];   out1[i] = ks_1[i] + sum_{elts[g]==1} b^g[i].
 * With G = 1 it has the bytes of se_amd_ct_galois_sp_device; with G >= 2 it does NOT equal the sum of single calls: it
 * rounds once.  G . B below 2^32; SE_ERR_NO_KEY as above.
 * The plan.  se_amd_bsgs_create_sp takes the arguments of se_amd_bsgs_create and pre-rotates the same way, but pt_primes
 * must equal np (the row at P enters the sum) and the plan serves the levels 1 .. np - 1.  It holds diagonals only; keys
 * are read at CALL time.  A plan has a kind: each call entry refuses the other kind with SE_ERR_INVALD_ARGUMENT and
 * writes nothing; se_amd_bsgs_destroy and se_amd_bsgs_workspace_bytes serve both.  se_amd_ct_bsgs_sp_device has the
 * argument list of se_amd_ct_bsgs_device and is fixed bit for bit as
 *     U[b] = many_ext(c; baby[b])                          [n1][Bc][L+1][n]
 *     V[g] = sum_b d'[g][b] . U[b]   on the rows E          [n2][Bc][L+1][n]
 *     W[g] = mod_down(V[g])                                 [n2][Bc][L][n]
 *     out  = accum_sp(W; giant)                             scale Delta . Delta_d, level L.
 * Workspace: the caller's, in stream order; no context scratch, no hidden allocation, no host synchronisation.  One record
 * needs 2 . ((n1 + n2) . (L + 1) + n2 . L) . n . 4 bytes (both halves of U, V and W; W does not overlay U);
 * se_amd_bsgs_workspace_bytes returns records times that.  The batch is walked in chunks of Bc = min(B, workspace_bytes /
 * per-record) records and every chunk size gives the same bits. */
int se_amd_ct_galois_many_ext_sp_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B,
                                        size_t primes, const uint32_t *elts /*host, [G]*/, size_t G, uint32_t *d_out0,
                                        uint32_t *d_out1, void *stream);
int se_amd_ct_mul_plain_sum_ext_sp_device(se_amd_ctx *ctx, const uint32_t *d_in0, const uint32_t *d_in1 /* NULL: one slab */,
                                          size_t E, size_t B, size_t primes, const uint32_t *d_pt, size_t Gout,
                                          uint32_t *d_out0, uint32_t *d_out1 /* NULL with d_in1 */, void *stream);
int se_amd_ct_mod_down_sp_device(se_amd_ctx *ctx, const uint32_t *d_in0, const uint32_t *d_in1 /* NULL: one slab */,
                                 size_t count, size_t primes, uint32_t *d_out0, uint32_t *d_out1 /* NULL with d_in1 */,
                                 void *stream);
int se_amd_ct_galois_accum_sp_device(se_amd_ctx *ctx, const uint32_t *d_in0, const uint32_t *d_in1, size_t B,
                                     size_t primes, const uint32_t *elts /*host, [G]*/, size_t G, uint32_t *d_out0,
                                     uint32_t *d_out1, void *stream);
int se_amd_bsgs_create_sp(se_amd_ctx *ctx, const uint32_t *baby /*host, [n1]*/, size_t n1,
                          const uint32_t *giant /*host, [n2]*/, size_t n2,
                          const uint32_t *d_diag /*device, [n2][n1][np][n]*/, size_t pt_primes, se_amd_bsgs **out);
int se_amd_ct_bsgs_sp_device(se_amd_ctx *ctx, const se_amd_bsgs *plan, const uint32_t *d_c0, const uint32_t *d_c1,
                             size_t B, size_t primes, uint32_t *d_out0, uint32_t *d_out1, void *d_workspace,
                             size_t workspace_bytes, void *stream);
/* ---- switch-key rings: bring records of many keys under one key, and sum them ------------------------------
 * The key rings above put one batch under K device keys, one key index per ciphertext; everything behind them -- sums
 * (se_amd_ct_lincomb_device: "All records of a row must be under the same key"), products, rotations, plans -- works
 * under ONE key.  A switching key closes the gap: a special-prime key whose diagonal hides P . s_from under s_to moves a
 * record from key `from` to key `to` at the record's own scale, with no lift and no level spent, exactly as a Galois key
 * does for sigma(s).  A ring holds K of them, chosen per record.  Notation is that of the special-prime block: p = np - 1,
 * P = q_p, records at level 1 <= L <= np - 1, E = {0 .. L-1, p}, R' = np - 1, centred(x, q) in (-q/2, q/2]; conventions
 * those of se_amd_ct_relin_sp_device: level-`primes` slabs [B][primes][n], 16-byte aligned; one asynchronous launch, no
 * scratch, no host synchronisation; outputs do not overlap inputs; nothing is written on an argument error; B = 0 resp.
 * G = 0 is a successful no-op; np >= 2.
 * WHO RUNS THE GENERATOR.  se_amd_gen_switch_keys_sp needs BOTH secrets, every s_from_k and s_to.  It belongs to the
 * authority that issued the device keys (the role of the reference's adapter), never to the evaluator: the evaluator
 * receives wk0 / wk1, which are public material like every evaluation key, and installs them.  A public-key form, in which
 * a device makes its own switching key from the target's public key, is out of scope.
 * Key k of the ring has the shape of every special-prime key: wk0, wk1 uint32 [K][R'][np][n], NTT form, canonical,
 *     wk1[k][j][i] = a_{k,j,i}
 *     wk0[k][j][i] = -a_{k,j,i} . s_to_hat_i + NTT_i(e_{k,j}) + [i == j] . (P mod q_j) . s_from_k_hat_j.
 * Minus its diagonal, row j of key k is exactly public key j of se_amd_gen_keys_batch with K = R', sk_in = sk_to replicated,
 * pk_seeds = a_seeds[k] and ep_seeds = e_seeds[k].  Column p has no diagonal and one key serves every level.  The generator
 * takes host pointers, installs nothing, keeps its device copies of secret material in wiped buffers, and refuses a 2-bit
 * code 3 in any of the K + 1 secret keys, K = 0, NULL pointers and np = 1.
 * se_amd_set_switch_keyring_sp validates every word < q_i (else SE_ERR_INVALD_ARGUMENT; also K = 0), builds the ring --
 * per key the device block of the other special-prime keys, with Shoup companions, keys at a fixed stride -- BESIDE the
 * installed ring and swaps it in at the end: a refused or failed install leaves the previous ring usable, and calls in
 * flight finish on the old one.  The ring is an installed set of its own: it neither touches nor is served by the
 * relinearisation key, the Galois keys, the digit keys or the secret / public rings.  Device memory: 16 (np - 1) np n bytes
 * per key (4096 x 3: 384 KiB, so 512 keys take 192 MiB).
 * se_amd_ct_switch_keyed_sp_device: for record b with k = d_key_idx[b], out0 = c0 + ks_0 and out1 = ks_1, ks the "key
 * switch of a level-L row polynomial" above applied to d = c1[b] under ring key k: BIT-IDENTICAL to
 * se_amd_ct_relin_sp_device(c0, 0, c1) with ring key k installed as the relinearisation key.  Defined on arbitrary residue
 * slabs and key words; no secret key is needed.  k >= K never forms an address: the workgroup compares the index with K
 * (wave-uniform), such a record gets all-zero outputs and status 2, the other records status 1 and are unaffected -- the
 * ring's convention, without a sanitising pass and without scratch.
 * se_amd_ct_switch_sum_keyed_sp_device: the CSR rows of se_amd_ct_lincomb_device, unweighted: row g takes the records b =
 * d_idx[t], t in [d_row_ptr[g], d_row_ptr[g + 1]); a record listed twice counts twice.  ONE division by P per row:
 *     D_{b,j}    = centred(INTT_j(c1[b][j]), q_j)                                               j < L
 *     ACC_k[i]   = sum_{b in row} sum_{j<L} NTT_i(D_{b,j} mod q_i) . ring[key_idx[b]]_k[j][i]   i in E (for i = j the factor is
 *                                                                                               c1[b][j] as it lies)
 *     delta_k    = centred(INTT_p(ACC_k[p]), P)
 *     out0[g][i] = (ACC_0[i] - NTT_i(delta_0 mod q_i)) . P^-1 + sum_{b in row} c0[b][i]         mod q_i, canonical
 *     out1[g][i] = (ACC_1[i] - NTT_i(delta_1 mod q_i)) . P^-1
 * The c0 terms are added after the division: they are exact.  Two facts.  (1) A row of one record is BIT-IDENTICAL to
 * se_amd_ct_switch_keyed_sp_device on that record.  (2) A row of m >= 2 records is NOT the modular sum of m single
 * switches: it carries centred(sum_b delta^b mod P) instead of m roundings delta^b, and differs wherever |sum_b delta^b| >
 * P/2.  One rounding instead of m, and (4 L - 2) m + 4 transforms per output row and prime against (4 L + 2) m.
 * Status (uint8 [G], optional): an empty row is all zero with status 1; a row with a record index >= B, a member whose key
 * index is >= K, or a d_row_ptr pair that decreases or reaches beyond nnz is all zero in both slabs with status 2.  Nothing
 * is read out of bounds, and the status is decided before anything of the row is written.
 * The result is under s_to at the records' scale and level: it goes straight into se_amd_ct_lincomb_device, a plan or
 * se_amd_decrypt_level_device.  A row runs on L workgroups whatever its length and is not sliced: sum a large batch in two
 * tiers, switch-sum in groups (tens of records), then se_amd_ct_lincomb_device over the group sums, which are all under s_to.
 * SE_ERR_NO_KEY without an installed switch ring; SE_ERR_INVALD_ARGUMENT for the argument errors of
 * se_amd_ct_relin_sp_device, a NULL d_key_idx, and in the sum form a NULL d_row_ptr, a NULL d_idx with nnz > 0, G or nnz at
 * or above 2^32.  Out of scope: slicing long rows, weighted rows, a public-key generator, several special primes, digit
 * switching keys, host-pointer and multi-device forms, installing the ring from device pointers. */
int se_amd_gen_switch_keys_sp(se_amd_ctx *ctx, size_t K, const uint8_t *sk_from /*[K][n/4]*/, const uint8_t *sk_to /*[n/4]*/,
                              const uint8_t *a_seeds /*[K][R'][64]*/, const uint8_t *e_seeds /*[K][R'][64]*/,
                              uint32_t *wk0, uint32_t *wk1 /*[K][R'][np][n], host out*/);
int se_amd_set_switch_keyring_sp(se_amd_ctx *ctx, size_t K, const uint32_t *wk0, const uint32_t *wk1);
int se_amd_ct_switch_keyed_sp_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                                     const uint32_t *d_key_idx /*[B]*/, uint32_t *d_out0, uint32_t *d_out1,
                                     uint8_t *d_status /*[B], optional*/, void *stream);
int se_amd_ct_switch_sum_keyed_sp_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                                         const uint32_t *d_key_idx /*[B]*/, size_t G, const uint32_t *d_row_ptr /*[G+1]*/,
                                         const uint32_t *d_idx /*[nnz]*/, size_t nnz, uint32_t *d_out0, uint32_t *d_out1
                                         /*[G][primes][n]*/, uint8_t *d_status /*[G], optional*/, void *stream);
/* Slot packing: per-entry rotations of many records summed in one call,
 *     out[g] = sum_{k in row g} rot_{elts[d_eidx[k]]}( record d_idx[k] ).
 * Devices send short records: a 16- or 128-entry vector in the low slots of a 2048-slot ciphertext at n = 4096, and every
 * later step pays for the empty slots.  Packing m = slots / width records into one divides all of that by m.  The same
 * entry is the per-record element list (the single form) and the shift-and-add across time-ordered records (a row of
 * several records with different steps).
 * Notation of the special-prime blocks above: p = np - 1, P = q_p, records [B][L][n] at level L = primes, 1 <= L <= np - 1,
 * E = {0 .. L-1, p} the output primes of the key switch, centred(x, q) in (-q/2, q/2], and (k0^e, k1^e) the INSTALLED
 * special-prime Galois key of elts[e] (se_amd_set_galois_keys_sp): no new key type and no new generator.
 * Elements: `elts` is a host list of 1 <= E <= SE_AMD_MAX_GALOIS_KEYS odd elements below 2n (the argument E is its
 * length).  Element 1 is allowed and needs no key: the identity, with no key switch.  A repeated element is allowed.
 * Entries: entry k is the pair (record d_idx[k], element elts[d_eidx[k]]); row g takes the entries k in [d_row_ptr[g],
 * d_row_ptr[g + 1]); an entry listed twice counts twice.  Single form: d_row_ptr == d_idx == NULL makes row g the one
 * entry (record g, element elts[d_eidx[g]]) and requires G == B == nnz: a different element per record.
 * Per row, with sigma_k the automorphism of elts[d_eidx[k]], b_k = d_idx[k], everything canonical:
 *     D_{k,j}    = centred(INTT_j(c1[b_k][j]), q_j)                                            j < L
 *     F_{k,j,i}  = NTT_i(sigma_k(D_{k,j}) mod q_i)                                             i in E (for i = j:
 *                                                                                              sigma_k(c1[b_k][j]) as it lies)
 *     ACC_h[i]   = sum_{k in row, elt_k != 1} sum_{j<L} F_{k,j,i} . k_h^{e_k}[j][i]   mod q_i,    h in {0, 1}
 *     delta_h    = centred(INTT_p(ACC_h[p]), P)
 *     ks_h[i]    = (ACC_h[i] - NTT_i(delta_h mod q_i)) . P^-1   mod q_i, i < L        (se_amd_rescale_constants(degree, np, ..))
 *     out0[g][i] = ks_0[i] + sum_{k in row} sigma_k(c0[b_k])[i]
 *     out1[g][i] = ks_1[i] + sum_{k in row, elt_k = 1} c1[b_k][i]
 * The c0 terms and the identity entries are added after the division: they are exact.  Five facts.
 * (1) A row of one entry with element g != 1 is BIT-IDENTICAL to se_amd_ct_galois_sp_device on that record with elt = g:
 *     the single form is a batch of such calls with a different element per record.
 * (2) A row that lists ONE record once per element of `elts` is BIT-IDENTICAL to se_amd_ct_galois_sum_sp_device on that
 *     record with the non-identity elements (the identity, if listed, is served by add_input = 1): the sums in ACC are
 *     exact and centring commutes with sigma, fact (1) of that block.
 * (3) A row of identity entries only has ks = 0 and is the plain modular sum of the records.
 * (4) A row of m >= 2 rotated entries is NOT the modular sum of m single rotations: it carries centred(sum_k delta^k mod P)
 *     instead of m roundings, and differs wherever |sum_k delta^k| > P/2.
 * (5) Scale and level are unchanged: the result is an ordinary level-L record under the same key.
 * One launch, no scratch, no global temporary: (4 L - 2) m + 4 transforms per output row and prime for m rotated entries
 * against (4 L + 2) m for m single rotations, whose m intermediate records and the sum over them are not needed either.
 * A row runs on L workgroups whatever its length and is not sliced: pack a long row in two tiers, in groups, then
 * se_amd_ct_lincomb_device over the group results.
 * Status (uint8 [G], optional): an empty row is all zero with status 1; a row with a d_idx[k] >= B, a d_eidx[k] >= E, or a
 * d_row_ptr pair that decreases or reaches beyond nnz is all zero in both slabs with status 2; other rows are unaffected.
 * Every index is compared before it forms an address, and the status is decided before anything of the row is written.
 * SE_ERR_INVALD_ARGUMENT, with nothing written, for a NULL ctx, slab, elts or d_eidx; exactly one of d_row_ptr / d_idx
 * NULL; the single form with G != B or nnz != B; E = 0 or E > SE_AMD_MAX_GALOIS_KEYS; an even element or one >= 2n;
 * primes outside [1, np - 1]; a context of one prime; B, G or nnz >= 2^32; a slab pointer that is not 16-byte aligned.
 * SE_ERR_NO_KEY when a listed element other than 1 has no installed SPECIAL-PRIME Galois key (digit keys, the
 * relinearisation key and the switch ring do not serve); the last-error text names the element.  G = 0 is a successful
 * no-op.  Out of scope: plaintext masks or weights per entry; a ring key that switches and rotates in one step
 * (se_amd_ct_switch_keyed_sp_device first); hoisting when one record appears under many elements
 * (se_amd_ct_galois_sum_sp_device); a digit-key twin; several special primes; host-pointer and multi-device forms. */
int se_amd_ct_pack_sp_device(se_amd_ctx *ctx, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                             const uint32_t *elts /*host, [E]*/, size_t E,
                             size_t G, const uint32_t *d_row_ptr /*[G+1] or NULL*/, const uint32_t *d_idx /*[nnz] or NULL*/,
                             const uint32_t *d_eidx /*[nnz]*/, size_t nnz,
                             uint32_t *d_out0, uint32_t *d_out1 /*[G][primes][n]*/,
                             uint8_t *d_status /*[G], optional*/, void *stream);
/* Encrypted inner products: grouped product sums.  A variance, an inner product of two senders' vectors, a polynomial
 * score are sums of products, and relinearisation is linear in d2: sum the tensors, key-switch once.  Row g takes the
 * pairs k in [d_row_ptr[g], d_row_ptr[g + 1]) (the CSR rows of se_amd_ct_lincomb_device, unweighted); pair k is record
 * d_ia[k] of (a0, a1) times record d_ib[k] of (b0, b1); with d_ia = d_ib = NULL pair k is (k, k) and nnz == Ba == Bb is
 * required.  A pair listed twice counts twice; the a and b slabs may be the same pointers (squares).  Per prime
 * j < primes and element, canonical in [0, q_j):
 *     T0[g] = sum_k x0 . y0     T1[g] = sum_k (x0 . y1 + x1 . y0)     T2[g] = sum_k x1 . y1      mod q_j
 * se_amd_ct_mul_sum_device, key-free, 1 <= primes <= np: (out0, out1, out2) = (T0, T1, T2), each [G][primes][n].  No key,
 * no scratch, one asynchronous launch, and no per-pair record in memory.  BIT-IDENTICAL to se_amd_ct_mul_device on the
 * pairs followed by the unweighted se_amd_ct_lincomb_device row sums of each slab: the map is exact modular arithmetic,
 * so any evaluation order gives those bits.  The result decrypts with se_amd_decrypt3_level_device, or goes into either
 * relinearisation (se_amd_ct_relin_device serves the digit key).
 * se_amd_ct_dot_sp_device, 1 <= primes <= np - 1, under the installed key of se_amd_set_relin_key_sp: with ks the "key
 * switch of a level-L row polynomial" above applied to d = T2[g] (centred digits, one division by P),
 *     out_k[g] = T_k[g] + ks_k          k = 0, 1,   [G][primes][n] each
 * in ONE launch, with no workspace and the tensor sums never in memory.  Three facts.  (1) A row of one pair is
 * BIT-IDENTICAL to se_amd_ct_mul_device followed by se_amd_ct_relin_sp_device on that pair.  (2) Any row is BIT-IDENTICAL
 * to se_amd_ct_mul_sum_device followed by se_amd_ct_relin_sp_device.  (3) A row of m >= 2 pairs is NOT the modular sum of
 * m relinearised products: it makes one rounding centred(INTT_p(ACC[p]), P) on the summed T2 instead of m, and it needs
 * 4 L + 2 transforms per output row and prime, not (4 L + 2) . m.
 * Scale and level: the product's D_a . D_b at the operands' level, which is unchanged; the result goes straight into
 * se_amd_ct_rescale_device.  Range: the sum of m products of messages must stay below Q_L / 2 like any record, so an
 * inner product of fresh records is one se_amd_ct_drop_primes_device to np - 1, one call, one rescale.  Both entries are
 * defined on arbitrary residue slabs (and key words); no secret key is needed.
 * Status (uint8 [G], optional): an empty row is all zero with status 1; a row with a d_ia[k] >= Ba, a d_ib[k] >= Bb, or a
 * d_row_ptr pair that decreases or reaches beyond nnz is all zero in every output slab with status 2, and the other rows
 * are unaffected.  Nothing is read out of bounds -- an index is compared before it forms an address -- and the status is
 * decided before anything of the row is written.  G = 0 is a successful no-op; Ba or Bb = 0 with non-empty rows gives
 * those rows status 2.  A row runs on L workgroups (dot_sp) whatever its length and is not sliced: sum long rows in two
 * tiers, groups of tens of pairs here, then se_amd_ct_lincomb_device over the group sums.
 * SE_ERR_INVALD_ARGUMENT, with nothing written: NULL ctx, slab or d_row_ptr; only one of d_ia / d_ib NULL; both NULL with
 * nnz != Ba or nnz != Bb; primes outside [1, np] resp. [1, np - 1], and se_amd_ct_dot_sp_device on a context of one
 * prime; Ba, Bb, G or nnz at or above 2^32; a slab pointer that is not 16-byte aligned.  SE_ERR_NO_KEY from
 * se_amd_ct_dot_sp_device without a special-prime relinearisation key: an installed digit key, Galois key or switch ring
 * does not serve.  Out of scope: a digit-key fused form, weighted rows, slicing long rows, a fused rescale, host-pointer
 * and multi-device forms. */
int se_amd_ct_mul_sum_device(se_amd_ctx *ctx, const uint32_t *d_a0, const uint32_t *d_a1, size_t Ba,
                             const uint32_t *d_b0, const uint32_t *d_b1, size_t Bb, size_t primes, size_t G,
                             const uint32_t *d_row_ptr /*[G+1]*/, const uint32_t *d_ia,
                             const uint32_t *d_ib /*[nnz] or both NULL*/, size_t nnz, uint32_t *d_out0, uint32_t *d_out1,
                             uint32_t *d_out2 /*[G][primes][n] each*/, uint8_t *d_status /*[G], optional*/, void *stream);
int se_amd_ct_dot_sp_device(se_amd_ctx *ctx, const uint32_t *d_a0, const uint32_t *d_a1, size_t Ba, const uint32_t *d_b0,
                            const uint32_t *d_b1, size_t Bb, size_t primes, size_t G, const uint32_t *d_row_ptr /*[G+1]*/,
                            const uint32_t *d_ia, const uint32_t *d_ib /*[nnz] or both NULL*/, size_t nnz,
                            uint32_t *d_out0, uint32_t *d_out1 /*[G][primes][n]*/, uint8_t *d_status /*[G], optional*/,
                            void *stream);
/* ---- Slot-wise polynomials: a power ladder and a fused weighted-sum rescale -----------------------------------------
 * se_amd_ct_affine_rescale_device, key-free: the weighted sum of T term records that live at their own levels, ONE
 * rescale of the sum and a constant, in one launch.  d_term0 / d_term1 are HOST arrays of T device pointers; term t is the
 * pair of level-term_primes[t] slabs [B][term_primes[t]][n] with term_primes[t] >= primes, of which only the first
 * `primes` rows of a record are read (the pt_primes convention of se_amd_ct_mul_plain_device); term_primes and w are host
 * arrays [T].  With
 *     acc_s[b][j] = sum_t (w_t mod q_j) . term_s[t][b][j]  mod q_j,   j < primes,
 * w mod q_j the non-negative residue of the int64,
 *     out1[b] = rescale(acc1[b]),   out0[b] = rescale(acc0[b]) + (c_after mod q_i) in every position of every row
 * i < primes - 1 (a constant polynomial is constant in NTT form), both [B][primes - 1][n], canonical.  `rescale` is exactly
 * the map of se_amd_ct_rescale_device: centred delta of the last row, exact quotient.  The map is defined on arbitrary
 * residue slabs and is BIT-IDENTICAL to se_amd_ct_drop_primes_device of every term to `primes`, the weighted modular sum,
 * se_amd_ct_rescale_device, then the constant added to slab 0 -- without the dropped copies and without the sum in
 * memory.  No scratch, no key, nothing uploaded (the residues of the weights and of the constant travel in the kernel's
 * argument block), one asynchronous launch; outputs must not overlap inputs (not checked).  Every int64 is a valid weight
 * and a valid constant.  CKKS meaning: the scale of the sum is w_t . scale_t, which the caller makes equal across the
 * terms; the rescale divides it by q_{primes-1}; c_after is a constant at the resulting scale.
 * SE_ERR_INVALD_ARGUMENT, with nothing written: a NULL ctx, pointer array, term_primes, w or output; a NULL term pointer; T
 * outside [1, SE_AMD_AFFINE_MAX_TERMS]; primes outside [2, np]; a term_primes[t] outside [primes, np]; a device pointer
 * that is not 16-byte aligned; B at or above 2^31.  B = 0 is a successful no-op. */
#define SE_AMD_AFFINE_MAX_TERMS 16
int se_amd_ct_affine_rescale_device(se_amd_ctx *ctx, const uint32_t *const *d_term0,
                                    const uint32_t *const *d_term1 /* HOST arrays of T device pointers */,
                                    const uint32_t *term_primes /* host [T] */, const int64_t *w /* host [T] */, size_t T,
                                    int64_t c_after, size_t B, size_t primes, uint32_t *d_out0,
                                    uint32_t *d_out1 /* [B][primes-1][n] */, void *stream);
/* Polynomial plans.  se_amd_poly_create (host-only, no device, no context) makes the schedule that evaluates
 * p(x) = sum_d a_d x^d slot-wise on level-`primes` records (L = primes) at scale scale_in; se_amd_ct_poly_sp_device runs it
 * under the installed special-prime relinearisation key (se_amd_set_relin_key_sp).  The schedule:
 * Ladder.  For d >= 2: depth(d) = ceil(log2 d), h(d) = 2^(depth(d) - 1), and x^d = x^h . x^(d-h).  The product is taken at
 * level m = L - depth(d) + 1; x^h lives at exactly that level, the other operand is dropped to it with
 * se_amd_ct_drop_primes_device when it is higher.  The product is a one-pair row of se_amd_ct_dot_sp_device, followed by
 * se_amd_ct_rescale_device.  x^d is then at level L - depth(d) with scale(d) = scale(h) . scale(d-h) / (double)q_{m-1};
 * scale(1) = scale_in.
 * Needed powers.  {d >= 1 : a_d != 0}, closed under d -> h(d), d - h(d).  Nothing else is computed: for an odd polynomial
 * of degree 7, x^6 is not.
 * Combine.  One se_amd_ct_affine_rescale_device call at level l = L - depth(D), D the degree; its terms are the powers with
 * a_d != 0, each read in place at its own level, with
 *     w_d = nearbyint(((a_d . scale_out) . (double)q_{l-1}) / scale(d)),     c_after = nearbyint(a_0 . scale_out),
 * IEEE doubles evaluated in that order, ties to even (Python's round on the same doubles gives the same integers).  The
 * result is at level l - 1, at scale scale_out by construction.
 * se_amd_poly_terms: the needed powers in increasing order -- power, level (primes of the record that holds it), scale(d)
 * and w_d (0 for a power with a_d = 0) -- at most `cap` of them into each array that is not NULL; returns their count.
 * se_amd_poly_result: out_primes = l - 1 and c_after.  se_amd_poly_workspace_bytes: what a call on `records` records needs:
 * the row pointers of the one-pair rows, both slabs of every power above 1 at its level, of one product and of one
 * dropped operand (0 for a plan of degree 1).
 * The call.  The workspace is the caller's, as with se_amd_ct_bsgs_device (device memory, 16-byte aligned); nothing is
 * allocated, nothing synchronises, every launch is on `stream`.  Launches: with K the needed powers above 1 and K' those
 * of them whose lower operand is dropped, 1 (the row pointers) + 2 K (product, rescale) + 1 (combine) kernels and 2 K'
 * pitched copies; a plan of degree 1 is the combine alone.  d_out0, d_out1 are [B][l - 1][n].
 * Range, the caller's: |p(x)| . scale_out . q_{l-1} < Q_l / 2 for the combine's sum, and every power x^d below
 * Q_level(d) / 2 at its scale(d) (its product below Q_m / 2 before the rescale).  Lift fresh records so that
 * scale_in is about q: one se_amd_ct_lincomb_device with the weight round(q_{L-1} / se_amd_scale(ctx)), which keeps every
 * scale(d) near q and every weight near a_d . scale_out.
 * se_amd_poly_create refuses, with SE_ERR_INVALD_ARGUMENT and *out untouched: an unsupported (n, np); degree outside
 * [1, SE_AMD_POLY_MAX_DEGREE]; a_D == 0; a non-finite coefficient or scale; a scale <= 0; primes outside
 * [depth(D) + 2, np - 1]; a |w_d| or |c_after| at or above 2^62; NULL coeff or out.  se_amd_ct_poly_sp_device refuses NULL
 * or misaligned pointers, a context whose (n, np) is not the plan's, B at or above 2^31 and work_bytes below
 * se_amd_poly_workspace_bytes(plan, B); it returns SE_ERR_NO_KEY without a special-prime relinearisation key (a digit key
 * does not serve); B = 0 is a successful no-op.
 * Out of scope: a digit-key form (on the special-prime path 4096 x 3 reaches degree 1 only), Paterson-Stockmeyer, a
 * Chebyshev basis, a ladder step fused with its rescale, multi-device forms. */
typedef struct se_amd_poly se_amd_poly;
#define SE_AMD_POLY_MAX_DEGREE 15
int se_amd_poly_create(size_t n, size_t np, size_t primes, const double *coeff /* host [degree+1], a_0 .. a_D */,
                       size_t degree, double scale_in, double scale_out, se_amd_poly **out);
void se_amd_poly_destroy(se_amd_poly *plan);
size_t se_amd_poly_terms(const se_amd_poly *plan, uint32_t *power, uint32_t *level, double *scale, int64_t *weight,
                         size_t cap);
int se_amd_poly_result(const se_amd_poly *plan, size_t *out_primes, int64_t *c_after);
size_t se_amd_poly_workspace_bytes(const se_amd_poly *plan, size_t records);
int se_amd_ct_poly_sp_device(se_amd_ctx *ctx, const se_amd_poly *plan, const uint32_t *d_c0, const uint32_t *d_c1,
                             size_t B, void *d_work, size_t work_bytes, uint32_t *d_out0, uint32_t *d_out1, void *stream);
/* Host-only: the constants the rescale from level `primes` uses: inv[j] = q_{primes-1}^-1 mod q_j and inv_shoup[j] =
 * floor(inv[j] * 2^32 / q_j) for j < primes - 1 (primes - 1 entries are written).  inv_shoup may be NULL.
 * SE_ERR_INVALD_ARGUMENT for an unsupported (degree, primes) or primes < 2. */
int se_amd_rescale_constants(size_t degree, size_t primes, uint32_t *inv, uint32_t *inv_shoup);
/* Host-only: the recombination constants the full-modulus decrypt uses, for inspection and CPU-side checks:
 * inv[j] = (q_0 ... q_{j-1})^-1 mod q_j and inv_shoup[j] = floor(inv[j] * 2^32 / q_j) for j = 1 .. np-1 (entry 0 is
 * 0).  inv_shoup may be NULL.  SE_ERR_INVALD_ARGUMENT for an unsupported (degree, nprimes). */
int se_amd_crt_constants(size_t degree, size_t nprimes, uint32_t *inv, uint32_t *inv_shoup);
/* prng_fill_buffer (rng.h:78-91): out[i] = SHAKE256(seed[i] || le64(ctr[i]))[0:outlen]. */
int se_amd_prng_blocks_device(se_amd_ctx *ctx, const uint8_t *d_seeds, const uint64_t *d_ctrs,
                              uint8_t *d_out, size_t outlen, size_t count, void *stream);
/* sample_poly_uniform for primes 0..np-1 in chain order (sample.c:39-57): out [B][np][n];
 * d_ctr_in may be NULL (= 0); d_ctr_out optional [B]. */
int se_amd_sample_uniform_device(se_amd_ctx *ctx, const uint8_t *d_seeds, const uint64_t *d_ctr_in,
                                 size_t B, uint32_t *d_out, uint64_t *d_ctr_out, void *stream);
/* sample_small_poly_ternary_prng_96 (sample.c:218-242): one int8 code (0,1,2) per coefficient
 * [B][n] (the 2-bit packing of sample.c:61-87 is applied by se_amd_pack_ternary_host). */
int se_amd_sample_ternary_device(se_amd_ctx *ctx, const uint8_t *d_seeds, size_t B, int8_t *d_codes,
                                 uint64_t *d_ctr_out, void *stream);
/* sample_poly_cbd_generic_prng_16 (sample.c:311-321): int8 [B][blocks*16], block k of ciphertext
 * b uses counter ctr_base[b] + k (ctr_base NULL = 0). */
int se_amd_sample_cbd_device(se_amd_ctx *ctx, const uint8_t *d_seeds, const uint64_t *d_ctr_base,
                             size_t B, size_t blocks_per_ct, int8_t *d_out, void *stream);
void se_amd_pack_ternary_host(const int8_t *codes, size_t n, uint8_t *packed /*[n/4]*/);
/* Known-answer access to the device word arithmetic the kernels are built from (modulo.h:21-116,
 * uintmodarith.h:26-346 as restated in kernels/modarith.cuh), element-wise for prime j:
 * op 0 barrett 32->32 (a), 1 barrett 64->32 (a), 2 mul_mod(a, b) by 64-bit Barrett, 3 mul_mod(a, b) by
 * the Shoup form, 4 add_mod, 5 neg_mod(a), 6 sub_mod, 7 signed reduction of (int64)a
 * (ckks_common.c:224-237), 8 canonicalisation of a < 4q, 9/10 the two outputs of the Harvey NTT
 * butterfly on (a, b) with root c (ntt.c:156-162), 11/12 of the Gentleman-Sande butterfly
 * (intt.c:188-195).  Operands are uint64 arrays (b, c may be NULL where unused). */
int se_amd_word_ops_device(se_amd_ctx *ctx, size_t prime, int op, const uint64_t *d_a, const uint64_t *d_b,
                           const uint64_t *d_c, uint32_t *d_out, size_t count, void *stream);

/* ---- formats on either side of the path (host only) ---------------------------------------- */
/* SEAL Ciphertext data of size 2 (adapter/fileops.cpp:515-527): out[i + j*n] = c0 prime j,
 * out[i + j*n + np*n] = c1 prime j, one uint64 per coefficient; out has 2*np*n entries. */
void se_amd_pack_seal_ciphertext_host(const uint32_t *c0, const uint32_t *c1, size_t n, size_t np,
                                      uint64_t *out);
/* print_poly_full / print_poly_flpt_full text lines (util_print.h:229-245,491-508):
 * "name : { v0, v1, ... }\n".  Return the length needed (excluding the NUL); write at most cap. */
size_t se_amd_format_poly_text(const char *name, const uint32_t *poly, size_t n, char *buf, size_t cap);
size_t se_amd_format_values_text(const char *name, const float *v, size_t len, char *buf, size_t cap);
/* One ciphertext as the adapter's verify path reads it (api_tests.c:30-42,75-90): optional
 * "v (cleartext)" line, then "c0" and "c1" lines per prime. */
int se_amd_write_ciphertext_text(const char *path, int append, const float *values, size_t vlen,
                                 const uint32_t *c0, const uint32_t *c1, size_t n, size_t np);
/* key files in the device-side formats (fileops.c:140-204) */
int se_amd_save_secret_key_file(const char *dir, size_t n, const uint8_t *sk_packed);
int se_amd_save_public_key_files(const char *dir, size_t n, size_t np, const uint32_t *q,
                                 const uint32_t *pk0, const uint32_t *pk1);

/* ---- profiling hooks ---------------------------------------------------------------------- */
/* When enabled, every kernel launched by the whole-path entries is bracketed by HIP events on the
 * caller's stream; after a stream sync se_amd_stage_ms returns the accumulated milliseconds and
 * launch counts per stage since the last reset. */
enum
{
    SE_AMD_STAGE_CBD = 0,
    SE_AMD_STAGE_UNIFORM = 1,
    SE_AMD_STAGE_TERNARY = 2,
    SE_AMD_STAGE_ENCODE_ENCRYPT = 3, /* fused kernel (asymmetric, encode-only, unsplit symmetric) */
    SE_AMD_STAGE_ENCODE_RNS = 4,     /* split symmetric path: encode -> RNS residues */
    SE_AMD_STAGE_NTT_FUSE = 5,       /* split symmetric path: per-prime NTT + ciphertext arithmetic */
    SE_AMD_STAGE_COUNT = 6
};
int se_amd_set_profiling(se_amd_ctx *ctx, int enabled);
int se_amd_stage_ms(se_amd_ctx *ctx, float *ms /*[SE_AMD_STAGE_COUNT]*/,
                    uint64_t *launches /*[SE_AMD_STAGE_COUNT]*/, int reset);
/* test hook: capacity of the per-ciphertext rejection list of the uniform sampler (default 256);
 * tiny values force the overflow path. */
/* Host-only (no device needed): the setup-time tables the context uploads, for inspection and for
 * CPU-side checks.  Any output pointer may be NULL.  q[np]; const_ratio[np][2] = floor(2^64/q) as
 * {lo, hi} (modulus.c:30-47); index_map[n] (ckks_common.c:32-68); ifft_w[n][2] = (cos, -sin) of
 * 2*pi*bitrev(t)/2n from the host libm (fft.c:39-45); ntt_rw / intt_rw [np][n][2] = (root,
 * floor(root*2^32/q)) with root[bitrev(i)] = psi^i resp. psi^-i (ntt.c:40-52, intt.c:26-58).
 * Returns SE_SUCCESS or SE_ERR_INVALD_ARGUMENT for an unsupported (degree, nprimes). */
int se_amd_host_tables(size_t degree, size_t nprimes, uint32_t *q, uint32_t *const_ratio,
                       double *scale, uint16_t *index_map, double *ifft_w, uint32_t *ntt_rw,
                       uint32_t *intt_rw);
/* SHA-256 (64 hex digits + NUL) of the IFFT root table this context's kernels read, copied back from the device:
 * W[t] = (cos, -sin) of 2*pi*bitrev(t)/2n for t = 0 .. n-1 as little-endian doubles -- the digest SURVEY.md 8(c)
 * trap T8 lists per n (fft.c:39-45: the roots are the HOST libm's; goldens generated on another libm may differ
 * in rare last-bit cases).  Start-up check on the box that runs the kernels (__graft_entry__.smoke()). */
int se_amd_ifft_table_sha256(se_amd_ctx *ctx, char out_hex[65]);
int se_amd_set_reject_list_capacity(se_amd_ctx *ctx, uint32_t cap);
/* test hook: redraw candidates the helper waves precompute per ciphertext (default n/32); tiny
 * values force the pooled fallback for the remaining draws. */
int se_amd_set_speculation_capacity(se_amd_ctx *ctx, uint32_t cap);
/* test hook: ciphertexts per chunk of the host-pointer pipeline (0 = automatic: up to 16384, at most
 * 4 GiB of output per chunk). */
int se_amd_set_host_chunk(se_amd_ctx *ctx, size_t ciphertexts);
/* Pre-allocate the internal scratch for batches of up to B plaintexts (keeps hipMalloc out of
 * the first timed call). */
int se_amd_reserve(se_amd_ctx *ctx, size_t B);
/* Test / A/B hook: which FORM of the samplers and pipelines a call takes.  Every bit only selects among bit-identical
 * forms (the timing ablations of rounds 1-5 that produced WRONG outputs -- bits 1, 2, 4 -- are gone: no setting of this
 * word changes a result):
 *   8 no helper waves, 16 helper waves without speculation, 32 / 64 force the lane / wave form of the chain kernels,
 *   128 early encoder at n = 16384, 256 speculation windows of one guess (forces the miss path), 512 / 1024 force /
 *   forbid the pair-form staged sampler, 4096 ternary window of blocks + 2 counters (forces the fallback), 8192 the
 *   fused n = 4096 symmetric / encode-only kernels keep the one-plane pair form instead of the two-way pair form.
 * The environment overrides SE_AMD_STAGED, SE_AMD_SPECULATION are read at context creation into
 * members of their own and survive this call. */
int se_amd_set_debug_flags(se_amd_ctx *ctx, uint32_t flags);
/* pipeline shape of the symmetric path (A/B experiments): overlap = use the auxiliary stream,
 * split = 0 fused kernel, 1 per-prime software pipeline, 2 choose per call (default 1, 2). */
int se_amd_set_pipeline(se_amd_ctx *ctx, int overlap, int split);
/* pipeline shape of the public-key path (A/B experiments): chunks the batch is cut into so that the CBD
 * sampler of chunk k+1 runs beside the fused kernel of chunk k (default 1 = serial, or
 * $SE_AMD_ASYM_CHUNKS; batches below 4096 ciphertexts per chunk always run serially). */
int se_amd_set_asym_chunks(se_amd_ctx *ctx, size_t chunks);
const char *se_amd_last_error(void);
const char *se_amd_version(void);

#ifdef __cplusplus
}
#endif

/* ---- layer 1b: the reference's lower surface under its own names (ckks_encode_base, ckks_setup,
 *      ckks_sym_init, ckks_encode_encrypt_sym, gen_pk, ntt_inpl, ifft_inpl, ...) ---------------- */
#include "seal_embedded_amd_lower.h"

#endif /* SEAL_EMBEDDED_AMD_H */
