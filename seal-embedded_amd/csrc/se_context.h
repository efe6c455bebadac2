// se_context.h -- internal: the per-parameter-set GPU context behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "kernels/kernel_args.h"
#include "se_devmem.h"
#include "se_host_tables.h"
#include "se_types.h"

namespace seamd {

// error codes of include/seal_embedded_amd.h (kept numerically identical; checked in se_api.cpp)
constexpr int kErrInvalid  = -22;    // SE_ERR_INVALD_ARGUMENT
constexpr int kErrNoDevice = -19;    // SE_ERR_NO_DEVICE
constexpr int kErrHip      = -1001;  // SE_ERR_HIP
constexpr int kErrNoKey    = -1002;  // SE_ERR_NO_KEY

constexpr int kStageCount = 6;  // cbd, uniform, ternary, encode_encrypt (fused), encode_rns, ntt_fuse

struct HostPipe;
struct Context;

// A linear transform y = d0 . x + sum_e d_e . rot_e(x) made ready (se_amd_lintrans_create): per entry the installed Galois
// key block with the diagonal folded in, and the diagonals themselves as (word, Shoup) rows for the c0 term.  A snapshot:
// nothing of it refers to the context's installed keys afterwards.  Freed with the device of `owner` current.
struct LintransPlan
{
    const Context *owner = nullptr;   // compared, never dereferenced
    int device           = 0;
    size_t levels        = 0;       // min(pt_primes, np), np - 1 of a special-prime plan: the calls it serves have
                                    // primes <= levels
    bool sp              = false;   // made from the special-prime keys (se_amd_lintrans_create_sp): R = np - 1 rows
    bool diag0           = false;
    std::vector<uint32_t> elts;
    std::vector<DevBuf<uint32_t>> keys;   // per entry [2][R][np][2][n], R = 2 np or np - 1 (sp)
    DevBuf<uint32_t> diag;                // [G + 1][np][2][n]; the last one is d0 (unused without diag0)
};

// A baby-step / giant-step linear transform made ready (se_amd_bsgs_create): the diagonals alone, pre-rotated by the
// inverse of their giant step, in the layout k_ct_mul_plain_sum reads.  It holds no key material: the Galois keys are
// looked up in the context at call time.  Element 1, where listed, stands FIRST in `baby` (the modular sum does not
// depend on the order), so the keyed baby steps are one contiguous stack for the many form.
struct BsgsPlan
{
    const Context *owner = nullptr;   // compared, never dereferenced
    int device           = 0;
    size_t n             = 0;
    size_t levels        = 0;       // min(pt_primes, np): the calls it serves have primes <= levels
    size_t pt_primes     = 0;
    bool sp              = false;   // made by se_amd_bsgs_create_sp: pt_primes = np, levels = np - 1, served by ct_bsgs_sp
    std::vector<uint32_t> baby, giant;   // baby: element 1 first where listed
    DevBuf<uint32_t> diag;               // [n2][n1][pt_primes][n], row (g, b) permuted by giant[g]^-1
};

// One installed family of evaluation keys (public material): digit keys (R = 2 np rows; se_amd_set_relin_key,
// se_amd_set_galois_keys) or special-prime keys (R = np - 1; the _sp setters).  Every key is one device block
// [2][R][np][2][n] made by build_evk (layout: kernels/kernel_args.h).
struct EvalKeys
{
    DevBuf<uint32_t> relin;                 // the relinearisation key; empty = none installed
    std::vector<uint32_t> elts;             // the installed Galois elements
    std::vector<DevBuf<uint32_t>> galois;   // one block per element of elts
    const uint32_t *find(uint32_t elt) const;   // the block of elt, or nullptr
};

struct StageEvent
{
    int stage;
    Event start, stop;
};

struct Context
{
    HostParams hp;
    DevParams dp;
    CrtParams crt;   // recombination constants of decrypt_full
    DevTables dt{};
    int device = 0;
    std::vector<uint16_t> index_map;  // host copy (SE_PTRS::index_map_ptr, tests)

    // read-only device slabs (NTT(s) is secret)
    DevBuf<uint16_t> d_inv_map, d_map, d_gather;
    DevBuf<double> d_ifft_w;
    DevBuf<uint32_t> d_ntt_rw, d_intt_rw, d_pk0, d_pk1;
    DevBuf<uint32_t> d_s_hat{Secret::yes};
    bool have_sk = false, have_pk = false;
    // key rings of the keyed entries (se_amd_set_{secret,public}_keyring): K keys, each in the layout of the
    // installed key ([np][n][2] (value, Shoup)), back to back; independent of d_s_hat / d_pk0 / d_pk1
    DevBuf<uint32_t> d_ring_sk{Secret::yes};   // [K][np][n][2] NTT(s) pairs
    DevBuf<uint32_t> d_ring_pk0, d_ring_pk1;   // [K][np][n][2]
    size_t ring_sk = 0, ring_pk = 0;           // keys in each ring (0 = no ring)
    EvalKeys evk[2];                           // the installed evaluation keys: [0] digit, [1] special-prime (index: sp)
    // the switch-key ring (se_amd_set_switch_keyring_sp): K special-prime key blocks [2][np - 1][np][2][n] back to back,
    // an installed set of its own (public material); record b of a switch call uses block key_idx[b]
    DevBuf<uint32_t> d_switch_ring;
    size_t switch_keys = 0;                    // keys in the ring (0 = no ring)
    DevBuf<uint32_t> d_kidx;                   // [cap] key index of each record, clamped below K (keyed calls)
    DevBuf<uint32_t> d_kbad;                   // [1 + cap] count + records whose index was out of range

    // scratch, grown on demand (ensure_scratch): `cap` ciphertexts, `rows` >= cap rows of the reject lists and
    // candidates (the virtual ciphertexts of the small-batch path need only these)
    DevBuf<int8_t> d_err{Secret::yes};     // [cap][2n]
    DevBuf<int8_t> d_ucodes{Secret::yes};  // [cap][n]
    DevBuf<uint64_t> d_ctr;                // [cap]
    DevBuf<uint32_t> d_rej;                // [rows][rej_cap]
    DevBuf<uint32_t> d_spec;               // [rows][spec_cap] speculative redraw candidates (helper waves)
    uint32_t spec_cap  = 128;
    DevBuf<uint32_t> d_a{Secret::yes};     // [B][np][n]: `a` when the caller does not want c1 back
    // small-batch prime speculation (encrypt_sym_small): virtual-ciphertext scratch and streams
    DevBuf<uint8_t> d_sp_seeds{Secret::yes};  // [total][64]
    DevBuf<uint64_t> d_sp_ctr;                // [total] guessed start counters
    DevBuf<uint64_t> d_sp_ctrout;             // [total] end counters under each guess
    DevBuf<uint32_t> d_sp_rows{Secret::yes};  // [total][n] a_j under each guess (the same data as d_a)
    DevBuf<uint8_t> d_sp_prime;               // [total] prime of each virtual ciphertext
    DevBuf<uint32_t> d_sp_fail;               // [1024] 0 = chain resolved, j = window of prime j missed
    uint32_t small_limit = getenv("SE_AMD_SMALL_LIMIT") ? (uint32_t)atoi(getenv("SE_AMD_SMALL_LIMIT")) : 65536;  // virtual ciphertexts a small call may fan out to
    // ... and the bytes their output rows may take (one n-word row per virtual ciphertext)
    size_t small_bytes = getenv("SE_AMD_SMALL_BYTES") ? (size_t)atoll(getenv("SE_AMD_SMALL_BYTES")) : ((size_t)1 << 30);
    Stream spec_stream;   // the guesses of ALL primes run as one launch on it
    // staged sampler (k_bulk_pair / k_candidates / k_resolve_wave): candidates on a stream of their own
    Stream cand_stream;
    Event ev_cand[kMaxPrimes];
    DevBuf<uint32_t> d_nrej;      // [cap] rejected coefficients of the current polynomial
    DevBuf<uint32_t> d_flagged;   // [1 + cap] staged forms: ciphertexts k_resolve_light left to k_resolve_wave
    DevBuf<uint8_t> d_compact;    // [cap] k_encode_rns -> k_ntt_fuse: plaintext b travels as one int32 row
    DevBuf<uint32_t> d_general;   // [1 + B] plaintexts the fast fused kernel declined (count, indices)
    uint32_t rej_cap   = 256;
    // ct_lincomb with a split row: canonical partial rows and the slices' invalid-entry flags (not secret: sums of
    // ciphertext residues), grown on demand (ensure_lincomb)
    DevBuf<uint32_t> d_lc_part;   // [slabs][G S][np][n]
    DevBuf<uint8_t> d_lc_flag;    // [G S]
    uint32_t lincomb_split = 0;   // test hook (se_amd_set_lincomb_split): slices per output row, 0 = lincomb_slices
    uint32_t debug_flags = 0;  // form selection of the samplers, pipelines and fused kernels (tests/tools only)

    // second stream: the CBD error sampler runs beside the uniform sampler (different seeds, no
    // data dependency); joined before the fused encode+encrypt kernel.
    Stream aux_stream;
    Event ev_fork, ev_join, ev_cbd, ev_enc;
    Event ev_prime[kMaxPrimes];
    // One set of scratch per context: successive calls are ordered on it.  Host threads serialise on
    // `mu`; a call waits (on its own stream) for `ev_done` of the previous call, whatever stream
    // that one ran on, before it touches the scratch or forks the auxiliary streams.
    std::mutex mu;
    Event ev_done;
    bool have_done     = false;
    int num_cus        = 256;
    // public-key path: chunks the batch is cut into so that the CBD sampler of chunk k+1 runs beside the
    // fused kernel of chunk k (se_context.cpp, encrypt_asym_impl); 1 = serial
    size_t asym_chunks = getenv("SE_AMD_ASYM_CHUNKS") ? (size_t)atoi(getenv("SE_AMD_ASYM_CHUNKS")) : 1;
    int spec_mode = -1;    // prime speculation of small symmetric calls: -1 = estimate per call, 0 never, 1 whenever planned
    int staged_mode = -1;  // pair-form staged sampler of the per-prime pipeline: -1 = by batch size, 0 never, 1 always (SE_AMD_STAGED)
    bool overlap = true;   // run independent kernels on the auxiliary stream
    int split_mode = 2;    // symmetric path: 0 = fused kernel, 1 = per-prime software pipeline
                           // (encode_rns + uniform_j || ntt_fuse_{j-1}), 2 = choose per call: the split
                           // form wins whenever the uniform sampler's chains leave SIMDs empty (fewer
                           // than 4 chain waves per CU) or the fused kernel spills (n >= 8192);
                           // at n = 4096, B = 65536 both measure the same and fused moves less data

    // host-pointer entry points: chunked PCIe pipeline (se_hostpipe.h), created on first use
    std::unique_ptr<HostPipe> host_pipe;

    // profiling
    bool profiling = false;
    std::vector<StageEvent> events;
    float stage_ms[kStageCount]          = {};
    uint64_t stage_launches[kStageCount] = {};

    ~Context();
    int init(size_t n, size_t nprimes, int device);
    int ensure_scratch(size_t B, size_t rows = 0);
    int ensure_general(size_t B);
    int ensure_keyed(size_t B);
    int begin_call(hipStream_t st);
    int end_call(hipStream_t st, int rc);
    // UniformArgs with what the context owns set: reject lists, candidate rows, their capacities, debug_flags
    UniformArgs uniform_args() const;
    // u codes (0/1/2 per coefficient) and e1 of ciphertext 0 of the last asymmetric call (host out)
    int fetch_asym_randomness(int8_t *ucodes, int8_t *e1);
    int set_secret_key(const uint8_t *sk_packed);
    int set_secret_key_impl(const uint8_t *sk_packed);   // caller holds `mu`
    int set_public_key(const uint32_t *pk0, const uint32_t *pk1);
    // key rings (host pointers, the layouts gen_keys_batch writes); replace the ring of that kind
    int set_secret_keyring(size_t K, const uint8_t *sk_packed);
    int set_public_keyring(size_t K, const uint32_t *pk0, const uint32_t *pk1);
    int gen_public_key(const uint8_t *sk_packed, const uint8_t *pk_seed, const uint8_t *ep_seed,
                       uint32_t *pk0_out, uint32_t *pk1_out);
    // K key pairs in one launch chain (host pointers); does not touch the context's installed keys
    int gen_keys_batch(size_t K, const uint8_t *sk_in, const uint8_t *sk_seeds, const uint8_t *pk_seeds,
                       const uint8_t *ep_seeds, uint8_t *sk_out, uint32_t *pk0_out, uint32_t *pk1_out);

    // public entries: serialised on the context's scratch (begin_call / end_call around *_impl)
    int encrypt_sym(const float *d_values, size_t B, const uint8_t *d_share_seeds,
                    const uint8_t *d_seeds, uint32_t *d_c0, uint32_t *d_c1, uint32_t *d_ntt_pte,
                    int64_t *d_pte, uint8_t *d_status, hipStream_t st);
    int encrypt_sym_seeded(const float *d_values, size_t B, const uint8_t *d_share_seeds,
                           const uint8_t *d_seeds, uint32_t *d_c0, uint8_t *d_status, hipStream_t st);
    int encrypt_asym(const float *d_values, size_t B, const uint8_t *d_seeds, uint32_t *d_c0,
                     uint32_t *d_c1, uint32_t *d_ntt_pte, int64_t *d_pte, uint8_t *d_status,
                     hipStream_t st);
    int encode_ntt(const float *d_values, size_t B, uint32_t *d_out, int64_t *d_pte,
                   uint8_t *d_status, hipStream_t st);
    // keyed entries: record b under ring key d_key_idx[b] (status 2 and zero c0 / c1 for an index >= K)
    int encrypt_sym_keyed(const float *d_values, size_t B, const uint32_t *d_key_idx, const uint8_t *d_share_seeds,
                          const uint8_t *d_seeds, uint32_t *d_c0, uint32_t *d_c1, uint32_t *d_ntt_pte,
                          int64_t *d_pte, uint8_t *d_status, hipStream_t st);
    int encrypt_asym_keyed(const float *d_values, size_t B, const uint32_t *d_key_idx, const uint8_t *d_seeds,
                           uint32_t *d_c0, uint32_t *d_c1, uint32_t *d_ntt_pte, int64_t *d_pte, uint8_t *d_status,
                           hipStream_t st);
    int decrypt_decode_keyed(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, const uint32_t *d_key_idx,
                             size_t prime, uint32_t *d_dec_ntt, uint32_t *d_pt, float *d_values, hipStream_t st);
    // full-modulus decrypt: all primes recombined (kernels/kernel_args.h, FullArgs); keyed: status 2 and zero
    // outputs for an index >= K
    int decrypt_full(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, int64_t *d_pte, float *d_values,
                     double *d_values_f64, uint8_t *d_status, hipStream_t st);
    int decrypt_full_keyed(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, const uint32_t *d_key_idx,
                           int64_t *d_pte, float *d_values, double *d_values_f64, uint8_t *d_status, hipStream_t st);
    // the same on records of `primes` <= np primes, decoded with the caller's scale (the parameter set (n, primes) is
    // a prefix of this one: same kernels, a DevParams copy with nprimes and scale replaced)
    int decrypt_level(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, double scale, int64_t *d_pte,
                      float *d_values, double *d_values_f64, uint8_t *d_status, hipStream_t st);
    int decrypt_level_keyed(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, double scale,
                            const uint32_t *d_key_idx, int64_t *d_pte, float *d_values, double *d_values_f64,
                            uint8_t *d_status, hipStream_t st);
    // degree-2 twins of the level entries: d = c0 + s (c1 + s c2) per prime, the rest unchanged
    int decrypt3_level(const uint32_t *d_c0, const uint32_t *d_c1, const uint32_t *d_c2, size_t B, size_t primes,
                       double scale, int64_t *d_pte, float *d_values, double *d_values_f64, uint8_t *d_status,
                       hipStream_t st);
    int decrypt3_level_keyed(const uint32_t *d_c0, const uint32_t *d_c1, const uint32_t *d_c2, size_t B, size_t primes,
                             double scale, const uint32_t *d_key_idx, int64_t *d_pte, float *d_values,
                             double *d_values_f64, uint8_t *d_status, hipStream_t st);
    // ciphertext products: the key-free tensor (MulArgs), the relinearisation key (host pointers) and the
    // relinearisation itself (RelinArgs); one launch each, no scratch
    int ct_mul(const uint32_t *d_a0, const uint32_t *d_a1, size_t Ba, const uint32_t *d_b0, const uint32_t *d_b1,
               size_t Bb, size_t primes, size_t P, const uint32_t *d_ia, const uint32_t *d_ib, uint32_t *d_out0,
               uint32_t *d_out1, uint32_t *d_out2, uint8_t *d_status, hipStream_t st);
    // the tensor summed over CSR rows of pairs (MulSumArgs): key-free to three slabs, or (dot) with the special-prime
    // relinearisation of every row's T2 inside the same launch, to two; one launch, no scratch
    int ct_mul_sum(const uint32_t *d_a0, const uint32_t *d_a1, size_t Ba, const uint32_t *d_b0, const uint32_t *d_b1,
                   size_t Bb, size_t primes, size_t G, const uint32_t *d_row_ptr, const uint32_t *d_ia,
                   const uint32_t *d_ib, size_t nnz, bool dot, uint32_t *d_out0, uint32_t *d_out1, uint32_t *d_out2,
                   uint8_t *d_status, hipStream_t st);
    // sp (here and on the Galois keys): the special-prime key of R' = np - 1 rows instead of the digit key of 2 np
    int gen_relin_key(const uint8_t *sk_packed, const uint8_t *a_seeds, const uint8_t *e_seeds, uint32_t *evk0_out,
                      uint32_t *evk1_out, bool sp = false);
    int set_relin_key(const uint32_t *evk0, const uint32_t *evk1, bool sp = false);
    int ct_relin(const uint32_t *d_d0, const uint32_t *d_d1, const uint32_t *d_d2, size_t B, size_t primes,
                 uint32_t *d_out0, uint32_t *d_out1, hipStream_t st);
    // slot rotations: Galois keys of G elements (host pointers, [G][R][np][n] per half) and the automorphism fused
    // with its key switch (GaloisArgs); one launch, no scratch
    int gen_galois_keys(const uint8_t *sk_packed, const uint32_t *elts, size_t G, const uint8_t *a_seeds,
                        const uint8_t *e_seeds, uint32_t *gk0_out, uint32_t *gk1_out, bool sp = false);
    int set_galois_keys(const uint32_t *elts, size_t G, const uint32_t *gk0, const uint32_t *gk1, bool sp = false);
    int ct_galois(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, uint32_t elt, uint32_t *d_out0,
                  uint32_t *d_out1, hipStream_t st);
    // special-prime key switch (KeySwitchSpArgs) on level-`primes` records, primes <= np - 1: the relinearisation of
    // (a0, a1, sw) = (d0, d1, d2) with elt 0, else the rotation of (a0, sw) = (c0, c1) by elt (a1 unused); one launch, no
    // scratch.  ct_drop_primes: rows 0 .. primes_out-1 of every record of one or two slabs, a pitched device copy
    int ct_key_switch_sp(const uint32_t *d_a0, const uint32_t *d_a1, const uint32_t *d_sw, size_t B, size_t primes,
                         uint32_t elt, uint32_t *d_out0, uint32_t *d_out1, hipStream_t st);
    int ct_drop_primes(const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t primes_in, size_t primes_out,
                       uint32_t *d_out0, uint32_t *d_out1, hipStream_t st);
    // switch-key ring: K special-prime keys that hide P . s_from_k under s_to (host pointers, [K][np - 1][np][n] per
    // half; the generator needs both secrets and installs nothing), the ring built beside the installed one, and the
    // switch of record b under ring key key_idx[b] (SwitchSpArgs): one record per output row, or with d_row_ptr the CSR
    // rows summed with one division by P per row; one launch, no scratch, no sanitising pass
    int gen_switch_keys(size_t K, const uint8_t *sk_from, const uint8_t *sk_to, const uint8_t *a_seeds,
                        const uint8_t *e_seeds, uint32_t *wk0_out, uint32_t *wk1_out);
    int set_switch_keyring(size_t K, const uint32_t *wk0, const uint32_t *wk1);
    int ct_switch_keyed_sp(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                           const uint32_t *d_key_idx, bool sum, size_t G, const uint32_t *d_row_ptr,
                           const uint32_t *d_idx, size_t nnz, uint32_t *d_out0, uint32_t *d_out1, uint8_t *d_status,
                           hipStream_t st);
    // slot packing (PackSpArgs): entry k = (record d_idx[k], element elts[d_eidx[k]]) rotated under the installed
    // special-prime Galois key of its element (element 1: the identity, no key) and the CSR rows summed with one
    // division by P per row; d_row_ptr = d_idx = NULL: row g is the entry (g, elts[d_eidx[g]]), G = B = nnz; elts is a
    // host pointer; one launch, no scratch
    int ct_pack_sp(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, const uint32_t *elts, size_t E,
                   size_t G, const uint32_t *d_row_ptr, const uint32_t *d_idx, const uint32_t *d_eidx, size_t nnz,
                   uint32_t *d_out0, uint32_t *d_out1, uint8_t *d_status, hipStream_t st);
    // hoisted rotations (GaloisHoistArgs): G rotations of every record from one digit decomposition, each to its own
    // output (sum false: outputs [G][B][primes][n]) or summed into one record, with the record itself when add_input
    // (sum true: outputs [B][primes][n]); elts is a host pointer; one launch, no scratch
    // sp (the sum form only; HoistSpArgs): on the special-prime Galois keys, one decomposition and one division by P
    // whatever G is
    int ct_galois_hoist(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, const uint32_t *elts,
                        size_t G, bool sum, bool add_input, uint32_t *d_out0, uint32_t *d_out1, hipStream_t st,
                        bool sp = false);
    // linear transforms (LintransArgs): the plan folds device diagonals [G][pt_primes][n] (+ d_diag0 [pt_primes][n] or
    // NULL) into the installed Galois keys of elts (host) and synchronises; a call is one launch, no scratch
    // sp: on the special-prime keys (pt_primes = np, levels 1 .. np - 1; HoistSpArgs); a plan serves the calls of its kind
    int lintrans_create(const uint32_t *elts, size_t G, const uint32_t *d_diag, const uint32_t *d_diag0,
                        size_t pt_primes, LintransPlan &plan, bool sp = false);
    int ct_lintrans(const LintransPlan *plan, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                    uint32_t *d_out0, uint32_t *d_out1, hipStream_t st, bool sp = false);
    // baby-step / giant-step linear transforms: the weighted sum over a stack (MulPlainSumArgs, key-free), the rotate-and-
    // accumulate of G different records (GaloisSetArgs, elts a host pointer, element 1 needs no key), one launch each;
    // the plan (device diagonals [n2][n1][pt_primes][n], host element lists; synchronises) and its call, which walks the
    // batch in chunks of what the caller's workspace holds: copies, the many form, the two steps above, all on `st`.
    // sp on the two steps: the forms ct_bsgs_sp chains -- the sum on stacks of extended records (primes + 1 rows, the
    // last one modulo the special prime; pt_primes is not read, the plaintexts have all np rows), the accumulate on the
    // special-prime keys with one division by P
    int ct_mul_plain_sum(const uint32_t *d_in0, const uint32_t *d_in1, size_t E, size_t B, size_t primes,
                         const uint32_t *d_pt, size_t Gout, size_t pt_primes, uint32_t *d_out0, uint32_t *d_out1,
                         hipStream_t st, bool sp = false);
    int ct_galois_accum(const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t primes, const uint32_t *elts,
                        size_t G, uint32_t *d_out0, uint32_t *d_out1, hipStream_t st, bool sp = false);
    int bsgs_create(const uint32_t *baby, size_t n1, const uint32_t *giant, size_t n2, const uint32_t *d_diag,
                    size_t pt_primes, BsgsPlan &plan, bool sp = false);
    int ct_bsgs(const BsgsPlan *plan, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                uint32_t *d_out0, uint32_t *d_out1, void *d_workspace, size_t workspace_bytes, hipStream_t st);
    // the same on the special-prime keys with the division by P deferred: the baby steps as extended records and the
    // division, one launch each and useful on their own beside the two sp steps above, and the call that chains the four
    // in the caller's workspace
    int ct_galois_many_ext_sp(const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes, const uint32_t *elts,
                              size_t G, uint32_t *d_out0, uint32_t *d_out1, hipStream_t st);
    int ct_mod_down_sp(const uint32_t *d_in0, const uint32_t *d_in1, size_t count, size_t primes, uint32_t *d_out0,
                       uint32_t *d_out1, hipStream_t st);
    int ct_bsgs_sp(const BsgsPlan *plan, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, size_t primes,
                   uint32_t *d_out0, uint32_t *d_out1, void *d_workspace, size_t workspace_bytes, hipStream_t st);
    // workspace bytes of one record of a plan's call, the only place they are computed: two halves each of the digit
    // plan's rot [n1] and inner [n2] of `primes` rows; sp: of U [n1] and V [n2] of primes + 1 rows and W [n2] of `primes`
    static size_t bsgs_record_bytes(bool sp, size_t n1, size_t n2, size_t primes, size_t n)
    {
        return 2 * ((n1 + n2) * (primes + sp) + sp * n2 * primes) * n * sizeof(uint32_t);
    }
    // key-free rescale (RescaleArgs) and slot-wise plaintext product (MulPlainArgs): one launch each, no scratch
    int ct_rescale(const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t primes, uint32_t *d_out0,
                   uint32_t *d_out1, hipStream_t st);
    int ct_mul_plain(const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t primes, const uint32_t *d_pt,
                     size_t P, size_t pt_primes, const uint32_t *d_pt_idx, uint32_t *d_out0, uint32_t *d_out1,
                     uint8_t *d_status, hipStream_t st);
    // slot-wise polynomials.  ct_affine_rescale (AffineRescaleArgs): the weighted sum of T term records at their own
    // levels, one rescale and a constant; host arrays of device pointers, levels and int64 weights; key-free, one launch, no
    // scratch.  ct_poly_sp: the schedule of a PolyPlan in the caller's workspace under the installed special-prime
    // relinearisation key -- the row pointers, then per power above 1 the drop (where the operand is higher), the one-pair
    // product rows and the rescale, then the combine; every launch on `st`, nothing allocated
    int ct_affine_rescale(const uint32_t *const *d_term0, const uint32_t *const *d_term1, const uint32_t *term_primes,
                          const int64_t *w, size_t T, int64_t c_after, size_t B, size_t primes, uint32_t *d_out0,
                          uint32_t *d_out1, hipStream_t st);
    int ct_poly_sp(const PolyPlan *plan, const uint32_t *d_c0, const uint32_t *d_c1, size_t B, void *d_work,
                   size_t work_bytes, uint32_t *d_out0, uint32_t *d_out1, hipStream_t st);
    // key-free weighted sums of records (kernels/kernel_args.h, LincombArgs)
    int ct_lincomb(const uint32_t *d_in0, const uint32_t *d_in1, size_t B, size_t G, const uint32_t *d_row_ptr,
                   const uint32_t *d_idx, const int32_t *d_w, size_t nnz, uint32_t *d_out0, uint32_t *d_out1,
                   uint8_t *d_status, hipStream_t st);
    uint32_t lincomb_slices(size_t G, size_t nnz, size_t slabs) const;
    int ensure_lincomb(size_t part_words, size_t flags);
    // sanitising pass of a keyed call (d_kidx / d_kbad from the caller's indices); the caller holds `mu`
    int key_prologue(const uint32_t *d_key_idx, size_t K, size_t B, hipStream_t st);
    int sample_uniform(const uint8_t *d_seeds, const uint64_t *d_ctr_in, size_t B, uint32_t *d_out,
                       uint64_t *d_ctr_out, hipStream_t st);
    // ring != NULL: the keyed kernels, record b under key ring->idx[b] (keyed entries above)
    int encrypt_sym_impl(const float *d_values, size_t B, const uint8_t *d_share_seeds,
                         const uint8_t *d_seeds, uint32_t *d_c0, uint32_t *d_c1, uint32_t *d_ntt_pte,
                         int64_t *d_pte, uint8_t *d_status, hipStream_t st, const KeyRing *ring = nullptr);
    int encrypt_asym_impl(const float *d_values, size_t B, const uint8_t *d_seeds, uint32_t *d_c0,
                          uint32_t *d_c1, uint32_t *d_ntt_pte, int64_t *d_pte, uint8_t *d_status,
                          hipStream_t st, const KeyRing *ring = nullptr);
    // Small batches (a handful of ciphertexts): all primes' uniform samplers at once under guessed
    // start counters (kernels/samplers.hip, k_spec_*).  small_batch_plan says whether a batch
    // qualifies (encrypt_sym dispatches on it).  A counter outside its window (~1e-7 per prime) is
    // redone on the device by the masked per-prime chain that follows the selection.
    bool small_batch_plan(size_t B, SpecPlan &plan, bool keyed = false) const;
    // speculation or the plain per-prime chain for this batch (estimated chain latencies of both)
    bool speculation_pays(size_t B, const SpecPlan &plan) const;
    // (the argument blocks are encrypt_sym_impl's: error sampler, encode kernels, sampler of `a` without its primes)
    int encrypt_sym_small(const SpecPlan &plan, const CbdArgs &ca, const EncArgs &ea, const UniformArgs &ua,
                          hipStream_t st, const KeyRing *ring);

    void stage_begin(int stage, hipStream_t st);
    void stage_end(hipStream_t st);
    void collect_events();

private:
    // What the K rows of a gen_keys_chain are: independent key pairs (gen_keys_batch), or the K = 2 np rows of an
    // evaluation key under ONE secret key (sk_in, n/4 bytes) with its diagonal term added to pk0 -- that of the
    // relinearisation key, or that of the Galois key of `elt`.  sp: the K = np - 1 rows of a special-prime key, whose
    // diagonal carries q_{np-1} mod q_j on row j instead of the digit weights on rows 2j, 2j + 1.  kSwitch (sp only): the
    // rows are under sk_in and the diagonal is (q_{np-1} mod q_j) . NTT_j(other), `other` the packed secret key the
    // switching key hides (host pointer, n/4 bytes).
    struct KeyChain
    {
        enum Kind { kPairs, kRelin, kGalois, kSwitch } kind;
        uint32_t elt = 0;   // kGalois only
        bool sp      = false;
        const uint8_t *other = nullptr;   // kSwitch only
    };
    // the launch chain of gen_keys_batch.  The caller holds `mu`.
    int gen_keys_chain(KeyChain chain, size_t K, const uint8_t *sk_in, const uint8_t *sk_seeds, const uint8_t *pk_seeds,
                       const uint8_t *ep_seeds, uint8_t *sk_out, uint32_t *pk0_out, uint32_t *pk1_out);
    // shared by the two evaluation keys and their two calls (se_context.cpp)
    bool evk_secret_ok(const uint8_t *sk_packed) const;
    size_t evk_rows(bool sp) const { return sp ? hp.nprimes - 1 : 2 * hp.nprimes; }
    bool special_prime_ok() const;
    int build_evk(const uint32_t *k0, const uint32_t *k1, size_t R, DevBuf<uint32_t> &stage, DevBuf<uint32_t> &block);
    int build_evk_at(const uint32_t *k0, const uint32_t *k1, size_t R, DevBuf<uint32_t> &stage, uint32_t *block);
    template <class Args>
    bool evk_call_args(Args &a, std::initializer_list<const void *> slabs, size_t B, size_t primes, bool sp = false) const;
    bool galois_elt_ok(uint32_t elt) const { return (elt & 1) && elt < 2 * hp.n; }   // odd and below 2n
    bool galois_elts_ok(const uint32_t *elts, size_t G, const char *count_msg, bool distinct = false) const;
    const uint32_t *galois_key(bool sp, uint32_t elt) const;
    // the rotation-family entries (se_context.cpp): one fill of the element-set block's call shape and slabs, one
    // resolver of elements into installed key blocks (the only loop over galois_key), one plan check, and the unchecked
    // "fill and launch" halves of the step entries that the composites chain
    bool set_call_args(GaloisSetArgs &a, const uint32_t *c0, const uint32_t *c1, uint32_t *out0, uint32_t *out1, size_t B,
                       size_t primes, bool sp) const;
    int resolve_keys(GaloisSetArgs &a, const uint32_t *elts, size_t G, bool sp, bool one_keyless) const;
    template <class Plan>
    bool plan_ok(const Plan *plan, bool sp, size_t primes, const char *what, const char *create,
                 const char *level_msg) const;
    int mul_plain_sum_step(const uint32_t *d_in0, const uint32_t *d_in1, size_t E, size_t B, size_t primes,
                           const uint32_t *d_pt, size_t Gout, size_t pt_primes, uint32_t *d_out0, uint32_t *d_out1, bool sp,
                           hipStream_t st);
    int mod_down_sp_step(const uint32_t *d_in0, const uint32_t *d_in1, size_t count, size_t primes, uint32_t *d_out0,
                         uint32_t *d_out1, hipStream_t st);
    int galois_accum_step(const GaloisSetArgs &aa, bool sp, hipStream_t st);
    int decrypt_level_impl(const uint32_t *d_c0, const uint32_t *d_c1, const uint32_t *d_c2, bool deg2, size_t B,
                           size_t primes, double scale, const uint32_t *d_key_idx, bool keyed, int64_t *d_pte,
                           float *d_values, double *d_values_f64, uint8_t *d_status, hipStream_t st);
    // the call protocol of the entries with scratch, and of the keyed ones on top of it (se_context.cpp)
    template <class Body>
    int call_scope(hipStream_t st, Body &&body);
    template <class Body>
    int keyed_call(const uint32_t *d_key_idx, size_t K, const uint32_t *k0, const uint32_t *k1, KeyRejectArgs ra,
                   size_t B, hipStream_t st, Body &&body);
};

void set_last_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what);

}  // namespace seamd

// the opaque handle of include/seal_embedded_amd.h
struct se_amd_ctx
{
    seamd::Context c;
};
struct se_amd_lintrans
{
    seamd::LintransPlan p;
};
struct se_amd_bsgs
{
    seamd::BsgsPlan p;
};
struct se_amd_poly
{
    seamd::PolyPlan p;
};

#define SEAMD_HIP(call)                                             \
    do                                                              \
    {                                                               \
        hipError_t e__ = (call);                                    \
        if (e__ != hipSuccess) return seamd::hip_fail(e__, #call);  \
    } while (0)
