// kernel_args.h -- argument blocks and launcher prototypes shared by the kernels and the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../se_types.h"

namespace seamd {

struct EncArgs
{
    const float *values;
    const int8_t *err;
    const int8_t *ucodes;
    uint32_t *c0;
    uint32_t *c1;
    uint32_t *ntt_pte;
    int64_t *pte;
    uint8_t *status;
    uint32_t *general;   // fused kernel only: [1 + B] count + indices of the plaintexts the fast form
                         // declined (not "small"), processed by k_encode_encrypt_general
    uint8_t *compact;    // split kernels only (optional): [B] k_encode_rns -> k_ntt_fuse, 1 = the plaintext
                         // was small and travels as ONE int32 row (in c0's last prime row) instead of np
                         // residue rows
    size_t count;        // fused kernel: plaintexts of the launch (set by the launcher: n = 4096 symmetric /
                         // encode-only workgroups take two plaintexts each)
    size_t first;        // fused kernel, pair forms: the first plaintext of workgroup 0 (set by the launcher)
    uint32_t debug_flags;   // form selection for tests / A/B runs (results are bit-identical): kEncFlagOnePlane
};
// EncArgs::debug_flags: the fast unkeyed n = 4096 symmetric / encode-only launches keep the one-plane pair form
// (k_encode_encrypt) instead of the two-way form (k_encode_encrypt_pair2)
constexpr uint32_t kEncFlagOnePlane = 8192;
struct UniformArgs
{
    const uint8_t *seeds;
    const uint64_t *ctr_in;
    uint64_t *ctr_out;
    uint32_t *out;
    uint32_t *rej_list;
    uint32_t rej_cap;
    uint32_t B;
    uint32_t prime_lo, prime_hi;
    uint32_t out_primes;
    uint32_t *spec;        // [B][spec_cap] scratch: candidates precomputed by helper waves
    uint32_t spec_cap;
    uint32_t master_waves; // waves of a workgroup that own ciphertexts (the rest are redraw helpers)
    uint32_t debug_flags;  // form selection for tests / A/B runs (results are bit-identical): 8 = no helper waves,
                           // 16 = helpers without speculation, 32 / 64 = always the lane / the wave form
    const uint32_t *only_from;  // optional [B]: ciphertext b takes part only if only_from[b] != 0 and
                                // prime_lo >= only_from[b] (redo of speculation misses)
    uint32_t out_prime_base;  // output row of prime j is (b * out_primes + j - out_prime_base): lets a
                              // single-prime launch (prime_lo = j) write one row per ciphertext
    uint32_t helper_fill;  // waves per workgroup that small batches are filled up to with helpers
                           // (0 = default 8 = two per SIMD; 4 leaves room for a co-resident
                           // 1024-thread transform workgroup at n = 16384)
    const uint8_t *prime_of;  // optional [B]: ciphertext b samples ONLY prime prime_of[b], into output row b
                              // (out_primes = 1; prime_lo / prime_hi / out_prime_base are ignored): the virtual
                              // ciphertexts of ALL guessed primes of the prime speculation in ONE launch
    uint32_t *nrej;           // staged form only: [B] rejected coefficients of the polynomial (k_bulk_pair ->
                              // k_resolve_wave)
    // staged forms: [1 + B] count + indices of the ciphertexts k_resolve_light could not finish (candidate row too
    // short, reject list overflowed); zeroed by the bulk kernel of the same prime, walked by a SMALL grid of
    // k_resolve_wave (a full grid of waves that read one word and leave cost 0.35-1.0 ms beside the throughput
    // kernels at B = 65 536).  NULL: k_resolve_wave is launched over every ciphertext and looks at the flag bit.
    uint32_t *flagged;
};
// Launches of at most this many ciphertexts take the wave-per-ciphertext kernel (k_sample_uniform_wave):
// 16 waves per CU = 4 per SIMD, where its ~7.8 us per permutation still beats the lane form's 8.6-10.7 us
// (tools/ubench5).
inline size_t uniform_wave_limit(unsigned num_cus) { return (size_t)16 * (num_cus ? num_cus : 256u); }
struct CbdArgs
{
    const uint8_t *seeds;
    const uint64_t *ctr_base;
    int8_t *out;
    uint32_t blocks_per_ct;
    uint32_t B;
};
struct TernaryArgs
{
    const uint8_t *seeds;
    int8_t *codes;
    uint64_t *ctr_out;
    uint32_t n;
    uint32_t B;
    const uint64_t *ctr_in;  // optional [B]: start counters (NULL = 0, the encrypt path)
    uint32_t num_cus;        // compute units of the device (0 = 256)
    uint32_t debug_flags;    // 32 = always the lane-per-ciphertext kernel (tests)
};

// Key ring of the keyed entries (se_context.h, Context::d_ring_*): K keys, each in the layout of the installed key
// (DevTables::s_hat / pk0 / pk1: [np][n][2] (value, Shoup)), back to back.  Handed only to the *_keyed kernels, which
// read record b's key at k0 / k1 + idx[b] * stride; the per-prime offset inside a key is the single key's.
struct KeyRing
{
    const uint32_t *k0;   // symmetric / decrypt: NTT(s) pairs; public key: pk0 pairs
    const uint32_t *k1;   // public key: pk1 pairs (else = k0)
    const uint32_t *idx;  // [B] key of each record, already clamped below K (Context::key_prologue)
    size_t stride;        // words per key: 2 np n
};

// ring != NULL: the keyed twins of the kernels (k_*_keyed), record b under key ring->idx[b]; the EncArgs /
// VerifyArgs of the launch are the unkeyed ones
hipError_t launch_encode_encrypt(const DevParams &, const DevTables &, const EncArgs &, int mode,
                                 size_t B, hipStream_t, const KeyRing *ring = nullptr);
hipError_t launch_encode_rns(const DevParams &, const DevTables &, const EncArgs &, bool add_err,
                             size_t B, hipStream_t);
hipError_t launch_ntt_fuse(const DevParams &, const DevTables &, const EncArgs &, int mode, int j,
                           size_t B, hipStream_t, const KeyRing *ring = nullptr);
hipError_t launch_decrypt_decode(const DevParams &, const DevTables &, const uint32_t *c0,
                                 const uint32_t *c1, uint32_t in_primes, int j, uint32_t *dec_ntt,
                                 uint32_t *pt, float *values, size_t B, hipStream_t,
                                 const KeyRing *ring = nullptr);
// Full-modulus decrypt (k_decrypt_full): all primes of a ciphertext in one launch, recombined to the centred
// integer over Q = q_0 ... q_{np-1}.  Every output is optional, at least one must be set.
struct FullArgs
{
    const uint32_t *c0;   // [B][np][n]
    const uint32_t *c1;   // [B][np][n]
    int64_t *pte;         // [B][n]    recombined m + e, natural order
    float *values;        // [B][n/2]  decoded slots
    double *values_f64;   // [B][n/2]  the same slots before the float conversion
    uint8_t *status;      // [B]       1 = every coefficient fits int64, else 0
    const uint32_t *c2;   // [B][np][n] degree-2 form only (the decrypt3 kernels): d = c0 + s (c1 + s c2)
};
hipError_t launch_decrypt_full(const DevParams &, const DevTables &, const CrtParams &, const FullArgs &, size_t B,
                               hipStream_t, const KeyRing *ring = nullptr);
// Weighted sums of records of one or two residue slabs (ct_ops.hip: k_ct_lincomb, k_ct_lincomb_sum), key-free:
//   out[g][j][i] = sum_k (w_k mod q_j) . in[idx_k][j][i]  mod q_j   over the entries k of output row g.
// CSR form: row g takes the entries [row_ptr[g], row_ptr[g+1]).  Dense form (row_ptr = idx = NULL): row g takes every
// record b with weight w[g B + b].  w = NULL: all ones.  Status 1, or 2 with an all-zero row for an index >= B or a
// row_ptr pair that decreases or passes nnz.
struct LincombArgs
{
    const uint32_t *in0, *in1;   // [B][np][n]; in1 / out1 NULL: one slab
    uint32_t *out0, *out1;       // [G][np][n]
    const uint32_t *row_ptr;     // [G + 1] or NULL
    const uint32_t *idx;         // [nnz] or NULL
    const int32_t *w;            // [nnz] or NULL
    uint8_t *status;             // [G], optional
    uint32_t *part;              // S > 1: [slabs][G S][np][n] canonical partial rows (context scratch)
    uint8_t *flag;               // S > 1: [G S] the slice saw an invalid entry
    uint32_t B, nnz;
    size_t G;
    size_t g0;                   // first output row of the launch (set by the launcher)
};
// S slices per output row (1 <= S <= 65 535): S = 1 writes the outputs directly, S > 1 goes through part / flag and a
// second launch that sums the S partial rows.  Every S gives the same bits (modular sums are exact).
hipError_t launch_ct_lincomb(const DevParams &, const LincombArgs &, uint32_t S, hipStream_t);
// Key-free rescale of one or two residue slabs (ct_ops.hip: k_ct_rescale): level `primes` -> level `primes` - 1,
//   out[b][j] = (in[b][j] - NTT_j(centred(INTT_last(in[b][last])) mod q_j)) . q_last^-1  mod q_j,   last = primes - 1.
struct RescaleArgs
{
    const uint32_t *in0, *in1;   // [B][primes][n]; in1 / out1 NULL: one slab
    uint32_t *out0, *out1;       // [B][primes - 1][n]
    uint32_t primes;             // 2 .. np
    uint32_t drop;               // mod-down only (k_ct_mod_down_sp): the prime of the last row, np - 1; rows j < primes - 1
                                 // are modulo q_j either way
};
hipError_t launch_ct_rescale(const DevParams &, const DevTables &, const RescaleParams &, const RescaleArgs &, size_t B,
                             hipStream_t);
// The same map with the special prime as the dropped one (k_ct_mod_down_sp): extended records [B][primes][n], primes =
// L + 1 <= np, whose last row is modulo q_drop, drop = np - 1 -> [B][L][n]; RescaleParams of level np.
hipError_t launch_ct_mod_down_sp(const DevParams &, const DevTables &, const RescaleParams &, const RescaleArgs &,
                                 size_t B, hipStream_t);
// Slot-wise product with encoded plaintexts (ct_ops.hip: k_ct_mul_plain), key-free:
//   out[b][j][i] = in[b][j][i] . pt[p(b)][j][i]  mod q_j,   j < primes,   p(b) = pt_idx[b], or 0 (P = 1) or b (P = B).
// Status 1, or 2 with all-zero rows for p(b) >= P.  out == in exactly is allowed.
struct MulPlainArgs
{
    const uint32_t *in0, *in1;   // [B][primes][n]; in1 / out1 NULL: one slab
    uint32_t *out0, *out1;       // [B][primes][n]
    const uint32_t *pt;          // [P][pt_primes][n], the first `primes` rows of a plaintext are read
    const uint32_t *pt_idx;      // [B] or NULL
    uint8_t *status;             // [B], optional
    uint32_t B, P;
    uint32_t primes, pt_primes;
};
hipError_t launch_ct_mul_plain(const DevParams &, const MulPlainArgs &, hipStream_t);
// Tensor product of two ciphertexts (ct_ops.hip: k_ct_mul), key-free: pair p = record ia[p] of (a0, a1) times record
// ib[p] of (b0, b1) (ia = ib = NULL: p, p), per prime j < primes and element, mod q_j:
//   out0 = x0 y0,   out1 = x0 y1 + x1 y0,   out2 = x1 y1.
// Status 1, or 2 with all-zero rows for ia[p] >= Ba or ib[p] >= Bb.  The a and b slabs may be the same memory.
struct MulArgs
{
    const uint32_t *a0, *a1;     // [Ba][primes][n]
    const uint32_t *b0, *b1;     // [Bb][primes][n]
    const uint32_t *ia, *ib;     // [P] each, or both NULL
    uint32_t *out0, *out1, *out2;   // [P][primes][n]
    uint8_t *status;             // [P], optional
    uint32_t P, Ba, Bb;
    uint32_t primes;
};
hipError_t launch_ct_mul(const DevParams &, const MulArgs &, hipStream_t);
// Grouped product sums (ct_ops.hip: k_ct_mul_sum, k_ct_dot_sp): output row g takes the pairs k in
// [row_ptr[g], row_ptr[g + 1]) (CSR rows as LincombArgs, unweighted), pair k = record ia[k] of (a0, a1) times record
// ib[k] of (b0, b1) (ia = ib = NULL: k, k), and per prime j < primes and element, canonical mod q_j:
//   T0[g] = sum_k x0 y0,   T1[g] = sum_k (x0 y1 + x1 y0),   T2[g] = sum_k x1 y1.
// k_ct_mul_sum stores (T0, T1, T2) and reads no key.  k_ct_dot_sp adds the special-prime key switch of d = T2[g] under
// the relinearisation key (KeySwitchSpArgs: acc_k, delta_k, ks_k) and stores out_k[g] = T_k[g] + ks_k: one division by
// P per row, and (T0, T1, T2) never in memory.
// status[g] (optional): 1; 2 with an all-zero row in every output slab for an ia[k] >= Ba, an ib[k] >= Bb or a row_ptr
// pair that decreases or passes nnz.  An empty row is all zero with status 1.
struct MulSumArgs
{
    const uint32_t *a0, *a1;        // [Ba][primes][n]
    const uint32_t *b0, *b1;        // [Bb][primes][n]
    const uint32_t *row_ptr;        // [G + 1]
    const uint32_t *ia, *ib;        // [nnz] each, or both NULL
    uint32_t *out0, *out1, *out2;   // [G][primes][n]; k_ct_dot_sp: out2 unused
    uint8_t *status;                // [G], optional
    const uint32_t *key;            // k_ct_dot_sp: the special-prime relinearisation key block
    size_t half;                    // words of one key half: R' np 2 n
    uint32_t G, nnz, Ba, Bb;
    uint32_t np;                    // columns of a key row (the context's primes)
    uint32_t primes;                // 1 .. np; k_ct_dot_sp: 1 .. np - 1
};
hipError_t launch_ct_mul_sum(const DevParams &, const MulSumArgs &, hipStream_t);
hipError_t launch_ct_dot_sp(const DevParams &, const DevTables &, const RescaleParams &, const MulSumArgs &, hipStream_t);
// The key switch of ct_ops.hip, shared by every kernel from here to launch_ct_galois_accum_sp (evk_row_coeffs, evk_digits, evk_mac;
// grid evk_grid(B, primes)).  `key` is one device evaluation-key block, built
// by Context::build_evk from the host's two halves: [2][R][np][2][n], R = 2 np rows of the CONTEXT's np columns, each
// column a row of n key words followed by the row of their Shoup companions floor(w 2^32 / q_i); half 1 starts `half`
// words behind half 0.  Every argument block names the fields the shared device code reads alike: key, half, np,
// primes, B.
// Relinearisation (k_ct_relin): level-`primes` (d0, d1, d2) -> (out0, out1) of the same level.
//   out0[b][i] = d0[b][i] + sum_{j < primes, t < 2} NTT_i(D_{j,t}) . key0[2j + t][i]   (out1: d1, key1)   mod q_i,
// D_{j,t} = the t-th 15-bit digit of the canonical coefficients of INTT_j(d2[b][j]).
struct RelinArgs
{
    const uint32_t *d0, *d1, *d2;   // [B][primes][n]
    uint32_t *out0, *out1;          // [B][primes][n]
    const uint32_t *key;
    size_t half;                    // words of one key half: R np 2 n
    size_t B;
    uint32_t np;                    // columns of a key row (the context's primes)
    uint32_t primes;                // 1 .. np
};
hipError_t launch_ct_relin(const DevParams &, const DevTables &, const RelinArgs &, hipStream_t);
// Slot rotation / conjugation (k_ct_galois): the automorphism sigma : x -> x^elt on both slabs of a level-`primes`
// record and the key switch of sigma(c1) with the Galois key of `elt` -- k_ct_relin on (sigma(c0), 0, sigma(c1)).
//   out0[b][i] = sigma(c0)[b][i] + sum_{j < primes, t < 2} NTT_i(D_{j,t}) . key0[2j + t][i]   (out1: no addend, key1),
// D_{j,t} = the t-th 15-bit digit of the canonical coefficients of sigma(INTT_j(c1[b][j])).
struct GaloisArgs
{
    const uint32_t *c0, *c1;        // [B][primes][n]
    uint32_t *out0, *out1;          // [B][primes][n]
    const uint32_t *key;
    size_t half;                    // words of one key half: R np 2 n
    size_t B;
    uint32_t np;                    // columns of a key row (the context's primes)
    uint32_t primes;                // 1 .. np
    uint32_t elt;                   // odd, below 2n (checked by the host: the kernel forms LDS addresses from it)
};
hipError_t launch_ct_galois(const DevParams &, const DevTables &, const GaloisArgs &, hipStream_t);
// Special-prime key switch (k_ct_relin_sp, k_ct_galois_sp): the last prime of the context, P = q_{np-1}, belongs to the
// key, records have `primes` <= np - 1 rows.  `key` is a device block [2][R'][np][2][n] of R' = np - 1 rows (build_evk).
// With D_j = centred(INTT_j(sw[b][j])) (sw = d2, or sigma(c1) for a rotation) and E = {0 .. primes-1, np-1}:
//   acc_k[i] = sum_{j < primes} NTT_i(D_j mod q_i) . key_k[j][i],  i in E;   delta_k = centred(INTT_p(acc_k[p]), P);
//   out_k[b][i] = a_k[b][i] + (acc_k[i] - NTT_i(delta_k mod q_i)) . P^-1   mod q_i,  i < primes,
// a0 = d0 resp. sigma(c0), a1 = d1 resp. 0.  The constants P^-1 mod q_i are the RescaleParams of level np.
struct KeySwitchSpArgs
{
    const uint32_t *a0, *a1;        // [B][primes][n]: d0, d1; rotation: c0, a1 unused
    const uint32_t *sw;             // [B][primes][n]: d2; rotation: c1
    uint32_t *out0, *out1;          // [B][primes][n]
    const uint32_t *key;
    size_t half;                    // words of one key half: R' np 2 n
    size_t B;
    uint32_t np;                    // columns of a key row (the context's primes, >= 2)
    uint32_t primes;                // 1 .. np - 1
    uint32_t elt;                   // 0: relinearisation; else odd, below 2n (checked by the host: LDS addresses)
};
hipError_t launch_ct_key_switch_sp(const DevParams &, const DevTables &, const RescaleParams &, const KeySwitchSpArgs &,
                                   hipStream_t);
// Switch-key ring (k_ct_switch_sp, k_ct_switch_sum_sp): `ring` holds K key blocks of the layout above, `stride` words
// apart; record b is switched under block key_idx[b].  An output row takes the records idx[row_ptr[g] .. row_ptr[g + 1])
// (the sum form, CSR rows as LincombArgs, unweighted), or the one record g (row_ptr = idx = NULL, rows = B).  With
// D_{b,j} = centred(INTT_j(c1[b][j])) and E as above:
//   acc_k[i] = sum_{b in row} sum_{j < primes} NTT_i(D_{b,j} mod q_i) . ring[key_idx[b]]_k[j][i],  i in E;
//   delta_k = centred(INTT_p(acc_k[p]), P);   ks_k[i] = (acc_k[i] - NTT_i(delta_k mod q_i)) . P^-1   mod q_i;
//   out0[g][i] = ks_0[i] + sum_{b in row} c0[b][i],   out1[g][i] = ks_1[i]:   one division by P per row.
// status[g] (optional): 1; 2 with an all-zero row in both slabs for a record index >= B, a member's key index >= K or a
// row_ptr pair that decreases or passes nnz.  An empty row is all zero with status 1.
struct SwitchSpArgs
{
    const uint32_t *c0, *c1;        // [B][primes][n]
    uint32_t *out0, *out1;          // [rows][primes][n]
    const uint32_t *ring;
    const uint32_t *key_idx;        // [B]
    const uint32_t *row_ptr, *idx;  // [rows + 1], [nnz]; both NULL: row g is the record g
    uint8_t *status;                // [rows], optional
    size_t half;                    // words of one key half: R' np 2 n
    size_t stride;                  // words from one key block to the next: 2 half
    size_t B, rows, nnz;            // each below 2^32
    uint32_t K;                     // keys in the ring
    uint32_t np;                    // columns of a key row (the context's primes, >= 2)
    uint32_t primes;                // 1 .. np - 1
};
hipError_t launch_ct_switch_sp(const DevParams &, const DevTables &, const RescaleParams &, const SwitchSpArgs &,
                               hipStream_t);
// Hoisted rotations (k_ct_galois_hoist): G rotations of every record from ONE digit decomposition of c1.  The digits
// D_{j,t} are those of the canonical coefficients of INTT_j(c1[b][j]) itself; sigma is applied to the TRANSFORMED digits,
// where it is the permutation src_g:
//   rot0[g][b][i][k] = c0[b][i][src_g(k)] + sum_{j < primes, t < 2} NTT_i(D_{j,t})[src_g(k)] . key0_g[2j + t][i][k]
//   rot1[g][b][i][k] =                      sum_{j < primes, t < 2} NTT_i(D_{j,t})[src_g(k)] . key1_g[2j + t][i][k].
// Many form (sum = 0): out[e][b] = rot[elt[e]], outputs [G][B][primes][n].  Sum form (sum = 1): out[b] = add_input .
// (c0, c1)[b] + sum_e rot[elt[e]], outputs [B][primes][n].  The elements and the key block of each travel in the
// argument block (kernarg): no device table, no scratch.
constexpr uint32_t kMaxGaloisKeys = 64;   // elements of one installed set, and of one call (SE_AMD_MAX_GALOIS_KEYS)
// The element-set block: what every kernel of a set of Galois elements reads alike, filled on the host by
// Context::evk_call_args (batch and key layout) and Context::resolve_keys (elements and key blocks).  The slab layouts
// differ per kernel and stand at its launcher.
struct GaloisSetArgs
{
    const uint32_t *c0, *c1;        // the input slabs
    uint32_t *out0, *out1;          // the output slabs
    size_t half;                    // words of one key half: R np 2 n (R' = np - 1 rows on the special-prime keys)
    size_t B;
    uint32_t np;                    // columns of a key row (the context's primes; >= 2 on the special-prime keys)
    uint32_t primes;                // 1 .. np (1 .. np - 1 on the special-prime keys)
    uint32_t G;                     // 1 .. kMaxGaloisKeys
    uint32_t elt[kMaxGaloisKeys];   // odd, below 2n (checked by the host: the kernel forms LDS addresses from them)
    const uint32_t *key[kMaxGaloisKeys];   // the device key block of elt[e]; NULL where the kernel needs none (elt[e] == 1)
};
struct GaloisHoistArgs : GaloisSetArgs
{
    uint32_t sum, add_input;        // 0 / 1 each; add_input only with sum
};
// in [B][primes][n]; out many: [G][B][primes][n], sum: [B][primes][n]
hipError_t launch_ct_galois_hoist(const DevParams &, const DevTables &, const GaloisHoistArgs &, hipStream_t);
// Linear transform (k_ct_lintrans): the sum form above with a plaintext weight per element, the diagonal method
//   out0[b][i][k] = d0[i][k] c0[b][i][k] + sum_e d_e[i][k] rot0[elt[e]][b][i][k]   (out1: c1 and rot1)   mod q_i.
// d_e does not depend on the key row, so it is folded into the key block when the plan is made (k_lintrans_fold):
// key[e] holds gk . d_e mod q_i with its Shoup companions in the installed block's layout, and the digit loop is the sum
// form's.  Only the epilogue carries weights: the (word, Shoup) rows diag[e][np][2][n], and diag0 [np][2][n] or NULL.
struct LintransArgs : GaloisSetArgs   // key[e]: the folded key block of entry e; primes 1 .. the plan's levels
{
    const uint32_t *diag;           // [G][np][2][n]
    const uint32_t *diag0;          // [np][2][n], or NULL: the record itself does not enter
};
// in, out [B][primes][n]
hipError_t launch_ct_lintrans(const DevParams &, const DevTables &, const LintransArgs &, hipStream_t);
// Hoisted rotations on the special-prime key (k_ct_galois_sum_sp, k_ct_lintrans_sp): the sum form and the linear
// transform above on blocks [2][R'][np][2][n] of R' = np - 1 rows, records of `primes` <= np - 1 rows.  With D_j =
// centred(INTT_j(c1[b][j])), E = {0 .. primes-1, np-1} and src_e the permutation of elt[e]:
//   acc_k[i][x] = sum_e sum_{j < primes} NTT_i(D_j mod q_i)[src_e(x)] . key_k[e][j][i][x],  i in E;
//   delta_k = centred(INTT_p(acc_k[p]), P);   ks_k[i] = (acc_k[i] - NTT_i(delta_k mod q_i)) . P^-1   mod q_i,  i < primes;
//   sum form (weighted = 0): out0 = ks_0 + add_input . c0 + sum_e sigma_e(c0),  out1 = ks_1 + add_input . c1, key[e] the
//     installed special-prime blocks;
//   weighted: out0 = ks_0 + d0 . c0 + sum_e d_e . sigma_e(c0),  out1 = ks_1 + d0 . c1, key[e] the plan's blocks with d_e
//     folded in on every column (np - 1 included), diag / diag0 as in LintransArgs.
// One decomposition and one division by P per record whatever G is.  The constants P^-1 mod q_i are the RescaleParams of
// level np.
struct HoistSpArgs : GaloisSetArgs
{
    uint32_t weighted, add_input;   // 0 / 1 each; add_input only without weighted
    const uint32_t *diag;           // weighted: [G][np][2][n]
    const uint32_t *diag0;          // weighted: [np][2][n], or NULL: the record itself does not enter
};
// in, out [B][primes][n]
hipError_t launch_ct_hoist_sp(const DevParams &, const DevTables &, const RescaleParams &, const HoistSpArgs &,
                              hipStream_t);
// Plan set-up (k_lintrans_fold), one entry per launch.  d = diag_in[i][k] mod q_i for columns i < pt, 0 beyond (any
// 32-bit word is valid input).  pair_out [np][2][n] = (d, its Shoup companion); with key_in (an installed block
// [2][rows][np][2][n]), key_out = the block of the words key_in . d mod q_i and their companions.  key_in NULL: pairs
// only.
hipError_t launch_lintrans_fold(const DevParams &, const uint32_t *key_in, uint32_t *key_out, size_t rows,
                                const uint32_t *diag_in, uint32_t *pair_out, uint32_t pt, hipStream_t);
// Baby-step / giant-step linear transforms (se_amd_ct_bsgs_device): the two device steps behind the many form, and the
// plan's set-up.
// Weighted sum over a stack (k_ct_mul_plain_sum), key-free:
//   out[g][b][i][k] = sum_{e < E} (pt[g][e][i][k] mod q_i) . in[e][b][i][k]   mod q_i, canonical,
// in [E][B][primes][n], pt [Gout][E][pt_primes][n] (any 32-bit word stands for its residue), out [Gout][B][primes][n].
struct MulPlainSumArgs
{
    const uint32_t *in0, *in1;      // [E][B][primes][n]; in1 NULL: one slab
    const uint32_t *pt;             // [Gout][E][pt_primes][n]
    uint32_t *out0, *out1;          // [Gout][B][primes][n]
    uint32_t B;
    uint32_t E, Gout;               // 1 .. kMaxGaloisKeys each; E B and Gout B below 2^32
    uint32_t primes, pt_primes;     // pt_primes >= primes
    uint32_t last_prime;            // the prime (and plaintext row) of row primes - 1: primes - 1 itself (the identity map),
                                    // or np - 1 on extended records, whose last row is modulo the special prime
};
hipError_t launch_ct_mul_plain_sum(const DevParams &, const MulPlainSumArgs &, hipStream_t);
// Rotate different ciphertexts and add (k_ct_galois_accum): out[b] = sum_{g < G} rho_g(in[g][b]) mod q_i, canonical, rho_g
// the map of GaloisArgs with elt[g] and key[g]; elt[g] == 1 is the identity (key[g] unused).  The elements and the key
// block of each travel in the argument block, a GaloisSetArgs as it is.
// in (c0, c1) [G][B][primes][n], out [B][primes][n]; G B below 2^32
hipError_t launch_ct_galois_accum(const DevParams &, const DevTables &, const GaloisSetArgs &, hipStream_t);
// Baby steps on the special-prime keys, UNDIVIDED (k_ct_galois_many_ext_sp): G rotations of a level-`primes` record
// (primes <= np - 1) as extended records of primes + 1 rows -- rows r < primes modulo q_r, row `primes` modulo P = q_{np-1}
// -- from ONE decomposition of c1.  With D_j, F_{j,i}, E and src_e as in HoistSpArgs and i_r = r, or np - 1 for r = primes:
//   out_k[e][b][r][x] = sum_{j < primes} F_{j,i_r}[src_e(x)] . key_k[e][j][i_r][x]  (+ (P mod q_r) . c0[b][r][src_e(x)] for
//   k = 0, r < primes)   mod q_{i_r}, canonical.  elt[e] == 1: out_k = (P mod q_r) . c_k[b][r], row `primes` zero, no key.
// "P times the rotated ciphertext plus the key-switch sum": k_ct_mod_down_sp of it is the rotation by elt[e].
// in [B][primes][n], out [G][B][primes + 1][n]; G B below 2^32; key[e] the special-prime block of elt[e]
hipError_t launch_ct_galois_many_ext_sp(const DevParams &, const DevTables &, const GaloisSetArgs &, hipStream_t);
// Giant steps on the special-prime keys with ONE division (k_ct_galois_accum_sp): G different level-`primes` records
// (a^g, b^g) = in[g][b] are rotated and added.  With D^g_j = centred(INTT_j(sigma_g(b^g[j])), q_j) for the keyed g (elt[g]
// != 1):  acc_k[i] = sum_g sum_j NTT_i(D^g_j mod q_i) . key_k[g][j][i], i in E;  delta_k, ks_k as in KeySwitchSpArgs;
//   out0 = ks_0 + sum_{keyed g} sigma_g(a^g) + sum_{elt[g] == 1} a^g,   out1 = ks_1 + sum_{elt[g] == 1} b^g.
// in (c0, c1) [G][B][primes][n], out [B][primes][n]; G B below 2^32; key[g] the special-prime block of elt[g]
hipError_t launch_ct_galois_accum_sp(const DevParams &, const DevTables &, const RescaleParams &, const GaloisSetArgs &,
                                     hipStream_t);
// Slot packing (k_ct_pack_sp, ct_pack.hip): entry k is (record idx[k], element elt[eidx[k]]); an output row takes the
// entries row_ptr[g] .. row_ptr[g + 1] (CSR rows as SwitchSpArgs), or the one entry (record g, elt[eidx[g]]) (row_ptr =
// idx = NULL, rows = B = nnz).  With sigma_k the automorphism of entry k, D_{k,j} = centred(INTT_j(c1[b_k][j])) and E as
// in KeySwitchSpArgs:
//   acc_h[i] = sum_{k in row, elt_k != 1} sum_{j < primes} NTT_i(sigma_k(D_{k,j}) mod q_i) . key[eidx[k]]_h[j][i],  i in E;
//   delta_h, ks_h as in KeySwitchSpArgs: one division by P per row;
//   out0[g][i] = ks_0[i] + sum_{k in row} sigma_k(c0[b_k])[i],   out1[g][i] = ks_1[i] + sum_{k in row, elt_k = 1} c1[b_k][i].
// The block's G is the number of listed elements and B the records of the input slabs; key[e] the special-prime block of
// elt[e], NULL for the identity.  status[g] (optional): 1; 2 with an all-zero row in both slabs for a record index >= B,
// an element index >= G or a row_ptr pair that decreases or passes nnz.  An empty row is all zero with status 1.
struct PackSpArgs : GaloisSetArgs
{
    const uint32_t *row_ptr, *idx;  // [rows + 1], [nnz]; both NULL: row g is the entry g
    const uint32_t *eidx;           // [nnz]
    uint8_t *status;                // [rows], optional
    size_t rows, nnz;               // each below 2^32
};
// in [B][primes][n], out [rows][primes][n]
hipError_t launch_ct_pack_sp(const DevParams &, const DevTables &, const RescaleParams &, const PackSpArgs &,
                             hipStream_t);
// The last step of a slot-wise polynomial (k_ct_affine_rescale, ct_poly.hip), key-free: the weighted sum of T term records
// that live at their own levels, one rescale of the sum and a constant.  Term t is the pair of slabs term0[t], term1[t]
// [B][term_primes[t]][n], term_primes[t] >= primes, of which the first `primes` rows of a record are read.  With
//   acc_s[b][j] = sum_t w[t][j] . term_s[t][b][j]  mod q_j,   j < primes,   last = primes - 1,
//   out_s[b][i] = (acc_s[b][i] - NTT_i(centred(INTT_last(acc_s[b][last])) mod q_i)) . q_last^-1 + (s == 0 ? c[i] : 0)  mod q_i,
// canonical, i < last: RescaleArgs' map on a row that is never in memory.  w[t][j] and c[i] are canonical residues the host
// forms from the int64 weights and constant; the block is a kernel argument, so nothing is uploaded.
constexpr uint32_t kAffineMaxTerms = 16;   // SE_AMD_AFFINE_MAX_TERMS
struct AffineRescaleArgs
{
    const uint32_t *term0[kAffineMaxTerms], *term1[kAffineMaxTerms];
    uint32_t term_primes[kAffineMaxTerms];   // rows of a record of term t
    uint32_t w[kAffineMaxTerms][kMaxPrimes];   // w_t mod q_j in [0, q_j)
    uint32_t c[kMaxPrimes];                    // c_after mod q_i in [0, q_i)
    uint32_t *out0, *out1;                     // [B][primes - 1][n]
    uint32_t T;                                // 1 .. kAffineMaxTerms
    uint32_t primes;                           // 2 .. np
};
hipError_t launch_ct_affine_rescale(const DevParams &, const DevTables &, const RescaleParams &, const AffineRescaleArgs &,
                                    size_t B, hipStream_t);
// out[k] = k for k < count: the row pointers of `count - 1` one-pair rows (stage_ops.hip), for the plans that call a CSR
// entry from a caller's workspace.
hipError_t launch_row_iota(uint32_t *out, size_t count, hipStream_t);
// Plan set-up: out[r][k] = in[r][src_elt(k)] on `rows` rows of n words, src the permutation of the automorphism of `elt`
// (odd, below 2n, checked by the host) on a bit-reversed NTT-form row.
hipError_t launch_bsgs_permute(const DevParams &, const uint32_t *in, uint32_t *out, size_t rows, uint32_t elt,
                               hipStream_t);
// Evaluation-key plumbing.  relin_key_rows: `rows` rows [np][n] of key words -> [rows][np][2][n] (words, Shoup
// companions).  evk_diag: key0[2j + t][j][k] += 2^(15 t) . d[k] mod q_j for t = 0, 1 on an [R][np][n]
// slab, s_hat = the canonical NTT(s) mod q_j, [n]: d = s_hat^2 with elt 0 (the relinearisation key), d[k] =
// s_hat[src_elt(k)], sigma_elt(s) in NTT form, else (the Galois key of elt).  sp: the special-prime key's slab
// [np - 1][np][n] instead, key0[j][j][k] += (q_{np-1} mod q_j) . d[k] for j < np - 1.  other (sp only): a switching key,
// d = s_hat as it is, the caller passing the canonical NTT form of the secret key the switching key hides.
hipError_t launch_relin_key_rows(const DevParams &, const uint32_t *in, uint32_t *out, size_t rows, hipStream_t);
hipError_t launch_evk_diag(const DevParams &, uint32_t j, uint32_t elt, bool sp, const uint32_t *s_hat,
                           uint32_t *key0, hipStream_t, bool other = false);
// key-ring install and the sanitising / rejecting passes of a keyed call (encode_encrypt.hip)
//   ring_secret_ntt : K packed secret keys [K][n/4] -> (NTT(s) mod q_j, Shoup) pairs of prime j of each ring key
//   ring_pairs      : K public-key slabs [K][np][n] (NTT form) -> [K][np][n][2] (value, Shoup)
//   key_sanitize    : idx[b] = min(raw[b], K - 1); bad = count + records with raw[b] >= K (bad[0] zeroed first)
//   key_reject      : for every record of `bad`: status 2 and zero rows (row b of rows[r] = words[r] words)
hipError_t launch_ring_secret_ntt(const DevParams &, const DevTables &, int j, const uint8_t *packed, uint32_t *ring,
                                  size_t K, hipStream_t);
hipError_t launch_ring_pairs(const DevParams &, const uint32_t *vals, uint32_t *pairs, size_t K, hipStream_t);
hipError_t launch_key_sanitize(const uint32_t *raw, uint32_t *idx, uint32_t *bad, size_t K, size_t B, hipStream_t);
struct KeyRejectArgs
{
    const uint32_t *bad;
    uint8_t *status;      // optional
    uint32_t *rows[3];    // optional
    size_t words[3];
};
hipError_t launch_key_reject(const DevParams &, const KeyRejectArgs &, size_t B, hipStream_t);
hipError_t launch_reduce_small(const DevParams &, const int8_t *e, uint32_t *out, size_t count, hipStream_t);
hipError_t launch_ntt_polys(const DevParams &, const DevTables &, int j, uint32_t *polys,
                            uint32_t *pairs, size_t count, hipStream_t);
hipError_t launch_make_pairs(const uint32_t *vals, uint32_t *pairs, uint32_t q, size_t count,
                             hipStream_t);
hipError_t launch_sample_uniform(const DevParams &, const UniformArgs &, hipStream_t);
// staged form, one prime per launch (kernels/samplers.hip: k_bulk_pair, k_candidates, k_resolve_wave)
hipError_t launch_uniform_bulk_pair(const DevParams &, const UniformArgs &, hipStream_t);
hipError_t launch_uniform_candidates(const UniformArgs &, hipStream_t);
hipError_t launch_uniform_resolve(const DevParams &, const UniformArgs &, hipStream_t);
// Small-batch prime speculation (se_context.cpp, encrypt_sym_small): the uniform sampler of prime
// j >= 1 is run for every plausible start counter of a window at once ("virtual ciphertexts"), so
// the primes of one ciphertext no longer wait for each other.
struct SpecPlan
{
    uint32_t nprimes;              // primes of the chain (speculated: 1 .. nprimes-1)
    uint32_t B;                    // real ciphertexts
    uint64_t base[kMaxPrimes];     // first guessed start counter of prime j
    uint32_t count[kMaxPrimes];    // guesses per ciphertext for prime j (0 for j = 0)
    uint32_t offset[kMaxPrimes];   // first virtual ciphertext of prime j
    uint32_t total;                // virtual ciphertexts in all
};
hipError_t launch_spec_setup(const SpecPlan &, const uint8_t *seeds, uint8_t *seeds_v, uint64_t *ctr_v,
                             uint8_t *prime_v, hipStream_t);
hipError_t launch_spec_select(const SpecPlan &, uint32_t n, uint64_t *ctr0, const uint64_t *ctrout_v,
                              const uint32_t *rows, uint32_t *c1, uint32_t *fail, hipStream_t);

// ---- explicit-operand stage kernels behind the reference-named lower surface (stage_ops.hip) ----
struct FftArgs
{
    const double *in;    // [count][n][2] interleaved complex128
    double *out_cplx;    // [count][n][2] (optional in mode 1)
    int64_t *out_int;    // mode 1: [count][n]
    uint32_t *fail_idx;  // mode 1: [count], preset to 0xFFFFFFFF
    int mode;            // 0 ifft_inpl, 1 ifft + round (ckks_encode_base tail), 2 fft_inpl
};
struct LowerSymArgs
{
    const uint8_t *s_small;  // 2-bit packed secret key(s): polynomial b uses s_small + b * s_stride bytes
    const int64_t *pte;      // [count][n] m + e, or NULL ...
    const int8_t *ep;        // ... then [count][n] small error (gen_pk)
    const uint32_t *a;       // uniform polynomial of this prime (NTT domain): a + b * a_stride
    uint32_t *c0, *ntt_pte;  // c0 + b * c0_stride; ntt_pte [count][n]
    uint32_t *s_save;        // optional [count][n]
    int j;
    uint32_t s_stride;       // bytes between the keys of consecutive polynomials (0 = one shared key)
    uint32_t a_stride;       // elements between consecutive polynomials of `a`  (0 = n)
    uint32_t c0_stride;      // elements between consecutive polynomials of `c0` (0 = n)
};
struct LowerAsymArgs
{
    const uint8_t *u_small;  // [count][n/4] 2-bit packed u
    const int8_t *e1;        // [count][n]
    const int64_t *pte;      // [count][n] m + e0
    const uint32_t *pk0, *pk1;  // [count][n] public key of this prime (in)
    uint32_t *c0, *c1, *ntt_pte;  // [count][n] (out)
    uint32_t *ntt_u_save, *ntt_e1_save;  // optional
    int j;
};
hipError_t launch_fft_polys(const DevParams &, const DevTables &, const FftArgs &, size_t count, hipStream_t);
hipError_t launch_reduce_poly(const DevParams &, int j, const int64_t *pte, const int8_t *e, uint32_t *out,
                              bool add, size_t total, hipStream_t);
hipError_t launch_word_ops(const DevParams &, int j, int op, const uint64_t *a, const uint64_t *b,
                           const uint64_t *c, uint32_t *out, size_t count, hipStream_t);
hipError_t launch_add_small(int64_t *m, const int8_t *e, size_t total, hipStream_t);
hipError_t launch_pack_ternary(const int8_t *codes, uint8_t *packed, size_t total_bytes, hipStream_t);
hipError_t launch_ternary_words(const uint32_t *in, uint32_t *out, uint32_t *nrej, uint32_t q, uint32_t n, int op,
                                hipStream_t);
hipError_t launch_expand_ternary(const uint8_t *packed, uint32_t *out, uint32_t q, uint32_t n, hipStream_t);
hipError_t launch_lower_sym_prime(const DevParams &, const DevTables &, const LowerSymArgs &, size_t count,
                                  hipStream_t);
hipError_t launch_lower_asym_prime(const DevParams &, const DevTables &, const LowerAsymArgs &, size_t count,
                                   hipStream_t);

hipError_t launch_sample_cbd(const CbdArgs &, hipStream_t);
hipError_t launch_sample_ternary(const TernaryArgs &, hipStream_t);
hipError_t launch_prng_blocks(const uint8_t *seeds, const uint64_t *ctrs, uint8_t *out,
                              uint32_t outlen, uint32_t count, hipStream_t);


}  // namespace seamd
