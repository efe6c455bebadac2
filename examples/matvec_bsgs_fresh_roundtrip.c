/*
 * matvec_bsgs_fresh_roundtrip.c -- matvec_bsgs_roundtrip.c on FRESH records: the 16 x 16 product y = M x by baby steps and
 * giant steps under the special-prime Galois keys, with no lift.  Every record holds a 16-vector x repeated through its
 * slots; the evaluator holds a fixed 16 x 16 real matrix M with entries in [-1/2, 1/2] as its sixteen generalised
 * diagonals and NO secret key, and computes
 *     y[k] = sum_e diag_e[k] . x[k + e],      diag_e[k] = M[k mod 16][(k + e) mod 16],   e = 4 g + b,
 * in ONE call, the rotation by e split into a baby step b = 0 .. 3 and a giant step 4 g = 0, 4, 8, 12 (INTEGRATION.md
 * section 4n).  SIX special-prime Galois keys (steps 1, 2, 3, 4, 8, 12) serve the sixteen diagonals.  The records are
 * dropped to np - 1 primes (the last prime of the context belongs to the keys); se_amd_bsgs_create_sp takes the diagonals,
 * encoded from M at the full scale Delta with ALL np rows, as a flat plan would; se_amd_ct_bsgs_sp_device keeps the baby
 * steps undivided, multiplies the diagonals in, divides by the special prime once per giant step and once more for their
 * sum, in the caller's workspace.  The result has scale Delta^2 at level np - 1: one se_amd_ct_rescale_device drops a prime,
 * se_amd_decrypt_level_device decodes at Delta^2 / q_{np-2}.  Prints the largest error.
 *
 *   gcc examples/matvec_bsgs_fresh_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o matvec_bsgs_fresh_roundtrip
 *   ./matvec_bsgs_fresh_roundtrip 4096 3 8
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "seal_embedded_amd.h"

#define CHECK_HIP(call)                                                                  \
    do                                                                                   \
    {                                                                                    \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess)                                                            \
        {                                                                                \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                   \
            exit(2);                                                                     \
        }                                                                                \
    } while (0)
#define CHECK_SE(call)                                                                   \
    do                                                                                   \
    {                                                                                    \
        int rc_ = (call);                                                                \
        if (rc_ != SE_SUCCESS)                                                           \
        {                                                                                \
            fprintf(stderr, "%s: %d (%s)\n", #call, rc_, se_amd_last_error());           \
            exit(2);                                                                     \
        }                                                                                \
    } while (0)

#define N1 4                /* baby steps 0 .. 3 */
#define N2 4                /* giant steps 0, 4, 8, 12 */
#define DIM (N1 * N2)       /* the matrix is DIM x DIM */
#define KEYS (N1 + N2 - 2)  /* step 0 of either list needs no key */

static void fill_seeds(uint8_t *s, size_t count, unsigned mul, unsigned add)
{
    for (size_t r = 0; r < count; r++)
        for (int k = 0; k < 64; k++) s[r * 64 + k] = (uint8_t)(mul * r + add + k);
}

/* the fixed matrix: entries k / 16, k = -8 .. 8 */
static double matrix(size_t r, size_t c) { return (double)((int)((7 * r + 3 * c + 1) % 17) - 8) / 16.0; }

int main(int argc, char **argv)
{
    size_t n       = argc > 1 ? (size_t)atol(argv[1]) : 4096;
    size_t nprimes = argc > 2 ? (size_t)atol(argv[2]) : 3;
    size_t B       = argc > 3 ? (size_t)atol(argv[3]) : 8;
    /* one prime for the keys, one for the rescale, one left to decrypt at */
    if (B == 0 || nprimes < 3 || nprimes > 13) return 2;
    const size_t slots = n / 2, rec = nprimes * n, L = nprimes - 1, lrec = L * n, low = (L - 1) * n, R = nprimes - 1;

    /* ---- the key holder: one secret key; the special-prime Galois keys of the six steps are public material, handed to
     * the evaluator ---- */
    se_amd_ctx *ctx;
    CHECK_SE(se_amd_create(&ctx, n, nprimes, 0));
    uint8_t *sk = (uint8_t *)calloc(n / 4, 1);                 /* 2-bit packed, codes 0 / 1 / 2 = -1 / 0 / +1 */
    for (size_t i = 0; i < n / 4; i++) sk[i] = (uint8_t)(((i * 37u) % 3u) * 0x55u);
    CHECK_SE(se_amd_set_secret_key(ctx, sk));
    uint32_t q[13];
    CHECK_SE(se_amd_moduli(ctx, q));
    uint32_t baby[N1], giant[N2], elts[KEYS];
    for (int b = 0; b < N1; b++) CHECK_SE(se_amd_galois_element(n, b, &baby[b]));
    for (int g = 0; g < N2; g++) CHECK_SE(se_amd_galois_element(n, N1 * g, &giant[g]));
    for (int b = 1; b < N1; b++) elts[b - 1] = baby[b];
    for (int g = 1; g < N2; g++) elts[N1 - 2 + g] = giant[g];
    uint8_t *a_seeds = (uint8_t *)malloc(KEYS * R * 64), *e_seeds = (uint8_t *)malloc(KEYS * R * 64);
    fill_seeds(a_seeds, KEYS * R, 29, 3);
    fill_seeds(e_seeds, KEYS * R, 11, 77);
    uint32_t *gk0 = (uint32_t *)malloc(KEYS * R * rec * 4), *gk1 = (uint32_t *)malloc(KEYS * R * rec * 4);
    CHECK_SE(se_amd_gen_galois_keys_sp(ctx, sk, elts, KEYS, a_seeds, e_seeds, gk0, gk1));
    CHECK_SE(se_amd_set_galois_keys_sp(ctx, elts, KEYS, gk0, gk1));

    /* ---- the sender: B records, a 16-vector with entries in [-1, 1) repeated through the slots ---- */
    float *x       = (float *)malloc(B * slots * sizeof(float));
    uint8_t *share = (uint8_t *)malloc(B * 64), *seeds = (uint8_t *)malloc(B * 64);
    for (size_t b = 0; b < B; b++)
        for (size_t i = 0; i < slots; i++)
            x[b * slots + i] = (float)((double)((((uint64_t)(i % DIM + 131 * b)) * 2654435761ull) % 2000ull) / 1000 - 1);
    fill_seeds(share, B, 1, 0);
    fill_seeds(seeds, B, 3, 128);

    /* ---- the evaluator's matrix as DIM generalised diagonals at the full scale, slot k of diagonal e = M[k mod 16][(k + e)
     * mod 16]; diagonal e = N1 g + b is entry [g][b] of the plan's [N2][N1] array, so the array is the diagonals in their
     * order ---- */
    float *diag = (float *)malloc(DIM * slots * sizeof(float));
    for (size_t e = 0; e < DIM; e++)
        for (size_t k = 0; k < slots; k++) diag[e * slots + k] = (float)matrix(k % DIM, (k + e) % DIM);

    void *d_values, *d_share, *d_seeds, *d_c0, *d_c1, *d_l0, *d_l1, *d_s0, *d_s1, *d_r0, *d_r1, *d_out, *d_status,
        *d_diag_values, *d_diag, *d_diag_status, *d_work;
    CHECK_HIP(hipMalloc(&d_values, B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, B * 64));
    CHECK_HIP(hipMalloc(&d_c0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_c1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_l0, B * lrec * 4));
    CHECK_HIP(hipMalloc(&d_l1, B * lrec * 4));
    CHECK_HIP(hipMalloc(&d_s0, B * lrec * 4));
    CHECK_HIP(hipMalloc(&d_s1, B * lrec * 4));
    CHECK_HIP(hipMalloc(&d_r0, B * low * 4));
    CHECK_HIP(hipMalloc(&d_r1, B * low * 4));
    CHECK_HIP(hipMalloc(&d_out, B * slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_status, B));
    CHECK_HIP(hipMalloc(&d_diag_values, DIM * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_diag, DIM * rec * 4));
    CHECK_HIP(hipMalloc(&d_diag_status, DIM));
    CHECK_HIP(hipMemcpy(d_values, x, B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_diag_values, diag, DIM * slots * sizeof(float), hipMemcpyHostToDevice));

    CHECK_SE(se_amd_encrypt_sym_device(ctx, (const float *)d_values, B, (const uint8_t *)d_share, (const uint8_t *)d_seeds,
                                       (uint32_t *)d_c0, (uint32_t *)d_c1, NULL, NULL, NULL, NULL));
    /* ---- the evaluator: no secret key is used from here ... ---- */
    /* once per matrix: encode the diagonals on all np rows, make the plan (it keeps the diagonals only, pre-rotated) */
    CHECK_SE(se_amd_encode_ntt_device(ctx, (const float *)d_diag_values, DIM, (uint32_t *)d_diag, NULL,
                                      (uint8_t *)d_diag_status, NULL));
    CHECK_HIP(hipDeviceSynchronize());
    se_amd_bsgs *plan;
    CHECK_SE(se_amd_bsgs_create_sp(ctx, baby, N1, giant, N2, (const uint32_t *)d_diag, nprimes, &plan));
    /* a workspace for half the batch: the call walks it in two chunks */
    const size_t work_bytes = se_amd_bsgs_workspace_bytes(plan, (B + 1) / 2, L);
    CHECK_HIP(hipMalloc(&d_work, work_bytes));
    /* per batch: drop the keys' prime, ONE baby-step / giant-step transform at the fresh scale, ONE rescale */
    CHECK_SE(se_amd_ct_drop_primes_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, B, nprimes, L,
                                          (uint32_t *)d_l0, (uint32_t *)d_l1, NULL));
    CHECK_SE(se_amd_ct_bsgs_sp_device(ctx, plan, (const uint32_t *)d_l0, (const uint32_t *)d_l1, B, L, (uint32_t *)d_s0,
                                      (uint32_t *)d_s1, d_work, work_bytes, NULL));
    CHECK_SE(se_amd_ct_rescale_device(ctx, (const uint32_t *)d_s0, (const uint32_t *)d_s1, B, L, (uint32_t *)d_r0,
                                      (uint32_t *)d_r1, NULL));
    /* ---- ... to here.  The key holder decrypts B ciphertexts of np - 2 primes. ---- */
    const double delta = se_amd_scale(ctx);
    const double scale = delta * delta / (double)q[L - 1];
    CHECK_SE(se_amd_decrypt_level_device(ctx, (const uint32_t *)d_r0, (const uint32_t *)d_r1, B, L - 1, scale, NULL, NULL,
                                         (double *)d_out, (uint8_t *)d_status, NULL));
    CHECK_HIP(hipDeviceSynchronize());
    se_amd_bsgs_destroy(plan);

    double *out     = (double *)malloc(B * slots * sizeof(double));
    uint8_t *status = (uint8_t *)malloc(B), diag_status[DIM];
    CHECK_HIP(hipMemcpy(out, d_out, B * slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(status, d_status, B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(diag_status, d_diag_status, DIM, hipMemcpyDeviceToHost));
    int failed = 0;
    for (size_t b = 0; b < B; b++) failed += status[b] != 1;
    for (size_t e = 0; e < DIM; e++) failed += diag_status[e] != 1;
    double max_err = 0.0, first = 0.0;
    for (size_t b = 0; b < B; b++)
        for (size_t i = 0; i < slots; i++)
        {
            double want = 0.0;
            for (size_t c = 0; c < DIM; c++) want += matrix(i % DIM, c) * (double)x[b * slots + c];
            if (b == 0 && i == 0) first = want;
            const double err = fabs(out[b * slots + i] - want);
            if (err > max_err) max_err = err;
        }
    printf("record 0, slot 0: (M x)[0] = %.5f (expected %.5f)\n", out[0], first);
    printf("failed=%d B=%zu n=%zu primes=%zu level=%zu dim=%d keys=%d scale=%.6e max_abs_error=%.3e\n", failed, B, n,
           nprimes, L - 1, DIM, KEYS, scale, max_err);

    CHECK_HIP(hipFree(d_values));
    CHECK_HIP(hipFree(d_share));
    CHECK_HIP(hipFree(d_seeds));
    CHECK_HIP(hipFree(d_c0));
    CHECK_HIP(hipFree(d_c1));
    CHECK_HIP(hipFree(d_l0));
    CHECK_HIP(hipFree(d_l1));
    CHECK_HIP(hipFree(d_s0));
    CHECK_HIP(hipFree(d_s1));
    CHECK_HIP(hipFree(d_r0));
    CHECK_HIP(hipFree(d_r1));
    CHECK_HIP(hipFree(d_out));
    CHECK_HIP(hipFree(d_status));
    CHECK_HIP(hipFree(d_diag_values));
    CHECK_HIP(hipFree(d_diag));
    CHECK_HIP(hipFree(d_diag_status));
    CHECK_HIP(hipFree(d_work));
    free(x), free(share), free(seeds), free(sk), free(a_seeds), free(e_seeds), free(gk0), free(gk1), free(out),
        free(status), free(diag);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
