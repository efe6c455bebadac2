/*
 * moving_sum_roundtrip.c -- a moving window on the machine in the middle: a sender encrypts B records, and an evaluator
 * that holds seven Galois keys but NO secret key replaces every slot by the sum of itself and its seven right-hand
 * neighbours, in ONE call.  The key holder decrypts one level lower: slot i of record b holds the sum of the slots
 * i .. i + 7 (indices mod n/2) of the sender's record b.
 *
 * A rotation belongs at a raised scale (there is no special prime), so the fresh records are
 * first lifted by se_amd_ct_lincomb_device with the single weight 2^30.  se_amd_ct_galois_sum_device with the elements
 * of the steps 1 .. 7 and add_input = 1 then gives record + sum of its seven rotations: the digits of c1 are decomposed
 * and transformed once, every step costs a permutation and a multiply-accumulate.
 * se_amd_ct_rescale_device drops the last prime, se_amd_decrypt_level_device decodes at Delta 2^30 / q_last.  Prints the
 * largest error over all slots.
 *
 *   gcc examples/moving_sum_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o moving_sum_roundtrip
 *   ./moving_sum_roundtrip 4096 3 8
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

#define WINDOW 8            /* slots of the window: the record and its rotations by 1 .. 7 */
#define STEPS (WINDOW - 1)
#define LIFT (1 << 30)

static void fill_seeds(uint8_t *s, size_t count, unsigned mul, unsigned add)
{
    for (size_t r = 0; r < count; r++)
        for (int k = 0; k < 64; k++) s[r * 64 + k] = (uint8_t)(mul * r + add + k);
}

int main(int argc, char **argv)
{
    size_t n       = argc > 1 ? (size_t)atol(argv[1]) : 4096;
    size_t nprimes = argc > 2 ? (size_t)atol(argv[2]) : 3;
    size_t B       = argc > 3 ? (size_t)atol(argv[3]) : 8;
    const size_t slots = n / 2, rec = nprimes * n, low = (nprimes - 1) * n, R = 2 * nprimes;
    if (B == 0 || nprimes < 2 || nprimes > 13) return 2;   /* the rescale needs a prime to drop */

    /* ---- the key holder: one secret key; the Galois keys of the seven steps are public material, handed to the
     * evaluator ---- */
    se_amd_ctx *ctx;
    CHECK_SE(se_amd_create(&ctx, n, nprimes, 0));
    uint8_t *sk = (uint8_t *)calloc(n / 4, 1);                 /* 2-bit packed, codes 0 / 1 / 2 = -1 / 0 / +1 */
    for (size_t i = 0; i < n / 4; i++) sk[i] = (uint8_t)(((i * 37u) % 3u) * 0x55u);
    CHECK_SE(se_amd_set_secret_key(ctx, sk));
    uint32_t q[13];
    CHECK_SE(se_amd_moduli(ctx, q));
    uint32_t elts[STEPS];
    for (int s = 0; s < STEPS; s++) CHECK_SE(se_amd_galois_element(n, s + 1, &elts[s]));
    uint8_t *a_seeds = (uint8_t *)malloc(STEPS * R * 64), *e_seeds = (uint8_t *)malloc(STEPS * R * 64);
    fill_seeds(a_seeds, STEPS * R, 29, 3);
    fill_seeds(e_seeds, STEPS * R, 11, 77);
    uint32_t *gk0 = (uint32_t *)malloc(STEPS * R * rec * 4), *gk1 = (uint32_t *)malloc(STEPS * R * rec * 4);
    CHECK_SE(se_amd_gen_galois_keys(ctx, sk, elts, STEPS, a_seeds, e_seeds, gk0, gk1));
    CHECK_SE(se_amd_set_galois_keys(ctx, elts, STEPS, gk0, gk1));

    /* ---- the sender: B records, slot values in [-1, 1) ---- */
    float *x       = (float *)malloc(B * slots * sizeof(float));
    uint8_t *share = (uint8_t *)malloc(B * 64), *seeds = (uint8_t *)malloc(B * 64);
    for (size_t b = 0; b < B; b++)
        for (size_t i = 0; i < slots; i++)
            x[b * slots + i] = (float)((double)((((uint64_t)(i + 131 * b)) * 2654435761ull) % 2000ull) / 1000 - 1);
    fill_seeds(share, B, 1, 0);
    fill_seeds(seeds, B, 3, 128);

    /* the lift: output row b = 2^30 . record b */
    uint32_t *row_ptr = (uint32_t *)malloc((B + 1) * 4), *idx = (uint32_t *)malloc(B * 4);
    int32_t *w        = (int32_t *)malloc(B * 4);
    for (size_t b = 0; b <= B; b++) row_ptr[b] = (uint32_t)b;
    for (size_t b = 0; b < B; b++) idx[b] = (uint32_t)b, w[b] = LIFT;

    void *d_values, *d_share, *d_seeds, *d_c0, *d_c1, *d_l0, *d_l1, *d_s0, *d_s1, *d_r0, *d_r1, *d_out, *d_row_ptr, *d_idx,
        *d_w, *d_lift_status, *d_status;
    CHECK_HIP(hipMalloc(&d_values, B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, B * 64));
    CHECK_HIP(hipMalloc(&d_c0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_c1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_l0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_l1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_s0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_s1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_r0, B * low * 4));
    CHECK_HIP(hipMalloc(&d_r1, B * low * 4));
    CHECK_HIP(hipMalloc(&d_out, B * slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_row_ptr, (B + 1) * 4));
    CHECK_HIP(hipMalloc(&d_idx, B * 4));
    CHECK_HIP(hipMalloc(&d_w, B * 4));
    CHECK_HIP(hipMalloc(&d_lift_status, B));
    CHECK_HIP(hipMalloc(&d_status, B));
    CHECK_HIP(hipMemcpy(d_values, x, B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_row_ptr, row_ptr, (B + 1) * 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_idx, idx, B * 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_w, w, B * 4, hipMemcpyHostToDevice));

    CHECK_SE(se_amd_encrypt_sym_device(ctx, (const float *)d_values, B, (const uint8_t *)d_share, (const uint8_t *)d_seeds,
                                       (uint32_t *)d_c0, (uint32_t *)d_c1, NULL, NULL, NULL, NULL));
    /* ---- the evaluator: no secret key is used from here ... ---- */
    CHECK_SE(se_amd_ct_lincomb_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, B, B, (const uint32_t *)d_row_ptr,
                                      (const uint32_t *)d_idx, (const int32_t *)d_w, B, (uint32_t *)d_l0, (uint32_t *)d_l1,
                                      (uint8_t *)d_lift_status, NULL));
    CHECK_SE(se_amd_ct_galois_sum_device(ctx, (const uint32_t *)d_l0, (const uint32_t *)d_l1, B, nprimes, elts, STEPS,
                                         /*add_input*/ 1, (uint32_t *)d_s0, (uint32_t *)d_s1, NULL));
    CHECK_SE(se_amd_ct_rescale_device(ctx, (const uint32_t *)d_s0, (const uint32_t *)d_s1, B, nprimes, (uint32_t *)d_r0,
                                      (uint32_t *)d_r1, NULL));
    /* ---- ... to here.  The key holder decrypts B ciphertexts of primes - 1 primes at Delta 2^30 / q_last. ---- */
    const double scale = se_amd_scale(ctx) * (double)LIFT / (double)q[nprimes - 1];
    CHECK_SE(se_amd_decrypt_level_device(ctx, (const uint32_t *)d_r0, (const uint32_t *)d_r1, B, nprimes - 1, scale, NULL,
                                         NULL, (double *)d_out, (uint8_t *)d_status, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    double *out          = (double *)malloc(B * slots * sizeof(double));
    uint8_t *lift_status = (uint8_t *)malloc(B), *status = (uint8_t *)malloc(B);
    CHECK_HIP(hipMemcpy(out, d_out, B * slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(lift_status, d_lift_status, B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(status, d_status, B, hipMemcpyDeviceToHost));
    int failed = 0;
    for (size_t b = 0; b < B; b++) failed += (lift_status[b] != 1) + (status[b] != 1);
    double max_err = 0.0, first = 0.0;
    for (size_t b = 0; b < B; b++)
        for (size_t i = 0; i < slots; i++)
        {
            double want = 0.0;
            for (size_t s = 0; s < WINDOW; s++) want += (double)x[b * slots + (i + s) % slots];
            if (b == 0 && i == 0) first = want;
            const double err = fabs(out[b * slots + i] - want);
            if (err > max_err) max_err = err;
        }
    printf("record 0, slot 0: moving sum %.5f (expected %.5f)\n", out[0], first);
    printf("failed=%d B=%zu n=%zu primes=%zu level=%zu window=%d scale=%.6e max_abs_error=%.3e\n", failed, B, n, nprimes,
           nprimes - 1, WINDOW, scale, max_err);

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
    CHECK_HIP(hipFree(d_row_ptr));
    CHECK_HIP(hipFree(d_idx));
    CHECK_HIP(hipFree(d_w));
    CHECK_HIP(hipFree(d_lift_status));
    CHECK_HIP(hipFree(d_status));
    free(x), free(share), free(seeds), free(sk), free(a_seeds), free(e_seeds), free(gk0), free(gk1), free(row_ptr),
        free(idx), free(w), free(out), free(lift_status), free(status);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
