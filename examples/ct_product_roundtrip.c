/*
 * ct_product_roundtrip.c -- a product of ciphertexts on the machine in the middle: B devices encrypt one record each, an
 * evaluator that holds the public relinearisation key but NO secret key squares every record slot by slot, adds the
 * squares and hands the sum on one level lower, and the key holder decrypts at that level: sum_b v_b^2 per slot (the
 * energy of the batch; with a mean beside it, its variance).
 *
 * se_amd_ct_mul_device with the same slabs on both sides gives the degree-2 form (d0, d1, d2) of every square at scale
 * Delta^2; se_amd_ct_relin_device brings it back to two slabs (same scale, same level); se_amd_ct_lincomb_device adds the
 * records (unit weights, one group); se_amd_ct_rescale_device drops the last prime and divides the scale by it.  The
 * result is a ciphertext of primes - 1 primes at Delta^2 / q_last, which se_amd_decrypt_level_device decodes.  Prints the
 * largest error over all slots against sum_b v_b^2.
 *
 *   gcc examples/ct_product_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o ct_product_roundtrip
 *   ./ct_product_roundtrip 4096 3 16
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

int main(int argc, char **argv)
{
    size_t n       = argc > 1 ? (size_t)atol(argv[1]) : 4096;
    size_t nprimes = argc > 2 ? (size_t)atol(argv[2]) : 3;
    size_t B       = argc > 3 ? (size_t)atol(argv[3]) : 16;
    const size_t slots = n / 2, rec = nprimes * n, low = (nprimes - 1) * n, R = 2 * nprimes;
    if (B == 0 || nprimes < 2 || nprimes > 13) return 2;   /* the rescale needs a prime to drop */

    /* ---- the key holder: one secret key, its relinearisation key (public material, handed to the evaluator) ---- */
    se_amd_ctx *ctx;
    CHECK_SE(se_amd_create(&ctx, n, nprimes, 0));
    uint8_t *sk = (uint8_t *)calloc(n / 4, 1);                 /* 2-bit packed, codes 0 / 1 / 2 = -1 / 0 / +1 */
    for (size_t i = 0; i < n / 4; i++) sk[i] = (uint8_t)(((i * 37u) % 3u) * 0x55u);
    CHECK_SE(se_amd_set_secret_key(ctx, sk));
    uint32_t q[13];
    CHECK_SE(se_amd_moduli(ctx, q));
    uint8_t *a_seeds = (uint8_t *)malloc(R * 64), *e_seeds = (uint8_t *)malloc(R * 64);
    for (size_t r = 0; r < R; r++)
        for (int k = 0; k < 64; k++)
        {
            a_seeds[r * 64 + k] = (uint8_t)(17 * r + k);
            e_seeds[r * 64 + k] = (uint8_t)(201 - k + 5 * r);
        }
    uint32_t *evk0 = (uint32_t *)malloc(R * rec * 4), *evk1 = (uint32_t *)malloc(R * rec * 4);
    CHECK_SE(se_amd_gen_relin_key(ctx, sk, a_seeds, e_seeds, evk0, evk1));
    CHECK_SE(se_amd_set_relin_key(ctx, evk0, evk1));

    /* ---- the devices: B records of slot values in [-1, 1) ---- */
    float *values  = (float *)malloc(B * slots * sizeof(float));
    uint8_t *share = (uint8_t *)malloc(B * 64), *seeds = (uint8_t *)malloc(B * 64);
    for (size_t b = 0; b < B; b++)
    {
        for (size_t i = 0; i < slots; i++)
            values[b * slots + i] = (float)((double)((((uint64_t)(i + b)) * 2654435761ull) % 2000ull) / 1000 - 1);
        for (int k = 0; k < 64; k++)
        {
            share[b * 64 + k] = (uint8_t)(k + b);
            seeds[b * 64 + k] = (uint8_t)(255 - k + 3 * b);
        }
    }

    void *d_values, *d_share, *d_seeds, *d_c0, *d_c1, *d_t0, *d_t1, *d_t2, *d_m0, *d_m1, *d_s0, *d_s1, *d_r0, *d_r1,
        *d_out, *d_mul_status, *d_agg_status, *d_status;
    CHECK_HIP(hipMalloc(&d_values, B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, B * 64));
    CHECK_HIP(hipMalloc(&d_c0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_c1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_t0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_t1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_t2, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_m0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_m1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_s0, rec * 4));
    CHECK_HIP(hipMalloc(&d_s1, rec * 4));
    CHECK_HIP(hipMalloc(&d_r0, low * 4));
    CHECK_HIP(hipMalloc(&d_r1, low * 4));
    CHECK_HIP(hipMalloc(&d_out, slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_mul_status, B));
    CHECK_HIP(hipMalloc(&d_agg_status, 1));
    CHECK_HIP(hipMalloc(&d_status, 1));
    CHECK_HIP(hipMemcpy(d_values, values, B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, B * 64, hipMemcpyHostToDevice));

    CHECK_SE(se_amd_encrypt_sym_device(ctx, (const float *)d_values, B, (const uint8_t *)d_share,
                                       (const uint8_t *)d_seeds, (uint32_t *)d_c0, (uint32_t *)d_c1, NULL, NULL, NULL,
                                       NULL));
    /* ---- the evaluator: no secret key is used from here ... ---- */
    CHECK_SE(se_amd_ct_mul_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, B, (const uint32_t *)d_c0,
                                  (const uint32_t *)d_c1, B, nprimes, B, NULL, NULL, (uint32_t *)d_t0, (uint32_t *)d_t1,
                                  (uint32_t *)d_t2, (uint8_t *)d_mul_status, NULL));
    CHECK_SE(se_amd_ct_relin_device(ctx, (const uint32_t *)d_t0, (const uint32_t *)d_t1, (const uint32_t *)d_t2, B,
                                    nprimes, (uint32_t *)d_m0, (uint32_t *)d_m1, NULL));
    CHECK_SE(se_amd_ct_lincomb_device(ctx, (const uint32_t *)d_m0, (const uint32_t *)d_m1, B, 1, NULL, NULL, NULL, B,
                                      (uint32_t *)d_s0, (uint32_t *)d_s1, (uint8_t *)d_agg_status, NULL));
    CHECK_SE(se_amd_ct_rescale_device(ctx, (const uint32_t *)d_s0, (const uint32_t *)d_s1, 1, nprimes, (uint32_t *)d_r0,
                                      (uint32_t *)d_r1, NULL));
    /* ---- ... to here.  The key holder decrypts one ciphertext of primes - 1 primes at Delta^2 / q_last. ---- */
    const double scale = se_amd_scale(ctx) * se_amd_scale(ctx) / (double)q[nprimes - 1];
    CHECK_SE(se_amd_decrypt_level_device(ctx, (const uint32_t *)d_r0, (const uint32_t *)d_r1, 1, nprimes - 1, scale, NULL,
                                         NULL, (double *)d_out, (uint8_t *)d_status, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    double *out         = (double *)malloc(slots * sizeof(double));
    uint8_t *mul_status = (uint8_t *)malloc(B), agg_status, status;
    CHECK_HIP(hipMemcpy(out, d_out, slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(mul_status, d_mul_status, B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(&agg_status, d_agg_status, 1, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(&status, d_status, 1, hipMemcpyDeviceToHost));
    int failed = (agg_status != 1) + (status != 1);
    for (size_t b = 0; b < B; b++) failed += mul_status[b] != 1;
    double max_err = 0.0, first = 0.0;
    for (size_t i = 0; i < slots; i++)
    {
        double want = 0.0;
        for (size_t b = 0; b < B; b++) want += (double)values[b * slots + i] * (double)values[b * slots + i];
        if (i == 0) first = want;
        const double err = fabs(out[i] - want);
        if (err > max_err) max_err = err;
    }
    printf("slot 0: sum of squares %.5f (expected %.5f)\n", out[0], first);
    printf("failed=%d B=%zu n=%zu primes=%zu level=%zu scale=%.6e max_abs_error=%.3e\n", failed, B, n, nprimes,
           nprimes - 1, scale, max_err);

    CHECK_HIP(hipFree(d_values));
    CHECK_HIP(hipFree(d_share));
    CHECK_HIP(hipFree(d_seeds));
    CHECK_HIP(hipFree(d_c0));
    CHECK_HIP(hipFree(d_c1));
    CHECK_HIP(hipFree(d_t0));
    CHECK_HIP(hipFree(d_t1));
    CHECK_HIP(hipFree(d_t2));
    CHECK_HIP(hipFree(d_m0));
    CHECK_HIP(hipFree(d_m1));
    CHECK_HIP(hipFree(d_s0));
    CHECK_HIP(hipFree(d_s1));
    CHECK_HIP(hipFree(d_r0));
    CHECK_HIP(hipFree(d_r1));
    CHECK_HIP(hipFree(d_out));
    CHECK_HIP(hipFree(d_mul_status));
    CHECK_HIP(hipFree(d_agg_status));
    CHECK_HIP(hipFree(d_status));
    free(values), free(share), free(seeds), free(sk), free(a_seeds), free(e_seeds), free(evk0), free(evk1), free(out),
        free(mul_status);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
