/*
 * rotate_fresh_roundtrip.c -- ONE rotation of fresh records at their own scale: B devices encrypt one record each, an
 * evaluator that holds the public special-prime Galois key of one step but NO secret key rotates every record by that
 * step, and the key holder decrypts at the SAME scale.  No lift, no rescale, no level spent on the rotation.
 *
 * The last prime of the context belongs to the key, so a fresh record (np primes) is first dropped to np - 1 primes by
 * se_amd_ct_drop_primes_device, which changes neither message nor scale; se_amd_ct_galois_sp_device rotates it with the
 * key of se_amd_gen_galois_keys_sp / se_amd_set_galois_keys_sp; se_amd_decrypt_level_device decodes np - 1 primes at the
 * context's scale.  Prints the largest error over all slots against the rolled values.
 *
 *   gcc examples/rotate_fresh_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o rotate_fresh_roundtrip
 *   ./rotate_fresh_roundtrip 4096 3 8 1
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
    size_t B       = argc > 3 ? (size_t)atol(argv[3]) : 8;
    long step      = argc > 4 ? atol(argv[4]) : 1;
    if (B == 0 || nprimes < 2 || nprimes > 13) return 2;   /* the key switch reserves the last prime */
    const size_t slots = n / 2, rec = nprimes * n, level = nprimes - 1, low = level * n, R = nprimes - 1;

    /* ---- the key holder: one secret key, the Galois key of the step (public material, handed to the evaluator) ---- */
    se_amd_ctx *ctx;
    CHECK_SE(se_amd_create(&ctx, n, nprimes, 0));
    uint8_t *sk = (uint8_t *)calloc(n / 4, 1);                 /* 2-bit packed, codes 0 / 1 / 2 = -1 / 0 / +1 */
    for (size_t i = 0; i < n / 4; i++) sk[i] = (uint8_t)(((i * 37u) % 3u) * 0x55u);
    CHECK_SE(se_amd_set_secret_key(ctx, sk));
    uint32_t elt;
    CHECK_SE(se_amd_galois_element(n, step, &elt));
    uint8_t *a_seeds = (uint8_t *)malloc(R * 64), *e_seeds = (uint8_t *)malloc(R * 64);
    for (size_t r = 0; r < R; r++)
        for (int k = 0; k < 64; k++)
        {
            a_seeds[r * 64 + k] = (uint8_t)(17 * r + k);
            e_seeds[r * 64 + k] = (uint8_t)(201 - k + 5 * r);
        }
    uint32_t *gk0 = (uint32_t *)malloc(R * rec * 4), *gk1 = (uint32_t *)malloc(R * rec * 4);
    CHECK_SE(se_amd_gen_galois_keys_sp(ctx, sk, &elt, 1, a_seeds, e_seeds, gk0, gk1));
    CHECK_SE(se_amd_set_galois_keys_sp(ctx, &elt, 1, gk0, gk1));

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

    void *d_values, *d_share, *d_seeds, *d_c0, *d_c1, *d_l0, *d_l1, *d_r0, *d_r1, *d_out, *d_status;
    CHECK_HIP(hipMalloc(&d_values, B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, B * 64));
    CHECK_HIP(hipMalloc(&d_c0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_c1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_l0, B * low * 4));
    CHECK_HIP(hipMalloc(&d_l1, B * low * 4));
    CHECK_HIP(hipMalloc(&d_r0, B * low * 4));
    CHECK_HIP(hipMalloc(&d_r1, B * low * 4));
    CHECK_HIP(hipMalloc(&d_out, B * slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_status, B));
    CHECK_HIP(hipMemcpy(d_values, values, B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, B * 64, hipMemcpyHostToDevice));

    CHECK_SE(se_amd_encrypt_sym_device(ctx, (const float *)d_values, B, (const uint8_t *)d_share,
                                       (const uint8_t *)d_seeds, (uint32_t *)d_c0, (uint32_t *)d_c1, NULL, NULL, NULL,
                                       NULL));
    /* ---- the evaluator: no secret key is used from here ... ---- */
    CHECK_SE(se_amd_ct_drop_primes_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, B, nprimes, level,
                                          (uint32_t *)d_l0, (uint32_t *)d_l1, NULL));
    CHECK_SE(se_amd_ct_galois_sp_device(ctx, (const uint32_t *)d_l0, (const uint32_t *)d_l1, B, level, elt,
                                        (uint32_t *)d_r0, (uint32_t *)d_r1, NULL));
    /* ---- ... to here.  The key holder decrypts np - 1 primes at the scale the records were encrypted at. ---- */
    const double scale = se_amd_scale(ctx);
    CHECK_SE(se_amd_decrypt_level_device(ctx, (const uint32_t *)d_r0, (const uint32_t *)d_r1, B, level, scale, NULL, NULL,
                                         (double *)d_out, (uint8_t *)d_status, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    double *out     = (double *)malloc(B * slots * sizeof(double));
    uint8_t *status = (uint8_t *)malloc(B);
    CHECK_HIP(hipMemcpy(out, d_out, B * slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(status, d_status, B, hipMemcpyDeviceToHost));
    int failed     = 0;
    double max_err = 0.0;
    const long half = (long)slots;
    for (size_t b = 0; b < B; b++)
    {
        failed += status[b] != 1;
        for (long i = 0; i < half; i++)
        {
            const long from  = (((i + step) % half) + half) % half;   /* a left rotation by `step` */
            const double err = fabs(out[b * slots + (size_t)i] - (double)values[b * slots + (size_t)from]);
            if (err > max_err) max_err = err;
        }
    }
    printf("record 0, slot 0: %.5f (expected %.5f)\n", out[0], (double)values[(size_t)(((step % half) + half) % half)]);
    printf("failed=%d B=%zu n=%zu primes=%zu level=%zu step=%ld scale=%.6e max_abs_error=%.3e\n", failed, B, n, nprimes,
           level, step, scale, max_err);

    CHECK_HIP(hipFree(d_values));
    CHECK_HIP(hipFree(d_share));
    CHECK_HIP(hipFree(d_seeds));
    CHECK_HIP(hipFree(d_c0));
    CHECK_HIP(hipFree(d_c1));
    CHECK_HIP(hipFree(d_l0));
    CHECK_HIP(hipFree(d_l1));
    CHECK_HIP(hipFree(d_r0));
    CHECK_HIP(hipFree(d_r1));
    CHECK_HIP(hipFree(d_out));
    CHECK_HIP(hipFree(d_status));
    free(values), free(share), free(seeds), free(sk), free(a_seeds), free(e_seeds), free(gk0), free(gk1), free(out),
        free(status);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
