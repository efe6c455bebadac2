/*
 * batch_roundtrip.c -- values beyond one prime, there and back: a small batch of slot values around +-1000 is
 * encrypted with se_amd_encrypt_sym_device and read back with se_amd_decrypt_full_device, which recombines all primes
 * of every ciphertext on the GPU.  (At scale 2^25 such values give |m + e| ~ 2^35: every single prime of the chain
 * wraps, so se_amd_decrypt_decode_device cannot recover them.)  Prints the largest error over the batch.
 *
 *   gcc examples/batch_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o batch_roundtrip
 *   ./batch_roundtrip 4096 3 16
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
    const size_t slots = n / 2, rec = nprimes * n;

    se_amd_ctx *ctx;
    CHECK_SE(se_amd_create(&ctx, n, nprimes, 0));
    uint8_t *sk = (uint8_t *)calloc(n / 4, 1);                 /* 2-bit packed, codes 0 / 1 / 2 = -1 / 0 / +1 */
    for (size_t i = 0; i < n / 4; i++) sk[i] = (uint8_t)(((i * 37u) % 3u) * 0x55u);
    CHECK_SE(se_amd_set_secret_key(ctx, sk));

    float *values  = (float *)malloc(B * slots * sizeof(float));
    uint8_t *share = (uint8_t *)malloc(B * 64), *seeds = (uint8_t *)malloc(B * 64);
    for (size_t b = 0; b < B; b++)
    {
        for (size_t i = 0; i < slots; i++)   /* [-1000, 1000) in steps of 0.01 */
            values[b * slots + i] = (float)((double)((((uint64_t)(i + b)) * 2654435761ull) % 200000ull) / 100 - 1000);
        for (int k = 0; k < 64; k++)
        {
            share[b * 64 + k] = (uint8_t)(k + b);
            seeds[b * 64 + k] = (uint8_t)(255 - k + 3 * b);
        }
    }

    void *d_values, *d_share, *d_seeds, *d_c0, *d_c1, *d_out, *d_enc_status, *d_status;
    CHECK_HIP(hipMalloc(&d_values, B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, B * 64));
    CHECK_HIP(hipMalloc(&d_c0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_c1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_out, B * slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_enc_status, B));
    CHECK_HIP(hipMalloc(&d_status, B));
    CHECK_HIP(hipMemcpy(d_values, values, B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, B * 64, hipMemcpyHostToDevice));

    CHECK_SE(se_amd_encrypt_sym_device(ctx, (const float *)d_values, B, (const uint8_t *)d_share,
                                       (const uint8_t *)d_seeds, (uint32_t *)d_c0, (uint32_t *)d_c1, NULL, NULL,
                                       (uint8_t *)d_enc_status, NULL));
    CHECK_SE(se_amd_decrypt_full_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, B, NULL, NULL,
                                        (double *)d_out, (uint8_t *)d_status, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    double *out     = (double *)malloc(B * slots * sizeof(double));
    uint8_t *status = (uint8_t *)malloc(B), *enc_status = (uint8_t *)malloc(B);
    CHECK_HIP(hipMemcpy(out, d_out, B * slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(status, d_status, B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(enc_status, d_enc_status, B, hipMemcpyDeviceToHost));
    int failed     = 0;
    double max_err = 0.0;
    for (size_t b = 0; b < B; b++)
    {
        if (enc_status[b] != 1 || status[b] != 1)
        {
            failed++;
            continue;
        }
        for (size_t i = 0; i < slots; i++)
        {
            const double err = fabs(out[b * slots + i] - (double)values[b * slots + i]);
            if (err > max_err) max_err = err;
        }
    }
    printf("failed=%d B=%zu n=%zu primes=%zu max_abs_error=%.3e\n", failed, B, n, nprimes, max_err);

    CHECK_HIP(hipFree(d_values));
    CHECK_HIP(hipFree(d_share));
    CHECK_HIP(hipFree(d_seeds));
    CHECK_HIP(hipFree(d_c0));
    CHECK_HIP(hipFree(d_c1));
    CHECK_HIP(hipFree(d_out));
    CHECK_HIP(hipFree(d_enc_status));
    CHECK_HIP(hipFree(d_status));
    free(values), free(share), free(seeds), free(sk), free(out), free(status), free(enc_status);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
