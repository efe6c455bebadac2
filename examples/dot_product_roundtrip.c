/*
 * dot_product_roundtrip.c -- encrypted inner products: two batches of B records under one key, x_0 .. x_{B-1} and
 * y_0 .. y_{B-1}, and per group g of consecutive indices the slot-wise inner product sum_{k in g} x_k . y_k, computed on
 * ciphertexts by ONE call.  Relinearisation is linear in the degree-2 slab, so se_amd_ct_dot_sp_device sums the tensors
 * of a group and key-switches the sum once: one division by the special prime and 4 L + 2 transforms per group and prime
 * whatever the group's size, and no per-pair record in memory.
 *
 *   encrypt both batches -> se_amd_ct_drop_primes_device to np - 1 (the last prime belongs to the key)
 *   -> se_amd_ct_dot_sp_device, rows = the groups      (scale Delta^2, level np - 1)
 *   -> se_amd_ct_rescale_device                        (scale Delta^2 / q_{np-2}, level np - 2)
 *   -> se_amd_decrypt_level_device at that scale.
 * Prints the largest error over all slots of all groups.  For a single product per output see ct_product_roundtrip.c.
 *
 *   gcc examples/dot_product_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o dot_product_roundtrip
 *   ./dot_product_roundtrip 4096 3 16 4        (n, primes, records B per batch, groups G)
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
    size_t G       = argc > 4 ? (size_t)atol(argv[4]) : 4;
    /* the key reserves the last prime and the rescale spends one more */
    if (B == 0 || G == 0 || G > B || nprimes < 3 || nprimes > 13) return 2;
    const size_t slots = n / 2, rec = nprimes * n, level = nprimes - 1, low = level * n, R = nprimes - 1;
    const size_t per = (B + G - 1) / G;                              /* pairs of a group */

    se_amd_ctx *ctx;
    CHECK_SE(se_amd_create(&ctx, n, nprimes, 0));
    uint8_t *sk = (uint8_t *)malloc(n / 4);
    for (size_t i = 0; i < n / 4; i++)
    {
        uint8_t byte = 0;
        for (unsigned c = 0; c < 4; c++) byte = (uint8_t)((byte << 2) | (((4 * i + c) * 2654435761u >> 7) % 3u));
        sk[i] = byte;                                                /* 2-bit codes 0 / 1 / 2 = -1 / 0 / +1 */
    }
    CHECK_SE(se_amd_set_secret_key(ctx, sk));
    uint8_t *a_seeds = (uint8_t *)malloc(R * 64), *e_seeds = (uint8_t *)malloc(R * 64);
    for (size_t r = 0; r < R; r++)
        for (int c = 0; c < 64; c++)
        {
            a_seeds[r * 64 + c] = (uint8_t)(17 * r + c);
            e_seeds[r * 64 + c] = (uint8_t)(201 - c + 5 * r);
        }
    uint32_t *evk0 = (uint32_t *)malloc(R * rec * 4), *evk1 = (uint32_t *)malloc(R * rec * 4);
    CHECK_SE(se_amd_gen_relin_key_sp(ctx, sk, a_seeds, e_seeds, evk0, evk1));
    CHECK_SE(se_amd_set_relin_key_sp(ctx, evk0, evk1));

    /* ---- the two batches: records 0 .. B-1 are x, records B .. 2B-1 are y; slot values in [-1, 1) ---- */
    float *values     = (float *)malloc(2 * B * slots * sizeof(float));
    uint8_t *share    = (uint8_t *)malloc(2 * B * 64), *seeds = (uint8_t *)malloc(2 * B * 64);
    uint32_t *row_ptr = (uint32_t *)malloc((G + 1) * 4);
    for (size_t b = 0; b < 2 * B; b++)
    {
        for (size_t i = 0; i < slots; i++)
            values[b * slots + i] = (float)((double)((((uint64_t)(i + 7 * b)) * 2654435761ull) % 2000ull) / 1000 - 1);
        for (int c = 0; c < 64; c++)
        {
            share[b * 64 + c] = (uint8_t)(c + b);
            seeds[b * 64 + c] = (uint8_t)(255 - c + 3 * b);
        }
    }
    for (size_t g = 0; g <= G; g++) row_ptr[g] = (uint32_t)(g * per < B ? g * per : B);

    void *d_values, *d_share, *d_seeds, *d_rows, *d_c0, *d_c1, *d_l0, *d_l1, *d_r0, *d_r1, *d_f0, *d_f1, *d_out, *d_status;
    CHECK_HIP(hipMalloc(&d_values, 2 * B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, 2 * B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, 2 * B * 64));
    CHECK_HIP(hipMalloc(&d_rows, (G + 1) * 4));
    CHECK_HIP(hipMalloc(&d_c0, 2 * B * rec * 4));
    CHECK_HIP(hipMalloc(&d_c1, 2 * B * rec * 4));
    CHECK_HIP(hipMalloc(&d_l0, 2 * B * low * 4));
    CHECK_HIP(hipMalloc(&d_l1, 2 * B * low * 4));
    CHECK_HIP(hipMalloc(&d_r0, G * low * 4));
    CHECK_HIP(hipMalloc(&d_r1, G * low * 4));
    CHECK_HIP(hipMalloc(&d_f0, G * (low - n) * 4));
    CHECK_HIP(hipMalloc(&d_f1, G * (low - n) * 4));
    CHECK_HIP(hipMalloc(&d_out, G * slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_status, 2 * B + 2 * G));
    CHECK_HIP(hipMemcpy(d_values, values, 2 * B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, 2 * B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, 2 * B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_rows, row_ptr, (G + 1) * 4, hipMemcpyHostToDevice));

    CHECK_SE(se_amd_encrypt_sym_device(ctx, (const float *)d_values, 2 * B, (const uint8_t *)d_share,
                                       (const uint8_t *)d_seeds, (uint32_t *)d_c0, (uint32_t *)d_c1, NULL, NULL,
                                       (uint8_t *)d_status, NULL));
    CHECK_SE(se_amd_ct_drop_primes_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, 2 * B, nprimes, level,
                                          (uint32_t *)d_l0, (uint32_t *)d_l1, NULL));
    /* side a: records 0 .. B-1 of the dropped slabs; side b: the B records behind them; pair k is (k, k) */
    const uint32_t *xa0 = (const uint32_t *)d_l0, *xa1 = (const uint32_t *)d_l1;
    const uint32_t *yb0 = xa0 + B * low, *yb1 = xa1 + B * low;
    CHECK_SE(se_amd_ct_dot_sp_device(ctx, xa0, xa1, B, yb0, yb1, B, level, G, (const uint32_t *)d_rows, NULL, NULL, B,
                                     (uint32_t *)d_r0, (uint32_t *)d_r1, (uint8_t *)d_status + 2 * B, NULL));
    CHECK_SE(se_amd_ct_rescale_device(ctx, (const uint32_t *)d_r0, (const uint32_t *)d_r1, G, level, (uint32_t *)d_f0,
                                      (uint32_t *)d_f1, NULL));
    uint32_t q[13];
    CHECK_SE(se_amd_moduli(ctx, q));
    const double delta = se_amd_scale(ctx), scale = delta * delta / (double)q[level - 1];
    CHECK_SE(se_amd_decrypt_level_device(ctx, (const uint32_t *)d_f0, (const uint32_t *)d_f1, G, level - 1, scale, NULL,
                                         NULL, (double *)d_out, (uint8_t *)d_status + 2 * B + G, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    double *out     = (double *)malloc(G * slots * sizeof(double));
    uint8_t *status = (uint8_t *)malloc(2 * B + 2 * G);
    CHECK_HIP(hipMemcpy(out, d_out, G * slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(status, d_status, 2 * B + 2 * G, hipMemcpyDeviceToHost));
    int failed     = 0;
    double max_err = 0.0;
    for (size_t s = 0; s < 2 * B + 2 * G; s++) failed += status[s] != 1;
    for (size_t g = 0; g < G; g++)
        for (size_t i = 0; i < slots; i++)
        {
            double want = 0.0;
            for (size_t k = row_ptr[g]; k < row_ptr[g + 1]; k++)
                want += (double)values[k * slots + i] * (double)values[(B + k) * slots + i];
            const double err = fabs(out[g * slots + i] - want);
            if (err > max_err) max_err = err;
        }
    printf("group 0, slot 0: %.5f\n", out[0]);
    printf("failed=%d B=%zu n=%zu primes=%zu level=%zu groups=%zu scale=%.6e max_abs_error=%.3e\n", failed, B, n, nprimes,
           level, G, scale, max_err);

    CHECK_HIP(hipFree(d_values));
    CHECK_HIP(hipFree(d_share));
    CHECK_HIP(hipFree(d_seeds));
    CHECK_HIP(hipFree(d_rows));
    CHECK_HIP(hipFree(d_c0));
    CHECK_HIP(hipFree(d_c1));
    CHECK_HIP(hipFree(d_l0));
    CHECK_HIP(hipFree(d_l1));
    CHECK_HIP(hipFree(d_r0));
    CHECK_HIP(hipFree(d_r1));
    CHECK_HIP(hipFree(d_f0));
    CHECK_HIP(hipFree(d_f1));
    CHECK_HIP(hipFree(d_out));
    CHECK_HIP(hipFree(d_status));
    free(values), free(share), free(seeds), free(row_ptr), free(sk), free(a_seeds), free(e_seeds), free(evk0), free(evk1),
        free(out), free(status);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
