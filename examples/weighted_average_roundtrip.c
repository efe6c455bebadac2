/*
 * weighted_average_roundtrip.c -- real-valued weights on the machine in the middle: B devices encrypt one record each,
 * an aggregator that holds no key forms G weighted sums with real weights w in [-1, 1] and hands them on one level
 * lower, and the key holder decrypts at that level.
 *
 * A real weight w is applied as the integer round(w . 2^30) (se_amd_ct_lincomb_device), which multiplies the CKKS scale
 * by 2^30; se_amd_ct_rescale_device then drops the last prime and divides the scale by it.  The result is a ciphertext
 * of primes - 1 primes at scale . 2^30 / q_last, which se_amd_decrypt_level_device decodes.  Group g = the records b
 * with b % G == g.  Prints the largest error over all slots against sum_k (round(w_k . 2^30) / 2^30) . v_k.
 *
 *   gcc examples/weighted_average_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o weighted_average_roundtrip
 *   ./weighted_average_roundtrip 4096 3 16
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

#define WEIGHT_BITS 30

int main(int argc, char **argv)
{
    size_t n       = argc > 1 ? (size_t)atol(argv[1]) : 4096;
    size_t nprimes = argc > 2 ? (size_t)atol(argv[2]) : 3;
    size_t B       = argc > 3 ? (size_t)atol(argv[3]) : 16;
    size_t G       = argc > 4 ? (size_t)atol(argv[4]) : 2;
    const size_t slots = n / 2, rec = nprimes * n, low = (nprimes - 1) * n;
    if (G == 0 || B == 0 || nprimes < 2 || nprimes > 13) return 2;   /* the rescale needs a prime to drop */

    /* ---- the devices: one key, B records of slot values in [-10, 10) ---- */
    se_amd_ctx *ctx;
    CHECK_SE(se_amd_create(&ctx, n, nprimes, 0));
    uint8_t *sk = (uint8_t *)calloc(n / 4, 1);                 /* 2-bit packed, codes 0 / 1 / 2 = -1 / 0 / +1 */
    for (size_t i = 0; i < n / 4; i++) sk[i] = (uint8_t)(((i * 37u) % 3u) * 0x55u);
    CHECK_SE(se_amd_set_secret_key(ctx, sk));
    uint32_t q[13];
    CHECK_SE(se_amd_moduli(ctx, q));

    float *values  = (float *)malloc(B * slots * sizeof(float));
    uint8_t *share = (uint8_t *)malloc(B * 64), *seeds = (uint8_t *)malloc(B * 64);
    for (size_t b = 0; b < B; b++)
    {
        for (size_t i = 0; i < slots; i++)
            values[b * slots + i] = (float)((double)((((uint64_t)(i + b)) * 2654435761ull) % 2000ull) / 100 - 10);
        for (int k = 0; k < 64; k++)
        {
            share[b * 64 + k] = (uint8_t)(k + b);
            seeds[b * 64 + k] = (uint8_t)(255 - k + 3 * b);
        }
    }

    /* ---- the aggregator's entry list in CSR form: row g = the records b with b % G == g; record b has the real
     *      weight wreal[b] in [-1, 1], handed to the entry as round(wreal . 2^30) ---- */
    uint32_t *row_ptr = (uint32_t *)malloc((G + 1) * sizeof(uint32_t)), *idx = (uint32_t *)malloc(B * sizeof(uint32_t));
    int32_t *w        = (int32_t *)malloc(B * sizeof(int32_t));
    double *wapplied  = (double *)malloc(B * sizeof(double));   /* the weight the integer stands for */
    size_t k = 0;
    for (size_t g = 0; g < G; g++)
    {
        row_ptr[g] = (uint32_t)k;
        for (size_t b = g; b < B; b += G)
        {
            const double wreal = (double)((b * 2246822519ull) % 20001ull) / 10000.0 - 1.0;
            idx[k]             = (uint32_t)b;
            w[k]               = (int32_t)lround(ldexp(wreal, WEIGHT_BITS));
            wapplied[b]        = ldexp((double)w[k], -WEIGHT_BITS);
            k++;
        }
    }
    row_ptr[G] = (uint32_t)k;

    void *d_values, *d_share, *d_seeds, *d_c0, *d_c1, *d_s0, *d_s1, *d_r0, *d_r1, *d_row_ptr, *d_idx, *d_w, *d_out,
        *d_agg_status, *d_status;
    CHECK_HIP(hipMalloc(&d_values, B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, B * 64));
    CHECK_HIP(hipMalloc(&d_c0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_c1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_s0, G * rec * 4));
    CHECK_HIP(hipMalloc(&d_s1, G * rec * 4));
    CHECK_HIP(hipMalloc(&d_r0, G * low * 4));
    CHECK_HIP(hipMalloc(&d_r1, G * low * 4));
    CHECK_HIP(hipMalloc(&d_row_ptr, (G + 1) * sizeof(uint32_t)));
    CHECK_HIP(hipMalloc(&d_idx, B * sizeof(uint32_t)));
    CHECK_HIP(hipMalloc(&d_w, B * sizeof(int32_t)));
    CHECK_HIP(hipMalloc(&d_out, G * slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_agg_status, G));
    CHECK_HIP(hipMalloc(&d_status, G));
    CHECK_HIP(hipMemcpy(d_values, values, B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_row_ptr, row_ptr, (G + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_idx, idx, B * sizeof(uint32_t), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_w, w, B * sizeof(int32_t), hipMemcpyHostToDevice));

    CHECK_SE(se_amd_encrypt_sym_device(ctx, (const float *)d_values, B, (const uint8_t *)d_share,
                                       (const uint8_t *)d_seeds, (uint32_t *)d_c0, (uint32_t *)d_c1, NULL, NULL, NULL,
                                       NULL));
    /* ---- the aggregator: no key is used from here ... ---- */
    CHECK_SE(se_amd_ct_lincomb_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, B, G,
                                      (const uint32_t *)d_row_ptr, (const uint32_t *)d_idx, (const int32_t *)d_w, B,
                                      (uint32_t *)d_s0, (uint32_t *)d_s1, (uint8_t *)d_agg_status, NULL));
    CHECK_SE(se_amd_ct_rescale_device(ctx, (const uint32_t *)d_s0, (const uint32_t *)d_s1, G, nprimes, (uint32_t *)d_r0,
                                      (uint32_t *)d_r1, NULL));
    /* ---- ... to here.  The key holder decrypts G ciphertexts of primes - 1 primes at the scale the two steps left. ---- */
    const double scale = ldexp(se_amd_scale(ctx), WEIGHT_BITS) / (double)q[nprimes - 1];
    CHECK_SE(se_amd_decrypt_level_device(ctx, (const uint32_t *)d_r0, (const uint32_t *)d_r1, G, nprimes - 1, scale, NULL,
                                         NULL, (double *)d_out, (uint8_t *)d_status, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    double *out     = (double *)malloc(G * slots * sizeof(double));
    uint8_t *status = (uint8_t *)malloc(G), *agg_status = (uint8_t *)malloc(G);
    CHECK_HIP(hipMemcpy(out, d_out, G * slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(status, d_status, G, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(agg_status, d_agg_status, G, hipMemcpyDeviceToHost));
    int failed     = 0;
    double max_err = 0.0;
    for (size_t g = 0; g < G; g++)
    {
        if (agg_status[g] != 1 || status[g] != 1)
        {
            failed++;
            continue;
        }
        double first = 0.0;
        for (size_t i = 0; i < slots; i++)
        {
            double want = 0.0;
            for (size_t b = g; b < B; b += G) want += wapplied[b] * (double)values[b * slots + i];
            if (i == 0) first = want;
            const double err = fabs(out[g * slots + i] - want);
            if (err > max_err) max_err = err;
        }
        printf("group %zu: %u records, slot 0 weighted sum %.4f (expected %.4f)\n", g, row_ptr[g + 1] - row_ptr[g],
               out[g * slots], first);
    }
    printf("failed=%d B=%zu G=%zu n=%zu primes=%zu level=%zu scale=%.6e max_abs_error=%.3e\n", failed, B, G, n, nprimes,
           nprimes - 1, scale, max_err);

    CHECK_HIP(hipFree(d_values));
    CHECK_HIP(hipFree(d_share));
    CHECK_HIP(hipFree(d_seeds));
    CHECK_HIP(hipFree(d_c0));
    CHECK_HIP(hipFree(d_c1));
    CHECK_HIP(hipFree(d_s0));
    CHECK_HIP(hipFree(d_s1));
    CHECK_HIP(hipFree(d_r0));
    CHECK_HIP(hipFree(d_r1));
    CHECK_HIP(hipFree(d_row_ptr));
    CHECK_HIP(hipFree(d_idx));
    CHECK_HIP(hipFree(d_w));
    CHECK_HIP(hipFree(d_out));
    CHECK_HIP(hipFree(d_agg_status));
    CHECK_HIP(hipFree(d_status));
    free(values), free(share), free(seeds), free(sk), free(row_ptr), free(idx), free(w), free(wapplied), free(out),
        free(status), free(agg_status);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
