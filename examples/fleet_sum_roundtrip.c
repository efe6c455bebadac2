/*
 * fleet_sum_roundtrip.c -- sums over a fleet whose devices hold DIFFERENT keys: B devices encrypt one record each under
 * one of K device keys, an evaluator that holds only the public switch-key ring brings every record under the
 * aggregator's key and adds the records of each group in ONE call, and the aggregator decrypts the group sums with its
 * own key alone, at the scale the records were encrypted at.  No lift, no rescale, no level spent.
 *
 * Three roles.  The AUTHORITY issued the K device keys and the aggregator key; it alone can run
 * se_amd_gen_switch_keys_sp, which needs both secrets, and hands the result -- public material -- to the evaluator.  The
 * EVALUATOR installs the ring (se_amd_set_switch_keyring_sp), drops the fresh records to np - 1 primes (the last prime
 * belongs to the keys) and calls se_amd_ct_switch_sum_keyed_sp_device with CSR rows that mix keys: one division by the
 * special prime per group.  The AGGREGATOR decrypts np - 1 primes with se_amd_decrypt_level_device.
 * Prints the largest error over all slots of all group sums.
 *
 *   gcc examples/fleet_sum_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o fleet_sum_roundtrip
 *   ./fleet_sum_roundtrip 4096 3 16 4        (n, primes, records B, device keys K; groups of K records)
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

/* a 2-bit packed ternary key (codes 0 / 1 / 2 = -1 / 0 / +1), different for every `which` */
static void make_key(uint8_t *sk, size_t n, unsigned which)
{
    for (size_t i = 0; i < n / 4; i++)
    {
        uint8_t byte = 0;
        for (unsigned c = 0; c < 4; c++)
            byte = (uint8_t)((byte << 2) | (((4 * i + c) * (2654435761u + 40503u * which) >> 7) % 3u));
        sk[i] = byte;
    }
}

int main(int argc, char **argv)
{
    size_t n       = argc > 1 ? (size_t)atol(argv[1]) : 4096;
    size_t nprimes = argc > 2 ? (size_t)atol(argv[2]) : 3;
    size_t B       = argc > 3 ? (size_t)atol(argv[3]) : 16;
    size_t K       = argc > 4 ? (size_t)atol(argv[4]) : 4;
    if (B == 0 || K == 0 || nprimes < 2 || nprimes > 13) return 2;   /* the key switch reserves the last prime */
    const size_t slots = n / 2, rec = nprimes * n, level = nprimes - 1, low = level * n, R = nprimes - 1;
    const size_t G = (B + K - 1) / K;                                /* groups of K consecutive records: every key once */

    /* ---- the authority: K device keys, the aggregator key, and the switching keys from each device key to it ---- */
    se_amd_ctx *ctx;
    CHECK_SE(se_amd_create(&ctx, n, nprimes, 0));
    uint8_t *sk_dev = (uint8_t *)malloc(K * (n / 4)), *sk_agg = (uint8_t *)malloc(n / 4);
    for (size_t k = 0; k < K; k++) make_key(sk_dev + k * (n / 4), n, (unsigned)k + 1);
    make_key(sk_agg, n, 0);
    uint8_t *a_seeds = (uint8_t *)malloc(K * R * 64), *e_seeds = (uint8_t *)malloc(K * R * 64);
    for (size_t r = 0; r < K * R; r++)
        for (int c = 0; c < 64; c++)
        {
            a_seeds[r * 64 + c] = (uint8_t)(17 * r + c);
            e_seeds[r * 64 + c] = (uint8_t)(201 - c + 5 * r);
        }
    uint32_t *wk0 = (uint32_t *)malloc(K * R * rec * 4), *wk1 = (uint32_t *)malloc(K * R * rec * 4);
    CHECK_SE(se_amd_gen_switch_keys_sp(ctx, K, sk_dev, sk_agg, a_seeds, e_seeds, wk0, wk1));

    /* ---- the devices: record b under device key b mod K, slot values in [-1, 1) ---- */
    float *values     = (float *)malloc(B * slots * sizeof(float));
    uint8_t *share    = (uint8_t *)malloc(B * 64), *seeds = (uint8_t *)malloc(B * 64);
    uint32_t *key_idx = (uint32_t *)malloc(B * 4), *row_ptr = (uint32_t *)malloc((G + 1) * 4);
    uint32_t *idx     = (uint32_t *)malloc(B * 4);
    for (size_t b = 0; b < B; b++)
    {
        key_idx[b] = (uint32_t)(b % K);
        idx[b]     = (uint32_t)b;
        for (size_t i = 0; i < slots; i++)
            values[b * slots + i] = (float)((double)((((uint64_t)(i + 7 * b)) * 2654435761ull) % 2000ull) / 1000 - 1);
        for (int c = 0; c < 64; c++)
        {
            share[b * 64 + c] = (uint8_t)(c + b);
            seeds[b * 64 + c] = (uint8_t)(255 - c + 3 * b);
        }
    }
    for (size_t g = 0; g <= G; g++) row_ptr[g] = (uint32_t)(g * K < B ? g * K : B);

    void *d_values, *d_share, *d_seeds, *d_kidx, *d_rows, *d_idx, *d_c0, *d_c1, *d_l0, *d_l1, *d_r0, *d_r1, *d_out, *d_status;
    CHECK_HIP(hipMalloc(&d_values, B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, B * 64));
    CHECK_HIP(hipMalloc(&d_kidx, B * 4));
    CHECK_HIP(hipMalloc(&d_rows, (G + 1) * 4));
    CHECK_HIP(hipMalloc(&d_idx, B * 4));
    CHECK_HIP(hipMalloc(&d_c0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_c1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_l0, B * low * 4));
    CHECK_HIP(hipMalloc(&d_l1, B * low * 4));
    CHECK_HIP(hipMalloc(&d_r0, G * low * 4));
    CHECK_HIP(hipMalloc(&d_r1, G * low * 4));
    CHECK_HIP(hipMalloc(&d_out, G * slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_status, B + G));
    CHECK_HIP(hipMemcpy(d_values, values, B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_kidx, key_idx, B * 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_rows, row_ptr, (G + 1) * 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_idx, idx, B * 4, hipMemcpyHostToDevice));

    /* keyed symmetric encryption stands in for the K devices: the secret ring holds the DEVICE keys only */
    CHECK_SE(se_amd_set_secret_keyring(ctx, K, sk_dev));
    CHECK_SE(se_amd_encrypt_sym_keyed_device(ctx, (const float *)d_values, B, (const uint32_t *)d_kidx,
                                             (const uint8_t *)d_share, (const uint8_t *)d_seeds, (uint32_t *)d_c0,
                                             (uint32_t *)d_c1, NULL, NULL, (uint8_t *)d_status, NULL));

    /* ---- the evaluator: the public ring, no secret key is used from here ... ---- */
    CHECK_SE(se_amd_set_switch_keyring_sp(ctx, K, wk0, wk1));
    CHECK_SE(se_amd_ct_drop_primes_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, B, nprimes, level,
                                          (uint32_t *)d_l0, (uint32_t *)d_l1, NULL));
    CHECK_SE(se_amd_ct_switch_sum_keyed_sp_device(ctx, (const uint32_t *)d_l0, (const uint32_t *)d_l1, B, level,
                                                  (const uint32_t *)d_kidx, G, (const uint32_t *)d_rows,
                                                  (const uint32_t *)d_idx, B, (uint32_t *)d_r0, (uint32_t *)d_r1,
                                                  (uint8_t *)d_status + B, NULL));
    /* ---- ... to here.  The aggregator decrypts the group sums under ITS key alone, at the records' scale. ---- */
    CHECK_SE(se_amd_set_secret_key(ctx, sk_agg));
    const double scale = se_amd_scale(ctx);
    CHECK_SE(se_amd_decrypt_level_device(ctx, (const uint32_t *)d_r0, (const uint32_t *)d_r1, G, level, scale, NULL, NULL,
                                         (double *)d_out, NULL, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    double *out     = (double *)malloc(G * slots * sizeof(double));
    uint8_t *status = (uint8_t *)malloc(B + G);
    CHECK_HIP(hipMemcpy(out, d_out, G * slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(status, d_status, B + G, hipMemcpyDeviceToHost));
    int failed     = 0;
    double max_err = 0.0;
    for (size_t s = 0; s < B + G; s++) failed += status[s] != 1;
    for (size_t g = 0; g < G; g++)
        for (size_t i = 0; i < slots; i++)
        {
            double want = 0.0;
            for (size_t b = row_ptr[g]; b < row_ptr[g + 1]; b++) want += (double)values[b * slots + i];
            const double err = fabs(out[g * slots + i] - want);
            if (err > max_err) max_err = err;
        }
    printf("group 0, slot 0: %.5f\n", out[0]);
    printf("failed=%d B=%zu n=%zu primes=%zu level=%zu keys=%zu groups=%zu scale=%.6e max_abs_error=%.3e\n", failed, B, n,
           nprimes, level, K, G, scale, max_err);

    CHECK_HIP(hipFree(d_values));
    CHECK_HIP(hipFree(d_share));
    CHECK_HIP(hipFree(d_seeds));
    CHECK_HIP(hipFree(d_kidx));
    CHECK_HIP(hipFree(d_rows));
    CHECK_HIP(hipFree(d_idx));
    CHECK_HIP(hipFree(d_c0));
    CHECK_HIP(hipFree(d_c1));
    CHECK_HIP(hipFree(d_l0));
    CHECK_HIP(hipFree(d_l1));
    CHECK_HIP(hipFree(d_r0));
    CHECK_HIP(hipFree(d_r1));
    CHECK_HIP(hipFree(d_out));
    CHECK_HIP(hipFree(d_status));
    free(values), free(share), free(seeds), free(key_idx), free(row_ptr), free(idx), free(sk_dev), free(sk_agg),
        free(a_seeds), free(e_seeds), free(wk0), free(wk1), free(out), free(status);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
