/*
 * slot_sum_roundtrip.c -- packed dot products on the machine in the middle: two senders encrypt B records each, every
 * record holding n/32 vectors of 16 entries back to back, and an evaluator that holds the public relinearisation key and
 * four Galois keys but NO secret key multiplies the records slot by slot and adds up the 16 products of every vector
 * with four rotate-and-adds.  The key holder decrypts one level lower: slot 16 k of record b holds the dot product of
 * the k-th vectors of the two senders' records b.
 *
 * se_amd_ct_mul_device and se_amd_ct_relin_device give the products at scale Delta^2 -- a raised scale, which is where a
 * rotation belongs (there is no special prime).  A rotate-and-add by s is
 * se_amd_ct_galois_device with the element of step s (slots move LEFT by s) written into the second half of a
 * 2B-record slab whose first half holds the records themselves, then se_amd_ct_lincomb_device with the CSR rows
 * {b, B + b}.  After the steps 1, 2, 4, 8 slot i holds the sum of the slots i .. i + 15.  se_amd_ct_rescale_device drops
 * the last prime, se_amd_decrypt_level_device decodes at Delta^2 / q_last.  Prints the largest error over all vectors.
 *
 *   gcc examples/slot_sum_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o slot_sum_roundtrip
 *   ./slot_sum_roundtrip 4096 3 8
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

#define VEC 16   /* entries of a vector */
#define STEPS 4  /* rotate-and-adds: steps 1, 2, 4, 8 */

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

    /* ---- the key holder: one secret key; its relinearisation key and the Galois keys of the four steps are public
     * material, handed to the evaluator ---- */
    se_amd_ctx *ctx;
    CHECK_SE(se_amd_create(&ctx, n, nprimes, 0));
    uint8_t *sk = (uint8_t *)calloc(n / 4, 1);                 /* 2-bit packed, codes 0 / 1 / 2 = -1 / 0 / +1 */
    for (size_t i = 0; i < n / 4; i++) sk[i] = (uint8_t)(((i * 37u) % 3u) * 0x55u);
    CHECK_SE(se_amd_set_secret_key(ctx, sk));
    uint32_t q[13];
    CHECK_SE(se_amd_moduli(ctx, q));
    uint8_t *a_seeds = (uint8_t *)malloc(STEPS * R * 64), *e_seeds = (uint8_t *)malloc(STEPS * R * 64);
    fill_seeds(a_seeds, R, 17, 0);
    fill_seeds(e_seeds, R, 5, 201);
    uint32_t *evk0 = (uint32_t *)malloc(R * rec * 4), *evk1 = (uint32_t *)malloc(R * rec * 4);
    CHECK_SE(se_amd_gen_relin_key(ctx, sk, a_seeds, e_seeds, evk0, evk1));
    CHECK_SE(se_amd_set_relin_key(ctx, evk0, evk1));
    uint32_t elts[STEPS];
    for (int s = 0; s < STEPS; s++) CHECK_SE(se_amd_galois_element(n, (int64_t)1 << s, &elts[s]));
    fill_seeds(a_seeds, STEPS * R, 29, 3);
    fill_seeds(e_seeds, STEPS * R, 11, 77);
    uint32_t *gk0 = (uint32_t *)malloc(STEPS * R * rec * 4), *gk1 = (uint32_t *)malloc(STEPS * R * rec * 4);
    CHECK_SE(se_amd_gen_galois_keys(ctx, sk, elts, STEPS, a_seeds, e_seeds, gk0, gk1));
    CHECK_SE(se_amd_set_galois_keys(ctx, elts, STEPS, gk0, gk1));

    /* ---- the senders: B records each, slot values in [-1, 1) ---- */
    float *x       = (float *)malloc(2 * B * slots * sizeof(float)), *y = x + B * slots;
    uint8_t *share = (uint8_t *)malloc(2 * B * 64), *seeds = (uint8_t *)malloc(2 * B * 64);
    for (size_t b = 0; b < 2 * B; b++)
        for (size_t i = 0; i < slots; i++)
            x[b * slots + i] = (float)((double)((((uint64_t)(i + 131 * b)) * 2654435761ull) % 2000ull) / 1000 - 1);
    fill_seeds(share, 2 * B, 1, 0);
    fill_seeds(seeds, 2 * B, 3, 128);

    /* the rotate-and-add lists: output row b = record b + record B + b of a 2B-record slab */
    uint32_t *row_ptr = (uint32_t *)malloc((B + 1) * 4), *idx = (uint32_t *)malloc(2 * B * 4);
    for (size_t b = 0; b <= B; b++) row_ptr[b] = (uint32_t)(2 * b);
    for (size_t b = 0; b < B; b++) idx[2 * b] = (uint32_t)b, idx[2 * b + 1] = (uint32_t)(B + b);

    void *d_values, *d_share, *d_seeds, *d_c0, *d_c1, *d_t0, *d_t1, *d_t2, *d_p0, *d_p1, *d_q0, *d_q1, *d_r0, *d_r1,
        *d_out, *d_row_ptr, *d_idx, *d_mul_status, *d_agg_status, *d_status;
    CHECK_HIP(hipMalloc(&d_values, 2 * B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, 2 * B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, 2 * B * 64));
    CHECK_HIP(hipMalloc(&d_c0, 2 * B * rec * 4));   /* records 0 .. B-1: the first sender's, B .. 2B-1: the second's */
    CHECK_HIP(hipMalloc(&d_c1, 2 * B * rec * 4));
    CHECK_HIP(hipMalloc(&d_t0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_t1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_t2, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_p0, 2 * B * rec * 4));   /* the two 2B-record slabs the rotate-and-adds alternate between */
    CHECK_HIP(hipMalloc(&d_p1, 2 * B * rec * 4));
    CHECK_HIP(hipMalloc(&d_q0, 2 * B * rec * 4));
    CHECK_HIP(hipMalloc(&d_q1, 2 * B * rec * 4));
    CHECK_HIP(hipMalloc(&d_r0, B * low * 4));
    CHECK_HIP(hipMalloc(&d_r1, B * low * 4));
    CHECK_HIP(hipMalloc(&d_out, B * slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_row_ptr, (B + 1) * 4));
    CHECK_HIP(hipMalloc(&d_idx, 2 * B * 4));
    CHECK_HIP(hipMalloc(&d_mul_status, B));
    CHECK_HIP(hipMalloc(&d_agg_status, STEPS * B));
    CHECK_HIP(hipMalloc(&d_status, B));
    CHECK_HIP(hipMemcpy(d_values, x, 2 * B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, 2 * B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, 2 * B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_row_ptr, row_ptr, (B + 1) * 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_idx, idx, 2 * B * 4, hipMemcpyHostToDevice));

    CHECK_SE(se_amd_encrypt_sym_device(ctx, (const float *)d_values, 2 * B, (const uint8_t *)d_share,
                                       (const uint8_t *)d_seeds, (uint32_t *)d_c0, (uint32_t *)d_c1, NULL, NULL, NULL,
                                       NULL));
    /* ---- the evaluator: no secret key is used from here ... ---- */
    const uint32_t *y0 = (const uint32_t *)d_c0 + B * rec, *y1 = (const uint32_t *)d_c1 + B * rec;
    CHECK_SE(se_amd_ct_mul_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, B, y0, y1, B, nprimes, B, NULL,
                                  NULL, (uint32_t *)d_t0, (uint32_t *)d_t1, (uint32_t *)d_t2, (uint8_t *)d_mul_status,
                                  NULL));
    uint32_t *cur0 = (uint32_t *)d_p0, *cur1 = (uint32_t *)d_p1, *nxt0 = (uint32_t *)d_q0, *nxt1 = (uint32_t *)d_q1;
    CHECK_SE(se_amd_ct_relin_device(ctx, (const uint32_t *)d_t0, (const uint32_t *)d_t1, (const uint32_t *)d_t2, B,
                                    nprimes, cur0, cur1, NULL));
    for (int s = 0; s < STEPS; s++)
    {
        CHECK_SE(se_amd_ct_galois_device(ctx, cur0, cur1, B, nprimes, elts[s], cur0 + B * rec, cur1 + B * rec, NULL));
        CHECK_SE(se_amd_ct_lincomb_device(ctx, cur0, cur1, 2 * B, B, (const uint32_t *)d_row_ptr,
                                          (const uint32_t *)d_idx, NULL, 2 * B, nxt0, nxt1,
                                          (uint8_t *)d_agg_status + s * B, NULL));
        uint32_t *t0 = cur0, *t1 = cur1;
        cur0 = nxt0, cur1 = nxt1, nxt0 = t0, nxt1 = t1;
    }
    CHECK_SE(se_amd_ct_rescale_device(ctx, cur0, cur1, B, nprimes, (uint32_t *)d_r0, (uint32_t *)d_r1, NULL));
    /* ---- ... to here.  The key holder decrypts B ciphertexts of primes - 1 primes at Delta^2 / q_last. ---- */
    const double scale = se_amd_scale(ctx) * se_amd_scale(ctx) / (double)q[nprimes - 1];
    CHECK_SE(se_amd_decrypt_level_device(ctx, (const uint32_t *)d_r0, (const uint32_t *)d_r1, B, nprimes - 1, scale, NULL,
                                         NULL, (double *)d_out, (uint8_t *)d_status, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    double *out         = (double *)malloc(B * slots * sizeof(double));
    uint8_t *mul_status = (uint8_t *)malloc(B), *agg_status = (uint8_t *)malloc(STEPS * B), *status = (uint8_t *)malloc(B);
    CHECK_HIP(hipMemcpy(out, d_out, B * slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(mul_status, d_mul_status, B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(agg_status, d_agg_status, STEPS * B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(status, d_status, B, hipMemcpyDeviceToHost));
    int failed = 0;
    for (size_t b = 0; b < B; b++) failed += (mul_status[b] != 1) + (status[b] != 1);
    for (size_t k = 0; k < STEPS * B; k++) failed += agg_status[k] != 1;
    double max_err = 0.0, first = 0.0;
    for (size_t b = 0; b < B; b++)
        for (size_t v = 0; v < slots / VEC; v++)
        {
            double want = 0.0;
            for (size_t i = 0; i < VEC; i++)
                want += (double)x[b * slots + VEC * v + i] * (double)y[b * slots + VEC * v + i];
            if (b == 0 && v == 0) first = want;
            const double err = fabs(out[b * slots + VEC * v] - want);
            if (err > max_err) max_err = err;
        }
    printf("record 0, vector 0: dot product %.5f (expected %.5f)\n", out[0], first);
    printf("failed=%d B=%zu n=%zu primes=%zu level=%zu vectors=%zu scale=%.6e max_abs_error=%.3e\n", failed, B, n,
           nprimes, nprimes - 1, B * (slots / VEC), scale, max_err);

    CHECK_HIP(hipFree(d_values));
    CHECK_HIP(hipFree(d_share));
    CHECK_HIP(hipFree(d_seeds));
    CHECK_HIP(hipFree(d_c0));
    CHECK_HIP(hipFree(d_c1));
    CHECK_HIP(hipFree(d_t0));
    CHECK_HIP(hipFree(d_t1));
    CHECK_HIP(hipFree(d_t2));
    CHECK_HIP(hipFree(d_p0));
    CHECK_HIP(hipFree(d_p1));
    CHECK_HIP(hipFree(d_q0));
    CHECK_HIP(hipFree(d_q1));
    CHECK_HIP(hipFree(d_r0));
    CHECK_HIP(hipFree(d_r1));
    CHECK_HIP(hipFree(d_out));
    CHECK_HIP(hipFree(d_row_ptr));
    CHECK_HIP(hipFree(d_idx));
    CHECK_HIP(hipFree(d_mul_status));
    CHECK_HIP(hipFree(d_agg_status));
    CHECK_HIP(hipFree(d_status));
    free(x), free(share), free(seeds), free(sk), free(a_seeds), free(e_seeds), free(evk0), free(evk1), free(gk0),
        free(gk1), free(row_ptr), free(idx), free(out), free(mul_status), free(agg_status), free(status);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
