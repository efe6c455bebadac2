/*
 * slot_pack_roundtrip.c -- slot packing: B devices send SHORT records, a vector of width = slots / B values in the low
 * slots of a ciphertext and zero elsewhere (16 records of 128 values at n = 4096).  The evaluator packs all of them into
 * ONE ciphertext with one call of se_amd_ct_pack_sp_device -- record k rotated right by k * width slots, all B added, one
 * division by the special prime -- so every later step, the download and the key holder's decrypt run on one full
 * ciphertext instead of B mostly empty ones.  No lift, no rescale, no level spent: the packed record is at the scale the
 * records were encrypted at.
 *
 * The key holder generates the special-prime Galois keys of the B - 1 steps -k * width (se_amd_galois_element rotates LEFT
 * by a positive step) and hands them -- public material -- to the evaluator; record 0 stays where it is: element 1, the
 * identity, which needs no key.  The evaluator drops the fresh records to np - 1 primes (the last prime belongs to the
 * keys) and makes the one call: a CSR row of B entries, entry k = (record k, element k).
 * Prints the largest error over all slots of the packed record against the concatenation of the B vectors.
 *
 *   gcc examples/slot_pack_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o slot_pack_roundtrip
 *   ./slot_pack_roundtrip 4096 3 16        (n, primes, records B: a divisor of n / 2, at most 64)
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
    const size_t slots = n / 2;
    if (B < 2 || B > SE_AMD_MAX_GALOIS_KEYS || slots % B || nprimes < 2 || nprimes > 13) return 2;
    const size_t width = slots / B, rec = nprimes * n, level = nprimes - 1, low = level * n, R = nprimes - 1;

    /* ---- the key holder: the secret key and the Galois keys of the B - 1 steps ---- */
    se_amd_ctx *ctx;
    CHECK_SE(se_amd_create(&ctx, n, nprimes, 0));
    uint8_t *sk = (uint8_t *)malloc(n / 4);
    for (size_t i = 0; i < n / 4; i++)
    {
        uint8_t byte = 0;
        for (unsigned c = 0; c < 4; c++) byte = (uint8_t)((byte << 2) | (((4 * i + c) * 2654435761u >> 7) % 3u));
        sk[i] = byte;
    }
    uint32_t *elts = (uint32_t *)malloc(B * 4);
    for (size_t k = 0; k < B; k++) CHECK_SE(se_amd_galois_element(n, -(int64_t)(k * width), &elts[k]));
    if (elts[0] != 1) return 2;                                      /* step 0 is the identity */
    const size_t Gk = B - 1;
    uint8_t *a_seeds = (uint8_t *)malloc(Gk * R * 64), *e_seeds = (uint8_t *)malloc(Gk * R * 64);
    for (size_t r = 0; r < Gk * R; r++)
        for (int c = 0; c < 64; c++)
        {
            a_seeds[r * 64 + c] = (uint8_t)(17 * r + c);
            e_seeds[r * 64 + c] = (uint8_t)(201 - c + 5 * r);
        }
    uint32_t *gk0 = (uint32_t *)malloc(Gk * R * rec * 4), *gk1 = (uint32_t *)malloc(Gk * R * rec * 4);
    CHECK_SE(se_amd_gen_galois_keys_sp(ctx, sk, elts + 1, Gk, a_seeds, e_seeds, gk0, gk1));

    /* ---- the devices: record b holds `width` values in [-1, 1) in its low slots ---- */
    float *values  = (float *)calloc(B * slots, sizeof(float));
    uint8_t *share = (uint8_t *)malloc(B * 64), *seeds = (uint8_t *)malloc(B * 64);
    uint32_t *row_ptr = (uint32_t *)malloc(2 * 4), *idx = (uint32_t *)malloc(B * 4);
    for (size_t b = 0; b < B; b++)
    {
        idx[b] = (uint32_t)b;                                        /* entry b = (record b, element b) */
        for (size_t i = 0; i < width; i++)
            values[b * slots + i] = (float)((double)((((uint64_t)(i + 7 * b)) * 2654435761ull) % 2000ull) / 1000 - 1);
        for (int c = 0; c < 64; c++)
        {
            share[b * 64 + c] = (uint8_t)(c + b);
            seeds[b * 64 + c] = (uint8_t)(255 - c + 3 * b);
        }
    }
    row_ptr[0] = 0, row_ptr[1] = (uint32_t)B;

    void *d_values, *d_share, *d_seeds, *d_rows, *d_idx, *d_c0, *d_c1, *d_l0, *d_l1, *d_r0, *d_r1, *d_out, *d_status;
    CHECK_HIP(hipMalloc(&d_values, B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, B * 64));
    CHECK_HIP(hipMalloc(&d_rows, 2 * 4));
    CHECK_HIP(hipMalloc(&d_idx, B * 4));
    CHECK_HIP(hipMalloc(&d_c0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_c1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_l0, B * low * 4));
    CHECK_HIP(hipMalloc(&d_l1, B * low * 4));
    CHECK_HIP(hipMalloc(&d_r0, low * 4));
    CHECK_HIP(hipMalloc(&d_r1, low * 4));
    CHECK_HIP(hipMalloc(&d_out, slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_status, B + 1));
    CHECK_HIP(hipMemcpy(d_values, values, B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_rows, row_ptr, 2 * 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_idx, idx, B * 4, hipMemcpyHostToDevice));

    CHECK_SE(se_amd_set_secret_key(ctx, sk));
    CHECK_SE(se_amd_encrypt_sym_device(ctx, (const float *)d_values, B, (const uint8_t *)d_share, (const uint8_t *)d_seeds,
                                       (uint32_t *)d_c0, (uint32_t *)d_c1, NULL, NULL, (uint8_t *)d_status, NULL));

    /* ---- the evaluator: the public Galois keys, one drop and ONE packing call; the same array serves as d_idx and as
     * d_eidx, entry k being (record k, element k) ---- */
    CHECK_SE(se_amd_set_galois_keys_sp(ctx, elts + 1, Gk, gk0, gk1));
    CHECK_SE(se_amd_ct_drop_primes_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, B, nprimes, level,
                                          (uint32_t *)d_l0, (uint32_t *)d_l1, NULL));
    CHECK_SE(se_amd_ct_pack_sp_device(ctx, (const uint32_t *)d_l0, (const uint32_t *)d_l1, B, level, elts, B, 1,
                                      (const uint32_t *)d_rows, (const uint32_t *)d_idx, (const uint32_t *)d_idx, B,
                                      (uint32_t *)d_r0, (uint32_t *)d_r1, (uint8_t *)d_status + B, NULL));
    /* ---- the key holder decrypts ONE record at the records' scale ---- */
    const double scale = se_amd_scale(ctx);
    CHECK_SE(se_amd_decrypt_level_device(ctx, (const uint32_t *)d_r0, (const uint32_t *)d_r1, 1, level, scale, NULL, NULL,
                                         (double *)d_out, NULL, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    double *out     = (double *)malloc(slots * sizeof(double));
    uint8_t *status = (uint8_t *)malloc(B + 1);
    CHECK_HIP(hipMemcpy(out, d_out, slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(status, d_status, B + 1, hipMemcpyDeviceToHost));
    int failed     = 0;
    double max_err = 0.0;
    for (size_t s = 0; s < B + 1; s++) failed += status[s] != 1;
    for (size_t b = 0; b < B; b++)
        for (size_t i = 0; i < width; i++)
        {
            const double err = fabs(out[b * width + i] - (double)values[b * slots + i]);
            if (err > max_err) max_err = err;
        }
    printf("slot 0: %.5f, slot %zu: %.5f\n", out[0], width, out[width]);
    printf("failed=%d B=%zu n=%zu primes=%zu level=%zu width=%zu packed=1 scale=%.6e max_abs_error=%.3e\n", failed, B, n,
           nprimes, level, width, scale, max_err);

    CHECK_HIP(hipFree(d_values));
    CHECK_HIP(hipFree(d_share));
    CHECK_HIP(hipFree(d_seeds));
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
    free(values), free(share), free(seeds), free(row_ptr), free(idx), free(sk), free(elts), free(a_seeds), free(e_seeds),
        free(gk0), free(gk1), free(out), free(status);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
