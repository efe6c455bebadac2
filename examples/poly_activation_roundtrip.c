/*
 * poly_activation_roundtrip.c -- a function applied to every slot of encrypted records: the logistic activation after a
 * linear layer, as its degree-7 Taylor polynomial
 *     p(x) = 1/2 + x/4 - x^3/48 + x^5/480 - 17 x^7/80640,
 * evaluated on ciphertexts by ONE call.  se_amd_poly_create makes the schedule on the host (the powers 1, 2, 3, 4, 5, 7 --
 * x^6 is not needed -- their levels and scales, the integer weights of the last step); se_amd_ct_poly_sp_device runs it
 * under the special-prime relinearisation key: five products, each a one-pair row of se_amd_ct_dot_sp_device and a
 * rescale, then one se_amd_ct_affine_rescale_device that sums the four terms at their own levels, rescales once and adds
 * the constant.
 *
 *   encrypt -> lift: se_amd_ct_lincomb_device with the weight round(q_{L-1} / Delta), so that scale_in is about q
 *   -> se_amd_ct_drop_primes_device to L = np - 1 (the last prime belongs to the key)
 *   -> se_amd_ct_poly_sp_device                          (level L - 4, scale_out = Delta)
 *   -> se_amd_decrypt_level_device at scale_out.
 * Prints the largest error against p(x) in double over all slots of all records.
 *
 *   gcc examples/poly_activation_roundtrip.c -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
 *       -Lseal-embedded_amd/lib -lseal_embedded_amd -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/seal-embedded_amd/lib -o poly_activation_roundtrip
 *   ./poly_activation_roundtrip 8192 6 4        (n, primes, records B)
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

#define DEGREE 7
static const double coeff[DEGREE + 1] = {0.5, 0.25, 0.0, -1.0 / 48, 0.0, 1.0 / 480, 0.0, -17.0 / 80640};

int main(int argc, char **argv)
{
    size_t n       = argc > 1 ? (size_t)atol(argv[1]) : 8192;
    size_t nprimes = argc > 2 ? (size_t)atol(argv[2]) : 6;
    size_t B       = argc > 3 ? (size_t)atol(argv[3]) : 4;
    /* the key reserves the last prime; degree 7 has depth 3 and the last step spends one more level */
    if (B == 0 || nprimes < 6 || nprimes > 13) return 2;
    const size_t slots = n / 2, rec = nprimes * n, L = nprimes - 1, R = nprimes - 1;

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
            a_seeds[r * 64 + c] = (uint8_t)(19 * r + c);
            e_seeds[r * 64 + c] = (uint8_t)(203 - c + 7 * r);
        }
    uint32_t *evk0 = (uint32_t *)malloc(R * rec * 4), *evk1 = (uint32_t *)malloc(R * rec * 4);
    CHECK_SE(se_amd_gen_relin_key_sp(ctx, sk, a_seeds, e_seeds, evk0, evk1));
    CHECK_SE(se_amd_set_relin_key_sp(ctx, evk0, evk1));

    /* ---- the plan: host only ---- */
    uint32_t q[13];
    CHECK_SE(se_amd_moduli(ctx, q));
    const double delta   = se_amd_scale(ctx);
    const int32_t lift   = (int32_t)nearbyint((double)q[L - 1] / delta);
    const double scale_in = (double)lift * delta, scale_out = delta;
    se_amd_poly *plan;
    CHECK_SE(se_amd_poly_create(n, nprimes, L, coeff, DEGREE, scale_in, scale_out, &plan));
    size_t out_primes;
    int64_t c_after;
    CHECK_SE(se_amd_poly_result(plan, &out_primes, &c_after));
    uint32_t power[16], level[16];
    double scale[16];
    int64_t weight[16];
    const size_t K = se_amd_poly_terms(plan, power, level, scale, weight, 16);
    for (size_t k = 0; k < K; k++)
        printf("x^%u: level %u, scale %.6e, weight %lld\n", power[k], level[k], scale[k], (long long)weight[k]);
    const size_t work_bytes = se_amd_poly_workspace_bytes(plan, B);

    /* ---- the records: slot values in [-1, 1) ---- */
    float *values     = (float *)malloc(B * slots * sizeof(float));
    uint8_t *share    = (uint8_t *)malloc(B * 64), *seeds = (uint8_t *)malloc(B * 64);
    uint32_t *row_ptr = (uint32_t *)malloc((B + 1) * 4), *idx = (uint32_t *)malloc(B * 4);
    int32_t *w        = (int32_t *)malloc(B * 4);
    for (size_t b = 0; b < B; b++)
    {
        for (size_t i = 0; i < slots; i++)
            values[b * slots + i] = (float)((double)((((uint64_t)(i + 7 * b)) * 2654435761ull) % 2000ull) / 1000 - 1);
        for (int c = 0; c < 64; c++)
        {
            share[b * 64 + c] = (uint8_t)(c + b);
            seeds[b * 64 + c] = (uint8_t)(255 - c + 3 * b);
        }
        row_ptr[b] = idx[b] = (uint32_t)b;
        w[b]                = lift;
    }
    row_ptr[B] = (uint32_t)B;

    void *d_values, *d_share, *d_seeds, *d_rows, *d_idx, *d_w, *d_c0, *d_c1, *d_s0, *d_s1, *d_l0, *d_l1, *d_work, *d_r0,
        *d_r1, *d_out, *d_status;
    CHECK_HIP(hipMalloc(&d_values, B * slots * sizeof(float)));
    CHECK_HIP(hipMalloc(&d_share, B * 64));
    CHECK_HIP(hipMalloc(&d_seeds, B * 64));
    CHECK_HIP(hipMalloc(&d_rows, (B + 1) * 4));
    CHECK_HIP(hipMalloc(&d_idx, B * 4));
    CHECK_HIP(hipMalloc(&d_w, B * 4));
    CHECK_HIP(hipMalloc(&d_c0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_c1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_s0, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_s1, B * rec * 4));
    CHECK_HIP(hipMalloc(&d_l0, B * L * n * 4));
    CHECK_HIP(hipMalloc(&d_l1, B * L * n * 4));
    CHECK_HIP(hipMalloc(&d_work, work_bytes));
    CHECK_HIP(hipMalloc(&d_r0, B * out_primes * n * 4));
    CHECK_HIP(hipMalloc(&d_r1, B * out_primes * n * 4));
    CHECK_HIP(hipMalloc(&d_out, B * slots * sizeof(double)));
    CHECK_HIP(hipMalloc(&d_status, 3 * B));
    CHECK_HIP(hipMemcpy(d_values, values, B * slots * sizeof(float), hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_share, share, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_seeds, seeds, B * 64, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_rows, row_ptr, (B + 1) * 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_idx, idx, B * 4, hipMemcpyHostToDevice));
    CHECK_HIP(hipMemcpy(d_w, w, B * 4, hipMemcpyHostToDevice));

    CHECK_SE(se_amd_encrypt_sym_device(ctx, (const float *)d_values, B, (const uint8_t *)d_share, (const uint8_t *)d_seeds,
                                       (uint32_t *)d_c0, (uint32_t *)d_c1, NULL, NULL, (uint8_t *)d_status, NULL));
    CHECK_SE(se_amd_ct_lincomb_device(ctx, (const uint32_t *)d_c0, (const uint32_t *)d_c1, B, B, (const uint32_t *)d_rows,
                                      (const uint32_t *)d_idx, (const int32_t *)d_w, B, (uint32_t *)d_s0, (uint32_t *)d_s1,
                                      (uint8_t *)d_status + B, NULL));
    CHECK_SE(se_amd_ct_drop_primes_device(ctx, (const uint32_t *)d_s0, (const uint32_t *)d_s1, B, nprimes, L,
                                          (uint32_t *)d_l0, (uint32_t *)d_l1, NULL));
    CHECK_SE(se_amd_ct_poly_sp_device(ctx, plan, (const uint32_t *)d_l0, (const uint32_t *)d_l1, B, d_work, work_bytes,
                                      (uint32_t *)d_r0, (uint32_t *)d_r1, NULL));
    CHECK_SE(se_amd_decrypt_level_device(ctx, (const uint32_t *)d_r0, (const uint32_t *)d_r1, B, out_primes, scale_out,
                                         NULL, NULL, (double *)d_out, (uint8_t *)d_status + 2 * B, NULL));
    CHECK_HIP(hipDeviceSynchronize());

    double *out     = (double *)malloc(B * slots * sizeof(double));
    uint8_t *status = (uint8_t *)malloc(3 * B);
    CHECK_HIP(hipMemcpy(out, d_out, B * slots * sizeof(double), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(status, d_status, 3 * B, hipMemcpyDeviceToHost));
    int failed     = 0;
    double max_err = 0.0;
    for (size_t s = 0; s < 3 * B; s++) failed += status[s] != 1;
    for (size_t b = 0; b < B; b++)
        for (size_t i = 0; i < slots; i++)
        {
            const double x = (double)values[b * slots + i];
            double want    = 0.0;
            for (int d = DEGREE; d >= 0; d--) want = want * x + coeff[d];
            const double err = fabs(out[b * slots + i] - want);
            if (err > max_err) max_err = err;
        }
    printf("record 0, slot 0: p(%.5f) = %.5f\n", (double)values[0], out[0]);
    printf("failed=%d B=%zu n=%zu primes=%zu level=%zu out_primes=%zu scale_out=%.6e c_after=%lld max_abs_error=%.3e\n",
           failed, B, n, nprimes, L, out_primes, scale_out, (long long)c_after, max_err);

    CHECK_HIP(hipFree(d_values));
    CHECK_HIP(hipFree(d_share));
    CHECK_HIP(hipFree(d_seeds));
    CHECK_HIP(hipFree(d_rows));
    CHECK_HIP(hipFree(d_idx));
    CHECK_HIP(hipFree(d_w));
    CHECK_HIP(hipFree(d_c0));
    CHECK_HIP(hipFree(d_c1));
    CHECK_HIP(hipFree(d_s0));
    CHECK_HIP(hipFree(d_s1));
    CHECK_HIP(hipFree(d_l0));
    CHECK_HIP(hipFree(d_l1));
    CHECK_HIP(hipFree(d_work));
    CHECK_HIP(hipFree(d_r0));
    CHECK_HIP(hipFree(d_r1));
    CHECK_HIP(hipFree(d_out));
    CHECK_HIP(hipFree(d_status));
    free(values), free(share), free(seeds), free(row_ptr), free(idx), free(w), free(sk), free(a_seeds), free(e_seeds),
        free(evk0), free(evk1), free(out), free(status);
    se_amd_poly_destroy(plan);
    se_amd_destroy(ctx);
    return failed == 0 && max_err < 0.1 ? 0 : 1;
}
