// se_host_tables.h -- parameter sets and setup-time tables, computed on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "se_types.h"

namespace seamd {

struct HostParams
{
    size_t n = 0, logn = 0, nprimes = 0;
    uint32_t q[kMaxPrimes]     = {};
    uint32_t cr_hi[kMaxPrimes] = {};
    uint32_t cr_lo[kMaxPrimes] = {};
    uint32_t psi[kMaxPrimes]   = {};  // primitive 2n-th root of unity mod q
    double scale               = 0;
};

// 0 on success; negative if (n, nprimes) is not one of the reference's default parameter sets.
int host_params_init(HostParams &hp, size_t n, size_t nprimes);
DevParams to_dev_params(const HostParams &hp);
CrtParams host_crt_params(const HostParams &hp);  // Garner constants of the chain (exact integer arithmetic)
// constants of the rescale from level `primes` (2 .. hp.nprimes): q_{primes-1}^-1 mod q_j, j < primes - 1
RescaleParams host_rescale_params(const HostParams &hp, size_t primes);
// A slot-wise polynomial p(x) = sum a_d x^d made ready (se_amd_poly_create): the schedule of include/seal_embedded_amd.h
// ("Slot-wise polynomials") and nothing else -- host data, no device, no key.  powers: the needed set in increasing order,
// powers[0] the input itself (d = 1, level L, scale_in).
struct PolyPower
{
    uint32_t d     = 0;
    uint32_t level = 0;       // primes of the record that holds x^d: L - depth(d)
    double scale   = 0;       // scale(d)
    int64_t w      = 0;       // the combine's weight w_d; 0 when a_d = 0 (then x^d is no term)
    bool term      = false;   // a_d != 0
};
struct PolyPlan
{
    size_t n = 0, np = 0;
    size_t L           = 0;   // level of the input records
    size_t comb_level  = 0;   // l = L - depth(degree): the combine's level; the result has l - 1 primes
    int64_t c_after    = 0;
    std::vector<PolyPower> powers;
    // words of a call's workspace for B records: the row pointers of B one-pair rows (padded to 16 bytes), both slabs of
    // every power above 1 at its own level, of one product (at most L rows) and of one dropped operand (at most L - 1)
    size_t workspace_words(size_t B) const;
};
// 0, or negative for what se_amd_poly_create refuses
int poly_plan_init(PolyPlan &plan, size_t n, size_t np, size_t primes, const double *coeff, size_t degree, double scale_in,
                   double scale_out);
bool host_known_prime(uint32_t q);  // one of the tabulated 27-/30-bit primes (parameters.c:129-174)

size_t bitrev(size_t x, size_t nbits);
void host_index_map(const HostParams &hp, std::vector<uint16_t> &map, std::vector<uint16_t> &inv);
void host_ifft_twiddles(const HostParams &hp, std::vector<double> &w);            // [n][2]
void host_ntt_root_pairs(const HostParams &hp, size_t j, std::vector<uint32_t> &rw);  // [n][2]
void host_intt_root_pairs(const HostParams &hp, size_t j, std::vector<uint32_t> &rw); // [n][2]
uint32_t host_inv_mod(uint32_t a, uint32_t q);

}  // namespace seamd
