"""The host model of the slot-wise polynomials: se_amd_ct_affine_rescale_device and the plans of se_amd_poly_create /
se_amd_ct_poly_sp_device of include/seal_embedded_amd.h, word for word from their definitions, on top of ct_model
(rescale_expect) and ct_model_dot (dot_sp_expect).  NumPy, Python integers and the oracle only: no torch, no package, no GPU.

Notation: o = Oracle(n, np); a term is a pair of slabs [B][term_primes][n] with term_primes >= primes, of which the first
`primes` rows of a record count; w and c_after are Python integers within int64.

    affine    acc_s[b][j] = sum_t (w_t mod q_j) . term_s[t][b][j] mod q_j, j < primes;  out_1 = rescale(acc_1),
              out_0 = rescale(acc_0) + (c_after mod q_i) in every position of row i
    ladder    depth(d) = ceil(log2 d), h(d) = 2^(depth(d) - 1), x^d = x^h . x^(d - h) at level m = L - depth(d) + 1 (the
              lower operand dropped to m), a one-pair row of the special-prime dot product, then the rescale;
              scale(d) = scale(h) . scale(d - h) / q_{m-1}
    combine   the affine map at level l = L - depth(D) over the powers with a_d != 0, w_d = round(((a_d . scale_out) .
              q_{l-1}) / scale(d)), c_after = round(a_0 . scale_out): IEEE doubles in that order, ties to even
"""
import numpy as np

from ct_model import rescale_expect
from ct_model_dot import dot_sp_expect


def weighted_sum_expect(o, terms, w, primes):
    """terms: slabs [B][>= primes][n]; w: Python ints -> uint32 [B][primes][n], sum_t (w_t mod q_j) . term_t[:, j] mod q_j
    in Python integers (object arrays): no word size to overflow."""
    B, n = terms[0].shape[0], terms[0].shape[2]
    acc = np.zeros((B, primes, n), dtype=object)
    for t, wt in zip(terms, w):
        for j in range(primes):
            acc[:, j] = (acc[:, j] + t[:, j].astype(object) * (int(wt) % o.q[j])) % o.q[j]
    return acc.astype(np.uint32)


def affine_rescale_expect(o, terms0, terms1, w, c_after, primes):
    """-> (out0, out1) uint32 [B][primes - 1][n]: rescale_expect of the weighted sums, then c_after mod q_i on slab 0."""
    out0 = rescale_expect(o, weighted_sum_expect(o, terms0, w, primes))
    out1 = rescale_expect(o, weighted_sum_expect(o, terms1, w, primes))
    for i in range(primes - 1):
        out0[:, i] = ((out0[:, i].astype(np.uint64) + np.uint64(int(c_after) % o.q[i])) % np.uint64(o.q[i])).astype(np.uint32)
    return out0, out1


def depth(d):
    """ceil(log2 d)."""
    return (d - 1).bit_length()


def poly_schedule(q, L, coeff, scale_in, scale_out):
    """The schedule of the header for p(x) = sum coeff[d] x^d on level-L records under the chain q -> dict(powers, levels,
    scales, weights: dicts by power over the needed set; terms: the powers with a_d != 0; c_after; level: l; out_primes:
    l - 1).  Doubles in the header's order; round() is ties-to-even on them."""
    D = len(coeff) - 1
    need = {d for d in range(1, D + 1) if coeff[d] != 0}
    for d in range(D, 1, -1):
        if d in need:
            h = 1 << (depth(d) - 1)
            need |= {h, d - h}
    powers = sorted(need)
    scales, levels = {1: float(scale_in)}, {}
    for d in powers:
        levels[d] = L - depth(d)
        if d >= 2:
            h, m = 1 << (depth(d) - 1), L - depth(d) + 1
            scales[d] = (scales[h] * scales[d - h]) / float(q[m - 1])
    lv = L - depth(D)
    terms = [d for d in powers if coeff[d] != 0]
    weights = {d: (round(((float(coeff[d]) * float(scale_out)) * float(q[lv - 1])) / scales[d]) if d in terms else 0)
               for d in powers}
    return dict(powers=powers, levels=levels, scales=scales, weights=weights, terms=terms,
                c_after=round(float(coeff[0]) * float(scale_out)), level=lv, out_primes=lv - 1)


def poly_expect(o, c0, c1, sched, k0, k1):
    """The composition on records (c0, c1) uint32 [B][L][n] under the special-prime relinearisation key (k0, k1): per needed
    power above 1 the one-pair rows of dot_sp_expect at level m on (x^h, x^(d-h) sliced to m rows) and rescale_expect; then
    affine_rescale_expect over the terms -> (out0, out1 [B][out_primes][n], powers: {d: (slab0, slab1)})."""
    B = c0.shape[0]
    rows = [[(b, b)] for b in range(B)]
    x = {1: (c0, c1)}
    for d in sched["powers"]:
        if d == 1:
            continue
        h, m = 1 << (depth(d) - 1), sched["levels"][d] + 1
        a0, a1 = x[h]
        assert a0.shape[1] == m
        b0, b1 = (s[:, :m] for s in x[d - h])
        p0, p1, _ = dot_sp_expect(o, a0, a1, np.ascontiguousarray(b0), np.ascontiguousarray(b1), rows, k0, k1)
        x[d] = (rescale_expect(o, p0), rescale_expect(o, p1))
    ts = sched["terms"]
    out0, out1 = affine_rescale_expect(o, [x[d][0] for d in ts], [x[d][1] for d in ts], [sched["weights"][d] for d in ts],
                                       sched["c_after"], sched["level"])
    return out0, out1, x


def poly_value(coeff, x):
    """p(x) in float64, Horner."""
    y = np.zeros_like(np.asarray(x, dtype=np.float64))
    for a in reversed(list(coeff)):
        y = y * x + float(a)
    return y


__all__ = ["weighted_sum_expect", "affine_rescale_expect", "depth", "poly_schedule", "poly_expect", "poly_value"]
