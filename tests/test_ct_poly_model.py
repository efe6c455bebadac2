"""The schedule of the polynomial plans (se_amd_poly_create, host-only) against tests/ct_model_poly.py, every refusal of
creation, and the model's rescale of a weighted sum against plain Python integer division.  No GPU: the plan entries need
no device."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from build_support import pkg  # noqa: F401  (a fixture)
from ct_model import centred, crt_centred
from ct_model_poly import affine_rescale_expect, depth, poly_schedule
from gpu_support import CEntry, hptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8192, 6), (16384, 13)]
LOGISTIC7 = [0.5, 0.25, 0.0, -1.0 / 48, 0.0, 1.0 / 480, 0.0, -17.0 / 80640]


def coefficients(kind):
    rng = np.random.default_rng(71)
    full = lambda D: list(rng.uniform(0.25, 1.0, D + 1) * rng.choice([-1.0, 1.0], D + 1))  # noqa: E731
    return {"1": full(1), "2": full(2), "3": full(3), "7": full(7), "7odd": LOGISTIC7, "8": full(8), "15": full(15)}[kind]


def test_model_imports_neither_torch_nor_pytest():
    code = ("import sys; sys.path[:0] = [%r, %r]; import ct_model_poly; "
            "assert not {'torch', 'pytest', 'seal_embedded_amd'} & set(sys.modules)" % (os.path.join(ROOT, "tests"), ROOT))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_depth_and_the_ladder_split():
    assert [depth(d) for d in range(1, 17)] == [0, 1, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4]
    assert all(depth(d) == math.ceil(math.log2(d)) for d in range(1, 16))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["1", "2", "3", "7", "7odd", "8", "15"])
def test_library_schedule_equals_the_model(pkg, shape, kind):
    """Powers, levels, scales (the same doubles), weights and c_after (the same integers), out_primes: the library's plan
    through se_amd_poly_terms / se_amd_poly_result equals poly_schedule.  The odd degree-7 polynomial computes the powers
    1, 2, 3, 4, 5, 7 and not 6.  Degree 15 has depth 4 and needs L >= 6: at 8192 x 6, where L <= 5, the plan is refused."""
    n, npr = shape
    q = [int(x) for x in pkg.host_tables(n, npr)["q"]]
    coeff = coefficients(kind)
    L = npr - 1
    scale_in, scale_out = float(q[L - 1]) * 1.0009765625, 2.0 ** 25
    if depth(len(coeff) - 1) + 2 > L:
        assert (shape, kind) == ((8192, 6), "15")
        with pytest.raises(pkg.SealEmbeddedAmdError):
            pkg.poly_create(n, npr, L, coeff, scale_in, scale_out)
        return
    sched = poly_schedule(q, L, coeff, scale_in, scale_out)
    plan = pkg.poly_create(n, npr, L, coeff, scale_in, scale_out)
    terms = plan.terms()
    assert [t["power"] for t in terms] == sched["powers"]
    if kind == "7odd":
        assert sched["powers"] == [1, 2, 3, 4, 5, 7] and sched["terms"] == [1, 3, 5, 7]
    if kind == "15":
        assert sched["powers"] == list(range(1, 16))
    for t in terms:
        d = t["power"]
        assert t["level"] == sched["levels"][d] == L - depth(d), d
        assert np.float64(t["scale"]).tobytes() == np.float64(sched["scales"][d]).tobytes(), d
        assert t["weight"] == sched["weights"][d], d
    assert plan.result() == (sched["out_primes"], sched["c_after"])
    assert sched["out_primes"] == L - depth(len(coeff) - 1) - 1
    # the workspace: the row pointers, both slabs of every power above 1, of one product and of one dropped operand
    B = 3
    rows = sum(sched["levels"][d] for d in sched["powers"] if d > 1) + 2 * L - 1
    want = 0 if len(sched["powers"]) == 1 else 4 * (((B + 1 + 3) // 4) * 4 + 2 * B * rows * n)
    assert plan.workspace_bytes(B) == want
    plan.close()


def test_weights_beyond_int32_are_kept(pkg):
    """A coefficient a . 2^30 with |a| >= 2: the weight the int32 sum cannot hold."""
    n, npr, L = 8192, 6, 5
    q = [int(x) for x in pkg.host_tables(n, npr)["q"]]
    plan = pkg.poly_create(n, npr, L, [0.0, 3.0], float(q[L - 1]), 2.0 ** 30)
    (t,) = plan.terms()
    assert t["weight"] == round((3.0 * 2.0 ** 30 * float(q[L - 1])) / float(q[L - 1])) == 3 << 30 and t["weight"] >= 2 ** 31
    plan.close()


def test_every_refusal_of_creation(pkg):
    """SE_ERR_INVALD_ARGUMENT and *out untouched: unsupported (n, np); degree 0 and 16; a_D = 0; a NaN / infinite
    coefficient or scale; a scale <= 0; primes outside [depth(D) + 2, np - 1]; a weight or a constant at or above 2^62;
    NULL coeff and out."""
    L = pkg.lib()
    n, npr = 8192, 6
    good = np.array([0.5, 0.25, 0.0, -1.0 / 48], dtype=np.float64)
    arr = lambda *v: np.array(v, dtype=np.float64)  # noqa: E731
    handle = C.c_void_p(0xDEAD)
    create = CEntry(L.se_amd_poly_create, n=n, np=npr, primes=5, coeff=hptr(good), degree=3, scale_in=2.0 ** 30,
                    scale_out=2.0 ** 25, out=C.byref(handle))
    keep = [good, arr(0.5, 0.25, 0.0, 0.0), arr(0.5, math.nan, 0.0, 1.0), arr(math.inf, 0.25, 0.0, 1.0),
            np.zeros(17), arr(2.0 ** 40, 1.0), arr(0.0, 2.0 ** 40)]
    create.refused([
        dict(n=3000), dict(n=8192, np=7), dict(np=0), dict(n=1024, np=1, primes=1, degree=1),
        dict(degree=0), dict(coeff=hptr(keep[4]), degree=16),
        dict(coeff=hptr(keep[1])),                                          # a_D = 0
        dict(coeff=hptr(keep[2])), dict(coeff=hptr(keep[3])),
        dict(scale_in=math.nan), dict(scale_out=math.inf), dict(scale_in=0.0), dict(scale_out=-1.0),
        dict(primes=3), dict(primes=6), dict(primes=0),                     # depth(3) + 2 = 4 .. np - 1 = 5
        dict(coeff=hptr(keep[5]), degree=1, scale_out=2.0 ** 30),           # |c_after| = 2^70
        dict(coeff=hptr(keep[6]), degree=1, scale_out=2.0 ** 30),           # |w_1| about 2^70
        dict(coeff=None), dict(out=None)])
    assert handle.value == 0xDEAD
    # 4096 x 3 reaches degree 1 only, at L = 2
    assert create(n=4096, np=3, primes=2, degree=1) == 0 and handle.value not in (None, 0xDEAD)
    L.se_amd_poly_destroy(handle)
    handle.value = 0xDEAD
    create.refused([dict(n=4096, np=3, primes=2, degree=2), dict(n=4096, np=3, primes=3, degree=1)])
    # the edges that pass: primes = depth + 2 and np - 1
    for primes in (4, 5):
        assert create(primes=primes) == 0
        L.se_amd_poly_destroy(handle)
    L.se_amd_poly_destroy(None)
    assert L.se_amd_poly_terms(None, None, None, None, None, 0) == 0 and L.se_amd_poly_workspace_bytes(None, 5) == 0


def test_the_models_rescale_of_a_weighted_sum_is_integer_division():
    """A constructed record at 4096 x 3, level 3: two terms whose residues are those of known integer polynomials U, V
    (|coefficients| < 2^40), so sum_t w_t term_t is the residue image of Y = w_0 U + w_1 V; the model's output must be the
    residues of round(Y / q_2) + c_after -- (Y - centred(Y mod q_2)) / q_2 in Python integers -- on both slabs."""
    from oracle import pyoracle
    pyoracle.build(ref=False)
    n, npr, primes = 4096, 3, 3
    o = pyoracle.Oracle(n, npr)
    q = o.q
    rng = np.random.default_rng(83)
    ints = [[int(v) for v in rng.integers(-2 ** 40, 2 ** 40, n)] for _ in range(4)]          # U0, V0 (slab 0), U1, V1
    slab = lambda y: np.stack([o.ntt(np.array([v % q[j] for v in y], dtype=np.uint32), j) for j in range(npr)])[None]  # noqa: E731
    w, c_after = [3 * 2 ** 30 + 5, -(2 ** 31) - 7], -12345
    out0, out1 = affine_rescale_expect(o, [slab(ints[0]), slab(ints[1])], [slab(ints[2]), slab(ints[3])], w, c_after, primes)
    for out, (u, v), c in ((out0, ints[:2], c_after), (out1, ints[2:], 0)):
        y = [w[0] * a + w[1] * b for a, b in zip(u, v)]
        assert max(abs(t) for t in y) < q[0] * q[1] * q[2] // 2
        delta = centred(np.array([t % q[2] for t in y], dtype=np.uint32), q[2])
        quo = [(t - int(dl)) // q[2] for t, dl in zip(y, delta)]
        assert all((t - int(dl)) % q[2] == 0 for t, dl in zip(y, delta))
        got = crt_centred(q[:2], [o.intt(out[0, j], j) for j in range(2)])
        assert got[0] == quo[0] + c                    # the constant polynomial lands on coefficient 0 alone
        assert got[1:] == quo[1:]
