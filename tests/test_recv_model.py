"""The constructed plaintexts of the receiving side (tests/recv_model.py) checked on the CPU: the constructors run their
own Python-integer assertions (which prime decides, that the plant alone decides), every record decrypts through the
oracle's primitives to the planted integers in both degrees, and the level expectation cuts the chain where it says."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vectors as V
from gpu_support import expectation, ntt_secret
from recv_model import (H, SHAPES, chain_products, ciphertext_of, edge_values, expect_at_level, in_range_vectors,
                        oracle_route, out_of_range_vectors, plant_positions)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE_IDS = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


@pytest.fixture(scope="module")
def cases():
    """cases(shape) -> the oracle, a key's NTT form and the named vectors of the shape, built once."""
    from oracle import pyoracle
    pyoracle.build(ref=False)
    cache = {}

    def get(shape):
        if shape not in cache:
            o = pyoracle.Oracle(*shape)
            inside = in_range_vectors(o)
            outside = out_of_range_vectors(o) if o.np >= 3 else []
            cache[shape] = dict(o=o, s_hat=ntt_secret(o, V.secret_key(o.n, seed=3)), inside=inside, outside=outside)
        return cache[shape]

    return get


def test_model_imports_neither_torch_nor_pytest():
    code = ("import sys; sys.path[:0] = [%r, %r]; import recv_model; "
            "assert not {'torch', 'pytest', 'seal_embedded_amd'} & set(sys.modules)"
            % (os.path.join(ROOT, "tests"), ROOT))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_constructed_vectors(cases, shape):
    """What the constructors promise beyond their own assertions: the in-range record holds each edge value at a low and
    at a high index; an out-of-range record differs from the in-range background in one coefficient, and the plants
    visit every position of plant_positions once there are eight of them."""
    c = cases(shape)
    o, n = c["o"], shape[0]
    name, vec = c["inside"][0]
    assert name == "multiples" and len(vec) == n and vec[0] == 0 and vec[1] == 1 and vec[2] == -1
    Q = chain_products(o)[o.np]
    vals = edge_values(o)
    assert vec[:len(vals)] == vals and vec[n - len(vals):] == vals and len(set(vals)) == len(vals)
    if o.np >= 3:
        assert H - 1 in vec and all(m * o.q[j] in vec for j in range(o.np) for m in (1, -1, 7, -7))
    else:
        assert max(vec) == (Q - 1) // 2 and min(vec) == -(Q - 1) // 2
    assert c["inside"][1] == ("zero", [0] * n)
    if o.np < 3:
        return
    recs = c["outside"]
    assert len(recs) == 6 + 2 * max(0, o.np - 3)
    for r in recs:
        diff = [k for k in range(n) if r["vec"][k] != recs[0]["vec"][k]]
        assert set(diff) <= {r["pos"], recs[0]["pos"]} and r["vec"][r["pos"]] == r["value"], r["name"]
        assert -Q // 2 < r["value"] <= Q // 2 and not -H <= r["value"] < H
    assert [r["pos"] for r in recs[:8]] == plant_positions(n)[:len(recs)]
    assert sorted({r["prime"] for r in recs}) == list(range(2, o.np))          # every later prime decides a record


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("degree", [1, 2])
def test_records_decrypt_to_the_planted_integers(cases, shape, degree):
    """ciphertext_of, then the oracle route (o.decrypt, o.intt, crt_centred; for degree 2 the same step twice), gives
    back every vector; expect_at_level(np) is the vector itself, with the status gpu_support.expectation computes."""
    c = cases(shape)
    o, s_hat = c["o"], c["s_hat"]
    rng = np.random.default_rng(17 * shape[0] + shape[1] + degree)
    named = c["inside"] + [(r["name"], r["vec"]) for r in c["outside"]]
    for i, (name, vec) in enumerate(named):
        rows = ciphertext_of(o, vec, s_hat, rng, degree)
        assert len(rows) == degree + 1 and all(r.shape == (o.np, o.n) and r.dtype == np.uint32 for r in rows)
        for r in rows[1:]:
            assert all((r[j] < o.q[j]).all() and {0, 1, o.q[j] - 1} <= set(r[j][[2, o.n // 2 + 1, o.n - 2]].tolist())
                       for j in range(o.np))
        status, y = expect_at_level(o, vec, o.np)
        assert y == vec and status == (1 if i < len(c["inside"]) else 0), name
        if degree == 1:
            e = expectation(o, rows[0], rows[1], s_hat)
            assert e["y"] == vec and e["status"] == status, name
        else:
            assert oracle_route(o, rows, s_hat) == vec, name


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] >= 4], ids=SHAPE_IDS)
def test_levels_cut_the_chain(cases, shape):
    """A record 12345 + Q'_j is 12345 at level j (status 1) and out of range at level j + 1; -7 q_j - Q'_j likewise with
    -7 q_j.  At the levels 1 and 2 every record is in range (Q'_2 < 2^60)."""
    c = cases(shape)
    o = c["o"]
    for r in c["outside"]:
        for p in (1, 2):
            assert expect_at_level(o, r["vec"], p)[0] == 1
        if not r["name"].startswith(("12345+", "-7q_")):
            continue
        j = r["prime"]
        status, y = expect_at_level(o, r["vec"], j)
        assert status == 1 and y[r["pos"]] == (12345 if r["value"] > 0 else -7 * o.q[j]), r["name"]
        assert [v for k, v in enumerate(y) if k != r["pos"]] == [v for k, v in enumerate(r["vec"]) if k != r["pos"]]
        assert expect_at_level(o, r["vec"], j + 1)[0] == 0, r["name"]
