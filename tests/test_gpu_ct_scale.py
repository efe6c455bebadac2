"""The ciphertext entries at scale (-m gpu): every entry of include/seal_embedded_amd.h that works on ciphertext records,
held to the host model bit for bit on EVERY record of a batch that fills the chip (tier A) and of a batch whose slabs
reach past word 2^32 (tier B).

A case is K distinct records (3 for n <= 4096, 2 above) built from ct_model's constructed inputs -- record 0 carries the
family's edge row, record 1 is all q_j - 1, the rest is random -- with random key words, the elements [3, n + 1] and
edge_diagonals.  Its expectation comes from the host model alone (ct_model and its companions, gpu_support.expectation
for the decrypts), never from a small call of the library.  The K records are tiled to B on the device (gpu_support.tiled:
record b is base[b % K]), the entry is called ONCE, and assert_tiles compares all B output records, the status bytes and
the guard words behind every output on the device.  Index lists and CSR rows repeat a local pattern per tile
(tiled_row_ptr, tiled_idx, tiled_entries), so that a row of tile t reads records of tile t alone and the outputs are
periodic too.  gpu_support's CPU test (tests/test_tiled_support.py) shows that the comparator cannot pass a wrong slab.

Tier A: B is the smallest multiple of the tile for which a (B, L) grid has at least 4 x 256 x (2048 / (n / 16))
workgroups, four rounds of the densest residency 256 compute units allow; the element-wise entries use the same B.
Several workgroups then share every compute unit, which none of the small bit-exact cases of the other modules reaches.

Tier B: 4096 x 3 (L = 3; L = 2 for the special-prime family), B so large that in every slab of the call at least one
whole tile lies past word 2^32; since every record is compared, byte 2^32 and word 2^31 are covered by the same run.  The
slabs are views of one pool that a module fixture allocates once; to stay at or under 96 GiB a call passes one input slab
for both halves (the headers forbid only outputs that overlap inputs) -- tier A keeps the halves distinct -- and the stack
sums take their one-slab form.  What departs from that, and why:
  - ct_galois_many_ext_sp: two elements of extended outputs would be 4 x 25.8 GB beside the input.  Its slabs cross byte
    2^32 and word 2^31 instead (B = 262 149, an 8.6 GB input); the [G][B] output stacks still reach past word 2^32, in
    the plane of the second element.
  - decrypt_level (at np and np - 1 primes) and decrypt3_level: the input halves cannot be one slab (c0 + c1 s of one
    uniform slab fits no int64, and the outputs of such a record are not defined), so at B = 524 292 the input slabs
    reach past word 2^32 while pte crosses element 2^31 and values, values_f64 cross byte 2^32; outputs past element
    2^32 would need inputs of more than 100 GB.  values_f64 is taken by a second call on the same batch.
  - ct_affine_rescale: three terms read the one level-3 slab with primes = 3 (mixed levels need a slab per level; tier A
    has them).
  - ct_lincomb with a row cut into S = 2 slices: the library allocates partial rows of its own, slabs x G x S records
    (32 GiB for one slab), so the call takes the one-slab form, runs last, and gives the pool up for a buffer of its own
    16 + 16 GiB: 66 GiB in all.
  - ct_poly_sp is left out: its workspace grows with B.
"""
import math

import numpy as np
import pytest

import vectors as V
from ct_model import (accum_expect, bsgs_expect, edge_diagonals, edge_row, galois_expect, galois_sp_expect, hoist_expect,
                      hoist_sp_expect, lincomb_expect, lintrans_expect, modular_sum, rand_key, rand_slab, random_keys,
                      relin_expect, relin_sp_expect, rescale_expect, stack_sum_expect)
from ct_model_bsgs_sp import (accum_sp_expect, bsgs_sp_expect, many_ext_expect, mod_down_expect, stack_sum_ext_expect)
from ct_model_dot import dot_sp_expect, mul_sum_expect
from ct_model_pack import pack_expect
from ct_model_poly import affine_rescale_expect, poly_expect, poly_schedule
from ct_model_switch import random_ring, switch_expect, switch_sum_expect
from gpu_support import (SENTINEL, assert_tiles, dev_t, env, expectation, fresh_records, host_u32,  # noqa: F401
                         ntt_secret, tiled, tiled_entries, tiled_idx, tiled_row_ptr, unit_values)

pytestmark = pytest.mark.gpu

GIB = 1 << 30
POOL_BYTES = 92 * GIB + (64 << 20)    # the slabs of the largest tier B call (decrypt3_level: 92.0 GiB)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def tile_of(n):
    return 3 if n <= 4096 else 2


def workgroups_needed(n):
    """Four rounds of the densest residency: 2048 threads per compute unit in workgroups of n / 16, 256 units."""
    return 4 * 256 * (2048 // (n // 16))


def chip_filling_batch(n, L, tile, launched):
    """The smallest multiple of `tile` for which the smallest launch of the call, launched(L, B, tile) workgroups, has at least
    workgroups_needed(n) of them."""
    B = tile
    while launched(L, B, tile) < workgroups_needed(n):
        B += tile
    return B


def launches(launched):
    """Marks a spec with the workgroups of the smallest launch its entry makes for B records in tiles of K at level L, read off the
    launch_* functions of kernels/ct_ops.hip, ct_pack.hip, ct_poly.hip and encode_encrypt.hip and the chunk walks of
    se_context.cpp.  An unmarked spec launches a (B, L) grid (evk_grid(B, primes)), or is one of the 256-thread
    element-wise kernels, which take the B of the transform kernels at their shape."""
    def mark(spec):
        spec.launched = launched
        return spec
    return mark


def launched_by(spec):
    return getattr(spec, "launched", lambda L, B, K: B * L)


class Stack:
    """Marks a host array [G][k]... whose device form is [G][tiles . k]...: every plane is tiled on its own."""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a)


# ---- the cases: one context per shape with every key installed, K records per family and level ----------------------
class Case:
    def __init__(self, env, shape):
        from oracle.pyoracle import Oracle
        self.env, self.shape = env, shape
        self.n, self.npr = shape
        self.K = tile_of(self.n)
        self.o = Oracle(*shape)
        self.q = self.o.q
        self.ctx = env["pkg"].Context(*shape)
        self.rng = np.random.default_rng(59 * self.n + self.npr)
        self.elts = [3, self.n + 1]
        self.table = env["pkg"].galois_table
        self.memo = {}

    def once(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def top(self, L):
        return (np.array(self.q[:L], dtype=np.uint32) - 1)[:, None]

    def slabs(self, L, edges):
        """Four slabs [K][L][n]: slabs 1 and 3 (the second halves of a call) carry the edge rows in record 0; record 1 of
        every slab is all q_j - 1."""
        def make():
            s = [rand_slab(self.rng, self.q, self.K, self.n, L) for _ in range(4)]
            for j in range(L):
                s[1][0, j] = edge_row(self.o, j, self.rng, self.elts, edges=edges)
                s[3][0, j] = edge_row(self.o, j, self.rng, self.elts, edges=edges)
            for x in s:
                x[1] = self.top(L)
            return s
        return self.once(("slabs", L, edges), make)

    def ext_slabs(self, L):
        """Two stacks [2][K][L + 1][n] of extended records (row L modulo the special prime): stack 1 carries the centring
        edges on the row at the special prime; record 1 of every plane is all q - 1."""
        def make():
            p, out = self.npr - 1, []
            rows = list(range(L)) + [p]
            for h in range(2):
                s = np.stack([self.rng.integers(0, self.q[i], (2, self.K, self.n), dtype=np.uint32) for i in rows], axis=2)
                s[:, 1] = (np.array([self.q[i] for i in rows], dtype=np.uint32) - 1)[:, None]
                if h == 1:
                    s[0, 0, L] = edge_row(self.o, p, self.rng, self.elts, edges="centring")
                    s[1, self.K - 1, L] = edge_row(self.o, p, self.rng, self.elts, edges="centring")
                out.append(s)
            return out
        return self.once(("ext", L), make)

    # digit keys: the Galois keys of [3, n + 1] and a relinearisation key
    def digit(self):
        def make():
            gk0, gk1 = random_keys(self.rng, self.q, 2, self.n, self.npr)
            rk0, rk1 = random_keys(self.rng, self.q, 1, self.n, self.npr)
            self.ctx.set_galois_keys(self.elts, gk0, gk1)
            self.ctx.set_relin_key(rk0[0], rk1[0])
            return dict(gk=(gk0, gk1), rk=(rk0[0], rk1[0]), key_of={g: k for k, g in enumerate(self.elts)})
        return self.once("digit", make)

    # special-prime keys: the Galois keys of [3, n + 1], a relinearisation key and a switch ring of three keys
    def sp(self):
        def make():
            p = self.npr - 1
            gk0 = np.stack([rand_key(self.rng, self.q, self.n) for _ in self.elts])
            gk1 = np.stack([rand_key(self.rng, self.q, self.n) for _ in self.elts])
            for k in (gk0[0], gk1[1]):
                k[0, 0, :4] = [0, 1, self.q[0] - 1, self.q[0] - 1]
                k[0, p, :4] = [0, 1, self.q[p] - 1, self.q[p] - 1]
            rk = rand_key(self.rng, self.q, self.n), rand_key(self.rng, self.q, self.n)
            ring = random_ring(self.rng, self.q, 3, self.n)
            self.ctx.set_galois_keys_sp(self.elts, gk0, gk1)
            self.ctx.set_relin_key_sp(*rk)
            self.ctx.set_switch_keyring_sp(*ring)
            return dict(keys={g: (gk0[k], gk1[k]) for k, g in enumerate(self.elts)}, rk=rk, ring=ring)
        return self.once("sp", make)

    def rotations(self, L, x0, x1, tag):
        """The many form's expectation, shared by the sum form and the linear transform."""
        d = self.digit()
        return self.once(("rot", L, tag), lambda: hoist_expect(self.table, self.o, x0, x1, self.elts, d["key_of"], *d["gk"]))

    def close(self):
        """The plans first, then the context with the keys and the scratch it holds on the device."""
        for plan in self.memo.pop("plans", []):
            plan.close()
        self.memo.clear()
        self.ctx.close()

    # real records under an installed secret key, for the decrypts
    def fresh(self):
        def make():
            env, ctx, o = self.env, self.ctx, self.o
            sk = V.secret_key(self.n, seed=5)
            ctx.set_secret_key(sk)
            c0, c1 = fresh_records(env, ctx, unit_values(self.K, self.n, 7000 + self.n), 300)
            t = [env["torch"].empty_like(c0) for _ in range(3)]
            ctx.ct_mul(c0, c1, c0, c1, *t)                               # inputs of decrypt3_level: the squares
            env["torch"].cuda.synchronize()
            return dict(s_hat=ntt_secret(o, sk), c=(host_u32(c0), host_u32(c1)), t=tuple(host_u32(x) for x in t))
        return self.once("fresh", make)


@pytest.fixture(scope="module")
def cases(env):
    """cases(shape) -> the Case of that shape, made once; cases.only(shape) closes the others (tier B keeps 4096 x 3)."""
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = Case(env, shape)
        return cache[shape]

    def only(shape):
        for other in [s for s in cache if s != shape]:
            cache.pop(other).close()
        return get(shape)

    get.only = only
    yield get
    for c in cache.values():
        c.close()


def keep(c, plan):
    """A plan lives as long as its case (Case.close closes it before the context)."""
    c.memo.setdefault("plans", []).append(plan)
    return plan


# ---- the entries: spec(c, L, alias, tier) -> what one call reads, what it must write, and the call ------------------
# A spec is dict(tile=records per tile, ins={name: host [k]... | Stack}, outs={name: expectation [k]... | Stack},
# status=uint8 [k] | None, work=bytes as a function of B | None, call=f(t) on the dict of device tensors by name,
# with t["B"], t["tiles"], t["status"], t["work"], t["work_bytes"]).  The same host array under two names is ONE device slab.
def halves(s, alias):
    """(c0, c1) of a call: two slabs, or with alias the slab of the edge rows for both."""
    return (s[1], s[1]) if alias else (s[0], s[1])


def spec_relin(c, L, alias, tier):
    s, rk = c.slabs(L, "digit"), c.digit()["rk"]
    d0, d1, d2 = (s[1], s[1], s[1]) if alias else (s[0], s[2], s[1])
    e0, e1 = relin_expect(c.o, d0, d1, d2, *rk)
    return dict(ins=dict(d0=d0, d1=d1, d2=d2), outs=dict(out0=e0, out1=e1),
                call=lambda t: c.ctx.ct_relin(t["d0"], t["d1"], t["d2"], t["out0"], t["out1"], primes=L))


def spec_galois(c, L, alias, tier):
    x0, x1 = halves(c.slabs(L, "digit"), alias)
    gk0, gk1 = c.digit()["gk"]
    e0, e1 = galois_expect(c.o, x0, x1, 3, gk0[0], gk1[0])
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1),
                call=lambda t: c.ctx.ct_galois(t["c0"], t["c1"], 3, t["out0"], t["out1"], primes=L))


def spec_galois_many(c, L, alias, tier):
    x0, x1 = halves(c.slabs(L, "digit"), alias)
    r0, r1 = c.rotations(L, x0, x1, alias)
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=Stack(r0), out1=Stack(r1)),
                call=lambda t: c.ctx.ct_galois_many(t["c0"], t["c1"], c.elts, t["out0"], t["out1"], primes=L))


def spec_galois_sum(add):
    def spec(c, L, alias, tier):
        x0, x1 = halves(c.slabs(L, "digit"), alias)
        r0, r1 = c.rotations(L, x0, x1, alias)
        e0, e1 = modular_sum(c.o, r0, x0 if add else None), modular_sum(c.o, r1, x1 if add else None)
        return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1), call=lambda t: c.ctx.ct_galois_sum(
            t["c0"], t["c1"], c.elts, t["out0"], t["out1"], add_input=add, primes=L))
    return spec


def spec_lintrans(c, L, alias, tier):
    x0, x1 = halves(c.slabs(L, "digit"), alias)
    rot = c.rotations(L, x0, x1, alias)
    c.digit()
    diag = c.once("diag", lambda: edge_diagonals(c.rng, c.q, 3, c.n))
    plan = c.once("lintrans", lambda: keep(c, c.ctx.lintrans_plan(
        c.elts, dev_t(c.env, diag[1:]), dev_t(c.env, diag[0]))))
    e0, e1 = lintrans_expect(c.o, rot, diag[1:], x0, x1, diag[0])
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1),
                call=lambda t: c.ctx.ct_lintrans(plan, t["c0"], t["c1"], t["out0"], t["out1"], primes=L))


def stacked_halves(s, alias):
    """(in0, in1) [2][K][L][n] of an accumulate call: plane 1 holds other records than plane 0."""
    in1 = np.stack([s[1], s[3]])
    return (in1, in1) if alias else (np.stack([s[0], s[2]]), in1)


def spec_galois_accum(c, L, alias, tier):
    in0, in1 = stacked_halves(c.slabs(L, "digit"), alias)
    d = c.digit()
    e0, e1 = accum_expect(c.o, in0, in1, c.elts, d["key_of"], *d["gk"])
    a0 = Stack(in0)
    return dict(ins=dict(in0=a0, in1=a0 if alias else Stack(in1)), outs=dict(out0=e0, out1=e1),
                call=lambda t: c.ctx.ct_galois_accum(t["in0"], t["in1"], c.elts, t["out0"], t["out1"], primes=L))


def bsgs_lists(c):
    """The 2 x 2 plan: baby steps [1, 3], giant steps [1, n + 1], four diagonals of arbitrary words."""
    return [1, 3], [1, c.n + 1], c.once("bsgs-diag", lambda: edge_diagonals(c.rng, c.q, 4, c.n).reshape(2, 2, c.npr, c.n))


def chunk_records(B, tier):
    """Tier A: a workspace for a quarter of the batch, so that the chunk walk runs; tier B: for 4096 records."""
    return max(1, B // 4) if tier == "A" else 4096


@launches(lambda L, B, K: (B // 4) * L)  # every launch takes a chunk of a quarter of the batch
def spec_bsgs(c, L, alias, tier):
    x0, x1 = halves(c.slabs(L, "digit"), alias)
    d = c.digit()
    baby, giant, diag = bsgs_lists(c)
    plan = c.once("bsgs", lambda: keep(c, c.ctx.bsgs_plan(baby, giant, dev_t(c.env, diag))))
    e0, e1 = bsgs_expect(c.table, c.o, x0, x1, baby, giant, diag, d["key_of"], *d["gk"])
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1),
                work=lambda B: c.ctx.bsgs_workspace_bytes(plan, chunk_records(B, tier), L),
                call=lambda t: c.ctx.ct_bsgs(plan, t["c0"], t["c1"], t["out0"], t["out1"], t["work"], primes=L,
                                             workspace_bytes=t["work_bytes"]))


def spec_relin_sp(c, L, alias, tier):
    s, rk = c.slabs(L, "centring"), c.sp()["rk"]
    d0, d1, d2 = (s[1], s[1], s[1]) if alias else (s[0], s[2], s[1])
    e0, e1 = relin_sp_expect(c.o, d0, d1, d2, *rk)
    return dict(ins=dict(d0=d0, d1=d1, d2=d2), outs=dict(out0=e0, out1=e1),
                call=lambda t: c.ctx.ct_relin_sp(t["d0"], t["d1"], t["d2"], t["out0"], t["out1"], primes=L))


def spec_galois_sp(c, L, alias, tier):
    x0, x1 = halves(c.slabs(L, "centring"), alias)
    e0, e1 = galois_sp_expect(c.o, x0, x1, 3, *c.sp()["keys"][3])
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1),
                call=lambda t: c.ctx.ct_galois_sp(t["c0"], t["c1"], 3, t["out0"], t["out1"], primes=L))


def spec_galois_sum_sp(c, L, alias, tier):
    x0, x1 = halves(c.slabs(L, "centring"), alias)
    keys = c.sp()["keys"]
    e0, e1, _ = hoist_sp_expect(c.o, x0, x1, c.elts, [keys[g] for g in c.elts], w0=1)
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1), call=lambda t: c.ctx.ct_galois_sum_sp(
        t["c0"], t["c1"], c.elts, t["out0"], t["out1"], add_input=True, primes=L))


def spec_lintrans_sp(c, L, alias, tier):
    x0, x1 = halves(c.slabs(L, "centring"), alias)
    keys = c.sp()["keys"]
    diag = c.once("diag-sp", lambda: edge_diagonals(c.rng, c.q, 3, c.n))
    plan = c.once("lintrans-sp", lambda: keep(c, c.ctx.lintrans_plan_sp(
        c.elts, dev_t(c.env, diag[1:]), dev_t(c.env, diag[0]))))
    e0, e1, _ = hoist_sp_expect(c.o, x0, x1, c.elts, [keys[g] for g in c.elts], diag[1:], diag[0])
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1),
                call=lambda t: c.ctx.ct_lintrans_sp(plan, t["c0"], t["c1"], t["out0"], t["out1"], primes=L))


@launches(lambda L, B, K: B * (L + 1))  # a row of workgroups for the special prime
def spec_galois_many_ext_sp(c, L, alias, tier):
    """Tier B falls back to the 8.6 GB rule (`past` = word 2^31 for every slab): two elements of extended outputs past
    word 2^32 would be 4 x 25.8 GB beside the input, over 96 GiB.  The [G][B] output stacks as a whole still reach past
    word 2^32, in the plane of the second element."""
    x0, x1 = halves(c.slabs(L, "centring"), alias)
    e0, e1 = many_ext_expect(c.table, c.o, x0, x1, c.elts, c.sp()["keys"])
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=Stack(e0), out1=Stack(e1)), past=2 ** 31,
                call=lambda t: c.ctx.ct_galois_many_ext_sp(t["c0"], t["c1"], c.elts, t["out0"], t["out1"], primes=L))


def spec_galois_accum_sp(c, L, alias, tier):
    in0, in1 = stacked_halves(c.slabs(L, "centring"), alias)
    e0, e1 = accum_sp_expect(c.o, in0, in1, c.elts, c.sp()["keys"])
    a0 = Stack(in0)
    return dict(ins=dict(in0=a0, in1=a0 if alias else Stack(in1)), outs=dict(out0=e0, out1=e1),
                call=lambda t: c.ctx.ct_galois_accum_sp(t["in0"], t["in1"], c.elts, t["out0"], t["out1"], primes=L))


@launches(lambda L, B, K: B * 2)  # dim3(count, 2): one workgroup per record and slab
def spec_mod_down_sp(c, L, alias, tier):
    ext = c.ext_slabs(L)
    x1 = ext[1][0]
    x0 = x1 if alias else ext[0][0]
    return dict(ins=dict(in0=x0, in1=x1), outs=dict(out0=mod_down_expect(c.o, x0), out1=mod_down_expect(c.o, x1)),
                call=lambda t: c.ctx.ct_mod_down_sp(t["in0"], t["out0"], t["in1"], t["out1"], primes=L, count=t["B"]))


def spec_mul_plain_sum_ext_sp(c, L, alias, tier):
    """Tier B: the one-slab form."""
    ext = c.ext_slabs(L)
    pt = c.once("ext-pt", lambda: edge_diagonals(c.rng, c.q, 4, c.n).reshape(2, 2, c.npr, c.n))
    t_pt = c.once("ext-pt-dev", lambda: dev_t(c.env, pt))
    ins = dict(in0=Stack(ext[1])) if alias else dict(in0=Stack(ext[0]), in1=Stack(ext[1]))
    outs = {f"out{h}": Stack(stack_sum_ext_expect(c.o, ins[f"in{h}"].a, pt)) for h in range(len(ins))}
    return dict(ins=ins, outs=outs, call=lambda t: c.ctx.ct_mul_plain_sum_ext_sp(
        t["in0"], t_pt, t["out0"], t.get("in1"), t.get("out1"), primes=L))


def ring_tile(c, s):
    """A tile in which every key of the ring of three meets a record: K records repeated to lcm(K, 3), key b mod 3."""
    T = c.K * 3 // math.gcd(c.K, 3)
    return T, [np.concatenate([x] * (T // c.K)) for x in s], np.arange(T, dtype=np.uint32) % 3


def spec_switch_keyed_sp(c, L, alias, tier):
    T, s, key_idx = ring_tile(c, c.slabs(L, "centring"))
    x0, x1 = halves(s, alias)
    e0, e1 = switch_expect(c.o, x0, x1, key_idx, *c.sp()["ring"])
    return dict(tile=T, ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1), status=np.ones(T, dtype=np.uint8),
                call=lambda t: c.ctx.ct_switch_keyed_sp(t["c0"], t["c1"], tiled_entries(c.env, key_idx, t["tiles"]),
                                                        t["out0"], t["out1"], primes=L, status=t["status"]))


def csr_of(env, rows, tile, tiles):
    """Local rows (lists of record indices of one tile) -> row_ptr, idx on the device for `tiles` tiles."""
    ptr = np.cumsum([0] + [len(r) for r in rows])
    return tiled_row_ptr(env, ptr, tiles), tiled_idx(env, [b for r in rows for b in r], tile, tiles)


@launches(lambda L, B, K: (B // K) * (2 if K == 3 else 3) * L)  # a (rows, L) grid: 2 rows per tile of 3, 3 per tile of 6
def spec_switch_sum_keyed_sp(c, L, alias, tier):
    """Rows of 2 and 3 records."""
    T, s, key_idx = ring_tile(c, c.slabs(L, "centring"))
    x0, x1 = halves(s, alias)
    rows = [[0, 1], [2, 1, 0]] if T == 3 else [[0, 1], [2, 3, 4], [5, 4]]
    e0, e1, _ = switch_sum_expect(c.o, x0, x1, key_idx, rows, *c.sp()["ring"])

    def call(t):
        row_ptr, idx = csr_of(c.env, rows, T, t["tiles"])
        c.ctx.ct_switch_sum_keyed_sp(t["c0"], t["c1"], tiled_entries(c.env, key_idx, t["tiles"]), row_ptr, idx,
                                     t["out0"], t["out1"], primes=L, status=t["status"])
    return dict(tile=T, ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1), status=np.ones(len(rows), dtype=np.uint8),
                call=call)


@launches(lambda L, B, K: (B // K) * 2 * L)  # a (rows, L) grid, two rows per tile
def spec_pack_sp(c, L, alias, tier):
    """Elements [1, 3, n + 1]; row 0 holds an identity entry, row 1 lists element 3 twice."""
    x0, x1 = halves(c.slabs(L, "centring"), alias)
    keys, K = c.sp()["keys"], c.K
    elts = [1] + c.elts
    rows = [[(0, 0), (1, 1)], [(K - 1, 1), (0, 1), (1, 2)]]
    e0, e1, _ = pack_expect(c.o, x0, x1, elts, rows, [None] + [keys[g] for g in c.elts])

    def call(t):
        row_ptr, idx = csr_of(c.env, [[b for b, _ in r] for r in rows], K, t["tiles"])
        eidx = tiled_entries(c.env, np.array([e for r in rows for _, e in r], dtype=np.uint32), t["tiles"])
        c.ctx.ct_pack_sp(t["c0"], t["c1"], elts, eidx, t["out0"], t["out1"], primes=L, row_ptr=row_ptr, idx=idx,
                         status=t["status"])
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1), status=np.ones(len(rows), dtype=np.uint8), call=call)


def pair_rows(K):
    """Rows of 1 and 3 pairs (ia, ib) of one tile."""
    return [[(0, 0)], [(1, 1), (K - 1, 0), (0, 1)]]


def pair_sides(s, alias):
    return (s[1], s[1], s[1], s[1]) if alias else (s[0], s[1], s[2], s[3])


def pair_csr(c, rows, t):
    row_ptr, ia = csr_of(c.env, [[a for a, _ in r] for r in rows], c.K, t["tiles"])
    return row_ptr, ia, tiled_idx(c.env, [b for r in rows for _, b in r], c.K, t["tiles"])


@launches(lambda L, B, K: (B // K) * 2 * L)  # a (rows, L) grid, two rows per tile
def spec_dot_sp(c, L, alias, tier):
    a0, a1, b0, b1 = pair_sides(c.slabs(L, "centring"), alias)
    rows = pair_rows(c.K)
    e0, e1, _ = dot_sp_expect(c.o, a0, a1, b0, b1, rows, *c.sp()["rk"])
    return dict(ins=dict(a0=a0, a1=a1, b0=b0, b1=b1), outs=dict(out0=e0, out1=e1), status=np.ones(2, dtype=np.uint8),
                call=lambda t: c.ctx.ct_dot_sp(t["a0"], t["a1"], t["b0"], t["b1"], *pair_csr(c, rows, t), t["out0"],
                                               t["out1"], primes=L, status=t["status"]))


@launches(lambda L, B, K: (B // 4) * min(L, 4))  # chunks of a quarter; ct_mod_down_sp launches (2 . chunk, 2)
def spec_bsgs_sp(c, L, alias, tier):
    x0, x1 = halves(c.slabs(L, "centring"), alias)
    keys = c.sp()["keys"]
    baby, giant, diag = bsgs_lists(c)
    plan = c.once("bsgs-sp", lambda: keep(c, c.ctx.bsgs_plan_sp(baby, giant, dev_t(c.env, diag))))
    e0, e1 = bsgs_sp_expect(c.table, c.o, x0, x1, baby, giant, diag, keys)
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1),
                work=lambda B: c.ctx.bsgs_workspace_bytes(plan, chunk_records(B, tier), L),
                call=lambda t: c.ctx.ct_bsgs_sp(plan, t["c0"], t["c1"], t["out0"], t["out1"], t["work"], primes=L,
                                                workspace_bytes=t["work_bytes"]))


@launches(lambda L, B, K: B * 2)  # its rescales and the affine step launch dim3(B, 2)
def spec_poly_sp(c, L, alias, tier):
    """A degree-3 plan."""
    x0, x1 = halves(c.slabs(L, "centring"), alias)
    coeff, scale_in, scale_out = [0.25, -0.5, 0.75, 1.0], float(c.q[L - 1]), 2.0 ** 25
    sched = poly_schedule(c.q, L, coeff, scale_in, scale_out)
    plan = c.once("poly", lambda: keep(c, c.env["pkg"].poly_create(c.n, c.npr, L, coeff, scale_in, scale_out)))
    e0, e1, _ = poly_expect(c.o, x0, x1, sched, *c.sp()["rk"])
    return dict(ins=dict(c0=x0, c1=x1), outs=dict(out0=e0, out1=e1), work=lambda B: plan.workspace_bytes(B),
                call=lambda t: c.ctx.ct_poly_sp(plan, t["c0"], t["c1"], t["out0"], t["out1"], t["work"],
                                                workspace_bytes=t["work_bytes"]))


@launches(lambda L, B, K: B * 2)  # dim3(B, 2)
def spec_rescale(c, L, alias, tier):
    """Two slabs; the centring edges stand on the row that is divided out."""
    def make():
        s = [x.copy() for x in c.slabs(L, "digit")[:2]]
        s[1][0, L - 1] = edge_row(c.o, L - 1, c.rng, c.elts, edges="centring")
        return s
    x0, x1 = halves(c.once(("rescale", L), make), alias)
    return dict(ins=dict(in0=x0, in1=x1), outs=dict(out0=rescale_expect(c.o, x0), out1=rescale_expect(c.o, x1)),
                call=lambda t: c.ctx.ct_rescale(t["in0"], t["out0"], t["in1"], t["out1"], primes=L))


@launches(lambda L, B, K: B * 2)  # dim3(B, 2)
def spec_affine_rescale(c, L, alias, tier):
    """Three terms and a constant.  Tier A: at the levels L - 1, L, L - 1 with primes = L - 1 (a wrong record stride reads
    other rows); tier B: three times the one level-L slab with primes = L."""
    s = c.slabs(L, "digit")
    w, c_after = [c.q[0] - 1, -(2 ** 62 - 1), 3], -1
    if alias:
        primes, terms0, terms1 = L, [s[1]] * 3, [s[1]] * 3
    else:
        low = c.once(("affine", L), lambda: [np.ascontiguousarray(x[:, :L - 1]) for x in s])
        primes, terms0, terms1 = L - 1, [low[0], s[2], low[3]], [low[1], s[3], low[2]]
    e0, e1 = affine_rescale_expect(c.o, terms0, terms1, w, c_after, primes)
    ins = {f"t{h}{k}": x for h, terms in enumerate((terms0, terms1)) for k, x in enumerate(terms)}
    return dict(ins=ins, outs=dict(out0=e0, out1=e1), call=lambda t: c.ctx.ct_affine_rescale(
        [t[f"t0{k}"] for k in range(3)], [t[f"t1{k}"] for k in range(3)], w, c_after, t["out0"], t["out1"], primes))


def decrypt_expect(c, primes, scale, c0, c1, c2=None):
    """The oracle's decrypt of the K records at `primes` rows -> pte, values, values_f64 [K]...; every record must fit."""
    from oracle.pyoracle import Oracle
    lo, s_hat = Oracle(c.n, primes), c.fresh()["s_hat"][:primes]
    if c2 is not None:                                                   # c0 + s (c1 + s c2): the inner bracket first
        c1 = np.stack([np.stack([lo.decrypt(c1[b, j], c2[b, j], s_hat[j], j) for j in range(primes)]) for b in range(c.K)])
    es = [expectation(lo, c0[b], c1[b], s_hat, scale) for b in range(c.K)]
    assert all(e["status"] == 1 for e in es)
    return {f: np.stack([e[f] for e in es]) for f in ("pte", "values", "values_f64")}


def spec_decrypt(drop, cubic=False, want=("pte", "values", "values_f64")):
    """decrypt_level at primes = np - drop, or decrypt3_level on the squares of the records; one workgroup per record
    (dim3(B)).  Tier B asks pte and values of one call and values_f64 of a second (`want`).
    Tier B falls back: the halves cannot be one slab (c0 + c1 s of one uniform slab fits no int64, and what such a
    record decrypts to is not defined), so only the input slabs reach past word 2^32; pte must cross element 2^31 and
    values, values_f64 byte 2^32 (`past`, in elements).  Outputs past element 2^32 would need inputs of over 100 GB."""
    def spec(c, L, alias, tier):
        f, primes = c.fresh(), L - drop
        src = f["t"] if cubic else f["c"]
        slabs = c.once(("dec", primes, cubic), lambda: [np.ascontiguousarray(x[:, :primes]) for x in src])
        scale = c.ctx.scale() ** 2 if cubic else c.ctx.scale() * 1.25
        exp = c.once(("dec-exp", primes, cubic), lambda: decrypt_expect(c, primes, scale, *slabs))
        ins = {f"c{k}": x for k, x in enumerate(slabs)}

        def call(t):
            kw = dict({k: t[k] for k in want}, status=t["status"])
            if cubic:
                c.ctx.decrypt3_level(t["c0"], t["c1"], t["c2"], primes, scale, **kw)
            else:
                c.ctx.decrypt_level(t["c0"], t["c1"], primes, scale, **kw)
        return dict(ins=ins, outs={k: exp[k] for k in want}, status=np.ones(c.K, dtype=np.uint8), call=call,
                    past={"pte": 2 ** 31, "values": 2 ** 30, "values_f64": 2 ** 29})
    return launches(lambda L, B, K: B)(spec)


def spec_mul_plain(c, L, alias, tier):
    """Indexed plaintexts: two of them, plaintext 1 all q_j - 1, the records of a tile take 1, 0, 1."""
    x0, x1 = halves(c.slabs(L, "digit"), alias)

    def make():
        pt = rand_slab(c.rng, c.q, 2, c.n)
        pt[1] = c.top(c.npr)
        return pt, dev_t(c.env, pt)
    pt, t_pt = c.once("pt", make)
    pidx = np.array([1, 0, 1][:c.K], dtype=np.uint32)
    e0, e1 = (np.stack([stack_sum_expect(c.o, x[None, b:b + 1], pt[None, pidx[b]:pidx[b] + 1])[0, 0] for b in range(c.K)])
              for x in (x0, x1))
    return dict(ins=dict(in0=x0, in1=x1), outs=dict(out0=e0, out1=e1), status=np.ones(c.K, dtype=np.uint8),
                call=lambda t: c.ctx.ct_mul_plain(t["in0"], t_pt, t["out0"], t["in1"], t["out1"],
                                                  pt_idx=tiled_entries(c.env, pidx, t["tiles"]), primes=L,
                                                  status=t["status"]))


def spec_mul(c, L, alias, tier):
    """Index lists: pair p of a tile is (ia[p], ib[p]) of that tile."""
    a0, a1, b0, b1 = pair_sides(c.slabs(L, "digit"), alias)
    rows = [[(1, 2 % c.K)], [(0, 1)], [(2 % c.K, 0)]][:c.K]
    e = mul_sum_expect(c.o, a0, a1, b0, b1, rows)

    def call(t):
        ia = tiled_idx(c.env, [r[0][0] for r in rows], c.K, t["tiles"])
        ib = tiled_idx(c.env, [r[0][1] for r in rows], c.K, t["tiles"])
        c.ctx.ct_mul(t["a0"], t["a1"], t["b0"], t["b1"], t["out0"], t["out1"], t["out2"], ia=ia, ib=ib, primes=L,
                     status=t["status"])
    return dict(ins=dict(a0=a0, a1=a1, b0=b0, b1=b1), outs=dict(out0=e[0], out1=e[1], out2=e[2]),
                status=np.ones(c.K, dtype=np.uint8), call=call)


def spec_mul_sum(c, L, alias, tier):
    a0, a1, b0, b1 = pair_sides(c.slabs(L, "digit"), alias)
    rows = pair_rows(c.K)
    e = mul_sum_expect(c.o, a0, a1, b0, b1, rows)
    return dict(ins=dict(a0=a0, a1=a1, b0=b0, b1=b1), outs=dict(out0=e[0], out1=e[1], out2=e[2]),
                status=np.ones(2, dtype=np.uint8),
                call=lambda t: c.ctx.ct_mul_sum(t["a0"], t["a1"], t["b0"], t["b1"], *pair_csr(c, rows, t), t["out0"],
                                                t["out1"], t["out2"], primes=L, status=t["status"]))


def spec_mul_plain_sum(c, L, alias, tier):
    """Stacks of two planes, two output planes.  Tier B: the one-slab form."""
    s = c.slabs(L, "digit")
    pt = c.once("sum-pt", lambda: edge_diagonals(c.rng, c.q, 4, c.n).reshape(2, 2, c.npr, c.n))
    t_pt = c.once("sum-pt-dev", lambda: dev_t(c.env, pt))
    in1 = Stack(np.stack([s[1], s[3]]))
    ins = dict(in0=in1) if alias else dict(in0=Stack(np.stack([s[0], s[2]])), in1=in1)
    outs = {f"out{h}": Stack(stack_sum_expect(c.o, ins[f"in{h}"].a, pt)) for h in range(len(ins))}
    return dict(ins=ins, outs=outs, call=lambda t: c.ctx.ct_mul_plain_sum(
        t["in0"], t_pt, t["out0"], t.get("in1"), t.get("out1"), primes=L))


def spec_lincomb(split):
    def spec(c, L, alias, tier):
        """K rows of 3 entries per tile, a repeated record in each, weights at the edges of int32.  A row cut into S > 1
        slices goes through partial rows that the library allocates itself, slabs x G x S records of them (`scratch`);
        tier B therefore takes the one-slab form for S = 2."""
        assert L == c.npr
        x0, x1 = halves(c.slabs(L, "digit"), alias)
        K, two = c.K, not (alias and split > 1)
        ws = [INT32_MIN, INT32_MAX, -1, 1, 0, INT32_MAX, INT32_MIN, -1, 1]
        rows = [[(r, ws[3 * r]), ((r + 1) % K, ws[3 * r + 1]), (r, ws[3 * r + 2])] for r in range(K)]
        model = [([b for b, _ in r], [w for _, w in r]) for r in rows]
        ins, outs = dict(in0=x1), dict(out0=lincomb_expect(x1, c.q, model))
        if two:
            ins, outs = dict(in0=x0, in1=x1), dict(out0=lincomb_expect(x0, c.q, model), out1=outs["out0"])

        def call(t):
            row_ptr, idx = csr_of(c.env, [[b for b, _ in r] for r in rows], K, t["tiles"])
            w = tiled_entries(c.env, np.array([w for r in rows for _, w in r], dtype=np.int32), t["tiles"])
            c.ctx.set_lincomb_split(split)
            try:
                c.ctx.ct_lincomb(t["in0"], t["out0"], t.get("in1"), t.get("out1"), row_ptr=row_ptr, idx=idx, w=w,
                                 status=t["status"])
            finally:
                c.ctx.set_lincomb_split(0)
        return dict(ins=ins, outs=outs, status=np.ones(K, dtype=np.uint8), call=call,
                    scratch=lambda B: (len(ins) * B * split * L * c.n * 4 if split > 1 else 0))
    return spec


def spec_drop_primes(c, L, alias, tier):
    x0, x1 = halves(c.slabs(L, "digit"), alias)
    cut = lambda x: np.ascontiguousarray(x[:, :L - 1])  # noqa: E731
    return dict(ins=dict(in0=x0, in1=x1), outs=dict(out0=cut(x0), out1=cut(x1)), call=lambda t: c.ctx.ct_drop_primes(
        t["in0"], t["out0"], t["in1"], t["out1"], primes_in=L, primes_out=L - 1))


# ---- one call on tiled slabs, every output compared ---------------------------------------------------------------------
class Pool:
    """Slabs as views of one int32 buffer, handed out front to back; without a buffer every slab is its own tensor."""

    def __init__(self, env, buf=None):
        self.env, self.buf, self.used, self.peak = env, buf, 0, 0

    def words(self, count):
        torch = self.env["torch"]
        if self.buf is None:
            return torch.empty(count, dtype=torch.int32, device=self.env["dev"])
        start = self.used
        self.used = -(-(start + count) // 64) * 64                      # 256-byte steps: aligned for every word size
        assert self.used <= self.buf.numel(), f"the pool holds {self.buf.numel()} words, the call needs more"
        self.peak = max(self.peak, self.used)
        return self.buf[start:start + count]


TORCH_OF = {"uint32": "int32", "int32": "int32", "int64": "int64", "float32": "float32", "float64": "float64"}


def typed(env, words, a, lead):
    """The first words of the int32 view `words` as a tensor of host array a's word type and the shape lead + a.shape[1:]."""
    dt = getattr(env["torch"], TORCH_OF[a.dtype.name])
    count = int(np.prod(lead + a.shape[1:])) * a.dtype.itemsize // 4
    return words[:count].view(dt).view(*lead, *a.shape[1:])


def slab_plan(spec):
    """Per slab of the call: (records per tile, elements per record, planes), for sizing a batch."""
    for name, a in list(spec["ins"].items()) + list(spec["outs"].items()):
        if isinstance(a, Stack):
            yield name, a.a.shape[1], int(np.prod(a.a.shape[2:])), a.a.shape[0]
        else:
            yield name, a.shape[0], int(np.prod(a.shape[1:])), 1


def run_spec(env, c, spec, tiles, pool, past=None, what=""):
    """Tile the inputs, fill the outputs with sentinels (two rows of guard words behind each), call once, compare every
    record of every output.  past: the word every slab must reach beyond by a whole tile (tier B), or None."""
    torch = env["torch"]
    tile, n = spec.get("tile", c.K), c.n
    B = tiles * tile
    t, slabs, checks = dict(B=B, tiles=tiles), {}, []
    for name, k, elems, planes in slab_plan(spec):
        if past is not None:
            limit = limit_of(spec, name, past)
            assert (tiles * k - k) * elems > limit, (what, name, tiles * k, elems, limit)
    for name, a in spec["ins"].items():
        if id(a) not in slabs:                                         # one host array, one device slab
            if isinstance(a, Stack):
                G, k = a.a.shape[:2]
                dst = typed(env, pool.words(G * tiles * k * int(np.prod(a.a.shape[2:]))), a.a[0], (G, tiles * k))
                for g in range(G):
                    tiled(env, a.a[g], tiles * k, out=dst[g])
            else:
                k = a.shape[0]
                dst = typed(env, pool.words(tiles * k * int(np.prod(a.shape[1:])) * a.dtype.itemsize // 4), a, (tiles * k,))
                tiled(env, a, tiles * k, out=dst)
            slabs[id(a)] = dst
        t[name] = slabs[id(a)]
    for name, a in spec["outs"].items():
        planes = a.a if isinstance(a, Stack) else a[None]
        G, k = planes.shape[:2]
        count = G * tiles * k * int(np.prod(planes.shape[2:])) * planes.dtype.itemsize // 4
        raw = pool.words(count + 2 * n)
        raw.fill_(SENTINEL)
        dst = typed(env, raw, planes[0], (G, tiles * k))
        t[name] = dst if isinstance(a, Stack) else dst[0]
        checks += [(f"{name}[{g}]" if G > 1 else name, dst[g], planes[g], raw[count:] if g == G - 1 else None)
                   for g in range(G)]
    if spec.get("status") is not None:
        t["status"] = torch.full((tiles * len(spec["status"]),), 77, dtype=torch.uint8, device=env["dev"])
        checks.append(("status", t["status"], spec["status"], None))
    if spec.get("work") is not None:
        t["work_bytes"] = int(spec["work"](B))
        assert t["work_bytes"] % 4 == 0
        raw = pool.words(t["work_bytes"] // 4 + 64)
        raw.fill_(SENTINEL)
        t["work"], work_guard = raw, raw[t["work_bytes"] // 4:]
    spec["call"](t)
    torch.cuda.synchronize()
    for name, got, exp, guard in checks:
        assert_tiles(env, got, exp, f"{what} {name}", guard=guard)
    if spec.get("work") is not None:
        assert bool((work_guard == SENTINEL).all()), f"{what}: words behind the workspace are written"
    return B


# ---- the table ----------------------------------------------------------------------------------------------------------
DIGIT_SHAPES = [((1024, 1), 1), ((2048, 1), 1), ((4096, 3), 3), ((4096, 3), 2), ((8192, 6), 6), ((16384, 13), 13)]
SP_SHAPES = [((4096, 3), 2), ((8192, 6), 5), ((16384, 13), 12)]
TRANSFORM_SHAPES = [((4096, 3), 3), ((8192, 6), 6), ((16384, 13), 13)]
ELEMENT_SHAPES = [((1024, 1), 1), ((2048, 1), 1), ((4096, 3), 3), ((16384, 13), 13)]

DIGIT = dict(ct_relin=spec_relin, ct_galois=spec_galois, ct_galois_many=spec_galois_many,
             ct_galois_sum=spec_galois_sum(False), ct_galois_sum_add_input=spec_galois_sum(True),
             ct_lintrans=spec_lintrans, ct_galois_accum=spec_galois_accum, ct_bsgs=spec_bsgs)
SPECIAL = dict(ct_relin_sp=spec_relin_sp, ct_galois_sp=spec_galois_sp, ct_galois_sum_sp=spec_galois_sum_sp,
               ct_lintrans_sp=spec_lintrans_sp, ct_galois_many_ext_sp=spec_galois_many_ext_sp,
               ct_galois_accum_sp=spec_galois_accum_sp, ct_mod_down_sp=spec_mod_down_sp,
               ct_mul_plain_sum_ext_sp=spec_mul_plain_sum_ext_sp, ct_switch_keyed_sp=spec_switch_keyed_sp,
               ct_switch_sum_keyed_sp=spec_switch_sum_keyed_sp, ct_pack_sp=spec_pack_sp, ct_dot_sp=spec_dot_sp,
               ct_bsgs_sp=spec_bsgs_sp)
TRANSFORM = dict(ct_rescale=spec_rescale, ct_affine_rescale=spec_affine_rescale, decrypt_level=spec_decrypt(0),
                 decrypt_level_below=spec_decrypt(1), decrypt3_level=spec_decrypt(0, cubic=True))
ELEMENT = dict(ct_mul_plain=spec_mul_plain, ct_mul=spec_mul, ct_mul_sum=spec_mul_sum,
               ct_mul_plain_sum=spec_mul_plain_sum, ct_lincomb_split1=spec_lincomb(1), ct_lincomb_split2=spec_lincomb(2),
               ct_drop_primes=spec_drop_primes)
RING_ENTRIES = ("ct_switch_keyed_sp", "ct_switch_sum_keyed_sp")         # their tile is lcm(K, 3) records
SPECS = {**DIGIT, **SPECIAL, **TRANSFORM, **ELEMENT, "ct_poly_sp": spec_poly_sp}


def entry_tile(name, n):
    K = tile_of(n)
    return K * 3 // math.gcd(K, 3) if name in RING_ENTRIES else K


def tier_a_cases():
    out = []
    for family, shapes in ((DIGIT, DIGIT_SHAPES), (SPECIAL, SP_SHAPES), (TRANSFORM, TRANSFORM_SHAPES),
                           (ELEMENT, ELEMENT_SHAPES)):
        for name in family:
            for shape, L in shapes:
                if name == "ct_drop_primes" and shape[1] == 1:
                    continue                                             # a record of one prime has no row to drop
                out.append((name, shape, L, chip_filling_batch(shape[0], L, entry_tile(name, shape[0]),
                                                               launched_by(family[name]))))
    out.append(("ct_poly_sp", (8192, 6), 5, chip_filling_batch(8192, 5, 2, launched_by(spec_poly_sp))))
    return out


TIER_A = tier_a_cases()


@pytest.mark.parametrize("name,shape,L,B", TIER_A, ids=[f"{e}-{s[0]}x{s[1]}-L{L}-B{B}" for e, s, L, B in TIER_A])
def test_chip_filling_batch(env, cases, name, shape, L, B):
    """Tier A: one call on the smallest batch with which the smallest launch the entry makes -- the grid its spec states,
    (B, L) where it states none -- is at least four rounds of the densest residency; every record, status byte and guard
    word against the host model of the K records."""
    n, tile, launched = shape[0], entry_tile(name, shape[0]), launched_by(SPECS[name])
    assert B % tile == 0 and launched(L, B, tile) >= workgroups_needed(n) > launched(L, B - tile, tile)
    c = cases(shape)
    spec = SPECS[name](c, L, False, "A")
    assert spec.get("tile", c.K) == tile
    assert run_spec(env, c, spec, B // tile, Pool(env), what=f"{name} {n}x{shape[1]} L={L} B={B}") == B


# ---- tier B ---------------------------------------------------------------------------------------------------------------
class BigPool:
    """The one buffer of tier B: allocated at the first call that needs it and kept for the calls after it.  A call whose
    entry allocates scratch of its own in the library takes a buffer of its own size in its place (hold), so that
    buffer and scratch together stay under the footprint; the next call allocates the pool again."""

    def __init__(self, env):
        self.env, self.buf = env, None

    def hold(self, nbytes, footprint):
        """A buffer of at least `nbytes`: the pool, or after a release one of exactly that size.  A card with less free
        memory than `footprint` plus 4 GiB skips."""
        torch = self.env["torch"]
        if self.buf is None or self.buf.numel() * 4 < nbytes:
            self.release()
            free = torch.cuda.mem_get_info()[0]
            if free < footprint + 4 * GIB:
                pytest.skip(f"tier B needs {footprint / GIB:.0f} GiB + 4 GiB free (the pool every tier B call shares, "
                            f"sized for the largest of them, not this call's own slabs), the card has "
                            f"{free / GIB:.1f} GiB free")
            self.buf = torch.empty(-(-nbytes // 256) * 64, dtype=torch.int32, device=self.env["dev"])
        return self.buf

    def release(self):
        self.buf = None
        self.env["torch"].cuda.empty_cache()


@pytest.fixture(scope="module")
def big(env):
    pool = BigPool(env)
    yield pool
    pool.release()


# ct_lincomb with S = 2 comes last: it gives the pool up for a buffer of its own size beside the library's partial rows
TIER_B = ([(name, 3) for name in DIGIT] + [(name, 2) for name in SPECIAL] + [(name, 3) for name in TRANSFORM]
          + [(name, 3) for name in ELEMENT if name != "ct_lincomb_split2"] + [("ct_lincomb_split2", 3)])


# the decrypts take pte and values of one call and values_f64 of a second one on the same batch
TIER_B_CALLS = {name: [spec_decrypt(drop, cubic, ("pte", "values")), spec_decrypt(drop, cubic, ("values_f64",))]
                for name, drop, cubic in (("decrypt_level", 0, False), ("decrypt_level_below", 1, False),
                                          ("decrypt3_level", 0, True))}


def limit_of(spec, name, past):
    limits = spec.get("past", {})
    return limits.get(name, past) if isinstance(limits, dict) else min(limits, past)


def tiles_past(spec, past):
    """The fewest tiles with which every slab of the call reaches more than a whole tile beyond its limit."""
    return max(limit_of(spec, name, past) // (k * elems) + 2 for name, k, elems, _ in slab_plan(spec))


def slab_bytes(spec, tiles, n):
    """What run_spec takes from the pool for this call: every distinct input, every output with its guard rows, the
    workspace; each rounded up to 256 bytes."""
    seen, total = set(), 0
    step = lambda nbytes: -(-nbytes // 256) * 256  # noqa: E731
    for name, a in spec["ins"].items():
        if id(a) not in seen:
            seen.add(id(a))
            h = a.a if isinstance(a, Stack) else a[None]
            total += step(h.shape[0] * tiles * h[0].size * h.dtype.itemsize)
    for a in spec["outs"].values():
        h = a.a if isinstance(a, Stack) else a[None]
        total += step(h.shape[0] * tiles * h[0].size * h.dtype.itemsize + 8 * n)
    if spec.get("work") is not None:
        total += step(int(spec["work"](tiles * spec.get("tile", 3))) + 256)
    return total


@pytest.mark.parametrize("name,L", TIER_B, ids=[f"{e}-4096x3-L{L}" for e, L in TIER_B])
def test_past_word_2_32(env, cases, big, name, L):
    """Tier B: one call whose every slab reaches past word 2^32 by at least a whole tile (the module's docstring lists
    the entries that cannot, and how far they reach instead); every record against the host model.  The footprint --
    the buffer the slabs are views of, the library's own scratch and 2 GiB for the comparator's temporaries, the keys
    and the index lists -- stays at or under 96 GiB."""
    torch = env["torch"]
    c = cases.only((4096, 3))                                            # the other shapes give their device memory back
    specs = [f(c, L, True, "B") for f in TIER_B_CALLS.get(name, [SPECS[name]])]
    tiles = max(tiles_past(spec, 2 ** 32) for spec in specs)
    tile = specs[0].get("tile", c.K)
    if not specs[0].get("past"):
        smallest = min(k * elems for _, k, elems, _ in slab_plan(specs[0]))
        assert (tiles - 1) * smallest > 2 ** 32                          # (B - K) x the smallest record, a tile at a time
    scratch = max(int(spec.get("scratch", lambda B: 0)(tiles * tile)) for spec in specs)
    need = max(slab_bytes(spec, tiles, c.n) for spec in specs)
    if scratch:
        big.release()                                                    # a buffer of this call's own size
    else:
        need = max(need, POOL_BYTES)                                     # the pool, kept for the calls after this one
    footprint = need + scratch + 2 * GIB
    assert footprint <= 96 * GIB, (name, need, scratch)
    pool = Pool(env, big.hold(need, footprint))
    torch.cuda.reset_peak_memory_stats()
    for spec in specs:
        pool.used = 0
        B = run_spec(env, c, spec, tiles, pool, past=2 ** 32, what=f"{name} B={tiles * tile}")
    assert torch.cuda.max_memory_allocated() + scratch <= footprint
    in_use = torch.cuda.mem_get_info()
    print(f"{name}: B = {B}, slabs {pool.peak * 4 / GIB:.1f} GiB, library scratch {scratch / GIB:.1f} GiB, "
          f"max_memory_allocated {torch.cuda.max_memory_allocated() / GIB:.1f} GiB, device memory in use after the call "
          f"{(in_use[1] - in_use[0]) / GIB:.1f} GiB")
    if scratch:
        big.release()
