#!/usr/bin/env python3
"""Alternating A/B of the two pair forms of the fused n = 4096 kernels in ONE process: the one-plane form
(k_encode_encrypt, debug flag 8192) against the two-way form (k_encode_encrypt_pair2, the default) on a BASELINE
workload at its bench batch:  python tools/pair2_ab.py [c2|c5] [--steps 40] [--rounds 3] [--out FILE]
A round times `steps` steps of one form, then of the other (the order alternates from round to round); the engine clock
is sampled (bench.ClockSampler) over each side.  The verdict is the rule of profiles/keyswitch_refactor_ab.json: the
two-way form's median step is below the one-plane form's in every round, and the mean difference exceeds the spread
(max - min) of the one-plane form's own round medians.  Prints one JSON line per round and one for the verdict."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import vectors as V
import bench
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="c2", choices=("c2", "c5"))
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("pair2_ab needs a GPU")
pkg = ge.load_package()
ONE_PLANE = 8192
n, npr, mode, B = bench.WORKLOADS[args.workload]
B = args.batch or B
dev = torch.device("cuda:0")
ctx = pkg.Context(n, npr)
ctx.reserve(B)
if mode == "sym":
    ctx.set_secret_key(V.secret_key(n))
vals = bench.bench_values_device(B, n, dev)
c0 = torch.empty((B, npr, n), dtype=torch.int32, device=dev)
if mode == "sym":
    ss_np, sd_np = V.bench_seeds(B)
    ss, sd = torch.from_numpy(ss_np).to(dev), torch.from_numpy(sd_np).to(dev)
    c1 = torch.empty_like(c0)
    step = lambda: ctx.encrypt_sym(vals, ss, sd, c0, c1)  # noqa: E731
else:
    step = lambda: ctx.encode_ntt(vals, c0)  # noqa: E731


def side(flags):
    ctx.set_debug_flags(flags)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    with bench.ClockSampler(torch, 0) as cs:
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    clk = cs.summary()
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                steps=len(ms), mean_mhz=round(clk["mean_mhz"], 1) if clk else None)


lines = []
for r in range(args.rounds):
    order = (ONE_PLANE, 0) if r % 2 == 0 else (0, ONE_PLANE)
    res = {f: side(f) for f in order}
    lines.append(dict(tool="pair2_ab", workload=args.workload, batch=B, round=r, first="one_plane" if r % 2 == 0 else "two_way",
                      one_plane=res[ONE_PLANE], two_way=res[0]))
    print(json.dumps(lines[-1]), flush=True)
ctx.set_debug_flags(0)
old = [ln["one_plane"]["median_ms"] for ln in lines]
new = [ln["two_way"]["median_ms"] for ln in lines]
diff = statistics.mean(o - v for o, v in zip(old, new))
spread = max(old) - min(old)
verdict = dict(tool="pair2_ab", workload=args.workload, batch=B, device=torch.cuda.get_device_name(0),
               one_plane_round_medians_ms=old, two_way_round_medians_ms=new, mean_difference_ms=round(diff, 4),
               one_plane_spread_ms=round(spread, 4), two_way_below_in_every_round=all(v < o for o, v in zip(old, new)),
               accepted=bool(all(v < o for o, v in zip(old, new)) and diff > spread))
print(json.dumps(verdict), flush=True)
if args.out:
    with open(args.out, "w") as f:
        for ln in lines + [verdict]:
            f.write(json.dumps(ln) + "\n")
