#!/usr/bin/env python3
"""Full-modulus decrypt against the per-prime entry, resident ciphertexts, HIP events, alternating in one process:
  A  one se_amd_decrypt_full_device call (values requested)
  B  np back-to-back se_amd_decrypt_decode_device calls (values requested): what looking at every prime costs
     without recombination
Prints per-alternation medians, the overall medians, the run-to-run spread of B (max - min of its alternation medians)
and the engine clock sampled while the loop runs.
  python tools/decrypt_full_timing.py [--n 4096 --primes 3 --batch 65536 --alternations 8 --reps 10]"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--primes", type=int, default=3)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--alternations", type=int, default=8)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--no-clock", action="store_true", help="do not sample rocm-smi (runs under a profiler)")
args = ap.parse_args()

import numpy as np
import torch

import __graft_entry__ as ge
import vectors as V

if not torch.cuda.is_available():
    sys.exit("decrypt_full_timing needs a GPU")
pkg = ge.load_package()
dev = torch.device("cuda:0")
n, npr, B = args.n, args.primes, args.batch
ctx = pkg.Context(n, npr)
ctx.set_secret_key(V.secret_key(n))
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
ss, sd = V.bench_seeds(B)
c0 = torch.zeros((B, npr, n), dtype=torch.int32, device=dev)
c1 = torch.zeros_like(c0)
ctx.encrypt_sym(t(V.bench_values(B, n)), t(ss), t(sd), c0, c1)
values = torch.zeros((B, n // 2), dtype=torch.float32, device=dev)
status = torch.zeros(B, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()


def run_a():
    ctx.decrypt_full(c0, c1, values=values, status=status)


def run_b():
    for j in range(npr):
        ctx.decrypt_decode(c0, c1, j, None, None, values)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


clocks, stop = [], threading.Event()


def sample_clock():
    while not stop.is_set():
        try:
            txt = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
            m = re.findall(r"sclk clock level:.*?\((\d+)Mhz\)", txt)
            if m:
                clocks.append(max(int(x) for x in m))   # the busy device of the visible ones
        except Exception:
            pass
        time.sleep(0.3)


for fn in (run_a, run_b):            # warm-up: code objects, clocks
    timed(fn, 5)
th = threading.Thread(target=sample_clock, daemon=True)
if args.no_clock:
    stop.set()
th.start()
a_all, b_all, a_med, b_med = [], [], [], []
for k in range(args.alternations):
    a = timed(run_a, args.reps)
    b = timed(run_b, args.reps)
    a_all += a
    b_all += b
    a_med.append(statistics.median(a))
    b_med.append(statistics.median(b))
    print(f"alternation {k}: A {a_med[-1]:.3f} ms   B {b_med[-1]:.3f} ms")
stop.set()
th.join(timeout=30)
assert bool((status == 1).all())
A, Bm = statistics.median(a_all), statistics.median(b_all)
spread = max(b_med) - min(b_med)
gb = 2 * B * npr * n * 4 / 1e9
print(f"n={n} primes={npr} B={B}: {len(a_all)} timed repetitions each")
print(f"A decrypt_full            median {A:.3f} ms  (min {min(a_all):.3f}, max {max(a_all):.3f})  "
      f"{B / A / 1e3:.2f} M ct/s, ciphertext read {gb / A * 1e3:.0f} GB/s")
print(f"B {npr} x decrypt_decode     median {Bm:.3f} ms  (min {min(b_all):.3f}, max {max(b_all):.3f})")
print(f"spread of B (max - min of alternation medians) {spread:.3f} ms;  A - B = {A - Bm:+.3f} ms;  A / B = {A / Bm:.3f}")
print("sclk while looping: " + (f"median {statistics.median(clocks)} MHz, min {min(clocks)}, max {max(clocks)} "
                                 f"({len(clocks)} samples)" if clocks else "not measured"))
ctx.close()
