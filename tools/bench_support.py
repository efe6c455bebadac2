"""What the *_bench.py tools share: the common options, the start-up, the HIP-event loop, the result record and the one
JSON line.  A tool is then its shapes, its contenders and its result.  Nothing here imports torch when the module is
imported: a tool parses its arguments first, so `--help` answers on a machine without a GPU."""
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def add_common_args(ap, reps, warmup):
    """--reps, --warmup and --out with the tool's own defaults."""
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--out", default="")


def start(tool):
    """After the arguments are parsed: the repository root on sys.path, torch, the package.  -> (package, torch,
    device); exits with "<tool> needs a GPU" where there is none."""
    sys.path[:0] = [ROOT]
    import torch
    if not torch.cuda.is_available():
        sys.exit(f"{tool} needs a GPU")
    import __graft_entry__ as ge
    return ge.load_package(), torch, torch.device("cuda:0")


def timed(fns, reps, warmup, clock=True, torch=None, sampler=None):
    """Every function `warmup` times, one device synchronize, then `reps` rounds in which the functions alternate, each
    call between two events of its own and waited for.  The engine clock is sampled (bench.ClockSampler) around the
    timed rounds only.  -> (per function the list of milliseconds in call order, the clock summary or None)."""
    if torch is None:
        import torch
    if clock and sampler is None:
        from bench import ClockSampler as sampler
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    with (sampler(torch, 0) if clock else contextlib.nullcontext()) as cs:
        for _ in range(reps):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
    return ms, (cs.summary() if clock else None)


def record(ms, **extra):
    """Median / min / max of a list of milliseconds and its length, then the caller's entries in the order given."""
    return dict(ms=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), reps=len(ms),
                **extra)


def per_s(count, ms):
    """`count` items per call -> items per second at the median."""
    return round(count / statistics.median(ms) * 1e3)


def tb_per_s(nbytes, ms):
    """`nbytes` per call -> TB/s at the median."""
    return round(nbytes / statistics.median(ms) / 1e9, 3)


def emit(result, out):
    """The result as one JSON line: printed, and written to `out` (its directory created) where that is set."""
    line = json.dumps(result)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def slab(q, shape, dev, gen):
    """Random residues below every prime of q: an int32 tensor of `shape` drawn from `gen`."""
    import torch
    return torch.randint(0, min(q), shape, dtype=torch.int32, device=dev, generator=gen)


def key_words(rng, q, rows, n, npr):
    """Random key words [rows][npr][n], the words of prime i below q[i], drawn from `rng`."""
    import numpy as np
    return np.stack([rng.integers(0, q[i], (rows, n), dtype=np.uint32) for i in range(npr)], axis=1)
