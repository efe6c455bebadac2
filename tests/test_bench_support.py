"""tools/bench_support.py, the harness of the *_bench.py tools: the order of operations of the event loop against a stub
torch and a stub sampler, the result record, the one JSON line, and the argument stage of every tool that uses it (it
answers --help without importing torch, and says "<tool> needs a GPU" where there is none).  No GPU."""
import argparse
import json
import os
import re
import subprocess
import sys

import pytest

from tools import bench_support as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ["ct_bsgs_bench", "ct_bsgs_sp_bench", "ct_dot_bench", "ct_galois_bench", "ct_galois_hoist_bench",
         "ct_keyswitch_sp_bench", "ct_keyswitch_sp_hoist_bench", "ct_lintrans_bench", "ct_mul_bench", "ct_pack_bench",
         "ct_poly_bench", "ct_switch_bench", "lincomb_bench", "rescale_bench"]


class StubEvent:
    def __init__(self, log, number):
        self.log, self.number = log, number

    def record(self):
        self.log.append(("record", self.number))

    def synchronize(self):
        self.log.append(("event_synchronize", self.number))

    def elapsed_time(self, end):
        return float(10 * self.number + end.number)            # names the pair of events it came from


class StubCuda:
    def __init__(self, log):
        self.log, self.events = log, 0

    def synchronize(self):
        self.log.append("device_synchronize")

    def Event(self, enable_timing=False):
        assert enable_timing
        self.events += 1
        return StubEvent(self.log, self.events)


class StubTorch:
    def __init__(self, log):
        self.cuda = StubCuda(log)


def stub_sampler(log):
    class Sampler:
        def __init__(self, torch, dev_index):
            log.append(("sampler", dev_index))

        def __enter__(self):
            log.append("enter")
            return self

        def __exit__(self, *a):
            log.append("exit")

        def summary(self):
            return {"mean_mhz": 2400.0}
    return Sampler


def run_timed(clock):
    log = []
    fns = [lambda: log.append("a"), lambda: log.append("b")]
    ms, summary = bs.timed(fns, 3, 2, clock=clock, torch=StubTorch(log), sampler=stub_sampler(log))
    return log, ms, summary


def test_timed_order_of_operations():
    log, ms, summary = run_timed(True)
    want = ["a", "b", "a", "b", "device_synchronize", ("sampler", 0), "enter"]
    for call in range(6):                                      # events 2 call + 1 and 2 call + 2 belong to call `call`
        e0, e1 = 2 * call + 1, 2 * call + 2
        want += [("record", e0), "ab"[call % 2], ("record", e1), ("event_synchronize", e1)]
    want.append("exit")
    assert log == want
    # nothing waits between the sampler's entry and the first record
    assert log[log.index("enter") + 1] == ("record", 1)
    assert log.count("device_synchronize") == 1
    # three entries per function, in call order: a had the event pairs (1, 2), (5, 6), (9, 10), b the ones between
    assert ms == [[12.0, 56.0, 100.0], [34.0, 78.0, 122.0]]
    assert summary == {"mean_mhz": 2400.0}


def test_timed_without_the_clock():
    log, ms, summary = run_timed(False)
    assert summary is None
    assert not [e for e in log if e in ("enter", "exit") or (isinstance(e, tuple) and e[0] == "sampler")]
    assert log[:5] == ["a", "b", "a", "b", "device_synchronize"] and log[5] == ("record", 1)
    assert [len(v) for v in ms] == [3, 3]


def test_record_median_rounding_and_key_order():
    odd = bs.record([3.0, 1.0, 2.0])
    assert odd == dict(ms=2.0, ms_min=1.0, ms_max=3.0, reps=3) and list(odd) == ["ms", "ms_min", "ms_max", "reps"]
    even = bs.record([4.0, 1.0, 2.0, 3.5])                     # the mean of the middle two
    assert even == dict(ms=2.75, ms_min=1.0, ms_max=4.0, reps=4)
    r = bs.record([0.123449, 0.123451, 0.99999], bytes=7, records_per_s=5)
    assert r == dict(ms=0.1235, ms_min=0.1234, ms_max=1.0, reps=3, bytes=7, records_per_s=5)
    assert list(r) == ["ms", "ms_min", "ms_max", "reps", "bytes", "records_per_s"]
    assert list(bs.record([1.0], tb_per_s=1, bytes=2)) == ["ms", "ms_min", "ms_max", "reps", "tb_per_s", "bytes"]


def test_rates_on_hand_computed_values():
    # 4096 records in a median of 0.5 ms: 8 192 000 a second; the unrounded median is the one used
    assert bs.per_s(4096, [0.75, 0.5, 0.25]) == 8192000
    assert bs.per_s(1000, [0.3, 0.4]) == round(1000 / 0.35 * 1e3) == 2857143
    # 3e9 bytes in a median of 1.5 ms: 2 TB/s; 1e9 bytes in 3 ms: 0.333
    assert bs.tb_per_s(3 * 10 ** 9, [1.0, 2.0]) == 2.0
    assert bs.tb_per_s(10 ** 9, [3.0]) == 0.333


def test_emit_prints_and_writes_one_line(tmp_path, capsys):
    result = dict(tool="t", nested=dict(b=1, a=[1, 2]), flag=True)
    out = tmp_path / "not" / "there" / "yet.json"
    bs.emit(result, str(out))
    line = json.dumps(result)
    assert capsys.readouterr().out == line + "\n"
    assert out.read_text() == line + "\n" and "\n" not in line
    bs.emit(result, "")
    assert capsys.readouterr().out == line + "\n"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["not"] and os.listdir(out.parent) == ["yet.json"]


def test_common_args_take_the_tools_defaults():
    ap = argparse.ArgumentParser()
    bs.add_common_args(ap, reps=40, warmup=3)
    assert vars(ap.parse_args([])) == dict(reps=40, warmup=3, out="")
    assert vars(ap.parse_args(["--reps", "7", "--warmup", "0", "--out", "x.json"])) == dict(reps=7, warmup=0, out="x.json")


def run_tool(tool, *args, flags=()):
    return subprocess.run([sys.executable, *flags, os.path.join(ROOT, "tools", tool + ".py"), *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("tool", TOOLS)
def test_help_answers_without_torch(tool):
    p = run_tool(tool, "--help", flags=("-X", "importtime"))
    assert p.returncode == 0, p.stderr[-2000:]
    assert "usage:" in p.stdout and "--reps" in p.stdout and "--warmup" in p.stdout and "--out" in p.stdout
    imported = re.findall(r"^import time:\s+\d+ \|\s+\d+ \|\s+(\S+)$", p.stderr, re.M)
    assert "bench_support" in imported and "argparse" in imported
    assert not [m for m in imported if m.split(".")[0] in ("torch", "numpy", "bench", "__graft_entry__")]


@pytest.mark.parametrize("tool", TOOLS)
def test_tool_without_a_gpu_says_so(tool):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    p = run_tool(tool)
    assert p.returncode != 0
    assert f"{tool} needs a GPU" in p.stderr and p.stdout == ""
