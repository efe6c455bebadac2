"""The library's host half on the CPU: the seven .cpp files between the C ABI and the kernels, compiled with plain g++ and
linked against a model of the HIP runtime (tests/c/hip_model.cpp), recording launch wrappers (tests/c/launch_model.cpp)
and a stand-alone driver (tests/c/host_driver.cpp).  No GPU, no runtime library, no Python in the process under test.

The model keeps order and provenance: a vector clock per stream, every operation logged with its thread, current device,
stream and pointers.  The driver prints one line per fact or finding and this module judges them:
  streams    every *_device entry, called from a fresh thread (current device 0) on a non-blocking stream of the context's
             device 2: nothing on a null stream, nothing before the caller's earlier work, everything joined at return
  refusals   a refused call makes no runtime call at all
  lifetimes  create -> use -> destroy leaves nothing alive; every allocation of every create fails once
  workspace  the plan entries stay inside the caller's workspace
  group      four model devices: every member on its own device, peer copies into the root's slice
  batch      se_encrypt_batch over three devices, and with the injected shard failure of the test-hooks build
  selftest   the checker flags each wrong sequence issued straight at the model
Two builds: address + undefined-behaviour sanitizer (every scenario) and thread sanitizer (the threaded ones)."""
import concurrent.futures
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seal-embedded_amd", "csrc")
TESTS_C = os.path.join(ROOT, "tests", "c")
HEADER = os.path.join(ROOT, "include", "seal_embedded_amd.h")
HOST_SOURCES = ["se_api", "se_context", "se_multi", "se_hostpipe", "se_lower", "se_formats", "se_host_tables"]
MODEL_SOURCES = ["hip_model", "launch_model", "host_driver"]
BUILDS = {
    "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    "tsan": ["-fsanitize=thread"],
}
STATIC_RUNTIME = {"asan": ["-static-libasan", "-static-libubsan"], "tsan": ["-static-libtsan"]}
THREADED = ["group", "batch", "threads"]
REPORT = re.compile(r"ERROR: AddressSanitizer|ERROR: LeakSanitizer|runtime error:|WARNING: ThreadSanitizer")


def _build(tmp, kind):
    flags = ["-std=c++17", "-O1", "-g", *BUILDS[kind], "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
             "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + TESTS_C]
    jobs = [(os.path.join(CSRC, s + ".cpp"), os.path.join(tmp, f"{kind}_{s}.o"), []) for s in HOST_SOURCES]
    jobs.append((os.path.join(CSRC, "se_api.cpp"), os.path.join(tmp, f"{kind}_se_api_hooks.o"), ["-DSEAMD_TEST_HOOKS"]))
    jobs += [(os.path.join(TESTS_C, s + ".cpp"), os.path.join(tmp, f"{kind}_{s}.o"), ["-Wall", "-Wextra", "-Werror"])
             for s in MODEL_SOURCES]
    return flags, jobs


def _link(kind, objects, exe):
    # the sanitizer's runtime linked statically where the toolchain has it: the program then starts whatever the
    # environment preloads; else the default (shared) runtime
    for extra in (STATIC_RUNTIME[kind], []):
        r = subprocess.run(["g++", *BUILDS[kind], *extra, *objects, "-o", exe, "-lpthread"], capture_output=True, text=True)
        if r.returncode == 0:
            return
    raise AssertionError("link failed:\n" + r.stderr)


def _parse(out):
    scenarios, cur = {}, None
    for line in out.splitlines():
        if line.startswith("== "):
            cur = scenarios.setdefault(line[3:], [])
        elif cur is not None:
            cur.append(line)
    return scenarios


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{'asan': run, 'asan_hooks': run, 'tsan': run, 'tsan_hooks': run}, run = (returncode, scenarios, stderr)."""
    if not shutil.which("g++") or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs g++ and the HIP headers")
    tmp = str(tmp_path_factory.mktemp("host_model"))
    compiles = []
    for kind in BUILDS:
        flags, jobs = _build(tmp, kind)
        compiles += [["g++", *flags, *extra, "-c", src, "-o", obj] for src, obj, extra in jobs]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        for cmd, r in zip(compiles, pool.map(lambda c: subprocess.run(c, capture_output=True, text=True), compiles)):
            assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr
    result = {}
    for kind in BUILDS:
        obj = lambda s: os.path.join(tmp, f"{kind}_{s}.o")
        common = [obj(s) for s in HOST_SOURCES[1:] + MODEL_SOURCES]
        _link(kind, [obj("se_api")] + common, os.path.join(tmp, kind))
        _link(kind, [obj("se_api_hooks")] + common, os.path.join(tmp, kind + "_hooks"))
        data = os.path.join(tmp, kind + "_data")
        os.makedirs(data)
        env = dict(os.environ, SE_AMD_DATA_PATH=data)
        for drop in ("SE_AMD_DEVICES", "SE_AMD_DEVICE", "SE_AMD_NUM_CUS", "SE_AMD_STAGED", "SE_AMD_SPECULATION",
                     "SE_AMD_INJECT_SHARD_FAILURE", "HIP_MODEL_DEVICES"):
            env.pop(drop, None)
        for name, exe, args, more in ((kind, kind, [] if kind == "asan" else THREADED, {}),
                                      (kind + "_hooks", kind + "_hooks", ["batch"], {"SE_AMD_INJECT_SHARD_FAILURE": "1"})):
            r = subprocess.run([os.path.join(tmp, exe), *args], capture_output=True, text=True, env=dict(env, **more),
                               timeout=300)
            result[name] = (r.returncode, _parse(r.stdout), r.stderr)
    return result


def _lines(run, scenario, prefix):
    return [l for l in run[1][scenario] if l.startswith(prefix + " ")]


def _fields(line):
    return dict(f.split("=", 1) for f in line.split() if "=" in f)


def _no_findings(run, scenario):
    bad = [l for l in run[1][scenario] if l.startswith(("finding ", "setup-failure "))]
    assert not bad, "\n".join(bad)
    assert "setup_failures 0" in run[1][scenario]


# ---- sanitizers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["asan", "asan_hooks", "tsan", "tsan_hooks"])
def test_the_run_ends_clean_under_its_sanitizer(runs, name):
    code, scenarios, err = runs[name]
    assert not REPORT.search(err), err[-4000:]
    assert code == 0, err[-4000:]
    assert scenarios["end"] == ["done"]


# ---- guards ---------------------------------------------------------------------------------------------------------------
def _header_stream_entries():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"\bint\s+(se_amd_\w+)\s*\(([^;{]*)\)\s*;", text)
            if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))}


def test_the_streams_scenario_covers_every_entry_of_the_header_that_takes_a_stream(runs):
    ran = {l.split()[1] for l in _lines(runs["asan"], "streams", "entry")}
    declared = _header_stream_entries()
    assert len(declared) > 40
    assert ran == declared, f"not run: {sorted(declared - ran)}; not in the header: {sorted(ran - declared)}"
    refused = {l.split()[1] for l in _lines(runs["asan"], "refusals", "refusal")}
    assert refused == declared


def test_the_launch_model_defines_exactly_the_wrappers_kernel_args_h_declares():
    names = re.compile(r"^hipError_t\s+(launch_\w+)\s*\(", re.M)
    with open(os.path.join(CSRC, "kernels", "kernel_args.h")) as f:
        declared = names.findall(f.read())
    with open(os.path.join(TESTS_C, "launch_model.cpp")) as f:
        defined = names.findall(f.read())
    assert len(declared) == len(set(declared)) == 55
    assert sorted(defined) == sorted(declared)


def test_the_model_defines_the_28_runtime_functions_the_host_half_calls():
    with open(os.path.join(TESTS_C, "hip_model.cpp")) as f:
        defined = set(re.findall(r"^(?:hipError_t|const char \*)\s*(hip[A-Z]\w+)\s*\(", f.read(), flags=re.M))
    assert len(defined) == 28, sorted(defined)


# ---- streams ----------------------------------------------------------------------------------------------------------------
# Host-blocking calls of the FIRST call of an entry, in the scenario's order.  The whole-path entries grow context scratch
# on demand ("not stream-ordered: call once with the largest B before timing"), which drains the device; the symmetric
# entry comes first and grows what the asymmetric and keyed ones then find in place, the seed-compressed form grows its
# slab for `a`, the keyed form its index scratch.  Every other entry is documented without scratch or host
# synchronisation and makes none on either call.
FIRST_CALL_BLOCKING = {
    "se_amd_encrypt_sym_device": 3,          # the declined list, the sampler scratch, the speculation rows
    "se_amd_encrypt_sym_seeded_device": 1,   # the slab that takes c1 = a
    "se_amd_encrypt_sym_keyed_device": 1,    # the clamped key indices
}


def test_every_stream_entry_stays_on_the_callers_stream_and_is_joined_at_return(runs):
    _no_findings(runs["asan"], "streams")
    entries = _lines(runs["asan"], "streams", "entry")
    assert entries
    for line in entries:
        name, f = line.split()[1], _fields(line)
        assert f["rc"] == "0,0", line
        assert int(f["launches"]) + int(f["copies"]) + int(f["memsets"]) > 0, line   # a good call does something
        # the second call is the one that counts: no entry blocks the host once its scratch is in place
        assert f["blocking"] == "0", line
        assert int(f["blocking_first"]) == FIRST_CALL_BLOCKING.get(name, 0), line
    # the other launch shapes of the whole-path entries (the default at this batch size is the small-batch form)
    variants = _lines(runs["asan"], "streams", "variant")
    shapes = {"fused", "pipeline", "staged", "fused_serial", "pipeline_serial"}
    assert {l.split()[1] for l in variants} >= {f"{e}/{s}" for s in shapes for e in
                                                ("se_amd_encrypt_sym_device", "se_amd_encrypt_sym_keyed_device",
                                                 "se_amd_encrypt_asym_device", "se_amd_encrypt_sym_seeded_device")}
    for line in variants:
        f = _fields(line)
        assert f["rc"] == "0,0" and int(f["launches"]) > 0 and f["blocking"] == "0", line
    assert runs["asan"][1]["streams"][-1] == "live 0 0 0"


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_a_refused_call_returns_an_error_and_makes_no_runtime_call(runs):
    _no_findings(runs["asan"], "refusals")
    cases = {}
    for line in _lines(runs["asan"], "refusals", "refusal"):
        _, name, what, *_ = line.split()
        f = _fields(line)
        assert int(f["rc"]) < 0 and f["calls"] == "0", line
        cases.setdefault(name, set()).add(what)
    for name, seen in cases.items():
        assert {"null_ctx", "null"} <= seen, (name, seen)
        if "_ct_" in name:   # the ciphertext entries: alignment everywhere; a level argument or a plan (or both)
            assert "misaligned" in seen, (name, seen)
            if name != "se_amd_ct_lincomb_device":   # full-level slabs only: no level argument and no plan
                assert {"primes=0", "primes=np+1"} <= seen or "foreign_plan" in seen, (name, seen)
            assert len(seen) >= 3, (name, seen)
    plans = {n for n, seen in cases.items() if "foreign_plan" in seen}
    assert plans == {"se_amd_ct_lintrans_device", "se_amd_ct_lintrans_sp_device", "se_amd_ct_bsgs_device",
                     "se_amd_ct_bsgs_sp_device", "se_amd_ct_poly_sp_device"}


# ---- lifetimes --------------------------------------------------------------------------------------------------------------
CREATES = ["se_amd_create", "se_amd_create_4096x3", "se_amd_group_create", "se_amd_lintrans_create",
           "se_amd_lintrans_create_sp", "se_amd_bsgs_create", "se_amd_bsgs_create_sp", "se_amd_poly_create"]
INSTALLS = ["se_amd_set_secret_key", "se_amd_set_public_key", "se_amd_set_secret_keyring", "se_amd_set_public_keyring",
            "se_amd_set_relin_key", "se_amd_set_galois_keys", "se_amd_set_relin_key_sp", "se_amd_set_galois_keys_sp",
            "se_amd_set_switch_keyring_sp"]


def test_create_use_destroy_leaves_nothing_alive_and_every_failed_allocation_is_cleaned_up(runs):
    _no_findings(runs["asan"], "lifetimes")
    good = {l.split()[1]: _fields(l) for l in _lines(runs["asan"], "lifetimes", "lifetime")}
    assert sorted(good) == sorted(CREATES + INSTALLS)
    for name, f in good.items():
        assert set(f["rc"].split(",")) == {"0"} and f["restored"] == "1", (name, f)
        if name != "se_amd_poly_create":   # host-only: it allocates nothing on the device
            assert int(f["allocations"]) > 0, (name, f)
    failed = {}
    for line in _lines(runs["asan"], "lifetimes", "failed-create"):
        name, f = line.split()[1], _fields(line)
        assert int(f["rc"]) < 0 and f["null"] == "1" and f["restored"] == "1" and f["retry_rc"] == "0", line
        failed.setdefault(name, set()).add(int(f["k"]))
    for line in _lines(runs["asan"], "lifetimes", "failed-install"):
        name, f = line.split()[1], _fields(line)
        assert int(f["rc"]) < 0 and f["restored"] == "1" and f["retry_rc"] == "0", line
        failed.setdefault(name, set()).add(int(f["k"]))
    for name, f in good.items():   # every allocation of every create has failed once
        assert failed.get(name, set()) == set(range(int(f["allocations"]))), name
    tail = runs["asan"][1]["lifetimes"]
    assert "live 0 0 0" in tail and "violations 0" in tail


# ---- workspace --------------------------------------------------------------------------------------------------------------
def test_the_plan_entries_stay_inside_the_callers_workspace_and_refuse_a_short_one(runs):
    _no_findings(runs["asan"], "workspace")
    used = {l.split()[1]: _fields(l) for l in _lines(runs["asan"], "workspace", "workspace")}
    assert sorted(used) == ["se_amd_ct_bsgs_device", "se_amd_ct_bsgs_device/one_record", "se_amd_ct_bsgs_sp_device",
                            "se_amd_ct_bsgs_sp_device/one_record", "se_amd_ct_poly_sp_device"]
    for name, f in used.items():
        # the workspace is one allocation of exactly *_workspace_bytes: used, to its last byte, never beyond
        assert int(f["uses"]) > 0 and f["outside"] == "0" and f["reach"] == f["bytes"], (name, f)
    for line in _lines(runs["asan"], "workspace", "call"):
        assert _fields(line)["rc"] == "0", line
    short = {l.split()[1]: _fields(l) for l in _lines(runs["asan"], "workspace", "refusal")}
    assert sorted(short) == ["se_amd_ct_bsgs_device/short", "se_amd_ct_bsgs_sp_device/short", "se_amd_ct_poly_sp_device/short"]
    for name, f in short.items():
        assert int(f["rc"]) < 0 and f["calls"] == "0", (name, f)


# ---- group ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["asan", "tsan"])
def test_group_members_work_on_their_own_devices_and_gather_into_the_roots_slices(runs, build):
    _no_findings(runs[build], "group")
    lines = _lines(runs[build], "group", "group")
    assert len(lines) == 12   # three entries x B in {10, 3} x with and without a root
    for line in lines:
        f = _fields(line)
        assert f["rc"] == "0" and f["findings"] == "0", line
        assert f["peer_copies"] == f["expected_peer_copies"], line
        if "/B=3/" in line:   # fewer units than devices: the last member does nothing
            assert f["launches"].endswith(",0") and "0" not in f["launches"].split(",")[:3], line
    assert runs[build][1]["group"][-1] == "live 0 0 0"


# ---- batch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["asan", "tsan"])
def test_the_sharded_host_batch_delivers_every_record_with_and_without_a_lost_shard(runs, build):
    for name, launches in ((build, lambda l: l[0] > 0 and l[1] > 0 and l[2] > 0),
                           (build + "_hooks", lambda l: l[0] > 0 and l[1] == 0 and l[2] == 2 * l[0])):
        _no_findings(runs[name], "batch")
        (line,) = _lines(runs[name], "batch", "batch")
        f = _fields(line)
        assert f["rc"] == "0" and f["undelivered_words"] == "0" and f["findings"] == "0", line
        per_device = [int(x) for x in f["launches"].split(",")]
        assert launches(per_device) and per_device[3] == 0, line   # the lost shard re-runs on the next healthy device
        assert runs[name][1]["batch"][-1] == "live 0 0 0"


@pytest.mark.parametrize("build", ["asan", "tsan"])
def test_two_threads_calling_two_entries_on_one_context(runs, build):
    _no_findings(runs[build], "threads")
    assert "threads rc=0,0 findings=0" in runs[build][1]["threads"]


# ---- selftest ---------------------------------------------------------------------------------------------------------------
SELFTEST = {
    "good_fork_join": set(),
    "launch_on_null_stream": {"null_stream"},
    "aux_never_joined": {"not_joined"},
    "launch_before_fork": {"not_after_entry"},
    "pointer_of_other_device": {"violation"},
    "copy_past_allocation": {"violation"},
    "free_of_unknown_pointer": {"violation"},
    "launch_under_wrong_device": {"wrong_device_launch"},
    "host_blocking_call": {"host_blocking"},
}
SELFTEST_TEXT = {
    "pointer_of_other_device": "memory of device 1 used under device 2",
    "copy_past_allocation": "past its end",
    "free_of_unknown_pointer": "free of an unknown pointer",
}


def test_the_checker_flags_every_wrong_sequence_by_name(runs):
    lines = runs["asan"][1]["selftest"]
    seen = {name: set() for name in SELFTEST}
    for line in lines:
        if line.startswith("finding "):
            _, name, category, *_ = line.split()
            seen[name].add(category)
    for name, expected in SELFTEST.items():
        assert expected <= seen[name], (name, seen[name])
        if not expected:
            assert not seen[name], (name, seen[name])
        if name in SELFTEST_TEXT:
            assert any(SELFTEST_TEXT[name] in l for l in lines if l.startswith(f"finding {name} ")), name
    # the sequences that are wrong in one way only are flagged in that way only
    for name in ("aux_never_joined", "launch_before_fork", "host_blocking_call"):
        assert seen[name] == SELFTEST[name], (name, seen[name])
    # an allocation left alive shows in the live count, and is gone once it is freed
    assert [l for l in lines if l.startswith("live ")] == ["live 1 0 0", "live 0 0 0"]
