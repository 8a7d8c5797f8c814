"""tools/probekit.py (what the probes share) and tools/ab.py (the A/B runner), without a GPU.

  child runner   jobs ok, ok, exit 3, ok: two lines come back, the fourth child never starts, the result is not 0, --out holds what it held
                 plus exactly those two lines; the same with a child that sleeps past a 1 s limit (status 124)
  forwarding     a child sees every option of a parser - one added after the fact among them - but --child, --out and --shapes
  host_stats     against numpy, with the key names the published lines use
  kernel_stats   two instantiations of one kernel in each of the three name forms merge into the call-weighted mean and the overall minimum;
                 kernels that are not asked for, one that only begins like one that is among them, are ignored
  ab.py          a command that fails on its second call: the target's bytes are put back, the third step never runs, the status is not 0;
                 with every step succeeding the variants alternate: round 1: a, b; round 2: a, b
  --help         of every probe with a command line and of ab.py: status 0 without torch or the library being loaded
"""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from tools import probekit as pk      # noqa: E402

CHILD = '''import json, sys, time
job = sys.argv[sys.argv.index("--child") + 1]
open(sys.argv[0] + "." + job + ".started", "w").close()
kind, _, n = job.partition("-")
if kind == "sleep":
    time.sleep(30)
print("noise before the line")
print(json.dumps(dict(job=job, argv=sys.argv[1:])), flush=True)
sys.exit(int(n) if kind == "exit" else 0)
'''


@pytest.fixture
def child(tmp_path):
    path = tmp_path / "child.py"
    path.write_text(CHILD)
    return str(path)


@pytest.mark.parametrize("bad, status", [("exit-3", 3), ("sleep-c", 124)])
def test_runner_stops_at_the_first_failure(child, tmp_path, capfd, bad, status):
    out = tmp_path / "sub" / "lines.jsonl"
    os.makedirs(out.parent)
    out.write_text("what was there\n")
    rc = pk.run_jobs(child, ["ok-a", "ok-b", bad, "ok-d"], ["--ticks", "2"], 1, str(out))
    assert rc != 0
    printed, err = capfd.readouterr()
    lines = printed.splitlines()
    assert [json.loads(t)["job"] for t in lines] == ["ok-a", "ok-b"]
    assert "%s ended with status %d" % (bad, status) in err
    assert os.path.exists(child + "." + bad + ".started") and not os.path.exists(child + ".ok-d.started")
    assert out.read_text() == "what was there\n" + "".join(t + "\n" for t in lines)


def test_runner_all_jobs(child, tmp_path, capfd):
    out = tmp_path / "new" / "lines.jsonl"      # the directory is made
    assert pk.run_jobs(child, ["ok-a", "ok-b"], [], 20, str(out)) == 0
    assert [json.loads(t)["job"] for t in out.read_text().splitlines()] == ["ok-a", "ok-b"]
    assert pk.run_jobs(child, ["ok-a"], [], 20, None) == 0


def test_options_are_forwarded(child, capfd):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="h1:1,h1:256")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--period", type=float, default=0.002)
    ap.add_argument("--parent-lib")
    ap.add_argument("--kt")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    pk.driver_options(ap, limit=7)
    ap.add_argument("--added-later", type=float, default=1e-9)      # an option a later change adds: nothing else names it
    a = ap.parse_args(["--parent-lib", "some/lib.so", "--profile", "--commit", "abc", "--out", "x.jsonl", "--period", "0.1"])
    args = pk.forwarded(a)
    assert pk.run_jobs(child, ["ok-a"], args, a.limit, None) == 0
    argv = json.loads(capfd.readouterr()[0].splitlines()[-1])["argv"]
    assert argv[:2] == ["--child", "ok-a"]
    seen = ap.parse_args(argv)
    want = dict(vars(a), child="ok-a", out=None, shapes="h1:1,h1:256")
    assert vars(seen) == want and seen.added_later == 1e-9 and seen.period == 0.1 and seen.profile and not seen.no_sweep and seen.kt is None
    for left_out in ("--out", "--shapes"):
        assert left_out not in argv
    assert argv.count("--child") == 1


def test_child_line_stamps_the_commit(capfd):
    a = argparse.Namespace(child="x", commit="abc")
    assert pk.child_line(a, dict(batch=1)) == 0
    assert json.loads(capfd.readouterr()[0]) == dict(batch=1, commit="abc")
    pk.child_line(argparse.Namespace(child="x", commit=None), dict(batch=1))
    assert json.loads(capfd.readouterr()[0]) == dict(batch=1)


def test_host_stats():
    v = np.random.default_rng(3).gamma(2.0, 1.5, size=37)
    s = pk.host_stats("step_inputs", list(v), "us")
    p05, p95 = np.percentile(v, [5, 95])
    assert s == {"step_inputs_us_median": np.median(v), "step_inputs_us_min": np.min(v), "step_inputs_us_p05": p05, "step_inputs_us_p95": p95}
    assert all(type(x) is float for x in s.values())
    assert sorted(pk.host_stats("tick_host", v, "ms")) == ["tick_host_ms_median", "tick_host_ms_min", "tick_host_ms_p05", "tick_host_ms_p95"]


def test_kernel_stats_merges_instantiations(tmp_path):
    rows = {"k_wbc<10>(bpmpc::DeviceModel const*, bpmpc::WbcArgs)": [4000, 6000, 5000],                     # plain
            "k_wbc<12>(bpmpc::DeviceModel const*, bpmpc::WbcArgs)": [1000],
            "void bpmpc::k_telemetry<10>(bpmpc::DeviceModel const*, bpmpc::TelemetryArgs)": [2000, 2000],        # void bpmpc::k<
            "void bpmpc::k_telemetry<12>(bpmpc::DeviceModel const*, bpmpc::TelemetryArgs)": [8000, 500, 9500, 6000],
            "void other::detail::k_tick_commands<10>(bpmpc::TickCommandArgs)": [3000],                  # ::k<
            "void other::detail::k_tick_commands<12>(bpmpc::TickCommandArgs)": [7000, 9000],
            "bpmpc::k_telemetry_reset(double*)": [100000],                                                      # begins like one that is asked for
            "void bpmpc::k_linearize_fast<10, false, true, false>(bpmpc::Launch)": [50000]}                     # not asked for
    path = str(tmp_path / "run_results.db")
    db = sqlite3.connect(path)
    db.execute("create table kernels (name text, duration integer)")
    db.executemany("insert into kernels values (?, ?)", [(n, d) for n, ds in rows.items() for d in ds])
    db.commit()
    db.close()
    split, launched = pk.kernel_stats(path, ("k_wbc", "k_telemetry", "k_tick_commands", "k_estimate"))
    assert sorted(split) == ["k_telemetry", "k_tick_commands", "k_wbc"]
    for k, ns in (("k_wbc", [4000, 6000, 5000, 1000]), ("k_telemetry", [2000, 2000, 8000, 500, 9500, 6000]), ("k_tick_commands", [3000, 7000, 9000])):
        assert sorted(split[k]) == ["avg_us", "calls", "min_us"]
        assert split[k]["calls"] == len(ns) and split[k]["min_us"] == min(ns) / 1e3
        assert split[k]["avg_us"] == pytest.approx(np.mean(ns) / 1e3, rel=1e-12)
    assert "bpmpc::k_telemetry_reset" in launched and "void bpmpc::k_telemetry<10>" in launched and len(launched) == len(rows)


FAKE = '''import os, sys
log, target, fail_at = sys.argv[1], sys.argv[2], int(sys.argv[3])
n = len(open(log).read().splitlines()) if os.path.exists(log) else 0
with open(log, "a") as f:
    f.write(open(target).read() + " " + os.environ.get("AB_TEST_KNOB", "-") + " " + " ".join(sys.argv[4:]) + "\\n")
print("line %d" % n)
sys.exit(5 if n + 1 == fail_at else 0)
'''


def _ab(tmp_path, fail_at, extra=()):
    fake, log, target = tmp_path / "fake.py", tmp_path / "log.txt", tmp_path / "lib.bin"
    fake.write_text(FAKE)
    target.write_bytes(b"original")
    for name in "ab":
        (tmp_path / name).write_bytes(name.encode())
    cmd = [sys.executable, os.path.join(ROOT, "tools", "ab.py"), "--lib", "a=%s" % (tmp_path / "a"), "--lib", "b=%s" % (tmp_path / "b"), "--target", str(target),
           "--limit", "20", *extra, "--", sys.executable, str(fake), str(log), str(target), str(fail_at)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    return r, log.read_text().splitlines(), target


def test_ab_restores_the_target_and_stops(tmp_path):
    r, ran, target = _ab(tmp_path, 2)
    assert r.returncode == 5
    assert ran == ["a - ", "b - "]      # the third step never ran
    assert target.read_bytes() == b"original" and not glob.glob(str(tmp_path / "*.ab_keep"))
    assert r.stdout.splitlines() == ["a [] line 0", "b [] ended with status 5"]


def test_ab_alternates_the_variants(tmp_path):
    r, ran, target = _ab(tmp_path, 0, ["--env", "AB_TEST_KNOB=7", "--args", "--batch 256|--batch 4096 --x"])
    assert r.returncode == 0
    order = [v for v in ("a -", "b -", "original 7") for _ in (0, 1)] * 2      # round 1: a, b, the environment; round 2 likewise; two argument sets each
    assert [t.rsplit(" --batch", 1)[0] for t in ran] == order
    assert [t.split(" ", 2)[2] for t in ran] == ["--batch 256", "--batch 4096 --x"] * 6
    assert target.read_bytes() == b"original"
    assert r.stdout.splitlines()[0] == "a [--batch 256] line 0" and r.stdout.splitlines()[5] == "[AB_TEST_KNOB=7] [--batch 4096 --x] line 5"


def test_ab_reports_a_bench_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import ab
    finally:
        sys.path.pop(0)
    line = json.dumps(dict(value=1.5, ms_per_step=2.5, fused=dict(value=3.5), kernel_ms_per_step=dict(lin=0.5)))
    assert ab.report(line) == "1.5 2.5 3.5 {'lin': 0.5}"
    assert ab.report(json.dumps(dict(value=1.5, ms_per_step=2.5, fused=None, kernel_ms_per_step=1.0))) == "1.5 2.5 None 1.0"
    assert ab.report("3 passed in 2.1s") == "3 passed in 2.1s"


PROBES = ["controller_tick_probe", "estimator_probe", "plan_geometry_probe", "plant_body_probe", "plant_input_probe", "plant_joint_probe", "plant_probe",
          "plant_sensor_probe", "plant_stand_probe", "policy_buffer_probe", "supervisor_probe", "supervisor_settle_probe", "telemetry_probe",
          "wbc_params_probe"]      # every probe with a command line; the others are plain scripts


@pytest.mark.parametrize("tool", PROBES + ["ab"])
def test_help(tool):
    script = "import runpy, sys; sys.argv = [%r, '--help']\ntry:\n    runpy.run_path(sys.argv[0], run_name='__main__')\nexcept SystemExit as e:\n" \
             "    assert not e.code, e.code\nassert 'torch' not in sys.modules and 'bipedal_control_amd' not in sys.modules\n"
    r = subprocess.run([sys.executable, "-c", script % os.path.join(ROOT, "tools", tool + ".py")], stdout=subprocess.PIPE, text=True, cwd=ROOT)
    assert r.returncode == 0 and "usage" in r.stdout
