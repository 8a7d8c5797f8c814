#!/usr/bin/env python3
"""What the tracking telemetry costs a controller tick, in one process per measurement on one box.

Per shape, `--repeats` rounds that alternate child processes:
  parent      the library of --parent-lib (built from the parent commit): the tick as it was                       (only with --parent-lib)
  detached    this library, a controller that never heard of the telemetry: the same three launches
  ring0       this library, a telemetry handle with ring_len 0 attached: k_telemetry behind every tick, statistics only
  ring256     this library, ring_len 256 attached: the sample also goes into the ring
Each child solves one batch (setup_commands + run), then times bpmpc_controller_tick on device tensors with a host clock around the call and the
synchronise of the solver's stream that drains it: the median, the minimum and the 5th / 95th percentile of `--ticks` calls.  A number here is a
call time as a caller sees it, not a kernel time; with --profile one more child per shape runs the ring256 variant under
`rocprofv3 --kernel-trace --stats` (a run of its own, no counters) and the per-kernel averages are read from its database.
One JSON line per measurement on stdout; --out appends them to a file (profiles/telemetry_probe.jsonl is where the published one belongs).
Every measurement runs in a child process of its own under a time limit; the first that fails or runs out of time ends the probe.
usage (GPU box, repository root): python tools/telemetry_probe.py [--shapes h1:1,h1:256,h1:4096] [--parent-lib FILE] [--profile] [--commit ID] [--out FILE]
"""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = "h1:1,h1:256,h1:4096"
RINGS = {"ring0": 0, "ring256": 256}
KERNELS = ("k_tick_observe_policy", "k_wbc", "k_tick_commands", "k_telemetry")


def measure(robot, B, variant, parent_lib, ticks, warmup):
    import ctypes as C
    import numpy as np
    import torch
    import bipedal_control_amd as bp
    from bipedal_control_amd import abi, api
    from tools.controller_tick_probe import _setup
    if variant == "parent":
        api._LIB = abi.bind(C.CDLL(os.path.abspath(parent_lib)), strict=False)      # an earlier commit's library: what it lacks is skipped
    stream = torch.cuda.Stream()
    mpc, ctrl, rbd = _setup(robot, B, stream.cuda_stream)
    tel = None
    if variant in RINGS:
        tel = bp.BatchedTelemetry(mpc.interface, B, ring_len=RINGS[variant])
        ctrl.attachTelemetry(tel)
    t_dev = torch.full((B,), 0.0025, dtype=torch.float64, device="cuda")
    r_dev = torch.tensor(rbd, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    times = []
    for k in range(warmup + ticks):
        t0 = time.perf_counter()
        ctrl.tick(t_dev, r_dev, fetch=False)
        mpc.synchronize()
        dt = time.perf_counter() - t0
        if k >= warmup:
            times.append(1e3 * dt)
    p05, p95 = (float(x) for x in np.percentile(times, [5, 95]))
    line = dict(probe="timing", robot=robot, batch=B, variant=variant, ticks=ticks, tick_host_ms_median=float(np.median(times)),
                tick_host_ms_min=float(np.min(times)), tick_host_ms_p05=p05, tick_host_ms_p95=p95,
                wbc_unsolved=int(ctrl.device_outputs()["wbc_status"].torch().sum().item()))
    if tel is not None:
        s = tel.stats(B)
        line.update(ring_len=RINGS[variant], samples=int(s["samples"].min()), frozen=int(s["frozen"].sum()), stats_finite=bool(np.isfinite(s["rows"]).all()))
        ctrl.attachTelemetry(None)
    return line


def kernel_split(robot, B, ticks, limit):
    """Per-kernel averages of the ring256 variant from a separate rocprofv3 --kernel-trace --stats run of this tool (a child process)."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
               "--child", "ring256:%s:%d" % (robot, B), "--ticks", str(ticks), "--warmup", "2"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            return r.returncode or 1, {"error": "rocprofv3 exit %d" % r.returncode, "stderr_tail": r.stderr[-400:]}
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, count(*), avg(duration), min(duration) from kernels group by name").fetchall()
    split = {}
    for name, calls, avg, mn in rows:
        for k in KERNELS:
            if name.startswith(k + "<") or name.startswith("void bpmpc::" + k + "<") or ("::" + k + "<") in name:
                split.setdefault(k, dict(calls=0, avg_us=0.0, min_us=float("inf")))
                e = split[k]
                e["avg_us"] = (e["avg_us"] * e["calls"] + avg / 1e3 * calls) / (e["calls"] + calls)
                e["calls"] += int(calls)
                e["min_us"] = min(e["min_us"], mn / 1e3)
    return 0, dict(probe="kernels", robot=robot, batch=B, variant="ring256", ticks=ticks, kernels=split,
                   launched=sorted({n.split("(")[0] for n, *_ in rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent-lib", help="libbpmpc.so built from the parent commit: timed beside this one")
    ap.add_argument("--profile", action="store_true", help="one more child per shape under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--commit", help="the commit the library was built from, recorded in every line")
    ap.add_argument("--limit", type=int, default=180, help="time limit of one child process [s]")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:      # one measurement, in this process
        what, robot, B = a.child.split(":")
        line = measure(robot, int(B), what, a.parent_lib, a.ticks, a.warmup)
        if a.commit:
            line["commit"] = a.commit
        print(json.dumps(line), flush=True)
        return 0
    variants = (["parent"] if a.parent_lib else []) + ["detached", "ring0", "ring256"]
    jobs = ["%s:%s" % (v, shape) for shape in a.shapes.split(",") for _ in range(a.repeats) for v in variants]
    if a.profile:
        jobs += ["profile:%s" % shape for shape in a.shapes.split(",")]
    lines = []
    for job in jobs:
        if job.startswith("profile:"):
            _, robot, B = job.split(":")
            rc, rec = kernel_split(robot, int(B), 20, a.limit)
            if a.commit:
                rec["commit"] = a.commit
            text = json.dumps(rec)
        else:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", job, "--ticks", str(a.ticks), "--warmup", str(a.warmup)]
            cmd += (["--parent-lib", a.parent_lib] if a.parent_lib else []) + (["--commit", a.commit] if a.commit else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            rc, text = r.returncode, (r.stdout.strip().splitlines() or [""])[-1]
        if rc != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
            print("telemetry_probe: %s ended with status %d; stopping" % (job, rc), file=sys.stderr)
            break
        print(text, flush=True)
        lines.append(text)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for text in lines:
                f.write(text + "\n")
    return 0 if len(lines) == len(jobs) else 1


if __name__ == "__main__":
    sys.exit(main())
