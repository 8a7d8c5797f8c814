#!/usr/bin/env python3
"""Latency of the controller tick (bpmpc_controller_tick: k_tick_observe_policy, k_wbc, k_tick_commands on the solver's stream).

Per shape: a solved batch (setup_commands + run), then `--warmup` + `--ticks` ticks with device inputs and no host outputs.  Two clocks:
  device   torch.cuda events on the solver's stream around each tick (what the three kernels and their gaps take)
  host     perf_counter around tick + synchronise (what a caller that waits for the result sees, launch overhead included)
With --profile every shape is run once more in a child process under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters); the
per-kernel averages are read from its rocpd database.  One JSON line per shape on stdout; --out writes them all to a file as well.
usage (GPU box, repository root): python tools/controller_tick_probe.py [--shapes h1:1,h1:256,h1:4096,g1:1024] [--ticks 50] [--profile]
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

SHAPES = "h1:1,h1:256,h1:4096,g1:1024"
NI = 40


def _setup(robot, B, stream):
    import numpy as np
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface(robot)
    horizon = NI * sc.DT
    tm = [bp.loadModeSequenceTemplate(itf.gaitFile, "trot")]
    x0 = sc.perturbed_initial_states(itf, B)
    cmd = np.tile(np.array([0.2, 0.0, 0.0, 0.0]), (B, 1))
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=sc.max_nodes_for(NI, horizon), return_gains=True, stream=stream)
    mpc.setup_commands(0.0, x0, tm, np.zeros(B, np.int32), sc.GAIT_START, cmd, horizon=horizon)
    mpc.enqueue()
    mpc.synchronize()
    ctrl = bp.BatchedController(mpc, bp.WeightedWbc(itf, max_batch=B))
    nj = itf.actuatedDofNum
    q = x0[:, 6:]
    rbd = np.concatenate([q[:, 3:6], q[:, 0:3], q[:, 6:], np.zeros((B, 6 + nj))], axis=1)     # at rest at the planned configuration
    return mpc, ctrl, rbd


def measure(robot, B, ticks, warmup):
    import numpy as np
    import torch
    stream = torch.cuda.Stream()
    mpc, ctrl, rbd = _setup(robot, B, stream.cuda_stream)
    t_dev = torch.full((B,), 0.0025, dtype=torch.float64, device="cuda")
    r_dev = torch.tensor(rbd, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(warmup):
        ctrl.tick(t_dev, r_dev, fetch=False)
    mpc.synchronize()
    dev_ms, host_ms = [], []
    for _ in range(ticks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        ctrl.tick(t_dev, r_dev, fetch=False)
        b.record(stream)
        mpc.synchronize()
        host_ms.append(1e3 * (time.perf_counter() - t0))
        dev_ms.append(a.elapsed_time(b))
    outs = ctrl.device_outputs()
    unsolved = int(outs["wbc_status"].torch().sum().item())
    return dict(robot=robot, batch=B, ticks=ticks, device_ms_median=float(np.median(dev_ms)), device_ms_min=float(np.min(dev_ms)),
                host_ms_median=float(np.median(host_ms)), host_ms_min=float(np.min(host_ms)), wbc_unsolved=unsolved)


def kernel_split(robot, B, ticks, timeout):
    """Per-kernel averages from a separate rocprofv3 --kernel-trace --stats run of this tool (child process)."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
               "--shapes", "%s:%d" % (robot, B), "--ticks", str(ticks), "--warmup", "2"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            return {"error": "rocprofv3 exit %d" % r.returncode, "stderr_tail": r.stderr[-400:]}
        db = sqlite3.connect(dbs[0])
        rows = db.execute("select name, count(*), avg(duration), min(duration) from kernels group by name").fetchall()
    split = {}
    for name, calls, avg, mn in rows:
        for k in ("k_tick_observe_policy", "k_wbc", "k_tick_commands"):
            if k in name:
                split[k] = dict(calls=int(calls), avg_us=avg / 1e3, min_us=mn / 1e3)
    if "k_tick_observe_policy" in split and "k_wbc" in split:
        split["observe_policy_over_wbc"] = split["k_tick_observe_policy"]["avg_us"] / split["k_wbc"]["avg_us"]
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-timeout", type=int, default=240)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []
    for shape in args.shapes.split(","):
        robot, B = shape.split(":")
        rec = measure(robot, int(B), args.ticks, args.warmup)
        if args.profile:
            rec["kernels"] = kernel_split(robot, int(B), min(args.ticks, 20), args.profile_timeout)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
