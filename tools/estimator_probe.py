#!/usr/bin/env python3
"""Latency of the batched state estimator (bpmpc_estimator_update: k_estimate on the estimator's stream) beside the controller tick.

Per shape: a solved batch (setup_commands + run), device sensor tensors, then `--warmup` + `--ticks` rounds that alternate
  tick        bpmpc_controller_tick on a device rbd                                           (three kernels on the solver's stream)
  estimated   bpmpc_estimator_update (only enqueued) + bpmpc_controller_tick_estimated        (the solver's stream waits for k_estimate)
each between two events on the solver's stream and followed by a synchronise; the medians and their difference - the estimator's share of a
tick as a caller sees it - are reported, with a host clock around the same calls.  With --parent-lib (the libbpmpc.so of the parent commit,
loaded beside this tree's in the same process) a third fleet ticks through that library in the same alternation: the same-box pair that says
whether the plain tick moved, `--repeats` medians of each giving the spread of the pair.  The estimator's stream is its own, so k_estimate itself is
taken from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--profile, a child process, no counters) and set beside k_wbc of the
same run.  One JSON line per shape on stdout; --out writes them all to a file as well (profiles/estimator_probe.jsonl is where the published one belongs).
usage (GPU box, repository root): python tools/estimator_probe.py [--shapes h1:1,h1:256,h1:4096,g1:1024] [--ticks 50] [--profile] [--out FILE]
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

from tools.controller_tick_probe import SHAPES, _setup      # noqa: E402
from tools.wbc_params_probe import library      # noqa: E402


def measure(robot, B, ticks, warmup, parent=None, repeats=1):
    import numpy as np
    import torch
    import bipedal_control_amd as bp
    from bipedal_control_amd import api
    stream = torch.cuda.Stream()
    mpc, ctrl, rbd = _setup(robot, B, stream.cuda_stream)
    p_stream = p_mpc = p_ctrl = None
    if parent is not None:
        p_stream = torch.cuda.Stream()
        with library(api, parent):
            p_mpc, p_ctrl, _ = _setup(robot, B, p_stream.cuda_stream)
    nj = ctrl.nj
    est = bp.BatchedStateEstimate(mpc.interface, kind="kalman", max_batch=B)
    dev = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device="cuda")      # noqa: E731
    t_dev, r_dev = torch.full((B,), 0.0025, dtype=torch.float64, device="cuda"), dev(rbd)
    quat = np.tile([0.0, 0.0, 0.0, 1.0], (B, 1))
    sensors = dict(joint_pos=dev(rbd[:, 6:6 + nj]), joint_vel=dev(np.zeros((B, nj))), quat=dev(quat), angular_vel_local=dev(np.zeros((B, 3))),
                   linear_accel_local=dev(np.tile([0.0, 0.0, 9.81], (B, 1))), mode=dev(np.full(B, 3), torch.int32))
    torch.cuda.synchronize()

    def plain():
        ctrl.tick(t_dev, r_dev, fetch=False)

    def estimated():
        est.update(period=0.0025, fetch=False, **sensors)
        ctrl.tick_estimated(t_dev, est, fetch=False)

    def parent_tick():
        with library(api, parent):
            p_ctrl.tick(t_dev, r_dev, fetch=False)

    def parent_sync():
        with library(api, parent):
            p_mpc.synchronize()

    variants = [("tick", plain, stream, mpc.synchronize), ("estimated", estimated, stream, mpc.synchronize)]
    if parent is not None:
        variants.append(("parent_tick", parent_tick, p_stream, parent_sync))
    for _ in range(warmup):
        for _, fn, _, sync in variants:
            fn()
            sync()
    medians = {name: [] for name, *_ in variants}
    times = {name: ([], []) for name, *_ in variants}
    for _ in range(repeats):
        once = {name: [] for name, *_ in variants}
        for _ in range(ticks):
            for name, fn, st, sync in variants:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record(st)
                fn()
                b.record(st)
                sync()
                times[name][1].append(1e3 * (time.perf_counter() - t0))
                times[name][0].append(a.elapsed_time(b))
                once[name].append(times[name][0][-1])
        for name in once:
            medians[name].append(float(np.median(once[name])))
    med = {k: (float(np.median(v[0])), float(np.median(v[1]))) for k, v in times.items()}
    x_hat = est.getState()[0]
    extra = {}
    if parent is not None:
        spread = max(max(medians[k]) - min(medians[k]) for k in ("tick", "parent_tick"))
        extra = dict(parent_tick_device_ms_median=med["parent_tick"][0], tick_minus_parent_ms=med["tick"][0] - med["parent_tick"][0],
                     repeat_medians_ms={k: medians[k] for k in ("tick", "parent_tick")}, pair_spread_ms=spread,
                     tick_within_spread_of_parent=bool(abs(med["tick"][0] - med["parent_tick"][0]) <= spread))
        plain()                            # both fleets end on a plain tick of the same inputs
        mpc.synchronize()
        parent_tick()
        parent_sync()
        same = torch.equal(ctrl_solution(api, None, ctrl), ctrl_solution(api, parent, p_ctrl))
        extra["plain_tick_same_bits_as_parent"] = bool(same)
        with library(api, parent):         # a handle is destroyed by the library that created it
            del p_ctrl, p_mpc
            import gc
            gc.collect()
    return dict(**extra, robot=robot, batch=B, ticks=ticks, tick_device_ms_median=med["tick"][0], estimated_device_ms_median=med["estimated"][0],
                estimator_device_ms_by_difference=med["estimated"][0] - med["tick"][0], tick_host_ms_median=med["tick"][1],
                estimated_host_ms_median=med["estimated"][1], tick_device_ms_min=float(np.min(times["tick"][0])),
                estimated_device_ms_min=float(np.min(times["estimated"][0])), x_hat_finite=bool(np.all(np.isfinite(x_hat))))


def ctrl_solution(api, lib, ctrl):
    """wbc_solution of the last tick as a host tensor, read through the library that owns the handle"""
    import ctypes as C
    o = api._TickOutputs()
    if lib is None:
        api._check(api.load_library().bpmpc_controller_device_outputs(ctrl._h, C.byref(o)))
    else:
        with library(api, lib):
            api._check(lib.bpmpc_controller_device_outputs(ctrl._h, C.byref(o)))
    B = ctrl.mpc.batch
    return api.DeviceArray(C.cast(o.wbc_solution, C.c_void_p).value, (B, ctrl.wbc.numDecisionVars), "<f8").torch().cpu()


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
        for k in ("k_estimate", "k_tick_observe_policy", "k_wbc", "k_tick_commands"):
            if k in name:
                split[k] = dict(calls=int(calls), avg_us=avg / 1e3, min_us=mn / 1e3)
    if "k_estimate" in split and "k_wbc" in split:
        split["estimate_over_wbc"] = split["k_estimate"]["avg_us"] / split["k_wbc"]["avg_us"]
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--parent-lib", help="libbpmpc.so built from the parent commit: its plain tick is timed in the same alternation")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-timeout", type=int, default=240)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []
    parent = None
    if args.parent_lib:
        import ctypes as C
        from bipedal_control_amd import abi
        parent = abi.bind(C.CDLL(os.path.abspath(args.parent_lib)), strict=False)      # the parent exports less than the header declares
        if hasattr(parent, "bpmpc_estimator_update"):
            raise SystemExit("--parent-lib already has bpmpc_estimator_update: not the parent commit's library")
    for shape in args.shapes.split(","):
        robot, B = shape.split(":")
        rec = measure(robot, int(B), args.ticks, args.warmup, parent, args.repeats)
        if args.profile:
            rec["kernels"] = kernel_split(robot, int(B), min(args.ticks, 20), args.profile_timeout)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
