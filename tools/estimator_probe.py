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
same run.  Every shape runs in a child process of its own under a time limit (--limit seconds), the alternation with the parent's library inside
that child; the first shape that fails or runs out of time, a failed profiler run included, ends the probe.  One JSON line per shape on stdout;
--out appends them to a file (profiles/estimator_probe.jsonl is where the published one belongs).
usage (GPU box, repository root): python tools/estimator_probe.py [--shapes h1:1,h1:256,h1:4096,g1:1024] [--ticks 50] [--profile] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402
from tools.probekit import library      # noqa: E402

SHAPES = "h1:1,h1:256,h1:4096,g1:1024"
RATIO = ("estimate_over_wbc", "k_estimate", "k_wbc")
KERNELS = ("k_estimate", "k_tick_observe_policy", "k_wbc", "k_tick_commands")


def measure(robot, B, ticks, warmup, parent=None, repeats=1):
    import numpy as np
    import torch
    import bipedal_control_amd as bp
    from bipedal_control_amd import api
    stream = torch.cuda.Stream()
    mpc, ctrl, rbd = pk.tick_fleet(robot, B, stream.cuda_stream)
    p_stream = p_mpc = p_ctrl = None
    if parent is not None:
        p_stream = torch.cuda.Stream()
        with library(api, parent):
            p_mpc, p_ctrl, _ = pk.tick_fleet(robot, B, p_stream.cuda_stream)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--parent-lib", help="libbpmpc.so built from the parent commit: its plain tick is timed in the same alternation")
    ap.add_argument("--profile", action="store_true")
    pk.driver_options(ap, limit=240)
    a = ap.parse_args()
    if a.child:      # one shape, in this process
        parent = None
        if a.parent_lib:
            parent = pk.parent_library(a.parent_lib)      # the parent exports less than the header declares
            if hasattr(parent, "bpmpc_estimator_update"):
                raise SystemExit("--parent-lib already has bpmpc_estimator_update: not the parent commit's library")
        robot, B = a.child.split(":")
        return pk.child_line(a, measure(robot, int(B), a.ticks, a.warmup, parent, a.repeats))
    return pk.run_jobs(__file__, a.shapes.split(","), pk.forwarded(a), a.limit, a.out, run=pk.run_child_profiled(KERNELS, RATIO))


if __name__ == "__main__":
    sys.exit(main())
