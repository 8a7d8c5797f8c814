#!/usr/bin/env python3
"""Latency of the controller tick (bpmpc_controller_tick: k_tick_observe_policy, k_wbc, k_tick_commands on the solver's stream).

Per shape: a solved batch (setup_commands + run), then `--warmup` + `--ticks` ticks with device inputs and no host outputs.  Two clocks:
  device   torch.cuda events on the solver's stream around each tick (what the three kernels and their gaps take)
  host     perf_counter around tick + synchronise (what a caller that waits for the result sees, launch overhead included)
With --profile every shape is run once more in a child process under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters); the
per-kernel averages are read from its rocpd database.  Every shape runs in a child process of its own under a time limit (--limit seconds); the
first shape that fails or runs out of time, a failed profiler run included, ends the probe.  One JSON line per shape on stdout; --out appends
them to a file.
usage (GPU box, repository root): python tools/controller_tick_probe.py [--shapes h1:1,h1:256,h1:4096,g1:1024] [--ticks 50] [--profile]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402

SHAPES = "h1:1,h1:256,h1:4096,g1:1024"
RATIO = ("observe_policy_over_wbc", "k_tick_observe_policy", "k_wbc")
KERNELS = ("k_tick_observe_policy", "k_wbc", "k_tick_commands")


def measure(robot, B, ticks, warmup):
    import numpy as np
    import torch
    stream = torch.cuda.Stream()
    mpc, ctrl, rbd = pk.tick_fleet(robot, B, stream.cuda_stream)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    pk.driver_options(ap, limit=240)
    a = ap.parse_args()
    if a.child:      # one shape, in this process
        robot, B = a.child.split(":")
        return pk.child_line(a, measure(robot, int(B), a.ticks, a.warmup))
    return pk.run_jobs(__file__, a.shapes.split(","), pk.forwarded(a), a.limit, a.out, run=pk.run_child_profiled(KERNELS, RATIO))


if __name__ == "__main__":
    sys.exit(main())
