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
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402

SHAPES = "h1:1,h1:256,h1:4096"
RINGS = {"ring0": 0, "ring256": 256}
KERNELS = ("k_tick_observe_policy", "k_wbc", "k_tick_commands", "k_telemetry")


def measure(robot, B, variant, parent_lib, ticks, warmup):
    import numpy as np
    import torch
    import bipedal_control_amd as bp
    if variant == "parent":
        pk.use_parent_library(parent_lib)
    stream = torch.cuda.Stream()
    mpc, ctrl, rbd = pk.tick_fleet(robot, B, stream.cuda_stream)
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
    line = dict(probe="timing", robot=robot, batch=B, variant=variant, ticks=ticks, **pk.host_stats("tick_host", times, "ms"),
                wbc_unsolved=int(ctrl.device_outputs()["wbc_status"].torch().sum().item()))
    if tel is not None:
        s = tel.stats(B)
        line.update(ring_len=RINGS[variant], samples=int(s["samples"].min()), frozen=int(s["frozen"].sum()), stats_finite=bool(np.isfinite(s["rows"]).all()))
        ctrl.attachTelemetry(None)
    return line


def profile(script, job, args, limit):
    """a job "profile:<shape>": the ring256 variant under the profiler, its per-kernel averages as the line; every other job is a plain child"""
    if not job.startswith("profile:"):
        return pk.run_child(script, job, args, limit)
    _, robot, B = job.split(":")
    status, split, launched = pk.kernel_split(script, ["--child", "ring256:%s:%s" % (robot, B), "--ticks", "20", "--warmup", "2"], KERNELS, limit)
    if status != 0:
        return status, ""
    rec = dict(probe="kernels", robot=robot, batch=int(B), variant="ring256", ticks=20, kernels=split, launched=launched)
    commit = args[args.index("--commit") + 1] if "--commit" in args else None
    return 0, json.dumps(dict(rec, commit=commit) if commit else rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent-lib", help="libbpmpc.so built from the parent commit: timed beside this one")
    ap.add_argument("--profile", action="store_true", help="one more child per shape under rocprofv3 --kernel-trace --stats")
    pk.driver_options(ap, limit=180)
    a = ap.parse_args()
    if a.child:      # one measurement, in this process
        what, robot, B = a.child.split(":")
        return pk.child_line(a, measure(robot, int(B), what, a.parent_lib, a.ticks, a.warmup))
    variants = (["parent"] if a.parent_lib else []) + ["detached", "ring0", "ring256"]
    jobs = ["%s:%s" % (v, shape) for shape in a.shapes.split(",") for _ in range(a.repeats) for v in variants]
    if a.profile:
        jobs += ["profile:%s" % shape for shape in a.shapes.split(",")]
    return pk.run_jobs(__file__, jobs, pk.forwarded(a), a.limit, a.out, run=profile)


if __name__ == "__main__":
    sys.exit(main())
