#!/usr/bin/env python3
"""Latency of the batched rigid-body plant (bpmpc_plant_step / bpmpc_plant_step_controlled: k_plant_step on the plant's stream) beside the
controller tick, in one process on one box.

Per shape: a solved batch (setup_commands + run), one tick for the joint commands, the plant set to the tick's rbd, device command tensors, then
`--warmup` + `--ticks` rounds that alternate
  tick             bpmpc_controller_tick on a device rbd                          (three kernels on the solver's stream; mpc.synchronize)
  step             bpmpc_plant_step on device tensors                             (one launch of `--substeps` substeps; the plant's stream drained
                                                                                  by a one-robot bpmpc_plant_get_state)
  step_controlled  bpmpc_plant_step_controlled on the tick's device outputs        (the same launch behind an event of the solver's stream)
each timed with a host clock around the call and the synchronise that ends it; the medians and minima are reported.  A number here is a call time
as a caller sees it (launch, kernel, synchronise), not a kernel time.  The state is set back before every timed step, so every step advances the
same standing robots.  One JSON line per shape on stdout; --out appends them to a file (profiles/plant_probe.jsonl is where the published one
belongs).  --kt K gives every robot the tangential stiffness K (BatchedPlant.setStiction; "kn": the robot's kn) before the rounds; without it the
handle never hears of stiction.  --commit names the commit the library was built from in every line.  Beside the median and the minimum a line
holds the 5th and 95th percentile of the 200 as the spread.  Every shape runs in a child process of its own under a time limit (--limit seconds);
the first shape that fails or runs out of time ends the probe.
usage (GPU box, repository root): python tools/plant_probe.py [--shapes h1:1,h1:256,h1:4096] [--ticks 200] [--substeps 4] [--kt K] [--commit ID] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402

SHAPES = "h1:1,h1:256,h1:4096"


def measure(robot, B, ticks, warmup, substeps, period, kt=None):
    import numpy as np
    import torch
    import bipedal_control_amd as bp
    stream = torch.cuda.Stream()
    mpc, ctrl, rbd = pk.tick_fleet(robot, B, stream.cuda_stream)
    nj = ctrl.nj
    ctrl.setJointGains(np.full(nj, bp.WbcParams.RECONFIGURE_MOTOR_KP), np.full(nj, bp.WbcParams.RECONFIGURE_MOTOR_KD))
    rbd[:, 5] -= 0.0025                                    # the soles a little in the ground: every contact closed
    plant = bp.BatchedPlant(mpc.interface, max_batch=B)
    if kt is not None:
        plant.batch = B
        plant.setStiction(plant.getParams()[0] if kt == "kn" else float(kt))
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")      # noqa: E731
    t_dev, r_dev = torch.full((B,), 0.0025, dtype=torch.float64, device="cuda"), dev(rbd)
    torch.cuda.synchronize()
    out = ctrl.tick(t_dev, r_dev)
    cmd = [dev(out["joint_cmd"][:, i]) for i in range(3)] + [dev(out["joint_kp"]), dev(out["joint_kd"])]
    torch.cuda.synchronize()
    plant.set_state(r_dev)

    def tick():
        ctrl.tick(t_dev, r_dev, fetch=False)
        mpc.synchronize()

    def step():
        plant.step(*cmd, period=period, substeps=substeps)
        plant.get_state(1)

    def step_controlled():
        plant.step_controlled(ctrl, period=period, substeps=substeps)
        plant.get_state(1)

    variants = [("tick", tick), ("step", step), ("step_controlled", step_controlled)]
    times = {name: [] for name, _ in variants}
    for k in range(warmup + ticks):
        for name, fn in variants:
            if name != "tick":
                plant.set_state(r_dev)
                plant.get_state(1)
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if k >= warmup:
                times[name].append(1e3 * dt)
    state = plant.get_state()
    line = dict(robot=robot, batch=B, ticks=ticks, substeps=substeps, period=period, state_finite=bool(np.isfinite(state).all()),
                contacts_closed=int(plant.outputs()["contact"].torch().sum().item()))
    if kt is not None:
        line["kt"] = float(plant.getStiction(0))
        line["anchored"] = int(plant.anchors()[1].sum())
    for name, _ in variants:
        line.update(pk.host_stats(name + "_host", times[name], "ms"))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--substeps", type=int, default=4)
    ap.add_argument("--period", type=float, default=0.002)
    ap.add_argument("--kt", help="tangential stiffness of every robot [N/m], or kn")
    pk.driver_options(ap, limit=240)
    a = ap.parse_args()
    if a.child:      # one shape, in this process
        robot, B = a.child.split(":")
        return pk.child_line(a, measure(robot, int(B), a.ticks, a.warmup, a.substeps, a.period, a.kt))
    return pk.run_jobs(__file__, a.shapes.split(","), pk.forwarded(a), a.limit, a.out)


if __name__ == "__main__":
    sys.exit(main())
