#!/usr/bin/env python3
"""What the plant's sensor model costs, and what it does to the Kalman estimate, in one process per measurement on one box.

timing (default)   Per shape, `--repeats` rounds that alternate child processes:
                     parent      the library of --parent-lib (built from the parent commit), an untouched handle          (only with --parent-lib)
                     untouched   this library, a handle that never heard of the sensor model
                     switched    this library, IMU-grade rows on every robot (gyro 2e-3, accel 2e-2, joint 1e-4, delay 1): k_plant_sense behind every step
                   Each child times bpmpc_plant_step on device tensors - a PD that holds the standing pose, `--substeps` substeps - with a host clock
                   around the call and the one-robot bpmpc_plant_get_state that drains the plant's stream: the median, the minimum and the 5th / 95th
                   percentile of `--ticks` calls.  The state is set back before every timed step.  A number here is a call time as a caller sees it,
                   not a kernel time.
--estimate         H1, batch 8: `--seconds` of plant.step under the holding PD with the Kalman filter behind it (update_from_plant), once with an
                   untouched handle and once with the IMU-grade rows; the largest and the root-mean-square error of the estimate's base position and
                   linear velocity against the plant's rbd over the second half of the run.  Context, not a claim.
One JSON line per measurement on stdout; --out appends them to a file (profiles/plant_sensor_probe.jsonl is where the published one belongs).
Every measurement runs in a child process of its own under a time limit; the first that fails or runs out of time ends the probe.
usage (GPU box, repository root): python tools/plant_sensor_probe.py [--shapes h1:1,h1:256,h1:4096] [--parent-lib FILE] [--estimate] [--commit ID] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402
from tools.probekit import IMU_GRADE      # noqa: E402

SHAPES = "h1:1,h1:256,h1:4096"


def measure(robot, B, variant, parent_lib, ticks, warmup, substeps, period):
    import numpy as np
    import bipedal_control_amd as bp
    if variant == "parent":
        pk.use_parent_library(parent_lib)
    _, plant, r_dev, cmd = pk.standing_plant(robot, B)
    if variant == "switched":
        plant.setSensorParams(bp.SensorParams(**IMU_GRADE).toRow())
        plant.seedSensors(1)
    times = []
    for k in range(warmup + ticks):
        plant.set_state(r_dev)
        plant.get_state(1)
        t0 = time.perf_counter()
        plant.step(*cmd, period=period, substeps=substeps)
        plant.get_state(1)
        dt = time.perf_counter() - t0
        if k >= warmup:
            times.append(1e3 * dt)
    line = dict(probe="timing", robot=robot, batch=B, variant=variant, ticks=ticks, substeps=substeps, period=period,
                state_finite=bool(np.isfinite(plant.get_state()).all()), **pk.host_stats("step_host", times, "ms"))
    if variant == "switched":
        line["sensor_ticks"] = int(plant.sensorState()["tick"][0])
    return line


def estimate(robot, B, noisy, seconds, substeps, period):
    import numpy as np
    import bipedal_control_amd as bp
    itf, rbd, cmd = pk.standing(robot, B)
    nv = 6 + itf.actuatedDofNum
    plant = bp.BatchedPlant(itf, max_batch=B)
    est = bp.BatchedStateEstimate(itf, kind="kalman", max_batch=B)
    if noisy:
        plant.setSensorParams(bp.SensorParams(**IMU_GRADE).toRow())
        plant.seedSensors(1)
    plant.set_state(rbd)
    n = int(round(seconds / period))
    pos, vel = [], []
    for k in range(n):
        plant.step(*cmd, period=period, substeps=substeps)
        e = est.update_from_plant(plant, period=period)
        truth = plant.get_state()
        if k >= n // 2:
            pos.append(e[:, 3:6] - truth[:, 3:6])
            vel.append(e[:, nv + 3:nv + 6] - truth[:, nv + 3:nv + 6])
    pos, vel = np.array(pos), np.array(vel)
    return dict(probe="estimate", robot=robot, batch=B, noisy=bool(noisy), seconds=seconds, substeps=substeps, period=period, rows=IMU_GRADE if noisy else None,
                finite=bool(np.isfinite(pos).all() and np.isfinite(vel).all()), base_height_end=float(truth[:, 5].mean()),
                position_error_max=float(np.abs(pos).max()), position_error_rms=float(np.sqrt((pos ** 2).mean())),
                velocity_error_max=float(np.abs(vel).max()), velocity_error_rms=float(np.sqrt((vel ** 2).mean())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--substeps", type=int, default=4)
    ap.add_argument("--period", type=float, default=0.002)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent-lib", help="libbpmpc.so built from the parent commit: timed beside this one on an untouched handle")
    ap.add_argument("--estimate", action="store_true", help="the Kalman estimate's error with and without noise instead of the timing")
    ap.add_argument("--seconds", type=float, default=1.0)
    pk.driver_options(ap, limit=180)
    a = ap.parse_args()
    if a.child:      # one measurement, in this process
        what, robot, B = a.child.split(":")
        if what in ("clean", "noisy"):
            return pk.child_line(a, estimate(robot, int(B), what == "noisy", a.seconds, a.substeps, a.period))
        return pk.child_line(a, measure(robot, int(B), what, a.parent_lib, a.ticks, a.warmup, a.substeps, a.period))
    if a.estimate:
        jobs = ["clean:h1:8", "noisy:h1:8"]
    else:
        variants = (["parent"] if a.parent_lib else []) + ["untouched", "switched"]
        jobs = ["%s:%s" % (v, shape) for shape in a.shapes.split(",") for _ in range(a.repeats) for v in variants]
    return pk.run_jobs(__file__, jobs, pk.forwarded(a), a.limit, a.out)


if __name__ == "__main__":
    sys.exit(main())
