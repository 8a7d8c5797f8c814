#!/usr/bin/env python3
"""What the plant's input model costs, in one process per measurement on one box.

Per shape, `--repeats` rounds that alternate child processes:
  parent      the library of --parent-lib (built from the parent commit), an untouched handle          (only with --parent-lib)
  untouched   this library, a handle that never heard of the input model
  switched    this library, one handle timed four ways in one process: untouched; the input model on every robot (the H1 file's 9 ms, 5 % loss, a
              50 N push of 0.1 s every second): k_plant_input in front of every step; the input model reset and IMU-grade sensor rows instead:
              k_plant_sense behind every step; and, beside them, a device-to-device copy that moves the bytes k_plant_input moves (4 * 5 * nj * 8 B
              per robot, half of them read and half written)
Each sample is a block of `--block` calls of bpmpc_plant_step on device tensors - a PD that holds the standing pose, `--substeps` substeps - that are
only enqueued, with a host clock around the block and the one-robot bpmpc_plant_get_state that drains the plant's stream, divided by the block's
length; the state is set back before every block.  The plant's stream is not exposed by the C ABI, so no event can be recorded on it: a number here
is the time per step of a stream that is kept busy, as a caller sees it, not a kernel time.  Per variant: the median, the minimum and the 5th / 95th
percentile of `--samples` samples after `--warmup`.
One JSON line per measurement on stdout; --out appends them to a file (profiles/plant_input_probe.jsonl is where the published one belongs).
Every measurement runs in a child process of its own under a time limit; the first that fails or runs out of time ends the probe.
usage (GPU box, repository root): python tools/plant_input_probe.py [--shapes h1:1,h1:256,h1:4096] [--parent-lib FILE] [--commit ID] [--out FILE]
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
INPUTS = dict(delay=0.009, dropout=0.05, push_force=50.0, push_interval=1.0, push_duration=0.1)


def measure(robot, B, variant, parent_lib, samples, warmup, block, substeps, period):
    import numpy as np
    import torch
    import bipedal_control_amd as bp
    if variant == "parent":
        pk.use_parent_library(parent_lib)
    itf, plant, r_dev, cmd = pk.standing_plant(robot, B)
    nj = itf.actuatedDofNum

    def steps():
        return pk.steps(plant, r_dev, cmd, samples, warmup, block, substeps, period)

    line = dict(probe="plant_input", robot=robot, batch=B, variant=variant, samples=samples, block=block, substeps=substeps, period=period,
                clock=pk.STEPS_CLOCK)
    line.update(pk.host_stats("step", steps(), "us"))
    if variant == "switched":
        plant.setInputParams(bp.InputParams(**INPUTS).toRow())
        plant.seedInputs(1)
        with_inputs = steps()
        state = plant.inputState()
        plant.resetInputParams()
        plant.setSensorParams(bp.SensorParams(**IMU_GRADE).toRow())
        plant.seedSensors(1)
        with_sensors = steps()
        plant.resetSensorParams()
        bytes_moved = B * 4 * 5 * nj * 8
        words = max(1, bytes_moved // 16)
        src, dst = torch.zeros(words, dtype=torch.float64, device="cuda"), torch.zeros(words, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        copies = []
        for k in range(warmup + samples):
            t0 = time.perf_counter()
            for _ in range(block):
                dst.copy_(src)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if k >= warmup:
                copies.append(1e6 * dt / block)
        base = line["step_us_median"]
        line.update(pk.host_stats("step_inputs", with_inputs, "us"))
        line.update(pk.host_stats("step_sensors", with_sensors, "us"))
        line.update(pk.host_stats("copy", np.array(copies), "us"))
        line.update(inputs=INPUTS, sensors=IMU_GRADE, input_ticks=int(state["tick"][0]), input_delay_steps=int(state["delay_steps"][0]),
                    input_extra_us=float(np.median(with_inputs) - base), sensor_extra_us=float(np.median(with_sensors) - base),
                    bytes_moved=int(bytes_moved), copy_bytes_each_way=int(8 * words))
    line["state_finite"] = bool(np.isfinite(plant.get_state()).all())
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--substeps", type=int, default=4)
    ap.add_argument("--period", type=float, default=0.002)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent-lib", help="libbpmpc.so built from the parent commit: timed beside this one on an untouched handle")
    pk.driver_options(ap, limit=120)
    a = ap.parse_args()
    if a.child:      # one measurement, in this process
        what, robot, B = a.child.split(":")
        return pk.child_line(a, measure(robot, int(B), what, a.parent_lib, a.samples, a.warmup, a.block, a.substeps, a.period))
    variants = (["parent"] if a.parent_lib else []) + ["untouched", "switched"]
    jobs = ["%s:%s" % (v, shape) for shape in a.shapes.split(",") for _ in range(a.repeats) for v in variants]
    return pk.run_jobs(__file__, jobs, pk.forwarded(a), a.limit, a.out)


if __name__ == "__main__":
    sys.exit(main())
