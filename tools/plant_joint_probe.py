#!/usr/bin/env python3
"""What the plant's joint model costs, in one process per measurement on one box.  Scenario and method are those of tools/plant_input_probe.py.

Per shape, `--repeats` rounds that alternate child processes:
  parent      the library of --parent-lib (built from the parent commit), an untouched handle          (only with --parent-lib)
  untouched   this library, a handle that never heard of the joint model: it launches k_plant_step as the parent does
  switched    this library, one handle timed twice in one process: untouched; then with JointParams.reference_mjcf rows (armature 0.1, damping 1) and
              finite limits 0.5 rad either side of the standing pose on every robot: k_plant_joint_step in place of k_plant_step
Each sample is a block of `--block` calls of bpmpc_plant_step on device tensors - a PD that holds the standing pose, `--substeps` substeps - that are
only enqueued, with a host clock around the block and the one-robot bpmpc_plant_get_state that drains the plant's stream, divided by the block's
length; the state is set back before every block.  The plant's stream is not exposed by the C ABI, so no event can be recorded on it: a number here
is the time per step of a stream that is kept busy, as a caller sees it, not a kernel time.  Per variant: the median, the minimum and the 5th / 95th
percentile of `--samples` samples after `--warmup`.
The condition the project puts on a model that is off until used: an untouched handle costs what the parent costs, within the difference between
the two rounds of one variant measured in the same call.  The probe reports the medians; it bounds nothing.  The cost of a switched handle is
reported, not bounded.
One JSON line per measurement on stdout; --out appends them to a file (profiles/plant_joint_probe.jsonl is where the published one belongs).
Every measurement runs in a child process of its own under a time limit; the first that fails or runs out of time ends the probe.
usage (GPU box, repository root): python tools/plant_joint_probe.py [--shapes h1:1,h1:256,h1:4096] [--parent-lib FILE] [--commit ID] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402

SHAPES = "h1:1,h1:256,h1:4096"
LIMIT_MARGIN = 0.5      # rad either side of the standing pose


def measure(robot, B, variant, parent_lib, samples, warmup, block, substeps, period):
    import numpy as np
    import bipedal_control_amd as bp
    if variant == "parent":
        pk.use_parent_library(parent_lib)
    itf, plant, r_dev, cmd = pk.standing_plant(robot, B)
    nj = itf.actuatedDofNum
    pose = r_dev[0, 6:6 + nj].cpu().numpy()

    def steps():
        return pk.steps(plant, r_dev, cmd, samples, warmup, block, substeps, period)

    line = dict(probe="plant_joint", robot=robot, batch=B, variant=variant, samples=samples, block=block, substeps=substeps, period=period,
                clock=pk.STEPS_CLOCK)
    line.update(pk.host_stats("step", steps(), "us"))
    if variant == "switched":
        rows = bp.JointParams.reference_mjcf(nj)
        rows.lower, rows.upper = pose - LIMIT_MARGIN, pose + LIMIT_MARGIN
        plant.setJointParams(rows.toRow())
        with_joints = steps()
        finite = bool(np.isfinite(plant.get_state()).all())
        plant.resetJointParams()
        line.update(pk.host_stats("step_joints", with_joints, "us"))
        line.update(joints=dict(armature=0.1, damping=1.0, limit_margin=LIMIT_MARGIN), joint_extra_us=float(np.median(with_joints) - line["step_us_median"]),
                    joints_state_finite=finite)
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
