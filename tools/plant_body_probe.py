#!/usr/bin/env python3
"""Two measurements of the plant's body rows (include/bpmpc.h "Plant", bodies), in one process per measurement on one box.

(a) What the body rows cost.  Scenario, method and protocol are those of tools/plant_joint_probe.py.  Per shape, `--repeats` rounds that alternate
    child processes:
      parent      the library of --parent-lib (built from the parent commit), an untouched handle          (only with --parent-lib)
      untouched   this library, a handle that never heard of body rows: it launches k_plant_step as the parent does
      switched    this library, one handle timed twice in one process: untouched; then with body rows on every robot (every body x 0.8 on the
                  even robots, a 10 kg payload on the base of the odd ones): k_plant_body_step in place of k_plant_step
    Each sample is a block of `--block` calls of bpmpc_plant_step on device tensors - a PD that holds the standing pose, `--substeps` substeps -
    that are only enqueued, with a host clock around the block and the one-robot bpmpc_plant_get_state that drains the plant's stream, divided by
    the block's length; the state is set back before every block.  A number here is the time per step of a stream that is kept busy, as a caller
    sees it, not a kernel time.  Per variant: the median, the minimum and the 5th / 95th percentile of `--samples` samples after `--warmup`.
    The probe reports the medians; it bounds nothing.
(b) The mass sweep.  The settle phase of tools/supervisor_settle_probe.py - H1 from standing_state, every robot in INIT under the reference's
    start-up gains (kp 80, kd 5), bpmpc_plant_step_supervised <- bpmpc_supervisor_update on the plant's rbd, kt = kn - with `--sweep-batch` robots
    whose every body is scaled by 0.1 ... 1.0, for `--settle-seconds`.  Per robot: the tick at which it became ready (null: never) and its base
    height at the end.  Recorded, not claimed: nothing asserts the outcome.
One JSON line per measurement on stdout; --out appends them to a file (profiles/plant_body_probe.jsonl is where the published one belongs).
Every measurement runs in a child process of its own under a time limit; the first that fails or runs out of time ends the probe.
usage (GPU box, repository root): python tools/plant_body_probe.py [--shapes h1:1,h1:256,h1:4096] [--parent-lib FILE] [--no-sweep] [--commit ID] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402
from tools.probekit import PERIOD, POS_TOL, RAMP_TIME, SETTLE_TIME, SUBSTEPS, VEL_TOL  # noqa: E402

SHAPES = "h1:1,h1:256,h1:4096"
PAYLOAD, PAYLOAD_POS = 10.0, (0.1, 0.0, 0.3)


def measure(robot, B, variant, parent_lib, samples, warmup, block, substeps, period):
    import numpy as np
    import bipedal_control_amd as bp
    if variant == "parent":
        pk.use_parent_library(parent_lib)
    itf, plant, r_dev, cmd = pk.standing_plant(robot, B)

    def steps():
        return pk.steps(plant, r_dev, cmd, samples, warmup, block, substeps, period)

    line = dict(probe="plant_body", robot=robot, batch=B, variant=variant, samples=samples, block=block, substeps=substeps, period=period,
                clock=pk.STEPS_CLOCK)
    line.update(pk.host_stats("step", steps(), "us"))
    if variant == "switched":
        base = bp.BodyParams.model(itf)
        pair = [base.scaled(0.8).row, base.payload(PAYLOAD, PAYLOAD_POS).row]
        plant.setBodyParams(np.array([pair[b % 2] for b in range(B)]))
        with_bodies = steps()
        finite = bool(np.isfinite(plant.get_state()).all())
        plant.resetBodyParams()
        line.update(pk.host_stats("step_bodies", with_bodies, "us"))
        line.update(bodies=dict(even="every body x 0.8", odd="%g kg at %s on the base" % (PAYLOAD, list(PAYLOAD_POS))),
                    body_extra_us=float(np.median(with_bodies) - line["step_us_median"]), bodies_state_finite=finite)
    line["state_finite"] = bool(np.isfinite(plant.get_state()).all())
    return line


def sweep(B, settle_seconds, kt):
    import numpy as np
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    from oracle import wbc_py as wp
    from tests import oracle_bridge as ob
    from tests.test_plant_reference import standing_state
    itf = sc.interface("h1")
    plant = bp.BatchedPlant(itf, max_batch=B)
    sup = bp.BatchedSupervisor(itf, max_batch=B)
    m = ob.model("h1")
    q, v, _ = standing_state(m, depth=0.0025)
    rbd0 = np.tile(wp.rbd_from(m, q, v), (B, 1))
    scales = np.linspace(0.1, 1.0, B)
    base = bp.BodyParams.model(itf)
    rows = [base.scaled(float(s)) for s in scales]
    if kt != "0":
        plant.setStiction(plant.getParams()[0] if kt == "kn" else float(kt))
    plant.setBodyParams(rows)
    sup.setParams(bp.SupervisorParams(ramp_time=RAMP_TIME, settle_pos_tol=POS_TOL, settle_vel_tol=VEL_TOL, settle_time=SETTLE_TIME).toRow())
    plant.set_state(rbd0)
    d_rbd = plant.outputs()["rbd"]

    def num(a):
        return [float(x) if np.isfinite(x) else None for x in a]

    ready_tick = [None] * B
    ticks = int(round(settle_seconds / PERIOD))
    lowest = np.full(B, np.inf)
    for k in range(ticks):
        sup.update(d_rbd, None, PERIOD)
        plant.step_supervised(sup, period=PERIOD, substeps=SUBSTEPS)
        s = sup.state(B)
        for b in range(B):
            if ready_tick[b] is None and s["ready"][b]:
                ready_tick[b] = k
        if k % 50 == 49 or k == ticks - 1:
            rbd = plant.get_state()
            lowest = np.where(np.isfinite(rbd[:, 5]), np.minimum(lowest, rbd[:, 5]), lowest)
    rbd = plant.get_state()
    nj = m["nj"]
    return dict(probe="plant_body_sweep", robot="h1", batch=B, init_gains="reference (kp 80, kd 5)", kt=float(plant.getStiction(0)), period=PERIOD, substeps=SUBSTEPS,
                ramp_time=RAMP_TIME, settle_pos_tol=POS_TOL, settle_vel_tol=VEL_TOL, settle_time=SETTLE_TIME, settle_seconds=settle_seconds,
                mass_scale=num(scales), total_mass=[r.total_mass for r in rows], start_base_height=num(rbd0[:, 5]), ready_tick=ready_tick,
                ready_at_end=[int(x) for x in s["ready"]], unsafe_at_end=[int(x) for x in s["unsafe"]], final_base_height=num(rbd[:, 5]),
                lowest_base_height_sampled=num(lowest), final_largest_joint_offset=num(np.abs(rbd[:, 6:6 + nj] - sup.getJointRows("q_init")).max(axis=1)),
                state_finite=[bool(np.all(np.isfinite(r))) for r in rbd])


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
    ap.add_argument("--no-steps", action="store_true", help="skip measurement (a)")
    ap.add_argument("--no-sweep", action="store_true", help="skip measurement (b)")
    ap.add_argument("--sweep-batch", type=int, default=16)
    ap.add_argument("--settle-seconds", type=float, default=2.0)
    ap.add_argument("--kt", default="kn", help="the plant's tangential contact stiffness in the sweep: 0, kn or a number")
    pk.driver_options(ap, limit=120)
    a = ap.parse_args()
    if a.child:      # one measurement, in this process
        if a.child == "sweep":
            return pk.child_line(a, sweep(a.sweep_batch, a.settle_seconds, a.kt))
        what, robot, B = a.child.split(":")
        return pk.child_line(a, measure(robot, int(B), what, a.parent_lib, a.samples, a.warmup, a.block, a.substeps, a.period))
    variants = (["parent"] if a.parent_lib else []) + ["untouched", "switched"]
    jobs = [] if a.no_steps else ["%s:%s" % (v, shape) for shape in a.shapes.split(",") for _ in range(a.repeats) for v in variants]
    jobs += [] if a.no_sweep else ["sweep"]
    return pk.run_jobs(__file__, jobs, pk.forwarded(a), a.limit, a.out)


if __name__ == "__main__":
    sys.exit(main())
