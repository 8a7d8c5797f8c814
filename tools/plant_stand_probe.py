#!/usr/bin/env python3
"""Do the robots stand in the plant under the whole controller?  The loop of INTEGRATION.md "Plant" - bpmpc_plant_step_controlled ->
bpmpc_estimator_update_from_plant -> bpmpc_controller_tick_estimated, the MPC re-armed every 10 ticks - for H1, batch 8, 2 s of simulated time
(1000 ticks of 2 ms, 4 substeps), once with kt = 0 (the regularised Coulomb damper alone) and once with kt = kn (stick-slip contacts).

Per run and robot: the first tick with safe == 0 (null: none), the lowest base height, the base height at the end, and the largest drift of a
contact point in the ground plane from where it stood after the first tick (over the ticks the point was in contact).  A run ends at the first
tick after which a robot's state is not finite (ticks_run, state_finite; that robot's final height is null).  A probe, not a test: nothing asserts
its outcome.  Each run is a child process of its own under a time limit (--limit seconds); a run that fails or runs out of time
ends the probe.  One JSON line per run on stdout; --out appends them to a file (profiles/plant_stand_probe.jsonl is where the published one
belongs).
--telemetry RING_LEN attaches a tracking-telemetry handle (BatchedTelemetry) with a ring of RING_LEN samples to the controller after the first
tick and appends, per run, one line to --telemetry-out (profiles/plant_stand_telemetry.jsonl): the statistics of all robots and the ring of the
first robot that froze (it went unsafe or its state stopped being finite), otherwise of the robot with the largest joint error.
--cmd-delay SECONDS runs the same scenario under the plant's input model with that command latency on every robot (InputParams.delay; 0.009 is
the reference's gazebo/delay for H1); the line records it as cmd_delay and the control steps it came to as cmd_delay_steps.
--joint-preset mjcf gives every robot the joint rows of JointParams.reference_mjcf (armature 0.1, damping 1: the <default> of the reference's H1
MJCF); --joint-limits urdf adds the model's <limit> as end stops (the committed models carry none, so it changes nothing for them).  With either
the plant steps in k_plant_joint_step; the line records both and the largest distance a joint went beyond a finite limit.
usage (GPU box, repository root): python tools/plant_stand_probe.py [--seconds 2.0] [--batch 8] [--cmd-delay SECONDS] [--joint-preset {none,mjcf}] [--joint-limits {none,urdf}] [--telemetry RING_LEN [--telemetry-every N]] [--commit ID] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import probekit as pk      # noqa: E402

PERIOD, SUBSTEPS, REARM, NI = 0.002, 4, 10, 20


def run(kt, B, seconds, ring_len=None, every=1, cmd_delay=0.0, joint_preset="none", joint_limits="none"):
    import numpy as np
    import torch
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    from oracle import wbc_py as wp
    from tests import oracle_bridge as ob
    from tests.test_plant_reference import standing_state
    itf = sc.interface("h1")
    horizon = NI * sc.DT
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=sc.max_nodes_for(NI, horizon), return_gains=True)
    wbc = bp.WeightedWbc(itf, max_batch=B)
    ctrl = bp.BatchedController(mpc, wbc)
    est = bp.BatchedStateEstimate(itf, kind="from_topic", max_batch=B)
    plant = bp.BatchedPlant(itf, max_batch=B)
    gaits = [bp.loadModeSequenceTemplate(sc.ROBOTS["h1"]["gait"], "stance")]
    m = ob.model("h1")
    nj = m["nj"]
    q, v, _ = standing_state(m, depth=0.0025)
    rng = np.random.default_rng(5)
    rbd0 = np.array([wp.rbd_from(m, q + 0.002 * rng.standard_normal(len(q)) * np.r_[np.zeros(6), np.ones(len(q) - 6)], v) for _ in range(B)])
    x0 = np.tile(itf.getInitialState(), (B, 1))
    x0[:, 6:] = np.c_[rbd0[:, 3:6], rbd0[:, 0:3], rbd0[:, 6:6 + nj]]
    ctrl.setJointGains(np.full(nj, bp.WbcParams.RECONFIGURE_MOTOR_KP), np.full(nj, bp.WbcParams.RECONFIGURE_MOTOR_KD))
    kn = plant.getParams()[0]
    if kt != "0":      # kt = 0: a handle that never hears of stiction
        plant.setStiction(kn if kt == "kn" else float(kt))
    if cmd_delay > 0.0:      # no delay: a handle that never hears of the input model
        plant.setInputParams(bp.InputParams(delay=cmd_delay).toRow())
    lower, upper = np.full(nj, -np.inf), np.full(nj, np.inf)
    if joint_preset != "none" or joint_limits != "none":      # neither: a handle that never hears of the joint model
        row = bp.JointParams.reference_mjcf(nj) if joint_preset == "mjcf" else bp.JointParams.neutral(nj)
        if joint_limits == "urdf":
            lower, upper = np.array(itf.get("joint_lower"), float), np.array(itf.get("joint_upper"), float)
            row.lower, row.upper = lower, upper
        plant.setJointParams(row.toRow())
    beyond = np.zeros(B)
    plant.set_state(rbd0)

    def arm(t, first):
        mpc.setup_commands(t, x0 if first else None, gaits, -1, 0.0, np.zeros(4), horizon=horizon, from_previous=not first)
        mpc.enqueue()

    def points(rbd):
        out = []
        for b in range(B):
            qb, _ = wp.measured_state(m, rbd[b])
            R, o, _ = wp.fk(m, qb)
            out.append(np.array(wp.contact_points(m, R, o))[:, :2])
        return np.array(out)

    def num(a):
        """a list of floats; null for a value that is not finite"""
        return [float(x) if np.isfinite(x) else None for x in a]

    ticks = int(round(seconds / PERIOD))
    arm(0.0, True)
    torch.cuda.synchronize()
    ctrl.tick(torch.zeros(B, dtype=torch.float64, device="cuda"), plant.outputs()["rbd"].torch(), period=PERIOD, fetch=False)
    tel = None
    if ring_len is not None:
        tel = bp.BatchedTelemetry(itf, B, ring_len=ring_len)
        tel.configure(every=every)
        ctrl.attachTelemetry(tel)
    first_unsafe = [None] * B
    lowest = np.full(B, np.inf)
    drift = np.zeros(B)
    start, finite = None, True
    for k in range(ticks):
        plant.step_controlled(ctrl, period=PERIOD, substeps=SUBSTEPS)
        est.update_from_plant(plant, period=PERIOD, fetch=False)
        t = torch.full((B,), PERIOD * (k + 1), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()      # t is filled on torch's stream, which the handles' streams do not wait for
        ctrl.tick_estimated(t, est, period=PERIOD, fetch=False)
        if k % REARM == REARM - 1:
            arm(PERIOD * (k + 1), False)
        torch.cuda.synchronize()
        rbd = plant.get_state()
        safe = ctrl.device_outputs()["safe"].torch().cpu().numpy()
        contact = plant.outputs()["contact"].torch().cpu().numpy()
        if not np.all(np.isfinite(rbd)):
            finite = False
            break
        p = points(rbd)
        start = p if start is None else start
        lowest = np.minimum(lowest, rbd[:, 5])
        beyond = np.maximum(beyond, np.maximum(rbd[:, 6:6 + nj] - upper, lower - rbd[:, 6:6 + nj]).max(axis=1).clip(min=0.0))
        moved = np.linalg.norm(p - start, axis=2) * (contact != 0)
        drift = np.maximum(drift, moved.max(axis=1))
        for b in range(B):
            if first_unsafe[b] is None and safe[b] == 0:
                first_unsafe[b] = k
    anchored = plant.anchors()[1]
    delayed = dict(cmd_delay=cmd_delay, cmd_delay_steps=[int(x) for x in plant.inputState()["delay_steps"]]) if cmd_delay > 0.0 else {}
    if joint_preset != "none" or joint_limits != "none":
        delayed.update(joint_preset=joint_preset, joint_limits=joint_limits, finite_limits=int(np.isfinite(lower).sum() + np.isfinite(upper).sum()),
                       largest_limit_excess=num(beyond))
    record = None
    if tel is not None:
        record = telemetry_record(tel, B, kt=float(plant.getStiction(0)), seconds=seconds, ticks_run=k + 1, period=PERIOD, every=every)
        ctrl.attachTelemetry(None)
    return record, dict(robot="h1", batch=B, seconds=seconds, ticks_run=k + 1, period=PERIOD, substeps=SUBSTEPS, rearm_every=REARM, kt=float(plant.getStiction(0)),
                state_finite=finite, first_unsafe_tick=first_unsafe, lowest_base_height=num(lowest), final_base_height=num(rbd[:, 5]),
                start_base_height=num(rbd0[:, 5]), largest_foot_drift=num(drift), anchored_at_end=[int(x) for x in anchored.sum(axis=1)], **delayed)


def telemetry_record(tel, B, **head):
    """The statistics of all robots and one robot's ring, oldest sample first, as plain lists (null for a value that is not finite)."""
    import numpy as np
    import bipedal_control_amd as bp

    def plain(a):
        a = np.asarray(a)
        return [plain(x) for x in a] if a.ndim else (int(a) if a.dtype.kind in "iu" else (float(a) if np.isfinite(a) else None))

    s = tel.stats(B)
    frozen = np.flatnonzero(s["frozen"])
    if len(frozen):
        robot, why = int(frozen[np.argmin(s["first_unsafe"][frozen])]), "the first robot that froze"
    else:
        robot, why = int(np.argmax(s["joint_max"].max(axis=1))), "no robot froze: the robot with the largest joint error"
    ring = tel.ring([robot], batch=B)
    n = int(ring["count"][0])
    fields = {k: plain(v[0, :n]) for k, v in ring.items() if k not in ("samples", "count")}
    return dict(head, robot="h1", batch=B, ring_len=tel.ring_len, groups=list(bp.TelemetrySample.GROUPS),
                stats={k: plain(v) for k, v in s.items() if k != "rows"}, ring_robot=robot, ring_choice=why, ring_count=n, ring=fields)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--telemetry", type=int, metavar="RING_LEN", help="attach a telemetry handle with a ring of RING_LEN samples and write its record")
    ap.add_argument("--telemetry-every", type=int, default=1, help="every how many ticks a sample goes into the ring")
    ap.add_argument("--telemetry-out", default=os.path.join(ROOT, "profiles", "plant_stand_telemetry.jsonl"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kts", default="0,kn")
    ap.add_argument("--cmd-delay", type=float, default=0.0, metavar="SECONDS", help="command latency of the plant's input model on every robot (0: none)")
    ap.add_argument("--joint-preset", choices=["none", "mjcf"], default="none", help="joint rows of every robot: ideal joints, or the reference's MJCF defaults")
    ap.add_argument("--joint-limits", choices=["none", "urdf"], default="none", help="end stops: none, or the model's <limit> tags")
    pk.driver_options(ap, limit=300)
    a = ap.parse_args()
    if a.child is not None:      # one run, in this process
        record, line = run(a.child, a.batch, a.seconds, a.telemetry, a.telemetry_every, a.cmd_delay, a.joint_preset, a.joint_limits)
        if record is not None:
            if a.commit:
                record["commit"] = a.commit
            os.makedirs(os.path.dirname(os.path.abspath(a.telemetry_out)), exist_ok=True)
            with open(a.telemetry_out, "a") as f:
                f.write(json.dumps(record) + "\n")
        return pk.child_line(a, line)
    return pk.run_jobs(__file__, a.kts.split(","), pk.forwarded(a), a.limit, a.out)


if __name__ == "__main__":
    sys.exit(main())
