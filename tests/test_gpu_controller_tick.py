"""GPU tier: the controller tick (BipedalController::update on the device, include/bpmpc.h "Controller tick") and MRT_BASE::evaluatePolicy
against the oracle's restatements:
  observation   [A(q) v / m, q] of oracle/wbc_py.py (centroidal_momentum_matrix, rbd_from)        1e-12 relative, four robots
  yaw unwrap    BipedalController.cpp:400-403 (tests/test_controller_tick.py unwrap)               exact
  safety flag   SafetyChecker.h:39-52 at 1.0471, pi/3, 1.0473                                      exact
  policy        time_segment / primal_solution_arrays / linear_controller_input / mode_at_time     x* 1e-13 absolute, u* 1e-13 relative to
                max(1, |u*|) (contact forces of some 100 N: 1e-13 absolute is two ulps there, and the two sides sum K x in different orders),
                modes exact
  WBC           the tick = evaluate_policy + bpmpc_wbc_update on a second handle with the same history: bit-identical; wbc_py.update 1e-8
  closed loop   setup_commands(x0 = NULL) after a tick starts from its observations, after a rollout from the rollout's end states."""
import math
import os

import numpy as np
import pytest

from oracle import reference_py as rp, wbc_py as wp
from tests import oracle_bridge as ob
from tests.test_controller_tick import unwrap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAITS = ["stance", "trot", "flying_trot"]
COMMANDS = [(0.3, 0.0), (-0.2, 0.2)]
NI = 40


def _solved(itf, gaits=GAITS, commands=COMMANDS, robot="h1"):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    prob = sc.gait_sweep_problem(itf, gaits, commands, n_intervals=NI)
    B = prob["x0"].shape[0]
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=sc.max_nodes_for(NI, prob["horizon"]), return_gains=True)
    t, x, u, K, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    return prob, mpc, (t, x, u, K, st)


def _rbd(m, x0, rng, speed=0.1, consistent_mode=None):
    """Measured states near the planned ones: q from the MPC state, random v (projected onto the stance constraints when asked)."""
    nv = 6 + m["nj"]
    q = np.array(x0[6:], float) + 0.01 * rng.standard_normal(nv)
    v = speed * rng.standard_normal(nv)
    if consistent_mode is not None:
        v = wp.consistent_measured_state(m, q, v, consistent_mode)
    return wp.rbd_from(m, q, v), q, v


def _observation(m, q, v):
    A, _ = wp.centroidal_momentum_matrix(m, np.asarray(q, float))
    return np.concatenate([A @ v / m["robot_mass"], q])


@pytest.mark.parametrize("robot", ["h1", "g1", "hunter", "openloong"])
def test_observation_matches_oracle(robot):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface(robot)
    m = ob.model(robot)
    prob, mpc, _ = _solved(itf, gaits=["trot"], commands=[(0.3, 0.0), (0.0, 0.1), (-0.2, 0.0)])
    B = prob["x0"].shape[0]
    ctrl = bp.BatchedController(mpc, bp.WeightedWbc(itf, max_batch=B))
    rng = np.random.default_rng(7)
    rbds, exp = [], []
    for b in range(B):
        nv = 6 + m["nj"]
        q = np.array(prob["x0"][b, 6:]) + 0.2 * rng.standard_normal(nv)
        q[3] = rng.uniform(-3.0, 3.0)                                # yaw anywhere: unwraps from 0 to itself (up to rounding)
        v = 0.8 * rng.standard_normal(nv)
        rbds.append(wp.rbd_from(m, q, v))
        exp.append(_observation(m, q, v))
    out = ctrl.tick(np.zeros(B), np.array(rbds))
    exp = np.array(exp)
    for b in range(B):
        err = np.abs(out["x_obs"][b] - exp[b]).max() / max(1.0, np.abs(exp[b]).max())
        assert err < 1e-12, (robot, b, err)
    assert np.array_equal(out["safe"], (np.abs(exp[:, 10:12]).max(axis=1) <= math.pi / 3).astype(np.int32))


def test_yaw_unwrap_and_safety_flag():
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface("h1")
    m = ob.model("h1")
    prob, mpc, _ = _solved(itf)
    B = prob["x0"].shape[0]
    assert B == 6
    ctrl = bp.BatchedController(mpc, bp.WeightedWbc(itf, max_batch=B))
    rng = np.random.default_rng(3)
    rbd = np.array([_rbd(m, prob["x0"][b], rng)[0] for b in range(B)])
    rbd[:, 0] = 3.10
    rbd[:, 1:3] = 0.0
    # roll / pitch at 1.0471, exactly pi/3 and 1.0473 (robots 0..2: pitch, 3..5: roll); rbd = [yaw, pitch, roll, ...]
    rbd[0, 1], rbd[1, 1], rbd[2, 1] = 1.0471, math.pi / 3, 1.0473
    rbd[3, 2], rbd[4, 2], rbd[5, 2] = 1.0471, math.pi / 3, 1.0473
    o1 = ctrl.tick(np.zeros(B), rbd)
    assert list(o1["safe"]) == [1, 1, 0, 1, 1, 0]
    y1 = unwrap(0.0, 3.10)                                           # from yaw_last = 0 (BipedalController::starting)
    assert np.all(o1["x_obs"][:, 9] == y1) and abs(y1 - 3.10) < 1e-15
    rbd2 = rbd.copy()
    rbd2[:, 0] = -3.10
    rbd2[:, 1:3] = 0.0
    rbd2[4, 1] = -1.0473                                             # only robot 4 tilts now
    o2 = ctrl.tick(np.full(B, 0.0025), rbd2)
    assert list(o2["safe"]) == [1, 1, 1, 1, 0, 1]
    assert np.all(o2["x_obs"][:, 9] == unwrap(y1, -3.10)) and abs(o2["x_obs"][0, 9] - 3.1832) < 1e-4
    o3 = ctrl.tick(np.full(B, 0.005), rbd2)                        # stays on the unwrapped branch
    assert np.all(o3["x_obs"][:, 9] == unwrap(unwrap(y1, -3.10), -3.10))
    ctrl.reset()
    o4 = ctrl.tick(np.full(B, 0.005), rbd2)                        # after reset the unwrap starts from 0 again
    assert np.all(o4["x_obs"][:, 9] == unwrap(0.0, -3.10))


def _policy_check(itf, mpc, prob, sol, feedback):
    t, x, u, K, st = sol
    B = prob["x0"].shape[0]
    rng = np.random.default_rng(1)
    refs = []
    for b in range(B):
        n = st[b].n_nodes
        nodes = ob.oracle_nodes(prob, b)
        assert nodes["N"] == n
        tp, xp, uff, KK = rp.primal_solution_arrays(nodes, x[b, :n + 1], u[b, :n], K[b, :n] if feedback else np.zeros_like(K[b, :n]))
        assert np.array_equal(tp, t[b, :n + 1])
        ev_nodes = [k for k in range(n) if nodes["kind"][k] == 1]
        sched = prob["schedule"][b]
        refs.append((tp, xp, uff, KK, ev_nodes, [float(e) for e in sched.eventTimes], [int(mm) for mm in sched.modeSequence]))
    queries = {
        "t0": lambda r: r[0][0],
        "mid-interval": lambda r: 0.5 * (r[0][3] + r[0][4]),
        "node": lambda r: r[0][7],
        "event": lambda r: r[0][r[4][0]] if r[4] else r[0][5],
        "before": lambda r: r[0][0] - 0.01,
        "after": lambda r: r[0][-1] + 0.01,
        "random": lambda r: rng.uniform(r[0][0], r[0][-1]),
    }
    events_seen = 0
    worst = 0.0
    for name, q in queries.items():
        tq = np.array([q(r) for r in refs])
        xq = prob["x0"] + 0.01 * rng.standard_normal(prob["x0"].shape)
        x_opt, u_opt, mode = mpc.evaluatePolicy(tq, xq)
        for b, (tp, xp, uff, KK, ev_nodes, ev, ms) in enumerate(refs):
            j, al = rp.time_segment(tp, tq[b])
            xs = al * xp[j] + (1.0 - al) * xp[j + 1]
            us = rp.linear_controller_input(tp, uff, KK, tq[b], xq[b])
            ex, eu = np.abs(x_opt[b] - xs).max(), np.abs(u_opt[b] - us).max() / max(1.0, np.abs(us).max())
            worst = max(worst, ex, eu)
            assert ex < 1e-13 and eu < 1e-13, (name, b, ex, eu)
            assert mode[b] == rp.mode_at_time(ev, ms, min(max(tq[b], tp[0]), tp[-1])), (name, b)
            events_seen += name == "event" and bool(ev_nodes)
    assert events_seen >= 4
    return worst


def test_policy_matches_oracle():
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface("h1")
    prob, mpc, sol = _solved(itf)
    _policy_check(itf, mpc, prob, sol, feedback=True)


def test_policy_without_feedback_matches_oracle(tmp_path):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    text = open(sc.H1["task"]).read()
    assert text.count("useFeedbackPolicy true") >= 1
    task = tmp_path / "task.info"
    # only the sqp block's flag (the first occurrence); the ddp block keeps its own
    task.write_text(text.replace("useFeedbackPolicy true", "useFeedbackPolicy false", 1))
    itf = bp.BipedalRobotInterface(str(task), sc.H1["urdf"], sc.H1["reference"])
    itf.gaitFile = sc.H1["gait"]
    assert itf.sqpSettings()["useFeedbackPolicy"] in (0, False)
    prob, mpc, sol = _solved(itf)
    _policy_check(itf, mpc, prob, sol, feedback=False)


def _tick_inputs(m, prob, rng, stance_bad=True):
    """Measured states: robots of the stance gait (0, 1) with an inconsistent velocity (their QP falls back, status 1), the others consistent."""
    B = prob["x0"].shape[0]
    out = []
    for b in range(B):
        bad = stance_bad and b < len(COMMANDS)
        out.append(_rbd(m, prob["x0"][b], rng, speed=0.3 if bad else 0.05, consistent_mode=None if bad else 3)[0])
    return np.array(out)


def test_tick_is_policy_then_wbc():
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface("h1")
    m = ob.model("h1")
    st = wp.load_settings(os.path.join(ROOT, "assets", "h1", "task.info"), m["nj"])
    prob, mpc, _ = _solved(itf)
    B = prob["x0"].shape[0]
    wbc, wbc2 = bp.WeightedWbc(itf, max_batch=8), bp.WeightedWbc(itf, max_batch=8)
    ctrl = bp.BatchedController(mpc, wbc)
    rng = np.random.default_rng(5)
    statuses = []
    for k in range(3):
        tq = np.full(B, 0.0025 * k)
        rbd = _tick_inputs(m, prob, rng)
        o = ctrl.tick(tq, rbd)
        x_opt, u_opt, mode = mpc.evaluatePolicy(tq, o["x_obs"])
        assert np.array_equal(x_opt, o["x_opt"]) and np.array_equal(u_opt, o["u_opt"]) and np.array_equal(mode, o["planned_mode"])
        sol, status = wbc2.update(x_opt, u_opt, rbd, mode)
        assert np.array_equal(sol, o["wbc_solution"]) and np.array_equal(status, o["wbc_status"]), k
        nj = m["nj"]
        assert np.array_equal(o["joint_cmd"][:, 0], x_opt[:, 12:]) and np.array_equal(o["joint_cmd"][:, 1], u_opt[:, 12:])
        assert np.array_equal(o["joint_cmd"][:, 2], sol[:, -nj:])
        statuses.append(status.copy())
        for b in (2, 4):
            so, p = wp.update(m, st, x_opt[b], u_opt[b], rbd[b], int(mode[b]))
            if p["status"] == 0 and status[b] == 0:
                assert np.abs(sol[b] - so).max() / max(1.0, np.abs(so).max()) < 1e-8, (k, b)
    statuses = np.array(statuses)
    assert statuses[:, :2].max() == 1 and statuses[:, 2:].min() == 0, statuses
    assert np.all(o["planned_mode"][:2] == 3)


def _closed_loop(itf, m, period=0.0025, ticks=4):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    B = 4
    horizon = NI * sc.DT
    tm = [bp.loadModeSequenceTemplate(sc.H1["gait"], g) for g in ("trot", "standing_trot")]
    gop = np.array([0, 1, 0, 1], np.int32)
    cmd = np.array([(0.3, 0, 0, 0.1), (0.2, 0, 0, 0.0), (-0.2, 0.05, 0, 0.0), (0.0, 0, 0, 0.3)], float)
    x0 = sc.perturbed_initial_states(itf, B)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=64, return_gains=True)
    ctrl = bp.BatchedController(mpc, bp.WeightedWbc(itf, max_batch=B))
    rng = np.random.default_rng(9)
    rec = []
    mpc.setup_commands(0.0, x0, tm, gop, sc.GAIT_START, cmd, horizon=horizon)
    mpc.enqueue()
    for k in range(ticks):
        rbd = np.array([_rbd(m, x0[b], rng, speed=0.05, consistent_mode=3)[0] for b in range(B)])
        rec.append(ctrl.tick(np.full(B, k * period), rbd))
    mpc.setup_commands(ticks * period, None, tm, gop, sc.GAIT_START, cmd, horizon=horizon, from_previous=True)
    rec.append({"x0": mpc.read("x0").reshape(B, -1).copy()})
    mpc.enqueue()
    _, x, u, _, _ = mpc.fetch()
    rec.append({"x": x, "u": u})
    xe1, _, _ = mpc.rollout(0.02)
    ctrl.tick(np.full(B, 0.02), rbd)
    xe2, _, _ = mpc.rollout(0.02)
    mpc.setup_commands(0.04, None, tm, gop, sc.GAIT_START, cmd, horizon=horizon, from_previous=True)
    rec.append({"x0_after_rollout": mpc.read("x0").reshape(B, -1).copy(), "xe2": xe2, "xe1": xe1})
    return rec


def test_closed_loop_through_the_tick():
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface("h1")
    m = ob.model("h1")
    rec = _closed_loop(itf, m)
    ticks = rec[:4]
    assert np.array_equal(rec[4]["x0"], ticks[-1]["x_obs"])               # the last tick's observations, bit for bit
    assert np.isfinite(rec[5]["x"]).all()
    assert np.array_equal(rec[6]["x0_after_rollout"], rec[6]["xe2"])       # rollout, tick, rollout: the rollout ran last
    rec2 = _closed_loop(itf, m)
    for a, b in zip(rec, rec2):
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_device_inputs_and_outputs():
    import torch
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface("h1")
    m = ob.model("h1")
    prob, mpc, _ = _solved(itf)
    B = prob["x0"].shape[0]
    wbc = bp.WeightedWbc(itf, max_batch=B)
    ctrl = bp.BatchedController(mpc, wbc)
    rbd = _tick_inputs(m, prob, np.random.default_rng(2))
    tq = np.full(B, 0.01)
    host = ctrl.tick(tq, rbd)
    ctrl.reset(); wbc.reset()
    t_dev = torch.tensor(tq, dtype=torch.float64, device="cuda")
    r_dev = torch.tensor(rbd, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = ctrl.tick(t_dev, r_dev)
    for k in host:
        assert np.array_equal(host[k], dev[k]), k
    ctrl.reset(); wbc.reset()
    assert ctrl.tick(t_dev, r_dev, fetch=False) is None                  # only enqueued
    views = ctrl.device_outputs()
    mpc.synchronize()
    for k, v in views.items():
        tv = v.torch()
        assert tv.device.type == "cuda" and tv.data_ptr() == v.ptr           # zero-copy
        assert np.array_equal(tv.cpu().numpy(), host[k]), k


def test_refusals():
    import ctypes as C
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface("h1")
    m = ob.model("h1")
    prob = sc.trot_problem(itf, batch=2, n_intervals=20)
    rbd = np.array([_rbd(m, prob["x0"][b], np.random.default_rng(b))[0] for b in range(2)])
    # DDP: the solution lives on the roll-out's time points
    ddp = bp.BatchedDdpMpc(itf, 2, 48)
    ddp.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    with pytest.raises(bp.BpmpcError) as ei:
        bp.BatchedController(ddp, bp.WeightedWbc(itf, max_batch=2)).tick(np.zeros(2), rbd)
    assert ei.value.status == -3
    with pytest.raises(bp.BpmpcError) as ei:
        ddp.evaluatePolicy(np.zeros(2), prob["x0"])
    assert ei.value.status == -3
    # before any run, after a setup without a run, batch mismatch
    mpc = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=32, return_gains=True)
    ctrl = bp.BatchedController(mpc, bp.WeightedWbc(itf, max_batch=4))
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    for call in (lambda: ctrl.tick(np.zeros(2), rbd), lambda: mpc.evaluatePolicy(np.zeros(2), prob["x0"])):
        with pytest.raises(bp.BpmpcError) as ei:
            call()
        assert ei.value.status == -1
    mpc.enqueue()
    assert ctrl.tick(np.zeros(2), rbd)["x_obs"].shape == (2, itf.stateDim)
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    with pytest.raises(bp.BpmpcError) as ei:
        ctrl.tick(np.zeros(2), rbd)
    assert ei.value.status == -1
    mpc.enqueue()
    lib = bp.load_library()
    d = np.zeros(4 * 2 * 16)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.bpmpc_controller_tick(ctrl._h, 1, dp, dp, 0, 0.0025, None) == -1
    assert lib.bpmpc_controller_tick(ctrl._h, 3, dp, dp, 0, 0.0025, None) == -1
    ip = np.zeros(4, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    assert lib.bpmpc_solver_evaluate_policy(mpc._h, 3, dp, dp, dp, dp, ip) == -1
