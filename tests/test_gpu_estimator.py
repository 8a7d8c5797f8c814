"""GPU tier: batched state estimation (include/bpmpc.h "State estimation"; BipedalController::updateStateEstimation, BipedalController.cpp:360-405)
against the numpy restatement tests/estimator_reference.py.  The reference declares the Kalman filter and does not implement it (its source
file is empty): the restatement follows the specification in include/bpmpc.h.
  one tick         H1, G1, Hunter, OpenLoong; all four modes from `mode` and from `contact`; random symmetric positive definite P and random x_hat
                   through set_state: x_hat, P, rbd, xy_reset
  sequences        64 robots x 400 ticks of 0.0025 s on H1 and G1, contact patterns switching every 0.3 s, half of the robots through `contact` and
                   half through `mode`: xy_reset identical at every robot and tick (the restatement's |det / 1e-6 - 1| >= 1e-8 everywhere, asserted
                   first), x_hat / rbd position and velocity / P to 1e-9 relative to max(1, |value|) - the project's tolerance of a fast kernel
                   against its reference kernel, some 450 x the spread between exact CPU solvers (2.2e-12 over 800 ticks) - and the angular and
                   joint parts of rbd to 1e-12
  from topic       1e-14 (atan2 / asin only), the clamp at a pitch near pi / 2 included
  isolation        masked reset and set_state: robots outside the mask bit-identical to a run without them, a reset robot = the same robot on a
                   fresh handle, a batch = its two halves on two handles
  parameters       rows read back and set again change no bit; a row per robot against the restatement with that robot's settings; device rows
                   and device masks are only enqueued and ordered before the next update
  tick_estimated   bit-identical to estimator.update followed by tick(rbd) on a twin, with host inputs and with device tensors; a 50-tick
                   closed loop with mode = the previous tick's planned_mode ends every tick with the wbc_status and safe of the same loop fed the
                   restatement's rbd
Every comparison prints its maximum before it asserts (pytest -s); no maxima are recorded here or in INTEGRATION.md yet."""
import shutil

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

from tests import estimator_reference as er
from tests import oracle_bridge as ob

pytestmark = pytest.mark.gpu
DT = 0.0025
TOL, TOL_ANGULAR, TOL_TOPIC = 1e-9, 1e-12, 1e-14
KEYS = ("joint_pos", "joint_vel", "quat", "angular_vel_local", "linear_accel_local")


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def _split(m, rbd):
    """(filter part, angular and joint part) of rbd rows"""
    nv = 6 + m["nj"]
    lin = np.r_[3:6, nv + 3:nv + 6]
    rest = np.setdiff1d(np.arange(2 * nv), lin)
    return rbd[..., lin], rbd[..., rest]


def _estimator(robot, B, kind="kalman", taskFile=None):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    return bp.BatchedStateEstimate(sc.interface(robot), kind=kind, taskFile=taskFile, max_batch=B)


def _update(est, s, rows=slice(None), source="mode", **kw):
    src = {"mode": s["mode"][rows]} if source == "mode" else {"contact": s["flags"][rows]}
    return est.update(*[s[k][rows] for k in KEYS], feet_heights=s["feet_heights"][rows], period=DT, **src, **kw)


def _ref_update(f, s, b):
    return f.update(s["joint_pos"][b], s["joint_vel"][b], s["quat"][b], s["angular_vel_local"][b], s["linear_accel_local"][b], s["flags"][b], DT,
                    s["feet_heights"][b])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("robot", ["h1", "g1", "hunter", "openloong"])
def test_one_tick_matches_restatement(robot):
    m = ob.model(robot)
    B = 16
    rng = np.random.default_rng(17)
    tr = er.SensorTrajectories(m, B, seed=5)
    s = tr.at(37)
    s["mode"] = np.array([0, 1, 2, 3] * 4, np.int32)
    s["flags"] = np.array([er.mode_flags(mo) for mo in s["mode"]], np.int32)
    x0 = rng.standard_normal((B, 18))
    P0 = np.zeros((B, 18, 18))
    for b in range(B):
        A = rng.standard_normal((18, 18))
        P0[b] = (A @ A.T + np.eye(18)) * (1e-5 if b >= 8 else 1.0)      # the second half stays below the xy reset's threshold
    worst = dict(x=0.0, P=0.0, lin=0.0, ang=0.0)
    for source in ("mode", "contact"):
        est = _estimator(robot, B)
        est.setState(x0, P0)
        gx, gP = est.getState(B)
        assert np.array_equal(gx, x0) and np.array_equal(gP, P0)
        rbd = _update(est, s, source=source)
        x, P = est.getState()
        xy = est.device_outputs()["xy_reset"].torch().cpu().numpy()
        for b in range(B):
            f = er.KalmanFilter(m)
            f.x, f.P = x0[b].copy(), P0[b].copy()
            r, fired, margin, cond = _ref_update(f, s, b)
            assert abs(margin - 1.0) >= 1e-8
            assert xy[b] == fired, (robot, source, b)
            lin, ang = _split(m, rbd[b])
            rl, ra = _split(m, r)
            worst = dict(x=max(worst["x"], _rel(x[b], f.x)), P=max(worst["P"], _rel(P[b], f.P)), lin=max(worst["lin"], _rel(lin, rl)),
                         ang=max(worst["ang"], _rel(ang, ra)))
            assert np.array_equal(P[b], P[b].T)
        assert set(xy.tolist()) == {0, 1}
    print("one tick", robot, worst)
    assert worst["x"] < TOL and worst["P"] < TOL and worst["lin"] < TOL and worst["ang"] < TOL_ANGULAR, worst


@pytest.mark.timeout(900)
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_sequences_match_restatement(robot):
    m = ob.model(robot)
    B, T, half = 64, 400, 32
    tr = er.SensorTrajectories(m, B, seed=2024)
    fs = [er.KalmanFilter(m) for _ in range(B)]
    # ---- the restatement alone first: the margin of the xy reset's threshold, everywhere
    ref_rbd, ref_xy, ref_x, ref_P = np.zeros((T, B, 2 * (6 + m["nj"]))), np.zeros((T, B), int), np.zeros((T, B, 18)), np.zeros((T, B, 18, 18))
    margin_min, cond_max, sensors = np.inf, 0.0, []
    for k in range(T):
        s = tr.at(k)
        sensors.append(s)
        for b in range(B):
            ref_rbd[k, b], ref_xy[k, b], margin, cond = _ref_update(fs[b], s, b)
            margin_min, cond_max = min(margin_min, abs(margin - 1.0)), max(cond_max, cond)
            ref_x[k, b], ref_P[k, b] = fs[b].x, fs[b].P
    print("sequence", robot, "smallest |det / 1e-6 - 1|", margin_min, "largest cond S", cond_max, "resets", int(ref_xy.sum()))
    assert margin_min >= 1e-8
    assert len({tuple(s["mode"]) for s in sensors}) >= 4 and {0, 1} == set(np.unique(np.array([s["flags"] for s in sensors])))
    # ---- the device: robots 0..31 report contact flags, robots 32..63 a mode number
    ec, em = _estimator(robot, half), _estimator(robot, half)
    worst = dict(x=0.0, P=0.0, lin=0.0, ang=0.0)
    for k in range(T):
        s = sensors[k]
        rbd = np.vstack([_update(ec, s, slice(0, half), "contact"), _update(em, s, slice(half, B), "mode")])
        xy = np.concatenate([e.device_outputs()["xy_reset"].torch().cpu().numpy() for e in (ec, em)])
        assert np.array_equal(xy, ref_xy[k]), (robot, k, np.nonzero(xy != ref_xy[k])[0])
        (xc, Pc), (xm, Pm) = ec.getState(), em.getState()
        x, P = np.vstack([xc, xm]), np.concatenate([Pc, Pm])
        lin, ang = _split(m, rbd)
        rl, ra = _split(m, ref_rbd[k])
        worst = dict(x=max(worst["x"], _rel(x, ref_x[k])), P=max(worst["P"], _rel(P, ref_P[k])), lin=max(worst["lin"], _rel(lin, rl)),
                     ang=max(worst["ang"], _rel(ang, ra)))
    print("sequence", robot, worst)
    assert worst["x"] < TOL and worst["P"] < TOL and worst["lin"] < TOL and worst["ang"] < TOL_ANGULAR, worst


@pytest.mark.timeout(300)
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_from_topic_matches_numpy(robot):
    m = ob.model(robot)
    nj = m["nj"]
    B = 12
    rng = np.random.default_rng(8)
    zyx = np.column_stack([rng.uniform(-3, 3, B), rng.uniform(-1.3, 1.3, B), rng.uniform(-3, 3, B)])
    zyx[0, 1], zyx[1, 1], zyx[2, 1] = np.pi / 2 - 1e-4, np.pi / 2 - 1e-7, -np.pi / 2 + 1e-4      # the first two beyond the clamp, the third not clamped
    quat = np.array([er.quat_from_zyx(z) for z in zyx])
    jp, jv = rng.standard_normal((B, nj)), rng.standard_normal((B, nj))
    pos, lin, ang = rng.standard_normal((B, 3)), rng.standard_normal((B, 3)), rng.standard_normal((B, 3))
    est = _estimator(robot, B, kind="from_topic")
    rbd = est.update(jp, jv, odom=(pos, quat, lin, ang))
    want = np.array([er.from_topic(m, jp[b], jv[b], pos[b], quat[b], lin[b], ang[b]) for b in range(B)])
    assert want[0, 1] == np.arcsin(.99999) and want[1, 1] == np.arcsin(.99999) and want[2, 1] < -1.57
    err = np.abs(rbd - want).max()
    print("from topic", robot, err)
    assert err < TOL_TOPIC
    nv = 6 + nj
    for cols in (slice(3, 6), slice(6, nv), slice(nv, 2 * nv)):         # what is passed through is passed through bit for bit
        assert np.array_equal(rbd[:, cols], want[:, cols])
    # the IMU members are not needed; the device tensors of the same inputs give the same bits
    dev = [torch.tensor(a, device="cuda") for a in (jp, jv, pos, quat, lin, ang)]
    torch.cuda.synchronize()
    assert est.update(dev[0], dev[1], odom=tuple(dev[2:]), fetch=False) is None
    assert np.array_equal(est.device_outputs()["rbd"].torch().cpu().numpy(), rbd)
    with pytest.raises(Exception):
        est.update(jp, jv)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_masked_reset_set_state_and_split_batches(robot):
    m = ob.model(robot)
    B, T, k_reset, k_set = 8, 100, 40, 70
    tr = er.SensorTrajectories(m, B, seed=77)
    mask = np.array([0, 1, 0, 0, 1, 1, 0, 0], np.int32)
    inside, outside = np.nonzero(mask)[0], np.nonzero(mask == 0)[0]
    rng = np.random.default_rng(3)
    xs = rng.standard_normal((B, 18))
    Ps = np.array([(lambda A: A @ A.T + np.eye(18))(rng.standard_normal((18, 18))) for _ in range(B)])
    plain, masked, lo, hi = _estimator(robot, B), _estimator(robot, B), _estimator(robot, B // 2), _estimator(robot, B // 2)
    fresh = stated = None
    for k in range(T):
        s = tr.at(k)
        if k == k_reset:
            masked.reset(mask)
            fresh = _estimator(robot, B)
        if k == k_set:
            masked.setState(xs, Ps, mask=mask)
            stated = _estimator(robot, B)
            stated.setState(xs, Ps)
        ra, rb = _update(plain, s), _update(masked, s)
        (xa, Pa), (xb, Pb) = plain.getState(), masked.getState()
        for a, b in ((ra, rb), (xa, xb), (Pa, Pb)):
            assert np.array_equal(a[outside], b[outside]), k
        if k < k_reset:
            assert np.array_equal(ra, rb)
        elif k < k_set:
            rf = _update(fresh, s)
            xf, Pf = fresh.getState()
            assert np.array_equal(rf[inside], rb[inside]) and np.array_equal(xf[inside], xb[inside]) and np.array_equal(Pf[inside], Pb[inside]), k
            assert not np.array_equal(ra[inside], rb[inside])
        else:
            rs = _update(stated, s)
            xs2, Ps2 = stated.getState()
            assert np.array_equal(rs[inside], rb[inside]) and np.array_equal(xs2[inside], xb[inside]) and np.array_equal(Ps2[inside], Pb[inside]), k
        # the batch as two halves on two handles
        rl, rh = _update(lo, s, slice(0, B // 2)), _update(hi, s, slice(B // 2, B))
        assert np.array_equal(np.vstack([rl, rh]), ra), k
        assert np.array_equal(np.concatenate([lo.getState()[1], hi.getState()[1]]), Pa), k
    # set_state without a covariance keeps P
    P_before = masked.getState()[1]
    masked.setState(xs, mask=mask)
    x_after, P_after = masked.getState()
    assert np.array_equal(P_after, P_before) and np.array_equal(x_after[inside], xs[inside])
    # a full reset is create's state
    masked.reset()
    x, P = masked.getState(B)
    assert not x.any() and np.array_equal(P, np.tile(100.0 * np.eye(18), (B, 1, 1)))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_parameter_rows(robot, tmp_path):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    m = ob.model(robot)
    B, T = 8, 20
    tr = er.SensorTrajectories(m, B, seed=31)
    never, same, per_robot, on_device = (_estimator(robot, B) for _ in range(4))
    d = never.getParams(-1)
    assert np.array_equal(d, er.DEFAULT_ROW)
    for b in range(B):
        assert np.array_equal(never.getParams(b), d)
    same.setParams(np.tile(d, (B, 1)))
    same.setParams(d, mask=np.arange(B) % 2 == 0)
    rng = np.random.default_rng(12)
    rows = np.tile(d, (B, 1)) * rng.uniform(0.3, 3.0, (B, 8))
    per_robot.setParams(rows)
    for b in range(B):
        assert np.array_equal(per_robot.getParams(b), rows[b])
    # device rows and a device mask: only enqueued, ordered before the next update
    dmask = torch.tensor(np.arange(B) % 2, dtype=torch.int32, device="cuda")
    drows = torch.tensor(rows, device="cuda")
    torch.cuda.synchronize()
    on_device.setParams(drows, mask=dmask)
    host_twin = _estimator(robot, B)
    host_twin.setParams(rows, mask=np.arange(B) % 2)
    fs = [er.KalmanFilter(m, rows[b]) for b in range(B)]
    worst = 0.0
    for k in range(T):
        s = tr.at(k)
        r0, r1, r2 = _update(never, s), _update(same, s), _update(per_robot, s)
        assert np.array_equal(r0, r1) and np.array_equal(never.getState()[1], same.getState()[1])
        assert np.array_equal(_update(on_device, s), _update(host_twin, s))
        x, P = per_robot.getState()
        for b in range(B):
            r, fired, margin, _ = _ref_update(fs[b], s, b)
            assert abs(margin - 1.0) >= 1e-8
            worst = max(worst, _rel(r2[b], r), _rel(x[b], fs[b].x), _rel(P[b], fs[b].P))
    print("per-robot rows", robot, worst)
    assert worst < TOL
    assert not np.array_equal(r0, r2)
    # bad host rows are refused, named, and change nothing
    bad = rows.copy()
    bad[3, 5] = 0.0
    with pytest.raises(bp.BpmpcError, match="footSensorNoiseVelocity"):
        per_robot.setParams(bad)
    bad[3, 5] = np.nan
    with pytest.raises(bp.BpmpcError, match="not finite"):
        per_robot.setParams(bad)
    for b in range(B):
        assert np.array_equal(per_robot.getParams(b), rows[b])
    per_robot.resetParams()
    assert np.array_equal(per_robot.getParams(3), d)
    with pytest.raises(bp.BpmpcError):                        # more robots than the handle holds: BPMPC_ERR_CAPACITY
        per_robot.setParams(np.tile(d, (B + 1, 1)))
    # settings from a task.info with a kalmanFilter block; absent keys keep the defaults
    task = str(tmp_path / "task.info")
    shutil.copy(sc.ROBOTS[robot]["task"], task)
    with open(task, "a") as f:
        f.write("\nkalmanFilter\n{\n  footRadius 0.035\n  footSensorNoiseVelocity 0.25\n}\n")
    custom = _estimator(robot, 2, taskFile=task)
    assert list(custom.getParams(-1)) == [0.035, 0.02, 0.02, 0.002, 0.005, 0.25, 0.01, 0.0] and np.array_equal(custom.getParams(1), custom.getParams(-1))
    assert np.array_equal(_estimator(robot, 2, taskFile=sc.ROBOTS[robot]["task"]).getParams(0), d)


def _fleet(robot):
    from bipedal_control_amd import scenarios as sc
    from tests.test_gpu_restart import NB, NI, Handles, _lib
    itf = sc.interface(robot)
    H = NI * sc.DT
    x0 = sc.perturbed_initial_states(itf, NB)
    cmd = np.array([(0.2 + 0.05 * b, 0.02 * b, 0.0, 0.05 * (b % 3)) for b in range(NB)])
    return itf, H, x0, cmd, lambda: Handles(itf, _lib(sc, robot), H)


class _StandingSensors(er.SensorTrajectories):
    """SensorTrajectories about the joints of the fleet's start states, so that the tick's observation is a standing robot"""

    def __init__(self, m, x0, seed):
        super().__init__(m, len(x0), seed)
        self.q0 = np.array(x0[:, 12:], float)
        self.ja *= 0.2
        self.ea *= 0.3
        self.yaw0 *= 0.1


@pytest.mark.timeout(600)
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_tick_estimated_equals_update_then_tick(robot):
    from tests.test_gpu_restart import NB, TICK, _same_tick
    m = ob.model(robot)
    itf, H, x0, cmd, handles = _fleet(robot)
    a, b = handles(), handles()
    ea, eb = _estimator(robot, NB), _estimator(robot, NB)
    tr = _StandingSensors(m, x0, seed=9)
    for h in (a, b):
        h.cycle(0.0, x0, cmd, H, False)
    # a tick needs an estimate for every robot of its batch: refused before the first update and after an update of fewer robots
    import bipedal_control_amd as bp
    with pytest.raises(bp.BpmpcError, match="last update"):
        b.ctrl.tick_estimated(np.zeros(NB), eb)
    _update(eb, tr.at(0), slice(0, NB // 2))
    with pytest.raises(bp.BpmpcError, match="last update"):
        b.ctrl.tick_estimated(np.zeros(NB), eb)
    eb.reset()
    modes = set()
    for k in range(40):
        s = tr.at(k)
        t = np.full(NB, 0.004 + DT * k)
        device = k % 2 == 1
        if not device:
            rbd = _update(ea, s)                               # synchronises; the plain tick then reads the estimator's buffer
            td = torch.tensor(t, device="cuda")
            torch.cuda.synchronize()
            oa = a.ctrl.tick(td, ea.device_outputs()["rbd"].torch())
            assert _update(eb, s, fetch=False) is None          # host arrays, only enqueued
            ob_ = b.ctrl.tick_estimated(t, eb)
        else:
            dev = {key: torch.tensor(s[key], device="cuda") for key in KEYS + ("feet_heights",)}
            dmode = torch.tensor(s["mode"], dtype=torch.int32, device="cuda")
            td = torch.tensor(t, device="cuda")
            torch.cuda.synchronize()
            rbd = ea.update(*[dev[key] for key in KEYS], mode=dmode, feet_heights=dev["feet_heights"], period=DT, fetch=False)
            load = ea.getState()                                # synchronises the estimator's stream for the plain tick
            oa = a.ctrl.tick(td, ea.device_outputs()["rbd"].torch())
            eb.update(*[dev[key] for key in KEYS], mode=dmode, feet_heights=dev["feet_heights"], period=DT, fetch=False)
            ob_ = b.ctrl.tick_estimated(td, eb)
            del load
        _same_tick(oa, ob_, range(NB))
        assert np.array_equal(ea.device_outputs()["rbd"].torch().cpu().numpy(), eb.device_outputs()["rbd"].torch().cpu().numpy())
        modes |= set(oa["planned_mode"].tolist())
        if k % 8 == 7:
            for h in (a, b):
                h.cycle(0.004 + DT * k, None, cmd, H, True)
    assert np.all(oa["safe"] == 1) and len(modes) >= 2


@pytest.mark.timeout(900)
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_closed_loop_with_planned_mode(robot):
    """50 ticks: setup_gaits(x0 = NULL), run, tick_estimated with mode = the previous tick's planned_mode (a device tensor: nothing is
    synchronised by hand), against the same loop ticked with the restatement's rbd."""
    from tests.test_gpu_restart import NB
    m = ob.model(robot)
    itf, H, x0, cmd, handles = _fleet(robot)
    dev, host = handles(), handles()
    est = _estimator(robot, NB)
    fs = [er.KalmanFilter(m) for _ in range(NB)]
    tr = _StandingSensors(m, x0, seed=21)
    for h in (dev, host):
        h.cycle(0.0, x0, cmd, H, False)
    mode_host = np.full(NB, 3)
    worst = 0.0
    for k in range(50):
        s = tr.at(k)
        t = np.full(NB, 0.004 + DT * k)
        est.update(*[s[key] for key in KEYS], feet_heights=s["feet_heights"], period=DT, mode=mode_host.astype(np.int32), fetch=False)
        od = dev.ctrl.tick_estimated(t, est)
        s["flags"] = np.array([er.mode_flags(mo) for mo in mode_host], np.int32)
        rbd = np.array([_ref_update(fs[b], s, b)[0] for b in range(NB)])
        oh = host.ctrl.tick(t, rbd)
        worst = max(worst, _rel(est.device_outputs()["rbd"].torch().cpu().numpy(), rbd))
        assert np.array_equal(od["wbc_status"], oh["wbc_status"]) and np.array_equal(od["safe"], oh["safe"]), k
        assert np.array_equal(od["planned_mode"], oh["planned_mode"]), k
        mode_host = od["planned_mode"].copy()
        if k % 10 == 9:
            for h in (dev, host):
                h.cycle(0.004 + DT * k, None, cmd, H, True)
    print("closed loop", robot, "rbd against the restatement", worst)
    assert worst < TOL
    # the same with the device output itself as the mode: enqueued only, ordered by the two handles' events
    planned = dev.ctrl.device_outputs()["planned_mode"].torch()
    s = tr.at(50)
    tensors = [torch.tensor(s[key], device="cuda") for key in KEYS]
    torch.cuda.synchronize()
    est.update(*tensors, mode=planned, period=DT, fetch=False)
    od = dev.ctrl.tick_estimated(np.full(NB, 0.004 + DT * 50), est)
    assert np.all(np.isfinite(od["joint_cmd"]))


def test_kernels_exist_without_scratch():
    from tests.test_kernel_resources import _kernels
    found = {n.split("(")[0]: scratch for n, scratch, vgpr, lds in _kernels() if n.startswith("k_estimate<")}
    assert found == {"k_estimate<10>": 0, "k_estimate<12>": 0}, found


@pytest.mark.timeout(120)
def test_refusals_on_a_live_handle():
    import bipedal_control_amd as bp
    est = _estimator("h1", 4)
    z = lambda *s: np.zeros(s)      # noqa: E731
    q = np.tile([0.0, 0.0, 0.0, 1.0], (5, 1))
    with pytest.raises(ValueError):                           # the mirror's check
        est.update(z(5, 10), z(5, 10), q, z(5, 3), z(5, 3), mode=z(5))
    lib = bp.load_library()
    import ctypes as C
    from bipedal_control_amd.api import _SensorInputs, _d, _i
    arrs = dict(jp=z(5, 10), jv=z(5, 10), q=q, w=z(5, 3), a=z(5, 3), mode=np.full(5, 3, np.int32), contact=np.ones((5, 4), np.int32))
    base = dict(joint_pos=_d(arrs["jp"]), joint_vel=_d(arrs["jv"]), quat=_d(arrs["q"]), angular_vel_local=_d(arrs["w"]), linear_accel_local=_d(arrs["a"]))
    rbd = z(5, 32)
    call = lambda batch, **kw: lib.bpmpc_estimator_update(est._h, batch, C.byref(_SensorInputs(**dict(base, **kw))), 0, DT, _d(rbd))      # noqa: E731
    assert call(4) == -1 and b"no contact source" in lib.bpmpc_last_error()
    assert call(4, mode=_i(arrs["mode"]), contact=_i(arrs["contact"])) == -1 and b"two contact sources" in lib.bpmpc_last_error()
    assert call(5, mode=_i(arrs["mode"])) == -6                                       # BPMPC_ERR_CAPACITY
    assert call(4, mode=_i(arrs["mode"]), quat=None) == -1 and b"null" in lib.bpmpc_last_error()
    arrs["mode"][2] = 4
    assert call(4, mode=_i(arrs["mode"])) == -1 and b"mode" in lib.bpmpc_last_error()
    arrs["mode"][2] = 3
    x_before = est.getState(4)
    assert call(4, mode=_i(arrs["mode"])) == 0
    assert not np.array_equal(est.getState(4)[1], x_before[1])
