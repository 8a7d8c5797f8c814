"""GPU tier of the supervisor (include/bpmpc.h "Supervisor"; csrc/supervisor.hip, csrc/kernels/supervisor.h) against the numpy restatement
tests/supervisor_reference.py.

  the episode    12 updates with requests in between: the ramp, the settle test holding and breaking, request(RUN) with only_ready both ways and
                 with a device mask, a tilt, a command that is not finite, a missing command, request(INIT) with a joint that is not a number at
                 the latch, request(STOPPED), a base below the height limit.  H1 batch 5 in a handle of 8 (the last wavefront holds one robot of
                 four; robots 5..7 keep their bits), G1 batch 3, batch 1.  Integers, clocks, counts and the RUN / STOPPED commands compare
                 exactly; INIT pos_des exactly outside the ramp and within 8 eps max(1, |q_latch|, |q_init|) inside it (one division and one
                 multiply-add that a compiler may fuse, each at most one ulp, with margin).
  host / device  the same episode from host arrays and from device tensors: the same bits
  pass-through   H1 batch 4, every robot in RUN: 10 ticks of step_supervised + update_controlled against step_controlled, bit for bit
  stop           one robot of four is shown a roll of pi / 3 + 0.01 at tick 3: STOPPED with cause 1 and the stop command from that update on,
                 the others bit for bit as without the tilt
  settle         H1 batch 4 in the plant from standing_state under INIT: the flags are the restatement's on the kernel's own measurements
  refusals       what needs a handle to be refused, with the entry named
"""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

from tests import supervisor_reference as sr

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = -1, -6
EPS = np.finfo(float).eps
PERIOD = 0.002
INTS = ("state", "cause", "unsafe", "ready")
COUNTS = ("init", "run", "stopped", "ready", "unsafe")


def _itf(robot):
    from bipedal_control_amd import scenarios as sc
    return sc.interface(robot)


def _dev(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _all_rows(sup):
    """every per-robot buffer of the handle over max_batch, as numpy"""
    torch.cuda.synchronize()
    return {k: v.torch().cpu().numpy().copy() for k, v in sup.outputs().items()}


class Episode:
    """The handle and the restatement side by side.  After a prologue that fills every row of the handle - one update over max_batch robots,
    then request(INIT) for all of them - the episode runs over `batch` robots."""

    def __init__(self, robot, batch, max_batch, device):
        import bipedal_control_amd as bp
        self.itf = itf = _itf(robot)
        self.nj = nj = itf.actuatedDofNum
        self.nv = 6 + nj
        self.B, self.M, self.device = batch, max_batch, device
        self.sup = bp.BatchedSupervisor(itf, max_batch)
        self.q0 = np.array(itf.get("default_joint_state"))
        self.ref = sr.Supervisor(max_batch, nj, self.q0)
        self.rng = np.random.default_rng(100 * batch + nj)
        assert np.array_equal(self.sup.getParams(), sr.DEFAULT_PARAMS) and np.array_equal(self.sup.getJointRows("q_init"), self.q0)
        assert np.array_equal(self.sup.getJointRows("kp_init", 0), self.ref.rows["kp_init"][0]) and np.array_equal(self.sup.getJointRows(2), self.ref.rows["kd_init"][0])
        assert np.all(np.isneginf(self.sup.getJointRows("lower"))) and np.all(np.isposinf(self.sup.getJointRows("upper", max_batch - 1)))
        first = self.sup.state(max_batch)
        assert not first["state"].any() and not first["ready"].any() and not first["elapsed"].any() and first["counts"]["init"] == 0
        # per-robot rows: the ramp of robot b is 0.006, 0 or 0.005 s; limits that bite for the odd joints of the odd robots
        rows = np.tile(bp.SupervisorParams(min_base_height=0.5, settle_pos_tol=0.3, settle_vel_tol=2.0, settle_time=0.004, stop_kd=1.5).toRow(), (max_batch, 1))
        rows[:, sr.RAMP_TIME] = np.array([0.006, 0.0, 0.005])[np.arange(max_batch) % 3]
        lower, upper = np.full((max_batch, nj), -np.inf), np.full((max_batch, nj), np.inf)
        lower[1::2, 1::2] = self.q0[1::2] + 0.01
        upper[1::2, 0::2] = self.q0[0::2] - 0.02
        kp = np.tile(np.linspace(60.0, 90.0, nj), (max_batch, 1)) + np.arange(max_batch)[:, None]
        if device:
            torch.cuda.synchronize()
            self.sup.setParams(_dev(rows))
            self.sup.setJointRows("lower", _dev(lower))
            self.sup.setJointRows("upper", _dev(upper))
            self.sup.setJointRows("kp_init", _dev(kp))
        else:
            self.sup.setParams(rows)
            self.sup.setJointRows("lower", lower)
            self.sup.setJointRows("upper", upper)
            self.sup.setJointRows("kp_init", kp)
        self.ref.params[:], self.ref.rows["lower"][:], self.ref.rows["upper"][:], self.ref.rows["kp_init"][:] = rows, lower, upper, kp
        assert np.array_equal(self.sup.getParams(max_batch - 1), rows[-1]) and np.array_equal(self.sup.getJointRows("upper", 1 % max_batch), upper[1 % max_batch])
        self.update(self.measurement(max_batch), None)
        self.request(sr.INIT, None)
        self.untouched = _all_rows(self.sup)

    def measurement(self, B, spread=0.1, speed=0.5):
        rbd = np.zeros((B, 2 * self.nv))
        rbd[:, 0] = self.rng.uniform(-3.0, 3.0, B)
        rbd[:, 1:3] = self.rng.uniform(-0.3, 0.3, (B, 2))
        rbd[:, 3:5], rbd[:, 5] = self.rng.uniform(-2.0, 2.0, (B, 2)), self.rng.uniform(0.6, 1.1, B)
        rbd[:, 6:self.nv] = self.q0 + self.rng.uniform(-spread, spread, (B, self.nj))
        rbd[:, self.nv:] = speed * self.rng.standard_normal((B, self.nv))
        return rbd

    def command(self):
        return [self.rng.standard_normal((self.B, self.nj)) for _ in range(5)]

    def update(self, rbd, cmd):
        if self.device:
            d_rbd, d_cmd = _dev(rbd), None if cmd is None else [_dev(a) for a in cmd]
            torch.cuda.synchronize()
            self.sup.update(d_rbd, d_cmd, PERIOD)
        else:
            self.sup.update(rbd, cmd, PERIOD)
        self.ref.update(rbd, cmd, PERIOD)

    def request(self, target, mask, only_ready=False, device_mask=False):
        if mask is not None and device_mask:
            d_mask = _dev(mask, torch.int32)
            torch.cuda.synchronize()
            self.sup.request(target, d_mask, only_ready)
        else:
            self.sup.request(target, None if mask is None else np.asarray(mask, np.int32), only_ready)
        self.ref.request(target, mask, only_ready, batch=None if mask is None else len(mask))

    def compare(self, tag):
        B, ref = self.B, self.ref
        got = self.sup.state(B, commands=True)
        for k in INTS:
            assert got[k].tolist() == getattr(ref, k)[:B].tolist(), (tag, k, got[k], getattr(ref, k)[:B])
        assert np.array_equal(got["elapsed"], ref.elapsed[:B]), (tag, "elapsed")
        assert [got["counts"][k] for k in COUNTS] == ref.counts[:5].tolist(), (tag, got["counts"], ref.counts)
        for b in range(B):
            p = ref.params[b]
            ramping = ref.state[b] == sr.INIT and not (p[sr.RAMP_TIME] == 0 or ref.elapsed[b] >= p[sr.RAMP_TIME])
            for k in sr.COMMAND_ROWS:
                if k == "pos_des" and ramping:
                    bound = 8 * EPS * np.maximum(1.0, np.maximum(np.abs(ref.q_latch[b]), np.abs(ref.rows["q_init"][b])))
                    assert np.all(np.abs(got[k][b] - ref.cmd[k][b]) <= bound), (tag, b, k)
                else:
                    assert np.array_equal(got[k][b], ref.cmd[k][b], equal_nan=True), (tag, b, k, got[k][b], ref.cmd[k][b])
        return got


def run_episode(robot, batch, max_batch, device=False):
    """the twelve updates of the module docstring; returns the handle's state after each"""
    e = Episode(robot, batch, max_batch, device)
    B, nj, nv = batch, e.nj, e.nv
    one = lambda *robots: [1 if b in robots else 0 for b in range(B)]      # noqa: E731
    every = [1] * B
    seen, log = set(), []

    def step(k, rbd, cmd):
        e.update(rbd, cmd)
        log.append(e.compare((robot, batch, k)))
        seen.update(e.ref.state[:B].tolist())

    def ask(*args, **kw):
        e.request(*args, **kw)
        seen.update(e.ref.state[:B].tolist())

    near = lambda: e.measurement(B, spread=0.005, speed=0.05)             # noqa: E731
    step(0, e.measurement(B, spread=0.4), None)                              # latch; robots with a ramp start it
    step(1, near(), None)
    step(2, near(), None)                                                    # the ramps end; the clamped joints of the odd robots stay off q
    step(3, near(), None)
    rbd = near()
    rbd[B - 1, nv + 6 + 3] = 2.5                                             # one joint velocity leaves the tolerance: ready drops for the last robot
    step(4, rbd, None)
    step(5, near(), None)
    assert e.ref.ready[:B].any() or B == 1, "the episode is meant to have ready robots"
    ready = e.ref.ready[:B].copy()
    ask(sr.RUN, every, only_ready=True)                                # exactly the ready robots
    assert e.ref.state[:B].tolist() == [sr.RUN if r else sr.INIT for r in ready]
    step(6, near(), e.command())
    ask(sr.RUN, one(B - 1, 1 % B), only_ready=False, device_mask=True)    # robots that are not ready, by a device mask
    assert e.ref.state[B - 1] == sr.RUN
    rbd, cmd = near(), e.command()
    rbd[0, 2] = np.pi / 3 + 0.01                                             # robot 0 tilts
    if B > 2:
        cmd[2][2, nj - 1] = np.nan                                           # robot 2's command is not finite
    step(7, rbd, cmd)
    assert e.ref.state[0] == sr.STOPPED and e.ref.cause[0] in (sr.ROLL, sr.ROLL | sr.COMMAND)
    step(8, near(), e.command())
    ask(sr.INIT, one(0))
    if B > 1:
        ask(sr.STOPPED, one(1))
    rbd = near()
    rbd[0, 6 + 4] = np.nan                                                   # not a number at the latch: q_init takes its place, bit 8
    step(9, rbd, e.command())
    assert e.ref.unsafe[0] & sr.MEASUREMENT and e.ref.state[0] == sr.INIT and (B == 1 or e.ref.cause[1] == sr.REQUEST)
    step(10, near(), None)                                                   # no command: every robot still in RUN stops with cause 16
    assert sr.RUN not in e.ref.state[:B].tolist()
    rbd = near()
    rbd[:, 5] = 0.45                                                         # below min_base_height
    step(11, rbd, None)
    assert np.all(e.ref.unsafe[:B] & sr.HEIGHT) and seen == {sr.INIT, sr.RUN, sr.STOPPED} and len(log) == 12
    after = _all_rows(e.sup)
    for k, a in after.items():
        if k != "counts":
            assert np.array_equal(a[B:], e.untouched[k][B:], equal_nan=True), (robot, batch, k)      # robots at or beyond batch: not one bit
    return log


@pytest.mark.parametrize("robot,batch,max_batch", [("h1", 5, 8), ("g1", 3, 3), ("h1", 1, 1)])
def test_episode_against_the_restatement(robot, batch, max_batch):
    run_episode(robot, batch, max_batch)


def test_host_arrays_and_device_pointers_give_the_same_bits():
    host = run_episode("h1", 5, 8, device=False)
    dev = run_episode("h1", 5, 8, device=True)
    for k, (a, b) in enumerate(zip(host, dev)):
        assert a["counts"] == b["counts"], k
        for key in INTS + ("elapsed",) + sr.COMMAND_ROWS:
            assert np.array_equal(a[key], b[key], equal_nan=True), (k, key)


# ---------------------------------------------------------------------------------------------------------------- the closed loop
NB, NI = 4, 20
TICK_KEYS = ("x_obs", "x_opt", "u_opt", "joint_cmd", "wbc_solution", "planned_mode", "wbc_status", "safe", "joint_torque")


class Loop:
    """plant -> estimator -> tick -> solver for four H1 robots from standing_state (the loop of tests/test_gpu_plant.py at batch 4)"""

    def __init__(self):
        import bipedal_control_amd as bp
        from bipedal_control_amd import scenarios as sc
        from oracle import wbc_py as wp
        from tests import oracle_bridge as ob
        from tests.test_plant_reference import standing_state
        self.itf = itf = sc.interface("h1")
        self.H = NI * sc.DT
        self.mpc = bp.BatchedSqpMpc(itf, max_batch=NB, max_nodes=sc.max_nodes_for(NI, self.H), return_gains=True)
        self.wbc = bp.WeightedWbc(itf, max_batch=NB)
        self.ctrl = bp.BatchedController(self.mpc, self.wbc)
        self.est = bp.BatchedStateEstimate(itf, kind="from_topic", max_batch=NB)
        self.plant = bp.BatchedPlant(itf, max_batch=NB)
        self.sup = bp.BatchedSupervisor(itf, max_batch=NB)
        self.gaits = [bp.loadModeSequenceTemplate(sc.ROBOTS["h1"]["gait"], "stance")]
        m = ob.model("h1")
        self.nj = m["nj"]
        q, v, self.hold = standing_state(m, depth=0.0025)
        rng = np.random.default_rng(5)
        self.rbd0 = np.array([wp.rbd_from(m, q + 0.002 * rng.standard_normal(len(q)) * np.r_[np.zeros(6), np.ones(len(q) - 6)], v) for _ in range(NB)])
        self.x0 = np.tile(itf.getInitialState(), (NB, 1))
        self.x0[:, 6:] = np.c_[self.rbd0[:, 3:6], self.rbd0[:, 0:3], self.rbd0[:, 6:6 + m["nj"]]]
        self.ctrl.setJointGains(np.full(m["nj"], bp.WbcParams.RECONFIGURE_MOTOR_KP), np.full(m["nj"], bp.WbcParams.RECONFIGURE_MOTOR_KD))

    def start(self):
        """state set, the solver armed, the first tick on the plant's rbd enqueued"""
        self.plant.set_state(self.rbd0)
        self.mpc.setup_commands(0.0, self.x0, self.gaits, -1, 0.0, np.zeros(4), horizon=self.H, from_previous=False)
        self.mpc.enqueue()
        t = torch.zeros(NB, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        self.ctrl.tick(t, self.plant.outputs()["rbd"].torch(), period=PERIOD, fetch=False)

    def snapshot(self):
        torch.cuda.synchronize()
        s = {k: v.torch().cpu().numpy().copy() for k, v in self.plant.outputs().items()}
        s.update({k: v.torch().cpu().numpy().copy() for k, v in self.ctrl.device_outputs().items() if k in TICK_KEYS})
        return s


def _times(ticks):
    out = [torch.full((NB,), PERIOD * (k + 1), dtype=torch.float64, device="cuda") for k in range(ticks)]
    torch.cuda.synchronize()
    return out


def _controlled(ticks):
    lp = Loop()
    lp.start()
    times, shots = _times(ticks), []
    for k in range(ticks):
        lp.plant.step_controlled(lp.ctrl, period=PERIOD, substeps=4)
        lp.est.update_from_plant(lp.plant, period=PERIOD, fetch=False)
        lp.ctrl.tick_estimated(times[k], lp.est, period=PERIOD, fetch=False)
        shots.append(lp.snapshot())
    return shots


@pytest.fixture(scope="module")
def controlled():
    """ten ticks of the loop without a supervisor: computed once, read by the pass-through and the stop test"""
    return _controlled(10)


def _supervised(ticks, tilt=None, read_every_tick=True):
    """the same loop through the supervisor, every robot in RUN.  tilt = (tick, robot): from that tick on the supervisor reads a copy of the
    plant's rbd in which the robot's roll is pi / 3 + 0.01 (the plant and the tick see the truth)."""
    lp = Loop()
    lp.start()
    lp.sup.request(sr.RUN)
    lp.sup.update_controlled(lp.ctrl, rbd=lp.plant.outputs()["rbd"].torch(), period=PERIOD)
    times, shots, sups = _times(ticks), [], []
    for k in range(ticks):
        lp.plant.step_supervised(lp.sup, period=PERIOD, substeps=4)
        lp.est.update_from_plant(lp.plant, period=PERIOD, fetch=False)
        lp.ctrl.tick_estimated(times[k], lp.est, period=PERIOD, fetch=False)
        if tilt is None:
            lp.sup.update_controlled(lp.ctrl, lp.est, period=PERIOD)
        else:
            torch.cuda.synchronize()
            shown = lp.plant.outputs()["rbd"].torch().clone()
            if k >= tilt[0]:
                shown[tilt[1], 2] = np.pi / 3 + 0.01
            torch.cuda.synchronize()
            lp.sup.update_controlled(lp.ctrl, rbd=shown, period=PERIOD)
        if read_every_tick or k == ticks - 1:
            shots.append(lp.snapshot())
            sups.append(lp.sup.state(NB, commands=True))
    return shots, sups


def test_pass_through(controlled):
    shots, sups = _supervised(10)
    free, _ = _supervised(10, read_every_tick=False)                         # no host synchronise inside: the events alone order the streams
    for k, (a, b) in enumerate(zip(shots, controlled)):
        for key in a:
            assert np.array_equal(a[key], b[key], equal_nan=True), (k, key)
        s = sups[k]
        assert s["state"].tolist() == [sr.RUN] * NB and not s["unsafe"].any() and s["counts"] == {"init": 0, "run": NB, "stopped": 0, "ready": 0, "unsafe": 0}
        cmd = a["joint_cmd"]
        assert np.array_equal(s["pos_des"], cmd[:, 0]) and np.array_equal(s["vel_des"], cmd[:, 1]) and np.array_equal(s["tau_ff"], cmd[:, 2])
    for key in free[0]:
        assert np.array_equal(free[0][key], controlled[-1][key], equal_nan=True), key


def test_stop(controlled):
    TILT_TICK, ROBOT = 3, 2
    shots, sups = _supervised(10, tilt=(TILT_TICK, ROBOT))
    others = [b for b in range(NB) if b != ROBOT]
    for k, (a, s) in enumerate(zip(shots, sups)):
        for key in a:
            assert np.array_equal(a[key][others], controlled[k][key][others], equal_nan=True), (k, key)
        if k < TILT_TICK:
            assert s["state"].tolist() == [sr.RUN] * NB
            continue
        assert s["state"].tolist() == [sr.STOPPED if b == ROBOT else sr.RUN for b in range(NB)] and s["cause"][ROBOT] == sr.ROLL
        assert s["counts"]["stopped"] == 1 and s["counts"]["run"] == NB - 1 and s["counts"]["unsafe"] == 1
        q = a["rbd"][ROBOT, 6:6 + s["pos_des"].shape[1]]                     # the stop command: the measured joints, no stiffness, stop_kd = 0
        assert np.array_equal(s["pos_des"][ROBOT], q) and not s["vel_des"][ROBOT].any() and not s["tau_ff"][ROBOT].any()
        assert not s["kp"][ROBOT].any() and not s["kd"][ROBOT].any()
        assert np.isclose(s["elapsed"][ROBOT], PERIOD * (k - TILT_TICK + 1))


def test_settle():
    import bipedal_control_amd as bp
    lp = Loop()
    nj, TICKS = lp.nj, 80
    row = bp.SupervisorParams(ramp_time=0.1, settle_pos_tol=0.2, settle_vel_tol=5.0, settle_time=0.02).toRow()
    lp.sup.setParams(row)
    lp.sup.setJointRows("kp_init", lp.hold["kp"])                            # the PD command that holds standing_state (tests/test_plant_reference.py)
    lp.sup.setJointRows("kd_init", lp.hold["kd"])
    ref = sr.Supervisor(NB, nj, np.array(lp.itf.get("default_joint_state")), params=row)
    ref.rows["kp_init"][:], ref.rows["kd_init"][:] = lp.hold["kp"], lp.hold["kd"]
    lp.plant.set_state(lp.rbd0)
    d_rbd = lp.plant.outputs()["rbd"]
    for k in range(TICKS):
        rbd = lp.plant.get_state()                                           # the kernel's own measurement
        lp.sup.update(d_rbd, None, PERIOD)
        ref.update(rbd, None, PERIOD)
        got = lp.sup.state(NB, commands=True)
        for key in INTS:
            assert got[key].tolist() == getattr(ref, key).tolist(), (k, key)
        assert np.array_equal(got["elapsed"], ref.elapsed) and [got["counts"][c] for c in COUNTS] == ref.counts[:5].tolist(), k
        assert all(np.all(np.isfinite(got[c])) for c in sr.COMMAND_ROWS), k
        lp.plant.step_supervised(lp.sup, period=PERIOD, substeps=4)
    ready = ref.ready.copy()
    print("settle: ready after", TICKS, "ticks", ready.tolist(), "base height", lp.plant.get_state()[:, 5])
    lp.sup.request(sr.RUN, only_ready=True)
    assert lp.sup.state(NB)["state"].tolist() == [sr.RUN if r else sr.INIT for r in ready]


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import bipedal_control_amd as bp
    lib = bp.load_library()
    itf = _itf("h1")
    nj = itf.actuatedDofNum
    sup = bp.BatchedSupervisor(itf, 4)
    rbd = np.zeros((4, 2 * (6 + nj)))
    sup.update(rbd, None, PERIOD)
    before = _all_rows(sup)

    def refused(call, status, *words):
        with pytest.raises(bp.BpmpcError) as err:
            call()
        msg = lib.bpmpc_last_error()
        assert err.value.status == status and all(w in msg for w in words), msg

    row = bp.SupervisorParams().toRow()
    for e, name in enumerate(bp.SupervisorParams.FIELDS):
        bad = np.tile(row, (4, 1))
        bad[3, e] = -0.5
        refused(lambda: sup.setParams(bad), INVALID, b"bpmpc_supervisor_set_params", b"row 3", ("entry %d (%s)" % (e, name)).encode(), b"negative")
    bad = np.tile(row, (4, 1))
    bad[1, 0] = np.nan
    refused(lambda: sup.setParams(bad), INVALID, b"row 1", b"entry 0 (tilt_limit)", b"not finite")
    sup.setParams(bad, mask=np.array([1, 0, 1, 1], np.int32))               # a row nobody takes is not looked at
    refused(lambda: sup.setParams(np.tile(row, (5, 1))), CAPACITY, b"bpmpc_supervisor_set_params", b"max_batch")
    good = np.zeros(nj)
    for which, value, why in (("q_init", np.inf, b"not finite"), ("kp_init", -1.0, b"negative"), ("kd_init", np.nan, b"not finite"), ("lower", np.nan, b"not a number"),
                              ("upper", np.nan, b"not a number")):
        r = good.copy()
        r[4] = value
        refused(lambda: sup.setJointRows(which, r), INVALID, b"bpmpc_supervisor_set_joint_rows", ("entry 4 (%s)" % which).encode(), why)
    sup.setJointRows("upper", np.full(nj, 0.5))
    sup.setJointRows("lower", np.full(nj, 0.5))                              # lower == upper is allowed
    refused(lambda: sup.setJointRows("lower", np.full(nj, 0.6)), INVALID, b"entry 0 (lower)", b"lower exceeds upper")
    refused(lambda: sup.setJointRows("upper", np.full(nj, 0.4), mask=np.array([0, 0, 1, 0], np.int32)), INVALID, b"(upper)", b"robot 2")
    sup.setJointRows("upper", np.full(nj, np.inf))
    sup.setJointRows("lower", np.full(nj, -np.inf))                          # +-infinity for these two rows
    refused(lambda: sup.setJointRows(5, good), INVALID, b"which")
    refused(lambda: sup.getJointRows(-1), INVALID, b"which")
    refused(lambda: sup.getJointRows(0, 4), CAPACITY, b"max_batch")
    refused(lambda: sup.request(3), INVALID, b"bpmpc_supervisor_request", b"target")
    refused(lambda: sup.request(-1), INVALID, b"target")
    refused(lambda: sup.request(sr.RUN, np.ones(5, np.int32)), CAPACITY, b"max_batch")
    for period in (0.0, -1.0, np.nan):
        refused(lambda: sup.update(rbd, None, period), INVALID, b"bpmpc_supervisor_update", b"period")
    refused(lambda: sup.update(np.zeros((5, 2 * (6 + nj))), None, PERIOD), CAPACITY, b"bpmpc_supervisor_update", b"max_batch")
    sup.resetParams()
    assert np.array_equal(sup.getParams(2), sr.DEFAULT_PARAMS)
    after = _all_rows(sup)
    for k in before:
        assert np.array_equal(before[k], after[k]), k                        # a refusal changes nothing
    g1 = bp.BatchedPlant(_itf("g1"), max_batch=4)
    refused(lambda: g1._call("bpmpc_plant_step_supervised", sup._h, 4, PERIOD, 4, None, None, 0), INVALID, b"bpmpc_plant_step_supervised", b"different robots")
