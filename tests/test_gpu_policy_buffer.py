"""GPU tier: the policy buffer (include/bpmpc.h "Policy buffer"): publish, adoption and buffered ticks against the tick without a buffer.

The yardstick is the existing tick, bit for bit: the buffer copies and selects, and the tick kernels are the same code, so every comparison is
np.array_equal over x_obs, x_opt, u_opt, joint_cmd, wbc_solution, planned_mode, safe and joint_torque and there is no tolerance anywhere.  Each
path has its own WBC and controller handle, reset before every compared tick, so the WBC's per-robot warm starts and yaw_last start equal.

Shapes: H1, batch 5 (one robot past the four a wave of the tick kernel holds) on two gait phases (two grids: p_grid is not the identity),
n_intervals = 30, max_nodes = 48, gains returned, feedback on - the smallest at which the gather, the masks and the last partial wave can go wrong.
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

from tests import oracle_bridge as ob
from tests.test_gpu_controller_tick import _rbd

pytestmark = pytest.mark.gpu

KEYS = ("x_obs", "x_opt", "u_opt", "joint_cmd", "wbc_solution", "planned_mode", "safe", "joint_torque")
NI, MAX_NODES = 30, 48
INVALID, UNSUPPORTED, CAPACITY = -1, -3, -6
COMMANDS = {"A": (0.3, 0.0, 0.0, 0.1), "B": (-0.2, 0.1, 0.0, -0.2), "C": (0.1, -0.1, 0.0, 0.3)}
T0 = {"A": 0.0, "B": 0.02, "C": 0.04}


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def _differ(a, b):
    return not np.array_equal(a["x_opt"], b["x_opt"]) and not np.array_equal(a["u_opt"], b["u_opt"])


def _rows(a, b, rows_of_a):
    """a on the robots of rows_of_a, b on the others: what a masked publish leaves"""
    sel = np.zeros(len(a["safe"]), bool)
    sel[list(rows_of_a)] = True
    return {k: np.where(sel.reshape((-1,) + (1,) * (a[k].ndim - 1)), a[k], b[k]) for k in KEYS}


class Rig:
    """A solver on two gait phases, a controller without a buffer (`plain`) and one with (`buf`), each with its own WBC, on the same solver."""

    def __init__(self, robot="h1", B=5, feedback=True, itf=None, sqp_iterations=0):
        import bipedal_control_amd as bp
        from bipedal_control_amd import scenarios as sc
        self.bp, self.sc, self.B = bp, sc, B
        self.itf = itf or sc.interface(robot)
        self.m = ob.model(robot)
        self.H = NI * sc.DT
        self.tm = [bp.loadModeSequenceTemplate(sc.ROBOTS[robot]["gait"], "trot")]
        self.gst = sc.GAIT_START + 0.1 * (np.arange(B) % 2)              # two phases of the gait: two grids
        self.x0 = sc.perturbed_initial_states(self.itf, B)
        self.mpc = bp.BatchedSqpMpc(self.itf, max_batch=B, max_nodes=MAX_NODES, return_gains=True, feedback_policy=feedback, sqp_iterations=sqp_iterations)
        self.pol = bp.PolicyBuffer(self.mpc, B)
        self.plain, self.buf = self.controller(), self.controller()
        self.buf.attachPolicy(self.pol)
        rng = np.random.default_rng(11)
        self.rbd = np.array([_rbd(self.m, self.x0[b], rng, speed=0.05, consistent_mode=3)[0] for b in range(B)])
        self.tq = 0.045 + 0.0173 * np.arange(B)                          # inside the horizons of A, B and C, no two robots on one node

    def controller(self):
        bp = self.bp
        c = bp.BatchedController(self.mpc, bp.WeightedWbc(self.itf, max_batch=self.B))
        nj = self.itf.actuatedDofNum
        c.setJointGains(np.full(nj, 40.0), np.full(nj, 1.5))           # joint_torque is more than the WBC torque
        return c

    def setup(self, name):
        self.mpc.setup_commands(T0[name], self.x0, self.tm, 0, self.gst, np.array(COMMANDS[name]) * np.ones((self.B, 1)), horizon=self.H)

    def solve(self, name):
        self.setup(name)
        self.mpc.enqueue()

    def tick(self, ctrl):
        """A tick at the fixed (t, rbd) from a fresh controller state"""
        ctrl.reset()
        ctrl.wbc.reset()
        return ctrl.tick(self.tq, self.rbd)

    def reference(self, name):
        """solve `name`; the bits of the tick without a buffer on it"""
        self.solve(name)
        return self.tick(self.plain)


def _status(bp, call):
    with pytest.raises(bp.BpmpcError) as e:
        call()
    return e.value.status


# ---------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("robot,B,feedback", [("h1", 5, True), ("h1", 5, False), ("g1", 3, True)])
def test_publish_and_update_equal_the_plain_tick(robot, B, feedback):
    r = Rig(robot, B, feedback)
    ref = r.reference("A")
    assert r.mpc.layout()["n_grids"] == 2
    r.pol.publish()
    assert r.pol.update() is True
    assert _same(r.tick(r.buf), ref)
    info = r.pol.info()
    assert list(info["generation"]) == [1] * B and np.all(info["t0"] == T0["A"])
    assert list(info["status"]) == [s.status for s in r.mpc.fetch()[4]]


def test_a_solve_in_flight_does_not_disturb_the_ticks():
    r = Rig()
    ref_a = r.reference("A")
    x_a = r.mpc.fetch()[1]
    r.pol.publish(); r.pol.update()
    assert _same(r.tick(r.buf), ref_a)
    r.setup("B")                                                        # between setup and run the solver holds no policy
    assert _status(r.bp, lambda: r.tick(r.plain)) == INVALID
    assert _same(r.tick(r.buf), ref_a)
    r.mpc.enqueue()
    assert _same(r.tick(r.buf), ref_a)                                  # enqueued behind nothing: the solve is still running or just over
    assert not np.array_equal(r.mpc.fetch()[1], x_a)
    ref_b = r.tick(r.plain)
    assert _differ(ref_a, ref_b)
    assert _same(r.tick(r.buf), ref_a)
    r.pol.publish()
    assert _same(r.tick(r.buf), ref_a)                                  # a publish alone changes no tick
    assert r.pol.update() is True
    assert _same(r.tick(r.buf), ref_b)
    assert list(r.pol.info()["generation"]) == [2] * 5


# ---------------------------------------------------------------------------------------------------------------- 3, 4
@pytest.mark.parametrize("device_mask", [False, True])
def test_masked_publish(device_mask):
    r = Rig()
    ref_a = r.reference("A")
    r.pol.publish(); r.pol.update()
    ref_b = r.reference("B")
    mask = np.array([1, 0, 1, 0, 0], np.int32)
    if device_mask:
        mask = torch.tensor(mask, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
    r.pol.publish(mask=mask)
    r.pol.update()
    out = r.tick(r.buf)
    assert _same(out, _rows(ref_b, ref_a, (0, 2)))
    assert _differ(ref_a, ref_b) and not _same(out, ref_a) and not _same(out, ref_b)
    info = r.pol.info()
    assert list(info["generation"]) == [2, 1, 2, 1, 1]
    assert list(info["t0"]) == [T0["B"], T0["A"], T0["B"], T0["A"], T0["A"]]


def test_two_publishes_before_one_adoption():
    r = Rig()
    ref_a = r.reference("A")
    r.pol.publish(); r.pol.update()
    ref_b = r.reference("B")
    r.pol.publish(mask=np.array([1, 1, 0, 0, 0], np.int32))
    assert _same(r.tick(r.buf), ref_a)                                  # a publish alone changes no tick
    ref_c = r.reference("C")
    r.pol.publish(mask=np.array([0, 1, 1, 0, 0], np.int32))
    assert _same(r.tick(r.buf), ref_a)
    assert r.pol.update() is True and r.pol.update() is False
    out = r.tick(r.buf)
    assert _same(out, _rows(ref_b, _rows(ref_c, ref_a, (1, 2)), (0,)))
    info = r.pol.info()
    assert list(info["generation"]) == [2, 2, 2, 1, 1]
    assert list(info["t0"]) == [T0["B"], T0["C"], T0["C"], T0["A"], T0["A"]]
    # and the slots keep turning over: a later full publish reaches every robot
    r.solve("A")
    r.pol.publish(); r.pol.update()
    assert _same(r.tick(r.buf), ref_a)


# ---------------------------------------------------------------------------------------------------------------- 5
def _skip_failed_generations(itf):
    r = Rig("h1", 3, True, itf=itf, sqp_iterations=1)
    r.solve("A")
    status = [s.status for s in r.mpc.fetch()[4]]
    r.pol.publish(); r.pol.update()
    first = r.tick(r.buf)
    assert list(r.pol.info()["generation"]) == [1, 1, 1] and list(r.pol.info()["status"]) == status
    r.solve("B")
    status_b = [s.status for s in r.mpc.fetch()[4]]
    r.pol.publish(skip_failed=True)
    r.pol.update()                                                      # adopted, or an empty turn-over of the slots: both are allowed
    return status, status_b, list(r.pol.info()["generation"]), first, r.tick(r.buf)


def test_skip_failed_reads_the_device_status(tmp_path):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    text = open(sc.H1["task"]).read()
    a = text.index("\nR\n{")
    bad = tmp_path / "task_negative_R.info"
    bad.write_text(text[:a] + text[a:].replace("scaling 1e-3", "scaling -1e-3", 1))
    itf = bp.BipedalRobotInterface(str(bad), sc.H1["urdf"], sc.H1["reference"])
    status, status_b, generation, first, second = _skip_failed_generations(itf)
    assert status == [2, 2, 2] and status_b == [2, 2, 2]
    assert generation == [1, 1, 1] and _same(first, second)
    status, status_b, generation, first, second = _skip_failed_generations(sc.interface("h1"))
    assert 2 not in status + status_b
    assert generation == [2, 2, 2] and _differ(first, second)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_update_without_waiting():
    r = Rig()
    assert r.pol.update(wait=False) is False                            # nothing outstanding
    ref_a = r.reference("A")
    r.pol.publish()
    r.mpc.synchronize()
    assert r.pol.update(wait=False) is True
    assert r.pol.update(wait=False) is False and r.pol.update(wait=True) is False
    assert _same(r.tick(r.buf), ref_a)
    ref_b = r.reference("B")
    r.pol.publish()
    r.mpc.synchronize()
    assert r.pol.update(wait=False) is True
    assert _same(r.tick(r.buf), ref_b) and _differ(ref_a, ref_b)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_refusals():
    r = Rig()
    bp, lib = r.bp, r.bp.load_library()
    assert _status(bp, lambda: r.pol.publish()) == INVALID              # no run yet
    r.setup("A")
    assert _status(bp, lambda: r.pol.publish()) == INVALID              # a setup without a run
    ref_a = (r.mpc.enqueue(), r.tick(r.plain))[1]
    assert _status(bp, lambda: r.tick(r.buf)) == INVALID and b"initial policy" in lib.bpmpc_last_error()
    assert _status(bp, lambda: r.pol.publish(mask=np.array([1, 1, 0, 0, 0], np.int32))) == INVALID      # the first publish sets the batch: every robot
    assert lib.bpmpc_policy_publish(r.pol._h, 3, None, 0, 0) == INVALID and b"batch" in lib.bpmpc_last_error()
    assert lib.bpmpc_policy_publish(r.pol._h, 6, None, 0, 0) == INVALID      # not the batch of the setup either
    assert _status(bp, lambda: r.pol.publish(skip_failed=True)) == INVALID      # nor a conditional one: not the initial policy
    assert r.pol.update() is False and _status(bp, lambda: r.tick(r.buf)) == INVALID
    r.pol.publish()
    assert _status(bp, lambda: r.tick(r.buf)) == INVALID                # published, not adopted
    assert r.pol.update() is True
    assert _same(r.tick(r.buf), ref_a)
    d = np.zeros(5 * 2 * 16).ctypes.data_as(C.POINTER(C.c_double))
    assert lib.bpmpc_controller_tick(r.buf._h, 4, d, d, 0, 0.0025, None) == INVALID and b"batch" in lib.bpmpc_last_error()
    # a restart: refused until the next adoption
    mask = np.array([0, 1, 0, 0, 0], np.int32)
    r.buf.restart(mask, r.rbd)
    assert _status(bp, lambda: r.tick(r.buf)) == INVALID and b"restart" in lib.bpmpc_last_error()
    assert _status(bp, lambda: r.pol.publish()) == INVALID              # the solver waits for its next setup and run
    r.mpc.setup_commands(T0["B"], None, r.tm, 0, r.gst, np.array(COMMANDS["B"]) * np.ones((5, 1)), horizon=r.H, from_previous=True)
    r.mpc.enqueue()
    assert _status(bp, lambda: r.tick(r.buf)) == INVALID
    r.pol.publish(); r.pol.update()
    out = r.buf.tick(r.tq, r.rbd)
    assert all(np.all(np.isfinite(out[k])) for k in KEYS)
    # another solver, a DDP solver
    other = bp.BatchedSqpMpc(r.itf, max_batch=5, max_nodes=MAX_NODES, return_gains=True)
    pol2 = bp.PolicyBuffer(other, 5)
    assert _status(bp, lambda: r.buf.attachPolicy(pol2)) == INVALID and b"another solver" in lib.bpmpc_last_error()
    assert _status(bp, lambda: bp.PolicyBuffer(bp.BatchedDdpMpc(r.itf, 5, MAX_NODES), 5)) == UNSUPPORTED
    assert _status(bp, lambda: bp.PolicyBuffer(other, 6)) == CAPACITY
    again = r.buf.tick(r.tq, r.rbd)                                     # every handle is still usable
    assert all(np.all(np.isfinite(again[k])) for k in KEYS)


# ---------------------------------------------------------------------------------------------------------------- 8
def _ordering_sequence(synchronise):
    """run A, publish, update, three ticks, setup + run + publish B, two ticks, update, tick, setup + run + publish C - into the slot the five ticks
    before the last turn-over were reading -, tick, update, tick.  Every tick has a controller and a WBC of its own on the one buffer, so each keeps its outputs to
    the end without anything being fetched; inputs are device tensors."""
    r = Rig()
    ctrls = [r.controller() for _ in range(8)]
    for c in ctrls:
        c.attachPolicy(r.pol)
    t_dev = torch.tensor(r.tq, dtype=torch.float64, device="cuda")
    rbd_dev = torch.tensor(r.rbd, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    after = torch.cuda.synchronize if synchronise else (lambda: None)
    it = iter(ctrls)

    def ticks(n):
        for _ in range(n):
            next(it).tick(t_dev, rbd_dev, fetch=False); after()

    r.solve("A"); after()
    r.pol.publish(); after()
    r.pol.update(); after()
    ticks(3)
    r.solve("B"); after()
    r.pol.publish(); after()
    ticks(2)
    r.pol.update(); after()
    ticks(1)
    r.solve("C"); after()
    r.pol.publish(); after()
    ticks(1)
    r.pol.update(); after()
    ticks(1)
    torch.cuda.synchronize()
    outs = [{k: v.torch().cpu().numpy() for k, v in c.device_outputs().items() if k in KEYS} for c in ctrls]
    return r, outs


def test_ordering_without_host_synchronisation():
    r, free = _ordering_sequence(False)
    _, synced = _ordering_sequence(True)
    for k, (a, b) in enumerate(zip(free, synced)):
        assert _same(a, b), k
    # the synchronised sequence is the plain tick on A (ticks 0-4), B (5, 6), C (7)
    refs = {name: r.reference(name) for name in "ABC"}
    for k, name in enumerate("AAAAABBC"):
        assert _same(synced[k], refs[name]), (k, name)
    assert _differ(refs["A"], refs["B"]) and _differ(refs["B"], refs["C"])


# ---------------------------------------------------------------------------------------------------------------- 9
NB, M, TICKS = 4, 10, 30


class _Loop:
    """The loop of tests/test_gpu_plant.py (plant, estimator, tick, a re-armed solve every M ticks) at batch 4, with or without the buffer"""

    def __init__(self, buffered):
        import bipedal_control_amd as bp
        from bipedal_control_amd import scenarios as sc
        from oracle import wbc_py as wp
        from tests.test_plant_reference import standing_state
        self.itf = itf = sc.interface("h1")
        self.H = 20 * sc.DT
        self.mpc = bp.BatchedSqpMpc(itf, max_batch=NB, max_nodes=sc.max_nodes_for(20, self.H), return_gains=True)
        self.wbc = bp.WeightedWbc(itf, max_batch=NB)
        self.ctrl = bp.BatchedController(self.mpc, self.wbc)
        self.est = bp.BatchedStateEstimate(itf, kind="from_topic", max_batch=NB)
        self.plant = bp.BatchedPlant(itf, max_batch=NB)
        self.pol = None
        if buffered:
            self.pol = bp.PolicyBuffer(self.mpc, NB)
            self.ctrl.attachPolicy(self.pol)
        self.gaits = [bp.loadModeSequenceTemplate(sc.ROBOTS["h1"]["gait"], "stance")]
        m = ob.model("h1")
        q, v, _ = standing_state(m, depth=0.0025)
        rng = np.random.default_rng(5)
        self.rbd0 = np.array([wp.rbd_from(m, q + 0.002 * rng.standard_normal(len(q)) * np.r_[np.zeros(6), np.ones(len(q) - 6)], v) for _ in range(NB)])
        self.x0 = np.tile(itf.getInitialState(), (NB, 1))
        self.x0[:, 6:] = np.c_[self.rbd0[:, 3:6], self.rbd0[:, 0:3], self.rbd0[:, 6:6 + m["nj"]]]
        self.ctrl.setJointGains(np.full(m["nj"], bp.WbcParams.RECONFIGURE_MOTOR_KP), np.full(m["nj"], bp.WbcParams.RECONFIGURE_MOTOR_KD))

    def arm(self, t, first):
        self.mpc.setup_commands(t, self.x0 if first else None, self.gaits, -1, 0.0, np.zeros(4), horizon=self.H, from_previous=not first)
        self.mpc.enqueue()

    def snapshot(self):
        s = {k: v.torch().cpu().numpy() for k, v in self.plant.outputs().items() if k in ("rbd", "joint_pos", "joint_vel", "contact_force")}
        s.update({k: v.torch().cpu().numpy() for k, v in self.ctrl.device_outputs().items() if k in KEYS})
        return s


def _run_loop(buffered, delay, read_every_tick, skip_failed=False):
    lp = _Loop(buffered)
    lp.plant.set_state(lp.rbd0)
    lp.arm(0.0, True)
    if buffered:
        lp.pol.publish(); lp.pol.update()
    t = torch.zeros(NB, dtype=torch.float64, device="cuda")
    times = [torch.full((NB,), 0.002 * (k + 1), dtype=torch.float64, device="cuda") for k in range(TICKS)]
    torch.cuda.synchronize()
    lp.ctrl.tick(t, lp.plant.outputs()["rbd"].torch(), period=0.002, fetch=False)
    shots, generations, armed = {}, {}, None
    for k in range(TICKS):
        lp.plant.step_controlled(lp.ctrl, period=0.002, substeps=4)
        lp.est.update_from_plant(lp.plant, period=0.002, fetch=False)
        lp.ctrl.tick_estimated(times[k], lp.est, period=0.002, fetch=False)
        if k % M == M - 1:
            lp.arm(0.002 * (k + 1), False)
            if buffered:
                lp.pol.publish(skip_failed=skip_failed)
                armed = k
        if buffered and armed is not None and k == armed + delay:
            assert lp.pol.update() is True
            armed = None
        if read_every_tick or k == TICKS - 1:
            torch.cuda.synchronize()
            shots[k] = lp.snapshot()
            if buffered and read_every_tick:
                generations[k] = int(lp.pol.info()["generation"][0])
    return shots, generations


def _loops_equal(a, b, ticks):
    for k in ticks:
        for key in a[k]:
            assert np.array_equal(a[k][key], b[k][key]), (k, key)


def test_the_whole_loop_with_no_delay_is_the_loop_without_a_buffer():
    plain, _ = _run_loop(False, 0, True)
    read, generations = _run_loop(True, 0, True)
    free, _ = _run_loop(True, 0, False)
    assert sorted(plain) == list(range(TICKS))
    _loops_equal(read, plain, range(TICKS))                             # tick by tick, setup_commands(x0 = NULL) picking tick_x up across the streams
    _loops_equal(free, plain, [TICKS - 1])                              # and with nothing synchronised in between
    assert generations[M - 2] == 1 and generations[M - 1] == 2 and generations[TICKS - 1] == 4


def test_the_whole_loop_with_a_delayed_policy():
    D = M // 2
    read, generations = _run_loop(True, D, True, skip_failed=True)
    free, _ = _run_loop(True, D, False, skip_failed=True)
    for k, s in read.items():
        assert all(np.all(np.isfinite(np.asarray(a, float))) for a in s.values()), k
        assert np.all(s["safe"] == 1), (k, s["safe"])
    _loops_equal(free, read, [TICKS - 1])
    # solve j is armed after tick j M - 1 and takes effect D ticks later: in between the ticks run on the generation before
    for j in (1, 2):
        for k in range(j * M - 1, j * M - 1 + D):
            assert generations[k] == j, (k, generations[k])
        assert generations[j * M - 1 + D] == j + 1


# ---------------------------------------------------------------------------------------------------------------- 10
def test_detached_is_the_controller_without_a_buffer():
    r = Rig()
    ref_a = r.reference("A")
    r.pol.publish(); r.pol.update()
    assert _same(r.tick(r.buf), ref_a)
    ref_b = r.reference("B")                                            # not published: the buffer still holds A
    assert _same(r.tick(r.buf), ref_a)
    r.buf.attachPolicy(None)
    assert _same(r.tick(r.buf), ref_b) and _differ(ref_a, ref_b)        # detached: the solver's arrays, like a controller that never had a buffer
    r.setup("C")
    assert _status(r.bp, lambda: r.tick(r.buf)) == INVALID              # and its refusals
    r.buf.attachPolicy(r.pol)
    assert _same(r.tick(r.buf), ref_a)
