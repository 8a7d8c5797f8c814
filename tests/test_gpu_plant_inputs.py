"""GPU tier: the plant's input model (include/bpmpc.h "Plant", inputs; k_plant_input in plant_input.hip) against the numpy restatement
tests/plant_input_reference.py and against handles that differ in one call.
H1 (nj = 10) and G1 (nj = 12), batch 5 in a handle of 8 (odd: masks and the max_batch stride matter), 20 control steps of 4 substeps at 2 ms (the
ring of 16 wraps) from the perturbed standing fleet of tests/test_gpu_plant_sensors.py; the command changes every step: cmd_n = cmd + 0.01 n.
  untouched        a handle that was switched, stepped and reset gives the bits of one that never was, and no tick passes; zero rows give the same
                   plant outputs and hand the incoming command and force on as bits
  restatement      every field set, different per robot: applied rows, lost, pushing, delay_steps, t, n exactly, the applied force to 1e-12 N
  delay twin       k = 0, 1, 4, 15, 2 per robot against an untouched twin stepped with the command of step max(n - k, 0), bit for bit
  three doors      step_controlled and step_supervised: zero rows equal the untouched loop; with 4 ms the applied rows are those of two ticks ago
  masks and seeds  masked calls leave the other robots' bits; seeds reproduce; host rows and device rows give the same bits
  refusals         applied() on an untouched handle and before the first step, bad rows, batch > max_batch
  the loop         50 ticks under the H1 file's 9 ms with 5 % loss stay finite
Every comparison prints its maximum before it asserts (pytest -s)."""
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

from tests import plant_input_reference as ir
from tests import test_gpu_plant as tp
from tests.test_gpu_plant_sensors import _fleet

pytestmark = pytest.mark.gpu
B, MAXB, STEPS, PERIOD, SUBSTEPS = 5, 8, 20, 0.002, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ir.ROWS
DELAYS = (0.0, 0.002, 0.009, 0.031, 0.005)
K = (0, 1, 4, 15, 2)              # their control steps at 2 ms
MASK = np.array([1, 0, 1, 0, 0], np.int32)
# the applied force: the device's and libm's sin / cos are within a few ulp on arguments up to 2 pi; times 100 N that is about 1e-13 N, plus an
# order of magnitude
FORCE_TOL = 1e-12


def _plant(robot):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    return bp.BatchedPlant(sc.interface(robot), max_batch=MAXB)


def _cmd(robot, n):
    """cmd_n = cmd + 0.01 n: the five rows [5, nj] each"""
    return [a + 0.01 * n for a in _fleet(robot)[1]]


def _force():
    f = np.random.default_rng(9).uniform(-5.0, 5.0, (B, 3))
    f[1, 2], f[3, 0] = -0.0, 0.0      # a negative zero has to come through as bits
    return f


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b, keys=None):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in (keys or a))


def _applied(plant):
    return {k: v.torch().cpu().numpy() for k, v in plant.applied().items()}


def _run(robot, configure=None, steps=STEPS, command=None, force=None, during=None, plant=None, switched=True):
    """`steps` control steps of a handle (`plant`, or a new one) that `configure` prepared, with command(n) (default: cmd_n) and the base force
    `force`; during(plant, n) runs before step n.  Per step: the plant's outputs, the applied command (switched handles) and the input state."""
    plant = plant or _plant(robot)
    if configure:
        configure(plant)
    plant.set_state(_fleet(robot)[0])
    outs, applied, state = [], [], []
    for n in range(steps):
        if during:
            during(plant, n)
        plant.step(*(command(n) if command else _cmd(robot, n)), base_force=force, period=PERIOD, substeps=SUBSTEPS)
        outs.append(tp._read(plant))
        applied.append(_applied(plant) if configure and switched else None)
        state.append(plant.inputState())
    return outs, applied, state, plant


def _rows(**fields):
    return np.tile(ir.row(**fields), (B, 1))


# ---------------------------------------------------------------------------------------------------------------- untouched
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_untouched_handle(robot):
    import bipedal_control_amd as bp
    force = _force()

    def switched_and_reset(plant):
        plant.setInputParams(_rows(delay=0.004, dropout=0.5, push_force=50.0, push_interval=0.004, push_duration=0.002))
        plant.seedInputs(3)
        plant.set_state(_fleet(robot)[0])
        plant.step(*_cmd(robot, 0), period=PERIOD, substeps=SUBSTEPS)
        s = plant.inputState()
        assert s["tick"].tolist() == [1] * B and s["steps"].tolist() == [1] * B and s["delay_steps"].tolist() == [2] * B
        plant.resetInputParams()
        assert not plant.getInputParams(2).any()
        with pytest.raises(bp.BpmpcError, match="untouched"):
            plant.applied()

    fresh, _, fresh_state, _ = _run(robot, force=force)
    reset, _, reset_state, _ = _run(robot, switched_and_reset, force=force, switched=False)
    for n in range(STEPS):
        assert _same(fresh[n], reset[n]), n
        for s in (fresh_state[n], reset_state[n]):      # nothing was launched: no tick has passed
            assert not any(s[k].any() for k in s), (n, s)
    # switched, every row zero: the same plant outputs, and the applied command and force are the incoming ones as bits
    outs, applied, state, plant = _run(robot, lambda p: p.seedInputs(5), force=force)
    worst = 0
    for n in range(STEPS):
        assert _same(fresh[n], outs[n]), n
        for r, c in zip(ROWS, _cmd(robot, n)):
            worst = max(worst, int((_bits(applied[n][r]) != _bits(c)).sum()))
        worst = max(worst, int((_bits(applied[n]["base_force"]) != _bits(force)).sum()))
        s = state[n]
        assert s["tick"].tolist() == [n + 1] * B and s["steps"].tolist() == [n + 1] * B
        assert not s["lost"].any() and not s["pushing"].any() and not s["delay_steps"].any()
    print("zero rows", robot, "entries whose bits differ from the incoming command or force:", worst)
    assert worst == 0
    assert np.signbit(applied[0]["base_force"][1, 2]) and not np.signbit(applied[0]["base_force"][3, 0])
    # without a caller's force the applied force is zero, and the plant the one that was given none
    none, _, _, _ = _run(robot, steps=3)
    zero, applied0, _, _ = _run(robot, lambda p: p.setInputParams(ir.row()), steps=3)
    assert all(_same(none[n], zero[n]) and not applied0[n]["base_force"].any() for n in range(3))


# ---------------------------------------------------------------------------------------------------------------- against the restatement
def _every_field():
    rows = _rows(dropout=0.3, push_interval=0.016, push_duration=0.004)
    rows[:, ir.FIELDS.index("delay")] = DELAYS
    rows[:, ir.FIELDS.index("push_force")] = (100.0, 80.0, 60.0, 40.0, 20.0)
    return rows


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_every_field_against_restatement(robot):
    """Applied rows, lost, pushing, delay_steps, t and n exactly; the applied force within FORCE_TOL.  The restatement is fed the step index as its
    command, so what it returns says which cmd_n the kernel has to have applied."""
    rows, seed, force = _every_field(), 11, _force()

    def configure(plant):
        plant.setInputParams(rows)
        plant.seedInputs(seed)
        assert np.array_equal(plant.getInputParams(3), rows[3]) and not plant.getInputParams().any()

    _, applied, state, _ = _run(robot, configure, force=force)
    models = [ir.Inputs(b, rows[b]) for b in range(B)]
    for m in models:
        m.seed_inputs(seed)
    ref = [[models[b].step(n, force[b], PERIOD) for b in range(B)] for n in range(STEPS)]
    # the condition under which this test says something, on the restatement alone
    lost = np.array([[ref[n][b][2] for n in range(STEPS)] for b in range(B)])
    pushed = np.array([[ref[n][b][3] for n in range(STEPS)] for b in range(B)])
    print("restatement", robot, "losses per robot", lost.sum(axis=1).tolist(), "pushed steps per robot", pushed.sum(axis=1).tolist())
    assert np.all(lost.sum(axis=1) >= 2) and np.all((1 - lost).sum(axis=1) >= 2)
    assert any(np.any(lost[b, 1:] & lost[b, :-1]) for b in range(B))
    assert np.all(pushed.sum(axis=1) >= 4) and [ref[0][b][4] for b in range(B)] == list(K)
    wrong, worst = 0, 0.0
    for n in range(STEPS):
        for b in range(B):
            src, f, was_lost, pushing, k = ref[n][b]
            for r, c in zip(ROWS, _cmd(robot, src)):
                wrong += int((_bits(applied[n][r][b]) != _bits(c[b])).sum())
            worst = max(worst, float(np.abs(applied[n]["base_force"][b] - f).max()))
            if not pushing:
                assert np.array_equal(_bits(applied[n]["base_force"][b]), _bits(force[b])), (n, b)
            else:
                assert applied[n]["base_force"][b, 2] == force[b, 2]
        s = state[n]
        assert s["lost"].tolist() == lost[:, n].tolist() and s["pushing"].tolist() == pushed[:, n].tolist() and s["delay_steps"].tolist() == list(K), n
        assert s["tick"].tolist() == [n + 1] * B and s["steps"].tolist() == [n + 1] * B
    print("restatement", robot, "applied entries with other bits:", wrong, " applied force, max |device - restatement| %.2e N" % worst)
    assert wrong == 0
    assert worst <= FORCE_TOL


# ---------------------------------------------------------------------------------------------------------------- delay twin
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_delay_against_an_untouched_twin(robot):
    rows = _rows()
    rows[:, ir.FIELDS.index("delay")] = DELAYS

    def late_command(n):      # robot b receives the command of step max(n - k_b, 0)
        per_robot = [_cmd(robot, max(n - k, 0)) for k in K]
        return [np.array([per_robot[b][r][b] for b in range(B)]) for r in range(len(ROWS))]

    late, _, state, _ = _run(robot, lambda p: p.setInputParams(rows))
    twin, _, twin_state, _ = _run(robot, command=late_command)
    differing = 0
    for n in range(STEPS):
        differing += sum(int(not np.array_equal(late[n][key], twin[n][key], equal_nan=True)) for key in late[n])
        assert state[n]["delay_steps"].tolist() == list(K) and not twin_state[n]["tick"].any()
    print("delay twin", robot, "outputs that differ over", STEPS, "steps:", differing)
    assert differing == 0
    plain, _, _, _ = _run(robot, steps=6)
    assert not np.array_equal(plain[5]["joint_pos"][2], late[5]["joint_pos"][2])      # the delay does change what the robot does


# ---------------------------------------------------------------------------------------------------------------- the three doors
TICKS = 10


def _door(door, configure=None):
    """TICKS ticks of the closed loop of tests/test_gpu_supervisor.py through step_controlled or step_supervised (every robot in RUN).  Per tick:
    the command the step was given (read before it), the snapshot after it, the applied command (a configured plant)."""
    from tests import supervisor_reference as sr
    from tests import test_gpu_supervisor as ts
    lp = ts.Loop()
    if configure:
        configure(lp.plant)
    lp.start()
    if door == "supervised":
        lp.sup.request(sr.RUN)
        lp.sup.update_controlled(lp.ctrl, rbd=lp.plant.outputs()["rbd"].torch(), period=PERIOD)
    times, given, shots, applied = ts._times(TICKS), [], [], []
    for k in range(TICKS):
        torch.cuda.synchronize()
        if door == "supervised":
            s = lp.sup.state(ts.NB, commands=True)
            given.append({r: s[r].copy() for r in ROWS})
            lp.plant.step_supervised(lp.sup, period=PERIOD, substeps=SUBSTEPS)
        else:
            o = {key: v.torch().cpu().numpy().copy() for key, v in lp.ctrl.device_outputs().items() if key in ("joint_cmd", "joint_kp", "joint_kd")}
            given.append({"pos_des": o["joint_cmd"][:, 0], "vel_des": o["joint_cmd"][:, 1], "tau_ff": o["joint_cmd"][:, 2], "kp": o["joint_kp"], "kd": o["joint_kd"]})
            lp.plant.step_controlled(lp.ctrl, period=PERIOD, substeps=SUBSTEPS)
        lp.est.update_from_plant(lp.plant, period=PERIOD, fetch=False)
        lp.ctrl.tick_estimated(times[k], lp.est, period=PERIOD, fetch=False)
        if door == "supervised":
            lp.sup.update_controlled(lp.ctrl, lp.est, period=PERIOD)
        shots.append(lp.snapshot())
        applied.append({key: v.copy() for key, v in _applied(lp.plant).items()} if configure else None)
    return given, shots, applied, lp


@pytest.mark.parametrize("door", ["controlled", "supervised"])
def test_three_doors(door):
    """bpmpc_plant_step is the door of every other test here; these are the other two"""
    _, plain, _, _ = _door(door)
    given, zero, applied, lp = _door(door, lambda p: p.seedInputs(1))
    differing = 0
    for k in range(TICKS):
        differing += sum(int(not np.array_equal(zero[k][key], plain[k][key], equal_nan=True)) for key in zero[k])
        differing += sum(int(not np.array_equal(_bits(applied[k][r]), _bits(given[k][r]))) for r in ROWS)
    print("door", door, "zero rows: arrays that differ from the untouched loop or the given command:", differing)
    assert differing == 0
    assert lp.plant.inputState()["tick"].tolist() == [TICKS] * len(plain[0]["rbd"])
    given, late, applied, lp = _door(door, lambda p: p.setInputParams(ir.row(delay=0.004)))
    differing = sum(int(not np.array_equal(_bits(applied[k][r]), _bits(given[max(k - 2, 0)][r]))) for k in range(TICKS) for r in ROWS)
    print("door", door, "delay 4 ms: applied rows that are not those of two ticks ago:", differing)
    assert differing == 0
    assert lp.plant.inputState()["delay_steps"].tolist() == [2] * len(plain[0]["rbd"])
    changing = {r: sum(int(not np.array_equal(given[k][r], given[k - 2][r])) for k in range(2, TICKS)) for r in ROWS}
    print("door", door, "ticks whose given row differs from that of two ticks before:", changing)
    assert any(changing.values())                                          # the command does change between ticks: the comparison above can fail
    assert all(np.all(np.isfinite(np.asarray(a, float))) for s in late for a in s.values())


# ---------------------------------------------------------------------------------------------------------------- masks and seeds
def test_masks_and_seeds():
    robot = "h1"
    rows = _every_field()
    rows2 = _rows(delay=0.004, dropout=0.6, push_force=30.0, push_interval=0.008, push_duration=0.002)
    AT, force = 6, _force()
    held = []

    def configure(seed):
        def go(plant):
            plant.setInputParams(rows)
            plant.seedInputs(seed)
        return go

    def masked_call(device):
        dev = (lambda a, dt: torch.tensor(a, dtype=dt, device="cuda")) if device else (lambda a, dt: a)

        def go(plant, n):
            if n == AT:
                args = dev(rows2, torch.float64), dev(MASK, torch.int32)
                held.append(args)      # device inputs are only enqueued: they outlive the call
                if device:
                    torch.cuda.synchronize()
                plant.setInputParams(args[0], mask=args[1])
                plant.seedInputs(9, mask=args[1])
        return go

    def everything(outs, applied, state, n):
        d = dict(outs[n])
        d.update({"applied_" + k: v for k, v in applied[n].items()})
        d.update({"state_" + k: v for k, v in state[n].items()})
        return d

    plain = _run(robot, configure(11), force=force)
    again = _run(robot, configure(11), force=force)
    other = _run(robot, configure(12), force=force)
    for n in range(STEPS):
        assert _same(everything(*plain[:3], n), everything(*again[:3], n)), n
    assert any(not np.array_equal(plain[2][n]["lost"], other[2][n]["lost"]) for n in range(STEPS))
    # masked set_input_params and seed_inputs before step AT, from host arrays and from device tensors
    keep, host = MASK == 0, None
    for device in (False, True):
        masked = _run(robot, configure(11), force=force, during=masked_call(device))
        for n in range(STEPS):
            a, b = everything(*masked[:3], n), everything(*plain[:3], n)
            for key in a:
                assert np.array_equal(a[key][keep], b[key][keep], equal_nan=True), (device, n, key)
            if n >= AT:
                assert masked[2][n]["tick"][~keep].tolist() == [n + 1 - AT] * 2 and masked[2][n]["steps"][~keep].tolist() == [n + 1 - AT] * 2
                assert masked[2][n]["delay_steps"][~keep].tolist() == [2, 2]
        assert np.array_equal(masked[3].getInputParams(2), rows2[2]) and np.array_equal(masked[3].getInputParams(1), rows[1])
        assert any(not np.array_equal(masked[2][n]["lost"][~keep], plain[2][n]["lost"][~keep]) for n in range(AT, STEPS))
        if host is None:
            host = masked
        else:
            assert all(_same(everything(*masked[:3], n), everything(*host[:3], n)) for n in range(STEPS))
    # a masked set_state before step AT: the robots of the mask forget their buffered commands (the command of step AT until their history is long
    # enough again) and keep their tick; the others keep their bits.  Delay alone, so that what is applied says which command it was
    late = _rows()
    late[:, ir.FIELDS.index("delay")] = DELAYS

    def restart(plant, n):
        if n == AT:
            plant.set_state(_fleet(robot)[2], mask=MASK)

    base = _run(robot, lambda p: p.setInputParams(late))
    again = _run(robot, lambda p: p.setInputParams(late), during=restart)
    for n in range(STEPS):
        for b, k in enumerate(K):
            first = AT if MASK[b] and n >= AT else 0
            for r, c in zip(ROWS, _cmd(robot, max(n - k, first))):
                assert np.array_equal(_bits(again[1][n][r][b]), _bits(c[b])), (n, b, r)
            if not MASK[b]:
                assert all(np.array_equal(again[0][n][key][b], base[0][n][key][b], equal_nan=True) for key in base[0][n]), (n, b)
        assert again[2][n]["tick"].tolist() == [n + 1] * B
        assert again[2][n]["steps"].tolist() == [n + 1 - (AT if MASK[b] and n >= AT else 0) for b in range(B)]


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import bipedal_control_amd as bp
    INVALID, CAPACITY = -1, -6
    robot = "h1"
    plant = _plant(robot)

    def refused(call, status, *words):
        with pytest.raises(bp.BpmpcError) as e:
            call()
        assert e.value.status == status and all(w in str(e.value) for w in words), str(e.value)

    refused(plant.applied, INVALID, "bpmpc_plant_applied_command", "untouched")
    rows = _every_field()
    plant.setInputParams(rows)
    refused(plant.applied, INVALID, "bpmpc_plant_applied_command", "no step has run")
    for field, bad, what in (("delay", -0.001, "negative"), ("dropout", 1.5, "above 1"), ("push_force", np.nan, "not finite"), ("push_interval", np.inf, "not finite"),
                             ("push_duration", -1.0, "negative")):
        wrong = rows.copy()
        wrong[2, ir.FIELDS.index(field)] = bad
        refused(lambda: plant.setInputParams(wrong), INVALID, "row 2", field, what)
    wrong = rows.copy()
    wrong[4, 6] = 1.0
    refused(lambda: plant.setInputParams(wrong), INVALID, "row 4", "reserved", "not zero")
    assert all(np.array_equal(plant.getInputParams(b), rows[b]) for b in range(B))      # no refusal changed a row
    wrong[4, 6] = 0.0
    wrong[4, 0] = -1.0
    plant.setInputParams(wrong, mask=MASK)                                              # a bad row nobody takes is not looked at
    assert np.array_equal(plant.getInputParams(4), rows[4])
    refused(lambda: plant.setInputParams(np.zeros((MAXB + 1, 8))), CAPACITY, "max_batch")
    refused(lambda: plant.seedInputs(1, mask=np.ones(MAXB + 1, np.int32)), CAPACITY, "max_batch")
    refused(lambda: plant._call("bpmpc_plant_get_input_state", MAXB + 1, None, None, None, None), CAPACITY, "max_batch")
    refused(lambda: plant._call("bpmpc_plant_get_input_params", MAXB, ir.row().ctypes.data_as(bp.api._dp)), CAPACITY, "max_batch")
    plant._call("bpmpc_plant_get_input_state", B, None, None, None, None)               # every pointer is nullable
    # the step still runs, and then there is an applied command
    plant.set_state(_fleet(robot)[0])
    plant.step(*_cmd(robot, 0), period=PERIOD, substeps=SUBSTEPS)
    assert set(plant.applied()) == set(ROWS) | {"base_force"}


# ---------------------------------------------------------------------------------------------------------------- the loop
def test_delayed_lossy_loop_stays_finite():
    """50 ticks of step_controlled -> update_from_plant -> tick_estimated under the delay of the reference's H1 file (gazebo/delay, 9 ms: four
    control steps) with 5 % packet loss: everything stays finite.  No bound on tracking is asserted: nobody has measured one; the figures are
    printed."""
    text = open(os.path.join(ROOT, "tests", "golden", "reference", "bipedal_robot_example", "unitree_h1", "h1_description", "config", "hw_sim.yaml")).read()
    delay = float(re.search(r"^\s*delay:\s*([0-9.eE+-]+)\s*$", text, flags=re.M).group(1))
    assert delay == 0.009
    lp = tp._Loop()
    NB, TICKS50, REARM = tp.NB, tp.TICKS, tp.REARM
    lp.plant.setInputParams(ir.row(delay=delay, dropout=0.05))
    lp.plant.seedInputs(2026)
    lp.plant.set_state(lp.rbd0)
    lp.arm(0.0, True)
    t = torch.zeros(NB, dtype=torch.float64, device="cuda")
    times = [torch.full((NB,), PERIOD * (k + 1), dtype=torch.float64, device="cuda") for k in range(TICKS50)]
    torch.cuda.synchronize()
    lp.ctrl.tick(t, lp.plant.outputs()["rbd"].torch(), period=PERIOD, fetch=False)
    losses = 0
    for k in range(TICKS50):
        lp.plant.step_controlled(lp.ctrl, period=PERIOD, substeps=SUBSTEPS)
        lp.est.update_from_plant(lp.plant, period=PERIOD, fetch=False)
        lp.ctrl.tick_estimated(times[k], lp.est, period=PERIOD, fetch=False)
        if k % REARM == REARM - 1:
            lp.arm(PERIOD * (k + 1), False)
            torch.cuda.synchronize()
            shot = lp.snapshot()
            shot.update(_applied(lp.plant))
            assert all(np.all(np.isfinite(np.asarray(a, float))) for a in shot.values()), k
            losses += int(lp.plant.inputState()["lost"].sum())
    state = lp.plant.inputState()
    assert state["tick"].tolist() == [TICKS50] * NB and state["delay_steps"].tolist() == [4] * NB
    print("delayed loop: base height", shot["odom_pos"][:, 2], "safe", shot["safe"], "losses seen at the re-arm points", losses)
