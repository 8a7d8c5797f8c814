"""GPU tier: the plant's joint model (include/bpmpc.h "Plant", joints; kernels/plant.h JOINT, k_plant_joint_step) against the numpy restatement
tests/plant_joint_reference.py and against known answers.
  one substep      H1 and G1, the five robots of test_plant_joint_reference.joint_cases: the neutral row; armature and damping only; friction with
                   one joint at exactly zero velocity; a joint beyond its upper limit; a joint beyond its lower limit with kt > 0 and closed
                   contacts.  Every output, the anchors and the flags at test_gpu_plant.TOL
  twenty substeps  one launch of 20 substeps against 20 restatement substeps at 100 x the restatement's own floor measured in the run (the factor of
                   test_gpu_plant); twenty launches of one substep: the same bits
  free fall        the known answer of test_plant_joint_reference on the device: 200 control steps of 4 substeps, both stops within 1e-6 rad of
                   q* = (kp hold + k_limit limit) / (kp + k_limit), no contact closes
  neutral rows     robots with the neutral row inside k_plant_joint_step against the same robots on a handle that runs k_plant_stick_step: within
                   TOL; whether the bits are equal is printed
  masks            rows set under a mask, once the kernel is already the joint kernel, leave every other robot's state, outputs and anchors bit
                   for bit; two runs agree bit for bit; host rows and device rows the same bits; reset_joint_params returns to the start row
  parent bits      an untouched handle, one on which only get_joint_params was called, one after reset_joint_params and one after refused calls
                   reproduce tests/golden/plant_parent_bits.npz
  refusals         capacity, bad host rows that change nothing, null pointers
  the other doors  one step through step_controlled and step_supervised with joint rows set gives the bits of step on the gathered command
No decision of a compared case is left to rounding (joint_reference asserts it).  Every comparison prints its maximum before it asserts (pytest -s)."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

from oracle import wbc_py as wp
from tests import oracle_bridge as ob
from tests import plant_joint_reference as jr
from tests import plant_reference as pr
from tests import test_gpu_plant as tp
from tests import test_plant_joint_reference as jc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plant_parent_bits.npz")
H = jc.H
INVALID, CAPACITY = -1, -6


def _everything(plant):
    """every output, the state, the anchors and the flags as numpy arrays"""
    out = tp._read(plant)
    out["state"] = plant.get_state()
    out["anchor"], out["anchored"] = plant.anchors()
    return out


def _same(a, b, rows=slice(None)):
    return all(np.array_equal(a[k][rows], b[k][rows], equal_nan=True) for k in a)


def _start(robot, rows=None, kt=None, device=False):
    """a plant on the states of joint_cases with its joint rows and stiffnesses (or the given ones) set"""
    m = ob.model(robot)
    q, v, cmd, force, ground, case_rows, case_kt = jc.joint_cases(robot)
    rows = case_rows if rows is None else rows
    plant = tp._plant(robot, tp.B5)
    plant.setStiction(case_kt if kt is None else kt)
    if device:
        d_rows = torch.tensor(rows, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        plant.setJointParams(d_rows)
    else:
        plant.setJointParams(rows)
    plant.set_state(np.array([wp.rbd_from(m, q[b], v[b]) for b in range(tp.B5)]))
    return plant, cmd, force, ground


def _step(plant, cmd, force, ground, substeps, launches=1):
    for _ in range(launches):
        plant.step(cmd["pos_des"], cmd["vel_des"], cmd["tau_ff"], cmd["kp"], cmd["kd"], base_force=force, feet_heights=ground, period=H * substeps, substeps=substeps)
    return _everything(plant)


def _compare(robot, out, steps, ground, tol, what):
    """every output of the device, the anchors and the flags against the restatement's last substep; the maxima by key"""
    m = ob.model(robot)
    worst = {}
    for b in range(tp.B5):
        s = steps[b][-1]
        ref = pr.sensors(m, s, ground=ground[b])
        assert np.array_equal(out["contact"][b], ref["contact"]), (robot, b, out["contact"][b], ref["contact"])
        assert np.array_equal(out["anchored"][b], s["anchored"]), (robot, b, out["anchored"][b], s["anchored"])
        qd, vd = wp.measured_state(m, out["rbd"][b])
        worst["q+"] = max(worst.get("q+", 0.0), tp._rel(qd, s["q"]))
        worst["v+"] = max(worst.get("v+", 0.0), tp._rel(vd, s["v"]))
        on = s["anchored"] != 0
        worst["anchor"] = max(worst.get("anchor", 0.0), tp._rel(out["anchor"][b][on], s["anchor"][on]) if on.any() else 0.0)
        for k in tp.SENSORS:
            if k != "contact":
                worst[k] = max(worst.get(k, 0.0), tp._rel(out[k][b], ref[k]))
    print("joints", robot, what, {k: "%.2e" % x for k, x in worst.items()})
    assert max(worst.values()) < tol, worst


# ---------------------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_one_substep_matches_restatement(robot):
    steps, floor = jc.joint_reference(robot, 1)
    print("restatement floor", robot, floor)
    plant, cmd, force, ground = _start(robot)
    _compare(robot, _step(plant, cmd, force, ground, 1), steps, ground, tp.TOL, "one substep")
    for b in range(tp.B5):
        assert np.array_equal(plant.getJointParams(b), jc.joint_cases(robot)[5][b])


def test_twenty_substeps_in_one_launch():
    """Tolerance: 100 x the restatement's own floor over the twenty substeps (the largest difference of v+ between numpy.linalg.solve and a Cholesky
    solve of the same system, relative to max(1, |v+|)), measured and printed in the run: 5.0e-15 here, so 5.0e-13.  Twenty launches of one
    substep give the bits of one launch of twenty, anchors and flags among them."""
    robot = "h1"
    steps, floor = jc.joint_reference(robot, tp.SUBSTEPS)
    tol = 100 * floor
    print("restatement floor over", tp.SUBSTEPS, "substeps", floor, "tolerance", tol)
    plant, cmd, force, ground = _start(robot)
    one = _step(plant, cmd, force, ground, tp.SUBSTEPS)
    _compare(robot, one, steps, ground, tol, "twenty substeps")
    plant, cmd, force, ground = _start(robot)
    many = _step(plant, cmd, force, ground, 1, launches=tp.SUBSTEPS)
    for k in one:
        assert np.array_equal(one[k], many[k]), k


# ---------------------------------------------------------------------------------------------------------------- a known answer
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_free_fall_known_answer(robot):
    m = ob.model(robot)
    nj = m["nj"]
    q, v, cmd, row, target = jc.free_fall_case(m)
    B = 2
    plant = tp._plant(robot, B)
    plant.setJointParams(row)
    plant.set_state(np.tile(wp.rbd_from(m, q, v), (B, 1)))
    arrays = [np.tile(cmd[k], (B, 1)) for k in ("pos_des", "vel_des", "tau_ff", "kp", "kd")]
    ground = np.full((B, 4), jc.GROUND)
    closed = 0
    for _ in range(jc.FREE_FALL_SUBSTEPS // 4):
        plant.step(*arrays, feet_heights=ground, period=4 * H, substeps=4)
        plant.get_state()
        closed += int(plant.outputs()["contact"].torch().cpu().numpy().any())
    out = _everything(plant)
    joints = out["joint_pos"]
    stops = [3, nj - 1]
    err = np.abs(joints - target)
    print("free fall on the device", robot, "|q - q*| at the two stops", err[:, stops].max(axis=0), "rad; the other joints from hold", np.delete(err, stops, axis=1).max(),
          "rad; base height", out["odom_pos"][:, 2])
    assert closed == 0 and not out["contact_force"].any()
    assert np.all(err[:, stops] < 1e-6), err[:, stops]
    assert np.array_equal(joints[0], joints[1])


# ---------------------------------------------------------------------------------------------------------------- neutral rows in the joint kernel
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_neutral_rows_in_the_joint_kernel(robot):
    """The same five robots with kt = (0, 0, 0, kn, kn) on a handle that runs k_plant_stick_step and on one that runs k_plant_joint_step with every
    row neutral, twenty substeps: within TOL.  Whether the bits are equal is printed, not asserted; include/bpmpc.h promises rounding only."""
    m = ob.model(robot)
    q, v, cmd, force, ground = tp._cases(robot)
    kt = np.array([0.0, 0.0, 0.0, pr.DEFAULT_ROW[0], pr.DEFAULT_ROW[0]])
    rbd = np.array([wp.rbd_from(m, q[b], v[b]) for b in range(tp.B5)])
    stick = tp._plant(robot, tp.B5)
    stick.setStiction(kt)
    stick.set_state(rbd)
    joint = tp._plant(robot, tp.B5)
    joint.setStiction(kt)
    joint.setJointParams(jr.neutral_row())
    joint.set_state(rbd)
    a, b = _step(stick, cmd, force, ground, tp.SUBSTEPS), _step(joint, cmd, force, ground, tp.SUBSTEPS)
    worst = {k: tp._rel(b[k], a[k]) for k in a}
    print("neutral rows in k_plant_joint_step against k_plant_stick_step", robot, "bits equal:", _same(a, b), {k: "%.2e" % x for k, x in worst.items() if x})
    assert np.array_equal(a["contact"], b["contact"]) and np.array_equal(a["anchored"], b["anchored"]) and a["anchored"][3:].any()
    assert max(worst.values()) < tp.TOL, worst


# ---------------------------------------------------------------------------------------------------------------- masks and determinism
def _run(change_at=None, device=False, steps=5):
    """everything after each of `steps` control steps of 4 substeps; change_at: the step before which robots 1 and 4 get another row"""
    robot = "h1"
    nj = ob.model(robot)["nj"]
    plant, cmd, force, ground = _start(robot, device=device)
    mask = np.array([0, 1, 0, 0, 1], np.int32)
    other = jr.joint_row(nj, armature=0.3, damping=4.0, friction_loss=0.5, upper=jc.joint_cases(robot)[0][1, 6:] - 0.01)
    shots = []
    for k in range(steps):
        if change_at == k:
            plant.setJointParams(other, mask=mask)
        shots.append(_step(plant, cmd, force, ground, 4))
    return shots, plant, mask, other


def test_masks_and_determinism():
    a, plant, mask, other = _run()
    assert all(np.all(np.isfinite(s["state"])) for s in a)
    b, _, _, _ = _run()
    d, _, _, _ = _run(device=True)
    assert all(_same(x, y) for x, y in zip(a, b)) and all(_same(x, y) for x, y in zip(a, d))
    c, changed, _, _ = _run(change_at=2)
    keep = mask == 0
    assert all(_same(x, y, keep) for x, y in zip(a, c)) and all(_same(x, y) for x, y in zip(a[:2], c[:2]))
    assert all(not np.array_equal(a[-1]["state"][i], c[-1]["state"][i]) for i in np.nonzero(mask)[0])
    rows = jc.joint_cases("h1")[5]
    for i in range(tp.B5):
        assert np.array_equal(changed.getJointParams(i), other if mask[i] else rows[i])
    assert np.array_equal(changed.getJointParams(), jr.neutral_row())
    # reset: every row the start row again, and the handle steps in the kernel it was created with
    changed.resetJointParams()
    changed.resetStiction()
    assert all(np.array_equal(changed.getJointParams(i), jr.neutral_row()) for i in range(tp.B5))
    gold = np.load(GOLDEN)
    tp._set_and_step(changed, "h1", tp.PERIOD, tp.SUBSTEPS)
    out = _everything(changed)
    for k in ("state",) + tp.SENSORS:
        assert np.array_equal(out[k], gold["h1_" + k]), k


# ---------------------------------------------------------------------------------------------------------------- the parent's bits
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_untouched_handles_keep_the_parent_bits(robot):
    gold = np.load(GOLDEN)
    for looked_at in (False, True):
        plant = tp._plant(robot, tp.B5)
        if looked_at:
            assert np.array_equal(plant.getJointParams(), jr.neutral_row()) and np.array_equal(plant.getJointParams(2), jr.neutral_row())
        tp._set_and_step(plant, robot, tp.PERIOD, tp.SUBSTEPS)
        out = _everything(plant)
        for k in ("state",) + tp.SENSORS:
            assert out[k].dtype == gold[robot + "_" + k].dtype and np.array_equal(out[k], gold[robot + "_" + k]), (robot, looked_at, k)
        assert not out["anchored"].any() and not out["anchor"].any()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import bipedal_control_amd as bp
    lib = bp.load_library()
    robot = "h1"
    nj = ob.model(robot)["nj"]
    plant = tp._plant(robot, tp.B5)

    def status(call):
        with pytest.raises(bp.BpmpcError) as e:
            call()
        return e.value.status, lib.bpmpc_last_error().decode()

    good = jr.joint_row(nj, armature=0.1, damping=1.0, lower=-1.0, upper=1.0)
    assert status(lambda: plant.setJointParams(np.tile(good, (tp.B5 + 1, 1))))[0] == CAPACITY
    assert status(lambda: plant.getJointParams(tp.B5))[0] == CAPACITY
    for entry, bad, name in ((3, -0.1, "armature[3]"), (12 + 9, np.inf, "damping[9]"), (24, np.nan, "friction_loss[0]"), (36 + 2, 1.0, "upper[2]"),
                             (48 + 2, -np.inf, "upper[2]"), (60, -1.0, "k_limit"), (61, np.nan, "c_limit"), (62, 0.0, "w_eps"), (63, 1.0, "reserved")):
        rows = np.tile(good, (tp.B5, 1))
        rows[3, entry] = bad
        code, msg = status(lambda: plant.setJointParams(rows))
        assert code == INVALID and name in msg and "row 3" in msg, msg
        assert plant.setJointParams(rows, mask=np.array([1, 1, 1, 0, 1], np.int32)) is None      # a row no robot takes is not looked at
        plant.resetJointParams()
    from bipedal_control_amd.api import _d
    rows = np.tile(good, (3, 1))
    assert lib.bpmpc_plant_set_joint_params(plant._h, tp.B5, None, _d(rows), 3, 0) == INVALID and b"n_rows" in lib.bpmpc_last_error()
    assert lib.bpmpc_plant_set_joint_params(plant._h, tp.B5, None, None, 1, 0) == INVALID and b"null" in lib.bpmpc_last_error()
    assert lib.bpmpc_plant_set_joint_params(None, tp.B5, None, _d(rows), 1, 0) == INVALID and b"null" in lib.bpmpc_last_error()
    assert lib.bpmpc_plant_get_joint_params(plant._h, 0, None) == INVALID and b"null" in lib.bpmpc_last_error()
    assert lib.bpmpc_plant_set_joint_params(plant._h, 0, None, _d(rows), 1, 0) == INVALID
    # a refusal on a handle in use changes neither a row nor the state, and an untouched handle stays untouched
    used, cmd, force, ground = _start(robot)
    _step(used, cmd, force, ground, 4)
    before = _everything(used)
    rows_before = [used.getJointParams(i) for i in range(tp.B5)]
    bad = np.tile(good, (tp.B5, 1))
    bad[4, 48 + 1] = bad[4, 36 + 1]      # lower = upper
    code, msg = status(lambda: used.setJointParams(bad))
    assert code == INVALID and "upper[1]" in msg and "not above lower" in msg
    assert _same(before, _everything(used)) and all(np.array_equal(used.getJointParams(i), rows_before[i]) for i in range(tp.B5))
    fresh = tp._plant(robot, tp.B5)
    assert status(lambda: fresh.setJointParams(bad))[0] == INVALID and status(lambda: fresh.setJointParams(np.tile(good, (tp.B5 + 1, 1))))[0] == CAPACITY
    gold = np.load(GOLDEN)
    tp._set_and_step(fresh, robot, tp.PERIOD, tp.SUBSTEPS)
    out = _everything(fresh)
    for k in ("state",) + tp.SENSORS:
        assert np.array_equal(out[k], gold[robot + "_" + k]), k


# ---------------------------------------------------------------------------------------------------------------- the other two doors
@pytest.mark.parametrize("door", ["controlled", "supervised"])
def test_the_other_doors(door):
    """bpmpc_plant_step is the door of every other test here.  One step of the closed loop of tests/test_gpu_supervisor.py through step_controlled or
    step_supervised, joint rows set (the MJCF defaults, finite limits, joint 3 of robots 1 and 3 beyond its upper limit), against a twin plant
    with the same rows and state that takes the gathered command through step: the same bits."""
    from tests import supervisor_reference as sr
    from tests import test_gpu_supervisor as ts
    lp = ts.Loop()
    nj, NB = lp.nj, ts.NB
    joints = lp.rbd0[:, 6:6 + nj]
    rows = np.array([jc.mjcf_row(nj, lower=joints[b] - 0.4, upper=joints[b] + 0.4) for b in range(NB)])
    rows[1, jr.UPPER + 3] = joints[1, 3] - 0.02
    rows[3, jr.UPPER + 3] = joints[3, 3] - 0.01
    lp.plant.setJointParams(rows)
    lp.start()
    if door == "supervised":
        lp.sup.request(sr.RUN)
        lp.sup.update_controlled(lp.ctrl, rbd=lp.plant.outputs()["rbd"].torch(), period=ts.PERIOD)
    torch.cuda.synchronize()
    if door == "supervised":
        s = lp.sup.state(NB, commands=True)
        given = [s[r].copy() for r in ("pos_des", "vel_des", "tau_ff", "kp", "kd")]
        lp.plant.step_supervised(lp.sup, period=ts.PERIOD, substeps=4)
    else:
        o = {key: v.torch().cpu().numpy().copy() for key, v in lp.ctrl.device_outputs().items() if key in ("joint_cmd", "joint_kp", "joint_kd")}
        given = [o["joint_cmd"][:, 0].copy(), o["joint_cmd"][:, 1].copy(), o["joint_cmd"][:, 2].copy(), o["joint_kp"], o["joint_kd"]]
        lp.plant.step_controlled(lp.ctrl, period=ts.PERIOD, substeps=4)
    torch.cuda.synchronize()
    got = _everything(lp.plant)
    twin = tp._plant("h1", NB)
    twin.setJointParams(rows)
    twin.set_state(lp.rbd0)
    twin.step(*given, period=ts.PERIOD, substeps=4)
    want = _everything(twin)
    plain = tp._plant("h1", NB)
    plain.set_state(lp.rbd0)
    plain.step(*given, period=ts.PERIOD, substeps=4)
    moved = tp._rel(_everything(plain)["state"], want["state"])
    print("door", door, "bits equal:", _same(got, want), "; the joint rows move the state by", moved)
    assert all(np.all(np.isfinite(np.asarray(a, float))) for a in got.values())
    assert _same(got, want)
    assert moved > 1e-6      # the rows do change what the step does: the comparison above can fail
