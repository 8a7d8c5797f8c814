"""GPU tier: the plant's stick-slip contacts (include/bpmpc.h "Plant", step 2 with kt > 0; kernels/plant.h STICK, k_plant_stick_step) against the
numpy restatement tests/plant_stiction_reference.py and against the bits of the plant as it was before it had them.
  parent's bits    tests/golden/plant_parent_bits.npz holds what k_plant_step gave on an MI355X at the commit before stiction (the five robots of
                   test_gpu_plant._cases, one launch of 20 substeps, H1 and G1; tests/golden/make_plant_parent_bits.py).  A handle that never heard
                   of stiction reproduces it bit for bit, and so does one with setStiction(0), which runs k_plant_stick_step; every flag stays 0.
  restatement      kt = kn, the scenario of tests/test_plant_stiction_reference.py (sticking, slipping, opening, re-closing points, an airborne robot;
                   every decision decisive - asserted there from the restatement alone).  One substep at a time at 1e-9; 20 substeps in one launch
                   and the two launches behind it at 100 x the restatement's own floor; every output, the anchors and the flags.  Twenty launches
                   of one substep give the bits of one launch of twenty.
  the foot holds   eight standing H1 under a constant horizontal push at mu = 0.1: the robots with kt = kn stop slipping, the others creep
  masks            setStiction on a mask from host arrays and from device tensors; a masked set_state clears the anchors of its robots only
  refusals
Every comparison prints its maximum before it asserts (pytest -s)."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

from oracle import wbc_py as wp
from tests import oracle_bridge as ob
from tests import plant_reference as pr
from tests import test_gpu_plant as tp
from tests import test_plant_stiction_reference as sc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plant_parent_bits.npz")
KT = sc.KT
H = sc.H


def _everything(plant):
    """every output, the state, the anchors and the flags as numpy arrays"""
    out = tp._read(plant)
    out["state"] = plant.get_state()
    out["anchor"], out["anchored"] = plant.anchors()
    return out


# ---------------------------------------------------------------------------------------------------------------- the parent's bits
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_parent_bits(robot):
    gold = np.load(GOLDEN)
    for touched in (False, True):
        plant = tp._plant(robot, tp.B5)
        if touched:
            plant.setStiction(0.0)
            assert plant.getStiction(0) == 0.0
        tp._set_and_step(plant, robot, tp.PERIOD, tp.SUBSTEPS)
        out = _everything(plant)
        for k in ("state",) + tp.SENSORS:
            assert out[k].dtype == gold[robot + "_" + k].dtype and np.array_equal(out[k], gold[robot + "_" + k]), (robot, touched, k)
        assert not out["anchored"].any() and not out["anchor"].any()


# ---------------------------------------------------------------------------------------------------------------- against the restatement
def _start(robot):
    m = ob.model(robot)
    q, v, cmd, force, _ = tp._cases(robot)
    plant = tp._plant(robot, tp.B5)
    plant.setStiction(KT)
    plant.set_state(np.array([wp.rbd_from(m, q[b], v[b]) for b in range(tp.B5)]))
    assert plant.getStiction(3) == KT and plant.getStiction() == 0.0
    return plant, cmd, force


def _step(plant, cmd, force, ground, substeps, launches=1):
    for _ in range(launches):
        plant.step(cmd["pos_des"], cmd["vel_des"], cmd["tau_ff"], cmd["kp"], cmd["kd"], base_force=force, feet_heights=ground, period=H * substeps, substeps=substeps)
    return _everything(plant)


def _compare(robot, out, steps, index, ground, tol, what, tol_force=None):
    """every output of the device, the anchors and the flags against the restatement's substep `index`; the maxima by key.  tol_force: the bound of
    contact_force where it is not tol"""
    m = ob.model(robot)
    worst = {}
    for b in range(tp.B5):
        s = steps[b][index]
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
    print("stiction", robot, what, {k: "%.2e" % x for k, x in worst.items()})
    assert max(x for k, x in worst.items() if k != "contact_force") < tol and worst["contact_force"] < (tol_force or tol), worst


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_one_substep_at_a_time_matches_restatement(robot):
    """Three launches of one substep, compared after each at 1e-9 relative to max(1, |value|) (test_gpu_plant.TOL): the first anchors every closed
    point (s = 0), the second and third decide between stick and slip on those anchors."""
    steps, floor, _ = sc.stiction_reference("h1") if robot == "h1" else sc.stiction_reference("g1", (3, 0, 0))
    stick = np.array([[s["stick"] for s in rows[:3]] for rows in steps])
    print("restatement floor", robot, floor, "decisions over three substeps: stick", int((stick == 1).sum()), "slip", int((stick == 0).sum()))
    assert (stick[:, 1:] == 1).any() and (stick[:, 1:] == 0).any()
    ground = sc.grounds(robot)[0]
    plant, cmd, force = _start(robot)
    for k in range(3):
        _compare(robot, _step(plant, cmd, force, ground, 1), steps, k, ground, tp.TOL, "substep %d" % k)


def test_twenty_substeps_and_two_more_launches():
    """Tolerance: 100 x the restatement's own floor over the 24 substeps of the scenario - the largest difference of v+ between numpy.linalg.solve
    and a Cholesky solve of the same system, relative to max(1, |v+|) - measured and printed in the run (8.7e-15 here, so 8.7e-13).  The launch of
    twenty substeps is held to it in every output, anchors and contact forces among them (the device's largest figure: 4.1e-13,
    linear_accel_local; contact forces 3.0e-13).
    The two launches behind it (2 substeps with robot 2's left foot over lowered ground, 2 substeps with it closed again) are held to it in every
    output but the contact forces.  Those were first held to it too, and missed: 4.4e-13 after 22 substeps, 1.37e-12 after 24, against 8.66e-13,
    with v+ at 1.6e-14.  The bound is below what the restatement knows of a contact force: f - D J v+ multiplies the solvers' difference in v+ by
    D, up to mu n / v_eps = 1e4 N s/m, and the restatement's two solvers alone differ by up to 8.8e-13 in a contact force of ONE substep from the
    same state (stiction_reference's third value, measured in the run).  So the contact forces of the two follow-on launches are held to
    100 x that figure, the restatement's own floor for the quantity compared, as the issue's rule is for v+."""
    robot = "h1"
    steps, floor, floor_force = sc.stiction_reference(robot)
    tol = 100 * floor
    print("restatement floor over", len(steps[0]), "substeps", floor, "tolerance", tol, "floor of the contact forces", floor_force)
    plant, cmd, force = _start(robot)
    at, first = 0, None
    for n, ground in zip(sc.LAUNCHES, sc.grounds(robot)):
        out = _step(plant, cmd, force, ground, n)
        at += n
        _compare(robot, out, steps, at - 1, ground, tol, "after %d substeps" % at, tol_force=None if first is None else 100 * floor_force)
        first = first or out
    # twenty launches of one substep: the bits of one launch of twenty, anchors and flags among them
    plant, cmd, force = _start(robot)
    many = _step(plant, cmd, force, sc.grounds(robot)[0], 1, launches=sc.LAUNCHES[0])
    for k in first:
        assert np.array_equal(first[k], many[k]), k


# ---------------------------------------------------------------------------------------------------------------- the foot holds
HOLD_KP, HOLD_KD, HOLD_MU, HOLD_PUSH = 2.0e4, 2.0e2, 0.1, 0.05


def test_the_foot_holds():
    """Eight H1 on standing_state (soles 2.5 mm in the ground), the joints held by a PD of 2e4 / 2e2, mu = 0.1, a constant push of 0.05 m g along x on
    the base: a tangential load of half the friction the weight affords (rho = 0.5).  250 control steps of 2 ms in 4 substeps.  Robots 0..3 have
    kt = 0 and creep; robots 4..7 have kt = kn: their points slip while the stance settles and then hold - closed, anchored, the anchors at step 250
    the bits of step 50 - and move less than half as far between steps 50 and 250 as the robots without.
    The restatement alone (tests/plant_stiction_reference.py, one robot of each kind on the CPU, the same force and gains, here at the full 250
    steps and not a shortened length): with kt = kn the last slip was in control step 21, from then on kt |s| stayed between 9.3 and 11.8 N under
    caps of 11 to 14 N, the anchors at steps 50 and 250 were equal, and the mean contact-point displacement between them was 0.023 mm against
    2.01 mm with kt = 0 (closed-form creep 0.4 s v_eps rho / sqrt(1 - rho^2) = 2.31 mm).  With a PD of 2000 / 40 the joints sag for 0.15 s and the
    feet slip until control step 75: the stiffer PD is what settles the stance before step 50."""
    from tests.test_plant_reference import standing_state
    B = 8
    m = ob.model("h1")
    nj = m["nj"]
    q, v, _ = standing_state(m, depth=0.0025)
    mg = m["mass"].sum() * pr.GRAVITY
    plant = tp._plant("h1", B)
    row = pr.DEFAULT_ROW.copy()
    row[3] = HOLD_MU
    plant.setParams(row)
    plant.setStiction(np.r_[np.zeros(4), np.full(4, row[0])])
    plant.set_state(np.tile(wp.rbd_from(m, q, v), (B, 1)))
    cmd = [np.tile(q[6:], (B, 1)), np.zeros((B, nj)), np.zeros((B, nj)), np.full((B, nj), HOLD_KP), np.full((B, nj), HOLD_KD)]
    force = np.tile([HOLD_PUSH * mg, 0.0, 0.0], (B, 1))
    shots = {}
    for k in range(1, 251):
        plant.step(*cmd, base_force=force, period=0.002, substeps=4)
        if k in (50, 250):
            shots[k] = _everything(plant)

    def points(out):
        p = []
        for b in range(B):
            qb, _ = wp.measured_state(m, out["rbd"][b])
            R, o, _ = wp.fk(m, qb)
            p.append(np.array(wp.contact_points(m, R, o))[:, :2])
        return np.array(p)

    moved = np.linalg.norm(points(shots[250]) - points(shots[50]), axis=2).mean(axis=1)      # per robot, mean over its four points
    rho = HOLD_PUSH / HOLD_MU
    print("mean contact-point displacement between steps 50 and 250 [m]: kt = 0", moved[:4], "kt = kn", moved[4:], "closed-form creep",
          0.4 * row[4] * rho / np.sqrt(1.0 - rho ** 2))
    assert np.all(np.isfinite(shots[250]["state"]))
    for k in (50, 250):
        assert shots[k]["contact"][4:].all() and shots[k]["anchored"][4:].all(), (k, shots[k]["contact"], shots[k]["anchored"])
        assert not shots[k]["anchored"][:4].any()
    assert np.array_equal(shots[250]["anchor"][4:], shots[50]["anchor"][4:])
    assert moved[4:].mean() < 0.5 * moved[:4].mean(), moved


# ---------------------------------------------------------------------------------------------------------------- masks and determinism
B8, STEPS8 = 8, 6


def _run8(device=False, stiction=True):
    """the first eight robots of test_gpu_plant._fleet67 for six control steps: states [steps, 8, 2 nv], anchors and flags after every step"""
    rbd, cmd, force, ground, _ = tp._fleet67()
    plant = tp._plant("h1", B8)
    dev = (lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device="cuda")) if device else (lambda a, dt=None: a)
    arrays = [dev(a[:B8]) for a in cmd] + [dev(force[:B8]), dev(ground[:B8])]
    mask = (np.arange(B8) % 3 == 0).astype(np.int32)
    kt = KT * (1.0 + 0.1 * np.arange(B8))
    if device:
        torch.cuda.synchronize()
    if stiction:
        plant.setStiction(dev(kt), mask=dev(mask, torch.int32) if device else mask)
    plant.set_state(dev(rbd[:B8]))
    states, anchors, flags = [], [], []
    for k in range(STEPS8):
        plant.step(*arrays[:5], base_force=arrays[5], feet_heights=arrays[6], period=0.002, substeps=4)
        states.append(plant.get_state())
        a, f = plant.anchors()
        anchors.append(a)
        flags.append(f)
    assert [plant.getStiction(b) for b in range(B8)] == [kt[b] if stiction and mask[b] else 0.0 for b in range(B8)]
    return np.array(states), np.array(anchors), np.array(flags), mask


def test_masks_and_determinism():
    a = _run8()
    mask = a[3]
    keep = mask == 0
    assert np.all(np.isfinite(a[0])) and a[2][:, ~keep].any() and not a[2][:, keep].any()
    for other in (_run8(), _run8(device=True)):                      # repeated; from device tensors
        assert all(np.array_equal(x, y) for x, y in zip(a, other))
    plain = _run8(stiction=False)                                    # a handle that never heard of stiction: the robots outside the mask go on bit for bit
    assert np.array_equal(plain[0][:, keep], a[0][:, keep]) and not plain[2].any()
    assert all(not np.array_equal(plain[0][:, i], a[0][:, i]) for i in np.nonzero(mask)[0])
    # a masked set_state clears the anchors of its robots only; the others' later states are those of a run without it
    for device in (False, True):
        rbd, cmd, force, ground, other = tp._fleet67()
        runs = []
        for at in (None, 3):
            plant = tp._plant("h1", B8)
            plant.setStiction(KT)
            plant.set_state(rbd[:B8])
            states = []
            for k in range(STEPS8):
                if at == k:
                    dev = (lambda x, dt: torch.tensor(x, dtype=dt, device="cuda")) if device else (lambda x, dt: x)
                    args = dev(other[:B8], torch.float64), dev(mask, torch.int32)
                    if device:
                        torch.cuda.synchronize()
                    before = plant.anchors()
                    plant.set_state(args[0], mask=args[1])
                    after = plant.anchors()
                    assert before[1][keep].any() and before[1][~keep].any()
                    assert not after[1][~keep].any() and not after[0][~keep].any()
                    assert np.array_equal(after[0][keep], before[0][keep]) and np.array_equal(after[1][keep], before[1][keep])
                plant.step(*[x[:B8] for x in cmd], base_force=force[:B8], feet_heights=ground[:B8], period=0.002, substeps=4)
                states.append(plant.get_state())
            runs.append(np.array(states))
        assert np.array_equal(runs[0][:, keep], runs[1][:, keep]) and np.array_equal(runs[0][:3], runs[1][:3])
        assert all(not np.array_equal(runs[0][3:, i], runs[1][3:, i]) for i in np.nonzero(mask)[0])
    # changing kt clears the anchors of the robots it changes; resetStiction clears everything
    plant = tp._plant("h1", B8)
    plant.setStiction(KT)
    plant.set_state(tp._fleet67()[0][:B8])
    rbd, cmd, force, ground, _ = tp._fleet67()
    plant.step(*[x[:B8] for x in cmd], base_force=force[:B8], feet_heights=ground[:B8], period=0.002, substeps=4)
    before = plant.anchors()
    assert before[1].any(axis=1).all()
    plant.setStiction(np.where(mask != 0, 2.0 * KT, KT))            # the robots outside the mask are given the value they have
    after = plant.anchors()
    assert not after[1][~keep].any() and np.array_equal(after[1][keep], before[1][keep]) and np.array_equal(after[0][keep], before[0][keep])
    plant.resetStiction()
    assert not plant.anchors()[1].any() and [plant.getStiction(b) for b in range(B8)] == [0.0] * B8


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import bipedal_control_amd as bp
    INVALID, CAPACITY = -1, -6
    rbd, cmd, force, ground, _ = tp._fleet67()
    plant = tp._plant("h1", 5)
    kt0 = KT * np.arange(1.0, 6.0)
    plant.setStiction(kt0)
    plant.set_state(rbd[:5])
    plant.step(*[a[:5] for a in cmd], base_force=force[:5], feet_heights=ground[:5])
    anchors = plant.anchors()
    assert anchors[1].any()
    lib = bp.load_library()

    def refused(call, status, word=None):
        with pytest.raises(bp.BpmpcError) as e:
            call()
        assert e.value.status == status, (e.value.status, lib.bpmpc_last_error())
        assert word is None or word in lib.bpmpc_last_error().decode(), lib.bpmpc_last_error()
        now = plant.anchors()
        assert [plant.getStiction(b) for b in range(5)] == list(kt0) and np.array_equal(now[0], anchors[0]) and np.array_equal(now[1], anchors[1])

    for bad in (-1.0, float("nan"), float("inf")):
        refused(lambda: plant.setStiction(bad), INVALID, "kt")
        row = kt0.copy()
        row[3] = bad
        refused(lambda: plant.setStiction(row), INVALID, "entry 3")
    from bipedal_control_amd.api import _d, _i
    three = np.full(3, KT)
    assert lib.bpmpc_plant_set_stiction(plant._h, 5, None, _d(three), 3, 0) == INVALID and b"n_rows" in lib.bpmpc_last_error()
    assert lib.bpmpc_plant_set_stiction(plant._h, 5, None, None, 1, 0) == INVALID and b"null" in lib.bpmpc_last_error()
    refused(lambda: plant.setStiction(np.full(6, KT), mask=np.ones(6, np.int32)), CAPACITY)
    six = np.zeros((6, 4, 2)), np.zeros((6, 4), np.int32)
    assert lib.bpmpc_plant_get_anchors(plant._h, 6, _d(six[0]), _i(six[1])) == CAPACITY
    kt = np.zeros(1)
    assert lib.bpmpc_plant_get_stiction(plant._h, 5, _d(kt)) == CAPACITY
    refused(lambda: plant.setStiction(-0.5, mask=np.array([0, 1, 0, 0, 0], np.int32)), INVALID, "kt")
    # a bad value for a robot outside the mask is no refusal: that robot takes nothing
    row = kt0.copy()
    row[2] = float("nan")
    plant.setStiction(row, mask=np.array([1, 1, 0, 1, 1], np.int32))
    assert [plant.getStiction(b) for b in range(5)] == list(kt0)
