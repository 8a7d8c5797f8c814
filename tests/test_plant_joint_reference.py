"""CPU tier of the plant's joint model (include/bpmpc.h "Plant", joints): properties of the numpy restatement tests/plant_joint_reference.py that
tests/test_gpu_plant_joints.py compares k_plant_joint_step against, and the scenarios the two files share.
  neutral row   the restatement returns exactly what plant_stiction_reference.substep returns, on the five robots of test_gpu_plant._cases (one
                airborne, four standing), H1 and G1, with kt = 0 and kt = kn
  free fall     a known answer.  A floating robot in uniform gravity feels no gravity torque at its joints, so with every joint held by a PD at
                its pose `hold` (kp 2000, kd 40), the rows of JointParams.reference_mjcf (armature 0.1, damping 1), joint 3 given
                upper = hold - 0.05 and the last joint lower = hold + 0.03, the two joints settle where the PD and the end-stop spring balance:
                q* = (kp hold + k_limit limit) / (kp + k_limit).  Base at z = 2 m, ground at -100 m, h = 0.5 ms, 800 substeps: |q - q*| < 1e-6 rad
                (measured here: 2.2e-9 rad H1, 2.4e-9 rad G1; the other joints within 1.4e-7 rad of hold), and no contact closes.
  friction law  one joint with friction_loss = F and tau_ff = F / 2 and no PD, the others held, in free fall: the steady velocity of the linearly
                implicit law c(v) v = tau with c = F / sqrt(v^2 + w_eps^2) is w_eps tau / sqrt(F^2 - tau^2); asserted within 1 % once the velocity
                has stopped changing (a substep changes it by less than 1e-4 of the closed form: measured here after 8 and 7 substeps, H1 3.1e-4 and
                G1 4.0e-5 from the closed form; the joint's own time constant is a substep or two, what remains is the held joints ringing)
  diagonal      armature and damping only ever add to the diagonal: A stays symmetric and its smallest eigenvalue is not below that of the
                neutral A at the same state
Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np

from tests import oracle_bridge as ob
from tests import plant_joint_reference as jr
from tests import plant_reference as pr
from tests import plant_stiction_reference as sr

H = 0.0005
KP, KD = 2000.0, 40.0
FREE_FALL_SUBSTEPS = 800
GROUND = -100.0


def mjcf_row(nj, **more):
    """the rows of JointParams.reference_mjcf: the <default> of the reference's H1 MJCF"""
    return jr.joint_row(nj, armature=0.1, damping=1.0, **more)


def free_fall_case(m):
    """(q, v, cmd, row, q*) of the free-fall known answer: every joint held at its pose, joint 3 beyond an upper stop, the last joint beyond a lower"""
    nj = m["nj"]
    q = np.array(m["initial_state"], float)[6:].copy()
    q[2] = 2.0
    hold = q[6:].copy()
    lower, upper = np.full(nj, -np.inf), np.full(nj, np.inf)
    upper[3], lower[nj - 1] = hold[3] - 0.05, hold[nj - 1] + 0.03
    row = mjcf_row(nj, lower=lower, upper=upper)
    cmd = dict(pos_des=hold, vel_des=np.zeros(nj), tau_ff=np.zeros(nj), kp=np.full(nj, KP), kd=np.full(nj, KD))
    k_limit = row[jr.K_LIMIT]
    target = hold.copy()
    target[3] = (KP * hold[3] + k_limit * upper[3]) / (KP + k_limit)
    target[nj - 1] = (KP * hold[nj - 1] + k_limit * lower[nj - 1]) / (KP + k_limit)
    return q, np.zeros(6 + nj), cmd, row, target


@functools.lru_cache(maxsize=None)
def free_fall(robot, substeps=FREE_FALL_SUBSTEPS):
    """the joints after `substeps` substeps of the restatement, the target, whether any contact ever closed"""
    m = ob.model(robot)
    q, v, cmd, row, target = free_fall_case(m)
    closed = False
    for _ in range(substeps):
        s = jr.substep(m, q, v, cmd, H, row, ground=np.full(4, GROUND))
        closed = closed or bool(s["closed"].any())
        q, v = s["q"], s["v"]
    return q[6:], target, closed


@functools.lru_cache(maxsize=None)
def joint_cases(robot):
    """The five robots of test_gpu_plant._cases with a joint row each, so that a batch covers every branch of the kernel: (q, v, cmd, force,
    ground, rows [5, 64], kt [5]).
      0  the neutral row (the airborne robot)
      1  armature and damping only
      2  friction on every joint, joint 4 at exactly zero velocity
      3  joint 1 beyond its upper limit by 0.02 rad, every other joint inside finite limits
      4  the last joint beyond its lower limit by 0.03 rad, armature, damping and friction, kt = kn and closed contacts"""
    from tests import test_gpu_plant as tp
    nj = ob.model(robot)["nj"]
    q, v, cmd, force, ground = tp._cases(robot)
    v = v.copy()
    v[2, 6 + 4] = 0.0
    rng = np.random.default_rng(100 + nj)
    rows = np.array([jr.neutral_row() for _ in range(tp.B5)])
    rows[1] = jr.joint_row(nj, armature=rng.uniform(0.02, 0.2, nj), damping=rng.uniform(0.2, 2.0, nj))
    rows[2] = jr.joint_row(nj, friction_loss=rng.uniform(0.2, 3.0, nj), w_eps=0.02)
    upper = q[3, 6:] + 0.5
    upper[1] = q[3, 6 + 1] - 0.02
    rows[3] = jr.joint_row(nj, lower=q[3, 6:] - 0.5, upper=upper, k_limit=8e3, c_limit=60.0)
    lower = np.full(nj, -np.inf)
    lower[nj - 1] = q[4, 6 + nj - 1] + 0.03
    rows[4] = jr.joint_row(nj, armature=0.1, damping=1.0, friction_loss=rng.uniform(0.0, 1.0, nj), lower=lower)
    kt = np.array([0.0, 0.0, 0.0, 0.0, pr.DEFAULT_ROW[0]])
    return q, v, cmd, force, ground, rows, kt


@functools.lru_cache(maxsize=None)
def joint_reference(robot, n):
    """n restatement substeps of joint_cases: per robot the list of substep dicts, and the restatement's own floor as test_gpu_plant._reference
    measures it (v+ of numpy.linalg.solve against a Cholesky solve of the same system, relative to max(1, |v+|)).  No decision of a compared
    substep is left to rounding: the contact asserts of the existing tests, and |q_j - limit_j| > 1e-6 for every joint and both limits."""
    from tests import test_gpu_plant as tp
    m = ob.model(robot)
    nj = m["nj"]
    q, v, cmd, force, ground, rows, kt = joint_cases(robot)
    lim = tp._limits(robot)
    steps, floor = [], 0.0
    for b in range(tp.B5):
        qb, vb, out = q[b], v[b], []
        anchor, anchored = sr.no_anchors()
        cb = {k: a[b] for k, a in cmd.items()}
        for _ in range(n):
            s = jr.substep(m, qb, vb, cb, H, rows[b], kt[b], anchor, anchored, ground=ground[b], w_ext=force[b], torque_limits=lim)
            assert np.abs(s["d"]).min() > 1e-6, (robot, b, s["d"])
            assert np.abs(s["n"] - pr.DEFAULT_ROW[5]).min() > 1e-6, (robot, b, s["n"])
            decided = (anchored != 0) & s["closed"]
            assert np.all(np.abs(s["phi"] - s["cap"])[decided] > 1e-6 * np.maximum(1.0, s["cap"][decided])), (robot, b, s["phi"], s["cap"])
            assert np.abs(qb[6:] - rows[b, jr.LOWER:jr.LOWER + nj]).min() > 1e-6 and np.abs(qb[6:] - rows[b, jr.UPPER:jr.UPPER + nj]).min() > 1e-6, (robot, b)
            sol = pr.cholesky_solve(s["A"], s["rhs"])
            floor = max(floor, float((np.abs(sol - s["v"]) / np.maximum(1.0, np.abs(s["v"]))).max()))
            out.append(s)
            qb, vb, anchor, anchored = s["q"], s["v"], s["anchor"], s["anchored"]
        steps.append(out)
    return steps, floor


def test_the_five_robots_cover_every_branch():
    from tests import test_gpu_plant as tp
    for robot in ("h1", "g1"):
        nj = ob.model(robot)["nj"]
        q, v, _, _, _, rows, kt = joint_cases(robot)
        steps, floor = joint_reference(robot, 1)
        first = [rows_b[0] for rows_b in steps]
        assert [jr.is_neutral(rows[b], nj) for b in range(tp.B5)] == [True, False, False, False, False]
        assert not first[1]["beyond"].any() and not rows[1, jr.FRICTION:jr.FRICTION + nj].any() and np.all(first[1]["c_joint"] > 0.0)
        assert v[2, 6 + 4] == 0.0 and first[2]["c_joint"][4] == rows[2, jr.FRICTION + 4] / rows[2, jr.W_EPS]
        assert first[3]["beyond"].tolist() == [j == 1 for j in range(nj)] and first[3]["tau_lim"][1] < 0.0
        assert first[4]["beyond"].tolist() == [j == nj - 1 for j in range(nj)] and first[4]["tau_lim"][nj - 1] > 0.0
        assert kt[4] > 0.0 and first[4]["closed"].any() and first[4]["anchored"].any() and not first[0]["closed"].any()
        print("joint cases", robot, "restatement floor", floor, "end-stop torques", first[3]["tau_lim"][1], first[4]["tau_lim"][nj - 1])


def test_neutral_row_is_the_plant_without_a_joint_model():
    from tests import test_gpu_plant as tp
    for robot in ("h1", "g1"):
        m = ob.model(robot)
        q, v, cmd, force, ground = tp._cases(robot)
        lim = tp._limits(robot)
        standing = []
        for b in range(tp.B5):
            cb = {k: a[b] for k, a in cmd.items()}
            for kt in (0.0, pr.DEFAULT_ROW[0]):
                ref = sr.substep(m, q[b], v[b], cb, H, kt, *sr.no_anchors(), ground=ground[b], w_ext=force[b], torque_limits=lim)
                for row in (None, jr.neutral_row(), jr.joint_row(m["nj"], k_limit=3e3, c_limit=7.0, w_eps=0.2)):      # the scalars alone change nothing
                    new = jr.substep(m, q[b], v[b], cb, H, row, kt, *sr.no_anchors(), ground=ground[b], w_ext=force[b], torque_limits=lim)
                    for k, val in ref.items():
                        assert np.array_equal(np.asarray(val), np.asarray(new[k])), (robot, b, kt, k)
                    assert not new["tau_lim"].any() and not new["c_joint"].any() and not new["beyond"].any()
            standing.append(bool(ref["closed"].any()))
        assert standing == [False, True, True, True, True]      # one airborne, four standing


def test_free_fall_known_answer():
    for robot in ("h1", "g1"):
        nj = ob.model(robot)["nj"]
        joints, target, closed = free_fall(robot)
        stops = [3, nj - 1]
        err = np.abs(joints - target)
        others = np.delete(err, stops).max()
        print("free fall", robot, FREE_FALL_SUBSTEPS, "substeps: |q - q*| at the two stops", err[stops], "rad; the other joints from hold", others, "rad")
        assert not closed
        assert abs(target[3] - joints[3]) < 1e-6 and abs(target[nj - 1] - joints[nj - 1]) < 1e-6, err[stops]
        assert others < 1e-6, others


def test_friction_law_steady_velocity():
    F, w_eps = 2.0, 0.01
    STEADY = 1e-4      # stopped changing: a substep moves the velocity by less than a hundredth of the bound asserted below
    tau = F / 2
    expected = w_eps * tau / np.sqrt(F * F - tau * tau)
    for robot in ("h1", "g1"):
        m = ob.model(robot)
        nj = m["nj"]
        j = nj - 1
        q = np.array(m["initial_state"], float)[6:].copy()
        q[2] = 2.0
        v = np.zeros(6 + nj)
        friction = np.zeros(nj)
        friction[j] = F
        row = jr.joint_row(nj, friction_loss=friction, w_eps=w_eps)
        kp, kd, tff = np.full(nj, KP), np.full(nj, KD), np.zeros(nj)
        kp[j], kd[j], tff[j] = 0.0, 0.0, tau
        cmd = dict(pos_des=q[6:].copy(), vel_des=np.zeros(nj), tau_ff=tff, kp=kp, kd=kd)
        change, n = np.inf, 0
        while change > STEADY * expected and n < 100:
            s = jr.substep(m, q, v, cmd, H, row, ground=np.full(4, GROUND))
            change = abs(s["v"][6 + j] - v[6 + j])
            q, v, n = s["q"], s["v"], n + 1
        w = v[6 + j]
        print("friction law", robot, "steady velocity", w, "closed form", expected, "relative difference", abs(w - expected) / expected, "after", n, "substeps")
        assert change <= STEADY * expected, (n, change)      # the velocity has stopped changing
        assert abs(w - expected) < 0.01 * expected


def test_armature_and_damping_only_add_to_the_diagonal():
    from tests import test_gpu_plant as tp
    rng = np.random.default_rng(7)
    for robot in ("h1", "g1"):
        m = ob.model(robot)
        nj = m["nj"]
        q, v, cmd, force, ground = tp._cases(robot)
        row = jr.joint_row(nj, armature=rng.uniform(0.0, 0.2, nj), damping=rng.uniform(0.0, 2.0, nj), friction_loss=rng.uniform(0.0, 1.0, nj))
        for b in (0, 1, 4):
            cb = {k: a[b] for k, a in cmd.items()}
            plain = jr.substep(m, q[b], v[b], cb, H, None, ground=ground[b], w_ext=force[b])["A"]
            A = jr.substep(m, q[b], v[b], cb, H, row, ground=ground[b], w_ext=force[b])["A"]
            assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
            extra = A - plain
            assert np.count_nonzero(extra - np.diag(np.diag(extra))) == 0 and np.all(np.diag(extra) >= 0.0) and not np.diag(extra)[:6].any()
            low, low_plain = np.linalg.eigvalsh(0.5 * (A + A.T)).min(), np.linalg.eigvalsh(0.5 * (plain + plain.T)).min()
            print("diagonal", robot, b, "smallest eigenvalue", low, "neutral", low_plain)
            assert low >= low_plain * (1.0 - 1e-12) and low > 0.0      # (1e-12: the rounding of the two eigenvalue computations)
            np.linalg.cholesky(A)
