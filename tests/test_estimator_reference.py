"""CPU tier of the state estimator, the numpy restatement on its own (tests/estimator_reference.py): quatToZyx against rot_zyx, the world angular
velocity, convergence of a robot at rest, P symmetric positive definite over 1000 ticks, and the margin of the xy reset's threshold on the
trajectories the GPU sequence test runs."""
import numpy as np
import pytest

from oracle import wbc_py as wp
from tests import estimator_reference as er
from tests import oracle_bridge as ob


def test_quat_to_zyx_inverts_rot_zyx_away_from_the_clamp():
    rng = np.random.default_rng(3)
    for _ in range(200):
        zyx = np.array([rng.uniform(-3.1, 3.1), rng.uniform(-1.4, 1.4), rng.uniform(-3.1, 3.1)])
        back = er.quat_to_zyx(er.quat_from_zyx(zyx))
        assert np.abs(back - zyx).max() < 1e-12
        assert np.abs(wp.rot_zyx(back) - wp.rot_zyx(zyx)).max() < 1e-12
    # the clamp: beyond asin(.99999) the pitch stays there; -pi/2 is not clamped (one-sided)
    top = er.quat_to_zyx(er.quat_from_zyx(np.array([0.3, np.pi / 2 - 1e-4, 0.0])))
    assert top[1] == np.arcsin(.99999)
    bottom = er.quat_to_zyx(er.quat_from_zyx(np.array([0.3, -np.pi / 2 + 1e-4, 0.0])))
    assert abs(bottom[1] + np.pi / 2 - 1e-4) < 1e-9


def test_world_angular_velocity_is_the_rotated_local_one():
    rng = np.random.default_rng(4)
    m = ob.model("h1")
    for _ in range(50):
        zyx = np.array([rng.uniform(-3, 3), rng.uniform(-1.2, 1.2), rng.uniform(-3, 3)])
        wl = rng.standard_normal(3)
        rbd, z2, rates = er.front_end(m, np.zeros(m["nj"]), np.zeros(m["nj"]), er.quat_from_zyx(zyx), wl)
        nv = 6 + m["nj"]
        assert np.abs(rbd[nv:nv + 3] - wp.rot_zyx(zyx) @ wl).max() < 1e-12
        assert np.abs(wp.euler_rate_map(z2) @ rates - wp.rot_zyx(z2) @ wl).max() < 1e-12


def test_observation_matrix_rows_have_at_most_two_entries():
    C = er.observation_matrix()
    assert C.shape == (28, 18) and np.all(np.count_nonzero(C, axis=1) <= 2)
    assert np.all(np.count_nonzero(C[:12], axis=1) == 2) and np.all(np.count_nonzero(C[12:], axis=1) == 1)


@pytest.mark.parametrize("pose", ["level", "tilted"])
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_robot_at_rest_converges_and_p_stays_spd(robot, pose):
    """A robot at rest, all four contacts closed, constant joints, the IMU measuring gravity only.  Level (yaw only): the four contact points
    share one height in the base frame and x_hat[2] goes to footRadius - (contact z).  Tilted: the heights differ by centimetres and, the four
    contacts being observed with equal weights, x_hat[2] goes to the mean of the four values footRadius - (contact z).  1e-9 is what is left of
    the start x_hat = 0 after 1000 ticks, orders of magnitude above the rounding of the recursion (some 1e-14)."""
    m = ob.model(robot)
    nj, nv = m["nj"], 6 + m["nj"]
    f = er.KalmanFilter(m)
    q = np.asarray(m["default_joint_state"], float)
    zyx = np.array([0.4, 0.0, 0.0]) if pose == "level" else np.array([0.4, 0.05, -0.03])
    quat = er.quat_from_zyx(zyx)
    a_local = wp.rot_zyx(zyx).T @ np.array([0.0, 0.0, er.GRAVITY])
    p, _ = er.contact_kinematics(m, zyx, np.zeros(3), q, np.zeros(nj))
    fired = []
    for k in range(1000):
        rbd, xy, margin, cond = f.update(q, np.zeros(nj), quat, np.zeros(3), a_local, [1, 1, 1, 1], 0.0025)
        fired.append(xy)
        assert np.array_equal(f.P, f.P.T)
        assert np.linalg.eigvalsh(f.P).min() > 0.0
    assert fired[0] == 1
    want = f.params[0] - p[2::3]
    if pose == "level":
        assert np.ptp(want) < 1e-12                      # flat feet: one height
        assert np.abs(f.x[2] - want).max() < 1e-9, (f.x[2], want)
    else:
        assert np.ptp(want) > 5e-3                       # the case is not the level one again
        assert abs(f.x[2] - want.mean()) < 1e-9, (f.x[2], want)
    assert np.abs(f.x[3:6]).max() < 1e-9
    assert np.abs(rbd[3:6] - f.x[0:3]).max() == 0.0 and np.abs(rbd[nv + 3:nv + 6] - f.x[3:6]).max() == 0.0
    assert np.abs(rbd[0:3] - zyx).max() < 1e-12 and np.array_equal(rbd[6:nv], q)


def _cholesky_solve(S, b):
    L = np.linalg.cholesky(S)
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def test_exact_solvers_agree():
    """LU, Cholesky and an explicit inverse on one trajectory: the spread that the GPU tolerance (1e-9) is compared with."""
    m = ob.model("h1")
    tr = er.SensorTrajectories(m, 1, seed=1)
    solvers = [np.linalg.solve, _cholesky_solve, lambda S, b: np.linalg.inv(S) @ b]
    fs = [er.KalmanFilter(m) for _ in solvers]
    worst = 0.0
    for k in range(200):
        s = tr.at(k)
        out = [f.update(s["joint_pos"][0], s["joint_vel"][0], s["quat"][0], s["angular_vel_local"][0], s["linear_accel_local"][0], s["flags"][0], 0.0025,
                        s["feet_heights"][0], solve=sv)[0] for f, sv in zip(fs, solvers)]
        worst = max(worst, np.abs(out[1] - out[0]).max(), np.abs(out[2] - out[0]).max())
    assert worst < 1e-10, worst
