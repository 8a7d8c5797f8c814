"""CPU tier of the plant's model (include/bpmpc.h "Plant"): properties of the numpy restatement tests/plant_reference.py that the GPU tests compare
k_plant_step against.
  airborne         no contact, no torque: the scheme advances the linear momentum by exactly -m g h.  With A(q) the centroidal momentum matrix,
                   (A(q) v+ - A(q) v) / (m h) + Adot v / m = (0, 0, -9.81) to 1e-9; the Adot v term (the restatement's nle holds it) vanishes for a
                   robot whose joints and orientation are at rest, and there the plain form (A(q) v+ - A(q) v) / (m h) = (0, 0, -9.81) is asserted
                   as well.  For moving joints that form holds to O(h) only, A being frozen at q: both figures are printed.
  standing         H1 on its initialState lowered until the soles are 5 mm in the ground, PD 2000 / 40, 40 substeps of 0.5 ms: everything finite and
                   the summed normal force within [0.5, 1.5] m g from substep 10 on, for the start-of-step normal force sum n_i and for the force the
                   ground applied (spring minus implicit damping).  Measured here: n_i 0.83 .. 1.11, applied 0.84 .. 1.12.  The bare spring sum
                   kn sum d_i is printed and not asserted: it starts at 4 kn 5 mm = 1.97 m g and no motion a net force of at most one m g can produce
                   takes 1.2 mm off the penetration within 5 ms (that needs 10 g), so it passes 1.5 m g only at substep 18 (1.71 at substep 10).
  sensors          quat -> quatToZyx (tests/estimator_reference.py) returns q[3:6]; R linear_accel_local - (0, 0, 9.81) returns a; the FROM_TOPIC
                   restatement on the odom block returns rbd."""
import numpy as np

from oracle import wbc_py as wp
from tests import estimator_reference as er
from tests import oracle_bridge as ob
from tests import plant_reference as pr

H = 0.0005


def _zero_cmd(nj):
    z = np.zeros(nj)
    return dict(pos_des=z, vel_des=z, tau_ff=z, kp=z, kd=z)


def _airborne_state(m, seed, moving):
    rng = np.random.default_rng(seed)
    nv = 6 + m["nj"]
    q = np.array(m["initial_state"], float)[6:] + 0.1 * rng.standard_normal(nv)
    q[2] = 2.0
    v = np.zeros(nv)
    v[0:3] = rng.standard_normal(3)
    if moving:
        v[3:] = 0.5 * rng.standard_normal(nv - 3)
    return q, v


def test_airborne_robot_falls_freely():
    for robot in ("h1", "g1"):
        m = ob.model(robot)
        mass = m["mass"].sum()
        for moving in (False, True):
            q, v = _airborne_state(m, 3, moving)
            s = pr.substep(m, q, v, _zero_cmd(m["nj"]), H)
            assert not s["closed"].any() and np.all(s["d"] < 0.0)
            A, _ = wp.centroidal_momentum_matrix(m, q)
            adot_v = (np.imag(wp.centroidal_momentum_matrix(m, q + 1j * 1e-30 * v)[0]) / 1e-30) @ v
            frozen = (A @ s["v"] - A @ v)[0:3] / (mass * H)
            exact = frozen + adot_v[0:3] / mass
            print("airborne", robot, "moving" if moving else "at rest", "frozen A", np.abs(frozen - [0, 0, -9.81]).max(), "with Adot v", np.abs(exact - [0, 0, -9.81]).max())
            assert np.abs(exact - [0.0, 0.0, -9.81]).max() < 1e-9
            if not moving:
                assert np.abs(frozen - [0.0, 0.0, -9.81]).max() < 1e-9


def standing_state(m, depth=0.005):
    """initialState lowered until the lowest contact points are `depth` in the ground; the PD command that holds its joints"""
    nj = m["nj"]
    q = np.array(m["initial_state"], float)[6:].copy()
    R, o, _ = wp.fk(m, q)
    q[2] -= np.array(wp.contact_points(m, R, o))[:, 2].min() + depth
    cmd = dict(pos_des=q[6:].copy(), vel_des=np.zeros(nj), tau_ff=np.zeros(nj), kp=np.full(nj, 2000.0), kd=np.full(nj, 40.0))
    return q, np.zeros(6 + nj), cmd


def test_standing_robot_settles():
    m = ob.model("h1")
    mg = m["mass"].sum() * 9.81
    q, v, cmd = standing_state(m)
    rows = []
    for k in range(40):
        s = pr.substep(m, q, v, cmd, H)
        q, v = s["q"], s["v"]
        assert np.all(np.isfinite(q)) and np.all(np.isfinite(v)) and np.all(np.isfinite(s["force"])), k
        assert s["closed"].all()
        rows.append((s["n"].sum() / mg, s["force"][:, 2].sum() / mg, s["spring"] / mg, np.abs(v).max()))
    rows = np.array(rows)
    print("standing: n / mg", rows[10:, 0].min(), rows[10:, 0].max(), "applied / mg", rows[10:, 1].min(), rows[10:, 1].max(),
          "spring / mg at 0, 10, 39", rows[0, 2], rows[10, 2], rows[39, 2], "max |v|", rows[:, 3].max())
    assert np.all(rows[10:, 0] >= 0.5) and np.all(rows[10:, 0] <= 1.5)
    assert np.all(rows[10:, 1] >= 0.5) and np.all(rows[10:, 1] <= 1.5)


def test_sensor_block_inverts():
    m = ob.model("h1")
    rng = np.random.default_rng(11)
    q, v, cmd = standing_state(m)
    q[3:6] = [0.4, -0.2, 0.3]
    v = 0.3 * rng.standard_normal(len(q))
    ground = np.array([0.002, -0.001, 0.0, 0.001])
    s = pr.substep(m, q, v, cmd, H, ground=ground, w_ext=[30.0, 0.0, 0.0])
    out = pr.sensors(m, s, ground=ground)
    assert np.abs(er.quat_to_zyx(out["quat"]) - s["q"][3:6]).max() < 1e-14
    R = wp.rot_zyx(s["q"][3:6])
    assert np.abs(R @ out["linear_accel_local"] - [0.0, 0.0, 9.81] - s["a"]).max() < 1e-9
    assert np.abs(R @ out["angular_vel_local"] - out["odom_ang_vel"]).max() < 1e-14
    topic = er.from_topic(m, out["joint_pos"], out["joint_vel"], out["odom_pos"], out["odom_quat"], out["odom_lin_vel"], out["odom_ang_vel"])
    assert np.abs(topic - out["rbd"]).max() < 1e-14
    assert np.array_equal(out["feet_heights"], ground) and out["contact"].dtype == np.int32 and out["contact_force"].shape == (4, 3)
