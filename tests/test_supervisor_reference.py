"""The numpy restatement of the supervisor (tests/supervisor_reference.py) against cases worked by hand from include/bpmpc.h "Supervisor"."""
import numpy as np

from tests import supervisor_reference as sr

NJ = 10
NV = 6 + NJ


def _rbd(q=None, v=None, roll=0.0, pitch=0.0, z=1.0):
    r = np.zeros((1, 2 * NV))
    r[0, 1], r[0, 2], r[0, 5] = pitch, roll, z
    if q is not None:
        r[0, 6:NV] = q
    if v is not None:
        r[0, NV + 6:] = v
    return r


def test_after_create_every_robot_is_in_init_with_the_default_rows():
    s = sr.Supervisor(3, 12, np.arange(12.0))
    assert s.state.tolist() == [0, 0, 0] and s.latch.tolist() == [1, 1, 1] and s.params[1, 0] == np.pi / 3 and not s.params[:, 1:].any()
    assert s.rows["kp_init"][2].tolist() == [80.0] * 12 and s.rows["kd_init"][0].tolist() == [5, 5, 5, 5, 5, 3, 5, 5, 5, 5, 5, 3]
    assert np.all(np.isneginf(s.rows["lower"])) and np.all(np.isposinf(s.rows["upper"]))
    assert sr.default_gains(10)[1].tolist() == [5.0] * 10


def test_clamp_order_at_equal_limits():
    """lower == upper: a target above goes to upper, a target below to lower, one between stays - with crossed limits (device rows are not
    validated) the reference's order decides: above upper first"""
    q_init = np.array([2.0, -2.0, 0.5] + [0.0] * 7)
    s = sr.Supervisor(1, NJ, q_init, lower=[0.5] * NJ, upper=[0.5] * NJ)
    s.update(_rbd())
    assert s.cmd["pos_des"][0].tolist() == [0.5] * NJ
    s = sr.Supervisor(1, NJ, q_init, lower=[1.0] * NJ, upper=[-1.0] * NJ)      # crossed
    s.update(_rbd())
    assert s.cmd["pos_des"][0, :3].tolist() == [-1.0, 1.0, -1.0]              # 2 > -1 -> upper; -2 < 1 -> lower; 0.5 > -1 -> upper


def test_ramp_time_zero_is_the_jump_and_a_ramp_interpolates():
    q_init = np.linspace(-0.5, 0.5, NJ)
    q0 = np.full(NJ, 0.25)
    s = sr.Supervisor(1, NJ, q_init)
    s.update(_rbd(q=q0), period=0.01)
    assert np.array_equal(s.cmd["pos_des"][0], q_init) and np.array_equal(s.q_latch[0], q0) and s.latch[0] == 0 and s.elapsed[0] == 0.01
    assert not s.cmd["vel_des"].any() and not s.cmd["tau_ff"].any() and s.cmd["kp"][0, 0] == 80.0 and s.cmd["kd"][0, 0] == 5.0
    p = sr.DEFAULT_PARAMS.copy()
    p[sr.RAMP_TIME] = 0.04
    s = sr.Supervisor(1, NJ, q_init, params=p)
    s.update(_rbd(q=q0), period=0.01)
    assert np.array_equal(s.cmd["pos_des"][0], q0 + (0.01 / 0.04) * (q_init - q0))
    s.update(_rbd(q=np.zeros(NJ)), period=0.01)                                 # the latch is not taken again
    assert np.array_equal(s.cmd["pos_des"][0], q0 + (0.02 / 0.04) * (q_init - q0)) and s.ready[0] == 0
    s.update(_rbd(), period=0.01)
    s.update(_rbd(), period=0.01)                                               # elapsed = 0.04 >= ramp_time: selected, not computed
    assert s.elapsed[0] == 0.01 + 0.01 + 0.01 + 0.01 and np.array_equal(s.cmd["pos_des"][0], q_init)


def test_a_nan_joint():
    q_init = np.linspace(-0.5, 0.5, NJ)
    q = np.full(NJ, 0.1)
    q[3] = np.nan
    p = sr.DEFAULT_PARAMS.copy()
    p[[sr.SETTLE_POS_TOL, sr.SETTLE_VEL_TOL, sr.STOP_KD]] = 10.0, 10.0, 2.5
    s = sr.Supervisor(1, NJ, q_init, params=p)
    s.update(_rbd(q=q))
    assert s.unsafe[0] == sr.MEASUREMENT and s.state[0] == sr.INIT and s.cause[0] == 0 and s.ready[0] == 0 and s.settled[0] == 0.0
    want = q.copy()
    want[3] = q_init[3]
    assert np.array_equal(s.q_latch[0], want) and np.all(np.isfinite(s.cmd["pos_des"]))
    # in RUN the same measurement stops the robot, and the stop command holds 0 for the joint that is not a number
    s.request(sr.RUN)
    cmd = [np.full((1, NJ), x) for x in (1.0, 2.0, 3.0, 4.0, 5.0)]
    s.update(_rbd(q=q), cmd)
    assert s.state[0] == sr.STOPPED and s.cause[0] == sr.MEASUREMENT and s.elapsed[0] == 0.002
    want[3] = 0.0
    assert np.array_equal(s.cmd["pos_des"][0], want) and not s.cmd["kp"].any() and s.cmd["kd"][0].tolist() == [2.5] * NJ and not s.cmd["tau_ff"].any()
    assert s.counts.tolist() == [0, 0, 1, 0, 1, 0, 0, 0]


def test_ready_drops_when_one_joint_velocity_leaves_the_tolerance():
    q_init = np.linspace(-0.5, 0.5, NJ)
    p = sr.DEFAULT_PARAMS.copy()
    p[[sr.SETTLE_POS_TOL, sr.SETTLE_VEL_TOL, sr.SETTLE_TIME]] = 0.05, 0.5, 0.02
    s = sr.Supervisor(1, NJ, q_init, params=p)
    v = np.zeros(NJ)
    s.update(_rbd(q=q_init + 0.04, v=v), period=0.01)
    assert s.settled[0] == 0.01 and s.ready[0] == 0
    s.update(_rbd(q=q_init + 0.04, v=v), period=0.01)
    assert s.settled[0] == 0.02 and s.ready[0] == 1 and s.counts.tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    v[7] = -0.500001
    s.update(_rbd(q=q_init + 0.04, v=v), period=0.01)
    assert s.settled[0] == 0.0 and s.ready[0] == 0
    s.request(sr.RUN, only_ready=True)
    assert s.state[0] == sr.INIT and s.elapsed[0] == 0.01 + 0.01 + 0.01                    # not ready: not one bit changes
    v[7] = 0.5                                                                   # <= holds at the tolerance
    s.update(_rbd(q=q_init + 0.04, v=v), period=0.01)
    s.update(_rbd(q=q_init + 0.04, v=v), period=0.01)
    assert s.ready[0] == 1
    s.request(sr.RUN, only_ready=True)
    assert s.state[0] == sr.RUN and s.ready[0] == 0 and s.elapsed[0] == 0.0 and s.settled[0] == 0.0


def test_a_run_robot_with_a_null_command_stops():
    s = sr.Supervisor(2, NJ, np.zeros(NJ))
    s.request(sr.RUN, mask=[1, 0])
    q = np.linspace(0.1, 1.0, NJ)
    rbd = np.vstack([_rbd(q=q), _rbd(q=q)])
    s.update(rbd, None)
    assert s.state.tolist() == [sr.STOPPED, sr.INIT] and s.cause.tolist() == [sr.COMMAND, 0] and s.unsafe.tolist() == [sr.COMMAND, 0]
    assert np.array_equal(s.cmd["pos_des"][0], q) and s.counts.tolist() == [1, 0, 1, 0, 1, 0, 0, 0]
    s.request(sr.RUN)                                                           # a stopped robot is not in INIT: RUN does not apply to it
    assert s.state.tolist() == [sr.STOPPED, sr.RUN] and s.cause[0] == sr.COMMAND
    s.request(sr.INIT, mask=[1, 0])
    assert s.state[0] == sr.INIT and s.cause[0] == 0 and s.latch[0] == 1


def test_limits_are_strict_and_a_nan_tilt_passes_them():
    p = sr.DEFAULT_PARAMS.copy()
    p[sr.MIN_BASE_HEIGHT] = 0.5
    s = sr.Supervisor(1, NJ, np.zeros(NJ), params=p)
    for roll, pitch, z, want in ((np.pi / 3, 0, 1, 0), (np.nextafter(np.pi / 3, 2), 0, 1, 1), (0, -1.2, 1, 2), (-1.1, 1.1, 0.49, 7), (0, 0, 0.5, 0),
                                 (np.nan, 0, 1, 8)):
        s.update(_rbd(roll=roll, pitch=pitch, z=z))
        assert s.unsafe[0] == want, (roll, pitch, z)
    s.request(sr.STOPPED)
    assert s.cause[0] == sr.REQUEST and s.state[0] == sr.STOPPED
