"""The numpy restatement of the plant's input model (tests/plant_input_reference.py) on its own, without the library: the integer nanoseconds and the
delay steps of the reference's shipped gazebo/delay settings, the ring on a ramp, loss, loss and delay together against a hand-written table, a
restart, and the push windows."""
import os
import re

import numpy as np
import pytest

from tests import plant_input_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.path.join(ROOT, "tests", "golden", "reference")
# the four shipped settings of BipedalHWSim's delay and the control steps they are at a 2 ms period
DELAY_FILES = (("bipedal_robot_example/unitree_h1/h1_description/config/hw_sim.yaml", 4),
               ("bipedal_robot_example/hunter/legged_hunter_config/config/gazebo/default.yaml", 4),
               ("bipedal_gazebo/config/default.yaml", 4),
               ("bipedal_robot_example/openloong_description/config/hw_gazebo.yaml", 1))
PERIOD = 0.002


def test_integer_nanoseconds():
    assert ir.ns(0.009) == 9000000 and ir.ns(0.002) == 2000000 and ir.ns(0.001) == 1000000 and ir.ns(0.0005) == 500000
    assert ir.ns(0.009) // ir.ns(0.002) == 4 and ir.ns(0.009) // ir.ns(0.001) == 9 and ir.ns(0.009) // ir.ns(0.0005) == 18
    assert ir.delay_steps(0.009, 0.002) == 4 and ir.delay_steps(0.009, 0.001) == 9 and ir.delay_steps(0.009, 0.0005) == 15      # capped
    # the clamps: not a number, negative, out of range
    assert ir.ns(float("nan")) == 0 and ir.ns(-1.0) == 0 and ir.ns(float("inf")) == 1 << 62 and ir.ns(1e300) == 1 << 62
    assert ir.delay_steps(float("nan"), PERIOD) == 0 and ir.delay_steps(-0.004, PERIOD) == 0 and ir.delay_steps(float("inf"), PERIOD) == 15
    assert ir.period_ns(1e-12) == 1
    assert ir.ns(0.5e-9) == 0 and ir.ns(1.5e-9) == 2 and ir.ns(2.5e-9) == 2       # ties to even


@pytest.mark.parametrize("path, steps", DELAY_FILES)
def test_shipped_delays(path, steps):
    text = open(os.path.join(REFERENCE, path)).read()
    delay = float(re.search(r"^\s*delay:\s*([0-9.eE+-]+)\s*$", text, flags=re.M).group(1))
    assert ir.delay_steps(delay, PERIOD) == steps


def _ramp(model, steps, period=PERIOD, start=0):
    return [model.step(float(n), None, period) for n in range(start, start + steps)]


@pytest.mark.parametrize("k", [0, 1, 4, 15])
def test_ramp_is_delayed_by_k_steps(k):
    """c_n = n comes out as max(n - k, 0) over 20 steps: the ring of 16 wraps"""
    m = ir.Inputs(0, ir.row(delay=k * PERIOD))
    out = _ramp(m, 20)
    assert [o[0] for o in out] == [float(max(n - k, 0)) for n in range(20)]
    assert all(o[4] == k and o[2] == 0 and o[3] == 0 and not o[1].any() for o in out)
    assert m.t == 20 and m.n == 20


def test_dropout_one_and_zero():
    held = _ramp(ir.Inputs(3, ir.row(dropout=1.0), seed=5), 20)
    assert [o[0] for o in held] == [0.0] * 20 and [o[2] for o in held] == [0] + [1] * 19      # the first command always arrives
    none = _ramp(ir.Inputs(3, ir.row(dropout=0.0), seed=5), 20)
    assert [o[0] for o in none] == [float(n) for n in range(20)] and not any(o[2] for o in none)
    above = _ramp(ir.Inputs(3, ir.row(dropout=7.0), seed=5), 5)                               # a device row: above 1 counts as 1
    assert [o[0] for o in above] == [0.0] * 5


def test_loss_and_delay_against_a_table():
    """seed 11, robot 0, dropout 0.3: the lost steps are found from the draws, the table below is written by hand from them.  arrived: a lost
    step repeats the entry before it; applied with k = 2: arrived two steps earlier, the first one until then."""
    lost = [n > 0 and ir.draw(11, 0, n)[0] < 0.3 for n in range(12)]
    assert [int(x) for x in lost] == [0, 0, 1, 1, 0, 0, 1, 0, 0, 1, 0, 0], lost
    arrived = [0.0, 1.0, 1.0, 1.0, 4.0, 5.0, 5.0, 7.0, 8.0, 8.0, 10.0, 11.0]
    applied = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 4.0, 5.0, 5.0, 7.0, 8.0, 8.0]
    out = _ramp(ir.Inputs(0, ir.row(delay=0.004, dropout=0.3), seed=11), 12)
    assert [o[2] for o in out] == [int(x) for x in lost]
    assert [o[0] for o in out] == applied
    plain = _ramp(ir.Inputs(0, ir.row(dropout=0.3), seed=11), 12)
    assert [o[0] for o in plain] == arrived


def test_restart_forgets_the_buffer():
    m = ir.Inputs(1, ir.row(delay=0.009))
    first = _ramp(m, 7)
    m.set_state()
    assert m.n == 0 and m.t == 7
    second = _ramp(m, 9, start=7)
    assert [o[0] for o in first] == [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0]
    assert [o[0] for o in second] == [7.0, 7.0, 7.0, 7.0, 7.0, 8.0, 9.0, 10.0, 11.0]      # the ramp from 7 again
    assert m.t == 16 and m.n == 9
    # a restart shields the first command from loss: n = 0
    m = ir.Inputs(1, ir.row(dropout=1.0))
    _ramp(m, 3)
    m.set_state()
    assert [o[0] for o in _ramp(m, 3, start=3)] == [3.0, 3.0, 3.0]


def test_push_windows():
    """interval 0.016, duration 0.004, period 0.002: W = 8, D = 2; exactly two pushed steps, adjacent, in each of the windows 0 and 1, each with its
    window's direction, norm push_force, z = 0, added to the caller's force"""
    assert ir.push_windows(40.0, 0.016, 0.004, PERIOD) == (8, 2)
    assert ir.push_windows(0.0, 0.016, 0.004, PERIOD) is None and ir.push_windows(40.0, 0.0, 0.004, PERIOD) is None
    assert ir.push_windows(40.0, 0.016, 0.0, PERIOD) == (8, 1) and ir.push_windows(40.0, 0.016, 1.0, PERIOD) == (8, 8)
    assert ir.push_windows(40.0, 0.001, 0.0, PERIOD) == (1, 1)
    f = np.array([1.0, -2.0, 3.0])
    for seed, robot in ((11, 0), (11, 3), (-5, 2)):
        m = ir.Inputs(robot, ir.row(push_force=40.0, push_interval=0.016, push_duration=0.004), seed=seed)
        out = [m.step(0.0, f, PERIOD) for _ in range(16)]
        for w in range(2):
            on = [n for n in range(8 * w, 8 * w + 8) if out[n][3]]
            assert len(on) == 2 and on[1] == on[0] + 1, (seed, robot, w, on)
            _, u_s, u_dir = ir.draw(seed, robot, w)
            assert on[0] - 8 * w == int(np.floor(u_s * 7))
            for n in on:
                push = out[n][1] - f
                assert push[2] == 0.0 and abs(np.hypot(push[0], push[1]) - 40.0) < 1e-12
                assert np.allclose(push[:2], 40.0 * np.array([np.cos(2 * np.pi * u_dir), np.sin(2 * np.pi * u_dir)]), rtol=0, atol=1e-12)
            assert np.array_equal(out[on[0]][1], out[on[1]][1])
        for n in range(16):
            if not out[n][3]:
                assert np.array_equal(out[n][1], f)
        assert not np.array_equal(out[[n for n in range(8) if out[n][3]][0]][1], out[[n for n in range(8, 16) if out[n][3]][0]][1])
    # without a caller's force the push stands alone; a full window pushes every step
    m = ir.Inputs(0, ir.row(push_force=10.0, push_interval=0.004, push_duration=0.004), seed=1)
    assert all(o[3] for o in (m.step(0.0, None, PERIOD) for _ in range(6)))


def test_draws_share_no_word_with_the_sensors():
    """blocks 64 and 65: beyond the sensors' blocks 0..32 at the same (seed, robot, counter)"""
    from tests import plant_sensor_reference as sr
    words = sr.blocks(7, 2, 5, np.arange(33))
    mine = sr.blocks(7, 2, 5, [ir.LOSS_BLOCK, ir.PUSH_BLOCK])
    assert not np.isin(mine, words).any()
    u = ir.draw(7, 2, 5)
    assert all(0.0 < x < 1.0 for x in u) and len(set(u)) == 3
