"""CPU tier of the command batch: the numpy restatement (tests/command_batch_reference.py) that the GPU tier compares the device against is
itself held to closed forms - the goal's reach time, hand-written windows of a route, the capacity of a window, the dropped-message rule."""
import math
import os

import numpy as np
import pytest

from oracle import ingest
from tests.command_batch_reference import GOAL, NONE, START, VELOCITY, CommandBatchReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = os.path.join(ROOT, "assets", "h1")
H = 0.45


@pytest.fixture(scope="module")
def model():
    return ingest.build_model(os.path.join(A, "h1_mpc.urdf"), os.path.join(A, "task.info"), os.path.join(A, "reference.info"))


def _state(model, x=0.0, y=0.0, yaw=0.0):
    s = np.zeros(model["nx"])
    s[6:10] = [x, y, 0.9, yaw]
    s[3:6] = [0.01, -0.02, 0.03]
    return s


def _route(model, times):
    xs = np.zeros((1, len(times), model["nx"]))
    xs[0, :, 6] = np.arange(len(times))                  # point i is recognisable by its x
    return np.array(times, float)[None, :], xs


def test_goal_reach_time_is_the_slower_of_turning_and_walking(model):
    ref = CommandBatchReference(model, 2, 8, 1.0)
    vr, vd = model["target_rotation_velocity"], model["target_displacement_velocity"]
    x = np.stack([_state(model, 0.1, -0.2, 3.0), _state(model, 0.1, -0.2, 3.0)])
    goals = np.array([[0.1 + 3 * vd * 0.01, -0.2 + 4 * vd * 0.01, 7.0, 3.0 + 2.0 * vr], [0.1 + 3 * vd, -0.2 - 4 * vd, 7.0, 3.0 - 0.5 * vr]])
    ref.goal(goals, 0.4, x)
    for b, (dyaw, dist) in enumerate([(2.0 * vr, 5 * vd * 0.01), (0.5 * vr, 5 * vd)]):
        ts, xs = ref.targets(b)
        dx, dy = goals[b, 0] - x[b, 6], goals[b, 1] - x[b, 7]
        assert ts[0] == 0.4 and ts[1] == 0.4 + max(abs(goals[b, 3] - x[b, 9]) / vr, math.sqrt(dx * dx + dy * dy) / vd)
        assert abs((ts[1] - ts[0]) - max(dyaw / vr, dist / vd)) < 1e-12       # 2 s of turning for robot 0, 5 s of walking for robot 1
        assert list(xs[1, 6:12]) == [goals[b, 0], goals[b, 1], model["com_height"], goals[b, 3], 0.0, 0.0]
        assert list(xs[0, 6:12]) == [x[b, 6], x[b, 7], model["com_height"], x[b, 9], 0.0, 0.0] and not xs[:, :6].any()
    assert ref.status().tolist() == [[1, 0, GOAL, 2], [1, 0, GOAL, 2]]


def test_window_of_a_route_is_the_hand_written_list(model):
    ref = CommandBatchReference(model, 1, 12, 1.0)
    ref.set_targets(*_route(model, [0.25 * k for k in range(12)]))          # 0, 0.25, .. 2.75: every time exact
    expected = {0.0: [0, 1, 2],                # t0 on the first point; 0.5 is the first point behind 0.45
                0.5: [1, 2, 3, 4],             # t0 on a point: the point before it is kept too (lower_bound - 1); 1.0 is behind 0.95
                0.6: [2, 3, 4, 5],             # 0.5 before the window, 0.75 and 1.0 inside [0.6, 1.05], 1.25 behind
                2.6: [10, 11],                 # the route ends inside the window
                9.0: [11]}                     # the route ended long ago: its last point (constant extrapolation)
    for t0, points in expected.items():
        ts, xs = ref.window(0, t0, H)
        assert list(xs[:, 6]) == points and list(ts) == [0.25 * k for k in points], t0


def test_nine_points_in_one_window_are_rejected(model):
    ref = CommandBatchReference(model, 3, 12, 1.0)
    times, states = _route(model, [k / 16.0 for k in range(12)])
    ref.set_targets(np.repeat(times, 3, 0), np.repeat(states, 3, 0), mask=[0, 0, 1])
    with pytest.raises(ValueError, match="robot 2: target trajectory has 9 points inside the horizon, the solver holds 8"):
        ref.window(2, 0.0, H)                  # points 0 .. 7 lie in [0, 0.45], point 8 (0.5) is the first one behind
    assert list(ref.window(2, 0.3, H)[1][:, 6]) == [4, 5, 6, 7, 8, 9, 10, 11]      # point 4 (0.25) before 0.3, the other seven inside: 8 still fit
    with pytest.raises(ValueError, match="robot 0: target trajectories need at least one point"):
        ref.window(0, 0.0, H)                  # outside the mask: never given a target


def test_message_at_time_zero_is_dropped_and_counted(model):
    ref = CommandBatchReference(model, 3, 8, 1.0)
    x = np.stack([_state(model, 0.0, 0.0, 0.1)] * 3)
    ref.start([0.0, 0.0, 0.3], x)
    assert ref.status().tolist() == [[0, 0, START, 1]] * 3
    ref.cmd_vel([0.2, 0.0, 0.0, 0.1], [0.0, 0.5, 0.0], x)
    ref.goal([1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], x, mask=[1, 0, 0])
    assert ref.status().tolist() == [[0, 2, START, 1], [1, 0, VELOCITY, 2], [0, 1, START, 1]]
    ts, xs = ref.targets(0)
    assert list(ts) == [0.0] and np.array_equal(xs[0], x[0])                 # start is no message: it was taken at t = 0
    ts, xs = ref.targets(1)
    assert list(ts) == [0.5, 1.5] and xs[1, 9] == x[1, 9] + 0.1 * 1.0        # TIME_TO_TARGET = the time horizon given
    fresh = CommandBatchReference(model, 1, 8, 1.0)
    fresh.cmd_vel([0.2, 0.0, 0.0, 0.1], 0.0, x[:1])
    assert fresh.status().tolist() == [[0, 1, NONE, 0]] and len(fresh.targets(0)[0]) == 0
