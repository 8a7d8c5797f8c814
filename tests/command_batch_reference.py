"""A numpy restatement of the command batch (bpmpc_command_batch, include/bpmpc.h) on the oracle's TargetTrajectoriesPublisher
(oracle/reference_py.py cmd_vel_to_target_trajectories / goal_to_target_trajectories): the stored trajectory per robot, the dropped-message
rule with its counters, and the window a setup takes of a stored trajectory (the lower_bound rule of the host path bpmpc_solver_setup)."""
import bisect

import numpy as np

from oracle import reference_py as rp

NONE, START, VELOCITY, GOAL, TRAJECTORY = range(5)
MAX_TARGET_POINTS = 8              # kMaxTargetPoints: what the solver's tables hold per robot


class CommandBatchReference:
    def __init__(self, model, max_batch, max_points, time_horizon):
        self.model, self.max_points, self.time_horizon = model, max_points, time_horizon
        self.times = [np.zeros(0) for _ in range(max_batch)]
        self.states = [np.zeros((0, model["nx"])) for _ in range(max_batch)]
        self.applied, self.dropped, self.source = np.zeros(max_batch, int), np.zeros(max_batch, int), np.zeros(max_batch, int)

    def _robots(self, n, mask):
        return [b for b in range(n) if mask is None or mask[b]]

    def start(self, t, x, mask=None):
        """BipedalController::starting: the single point at the observation."""
        x = np.atleast_2d(x)
        t = np.broadcast_to(np.asarray(t, float), (len(x),))
        for b in self._robots(len(x), mask):
            self.times[b], self.states[b], self.source[b] = np.array([t[b]]), np.array(x[b], float)[None, :].copy(), START

    def _message(self, source, rows, t, x, mask, build):
        x, rows = np.atleast_2d(x), np.broadcast_to(np.asarray(rows, float), (len(np.atleast_2d(x)), 4))
        t = np.broadcast_to(np.asarray(t, float), (len(x),))
        for b in self._robots(len(x), mask):
            if t[b] == 0.0:                       # TargetTrajectoriesPublisher.h:49,75: no observation has arrived yet, the message is ignored
                self.dropped[b] += 1
                continue
            ts, xs = build(rows[b], float(t[b]), x[b])
            self.times[b], self.states[b], self.source[b] = np.array(ts, float), np.array(xs, float), source
            self.applied[b] += 1

    def cmd_vel(self, cmd, t, x, mask=None, time_to_target=0.0):
        T = time_to_target if time_to_target > 0 else self.time_horizon
        self._message(VELOCITY, cmd, t, x, mask, lambda c, tb, xb: rp.cmd_vel_to_target_trajectories(self.model, c, tb, xb, T))

    def goal(self, goal, t, x, mask=None):
        self._message(GOAL, goal, t, x, mask, lambda g, tb, xb: rp.goal_to_target_trajectories(self.model, g, tb, xb))

    def set_targets(self, times, states, n_points=None, mask=None):
        times, states = np.asarray(times, float), np.asarray(states, float)
        for b in self._robots(len(times), mask):
            n = times.shape[1] if n_points is None else int(np.broadcast_to(n_points, (len(times),))[b])
            assert 1 <= n <= self.max_points
            self.times[b], self.states[b], self.source[b] = times[b, :n].copy(), states[b, :n].copy(), TRAJECTORY

    def targets(self, b):
        return self.times[b], self.states[b]

    def status(self, batch=None):
        B = batch or len(self.times)
        return np.stack([self.applied[:B], self.dropped[:B], self.source[:B], [len(t) for t in self.times[:B]]], axis=1).astype(np.int32)

    def window(self, b, t0, horizon):
        """The points a setup at t0 keeps of robot b's trajectory: the last one at or before t0, the ones inside [t0, t0 + horizon], the first
        one behind the window.  ValueError (naming the robot) without a target or with more than MAX_TARGET_POINTS points."""
        ts, xs = self.times[b], self.states[b]
        if len(ts) < 1:
            raise ValueError("robot %d: target trajectories need at least one point" % b)
        i0 = max(0, bisect.bisect_left(ts, t0) - 1)
        i1 = min(len(ts) - 1, bisect.bisect_left(ts, t0 + horizon))
        if i1 - i0 + 1 > MAX_TARGET_POINTS:
            raise ValueError("robot %d: target trajectory has %d points inside the horizon, the solver holds %d" % (b, i1 - i0 + 1, MAX_TARGET_POINTS))
        return ts[i0:i1 + 1].copy(), xs[i0:i1 + 1].copy()
