"""numpy restatement of the tracking telemetry (include/bpmpc.h "Tracking telemetry"; csrc/kernels/telemetry.h): the sample, the seven error
groups, the statistics row, the ring with its decimation, and the freeze.  The kinematics are oracle/wbc_py.py fk / contact_points.

The error norms are restated in the order the kernel states for them (kernels/telemetry.h, header), so that maxima can be compared exactly:
contact errors sqrt((dx dx + dy dy) + dz dz); the squared base-position, base-angle and joint errors summed over the 16 lanes of a row by four
rotate-and-add steps (lane l adds the value of lane l - n, n = 1, 2, 4, 8), read in lane 0, 1 and 6; robots of more than 16 coordinates add the
upper row's sum to the lower's."""
import math

import numpy as np

from oracle import wbc_py as wp

STATS_STRIDE = 40
SAMPLES, FIRST_UNSAFE, JOINT_MAX = 21, 22, 23
GROUPS = 7


def stride(nj):
    return 40 + 2 * nj


def normalize_angle(a):
    """tick_normalize_angle: onto (-pi, pi]"""
    r = np.fmod(a + math.pi, 2.0 * math.pi)
    return np.where(r <= 0.0, r + math.pi, r - math.pi)


def sample(m, x_opt, rbd, t=None, safe=None, mode=None, n=0):
    nj = m["nj"]
    s = np.zeros(stride(nj))
    q_des = np.array(x_opt[6:12 + nj], float)
    q_meas = np.r_[rbd[3:6], rbd[0:3], rbd[6:6 + nj]].astype(float)
    s[0:6], s[6:12] = q_des[:6], q_meas[:6]
    for p, q in enumerate((q_des, q_meas)):
        if np.all(np.isfinite(q)):
            R, o, _ = wp.fk(m, q)
            s[12 + 12 * p:24 + 12 * p] = np.array(wp.contact_points(m, R, o)).reshape(-1)
        else:
            s[12 + 12 * p:24 + 12 * p] = np.nan      # which of them a kernel leaves finite is not specified; the entry test covers q itself
    s[36:36 + nj], s[36 + nj:36 + 2 * nj] = q_des[6:], q_meas[6:]
    s[36 + 2 * nj:] = [0.0 if t is None else t, 0.0 if safe is None else safe, 0.0 if mode is None else mode, n]
    return s


def _row_sum(v, lane):
    """sum over a 16-lane row as four rotate-and-add steps leave it in `lane`"""
    x = np.array(v, float)
    for n in (1, 2, 4, 8):
        x = x + np.roll(x, n)
    return x[lane]


def _lane_sum(per_coordinate, lane):
    g = len(per_coordinate)
    lanes = np.zeros(16 if g <= 16 else 32)
    lanes[:g] = per_coordinate
    total = _row_sum(lanes[:16], lane % 16)
    if len(lanes) == 32:
        total = total + _row_sum(lanes[16:], lane % 16)
    return total


def errors(s, nj):
    """(e [7], |joint error| [nj]) of a sample row"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.zeros(6 + nj)
        d[0:3] = s[0:3] - s[6:9]
        d[3:6] = normalize_angle(s[3:6] - s[9:12])
        d[6:] = s[36:36 + nj] - s[36 + nj:36 + 2 * nj]
        sq = d * d
        pick = lambda lo, hi: np.where((np.arange(6 + nj) >= lo) & (np.arange(6 + nj) < hi), sq, 0.0)      # noqa: E731
        e = np.zeros(GROUPS)
        e[0] = np.sqrt(_lane_sum(pick(0, 3), 0))
        e[1] = np.sqrt(_lane_sum(pick(3, 6), 1))
        for i in range(4):
            c = s[12 + 3 * i:15 + 3 * i] - s[24 + 3 * i:27 + 3 * i]
            e[2 + i] = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        e[6] = np.sqrt(_lane_sum(pick(6, 6 + nj), 6))
        return e, np.abs(d[6:])


class Telemetry:
    """The record of one batch: update() as the kernel, reset(mask), ring(b) oldest first."""

    def __init__(self, m, batch, ring_len=0, every=1, freeze_on_unsafe=True):
        self.m, self.nj, self.B, self.L = m, m["nj"], batch, ring_len
        self.every, self.freeze = every, freeze_on_unsafe
        self.reset()

    def reset(self, mask=None):
        if mask is None:
            mask = np.ones(self.B, int)
            self.n, self.rec, self.frozen = np.zeros(self.B, int), np.zeros(self.B, int), np.zeros(self.B, int)
            self.stats = np.zeros((self.B, STATS_STRIDE))
            self.rings = np.zeros((self.B, max(self.L, 1), stride(self.nj)))
            self.last = np.zeros((self.B, stride(self.nj)))
        for b in np.flatnonzero(mask):
            self.n[b] = self.rec[b] = self.frozen[b] = 0
            self.stats[b] = 0.0
            self.stats[b, FIRST_UNSAFE] = -1.0
            self.last[b] = 0.0

    def update(self, x_opt, rbd, t=None, safe=None, mode=None, samples=None):
        """samples [B, stride]: rows to take instead of computing them (their n is checked against the record's)"""
        nj = self.nj
        for b in range(self.B):
            if self.frozen[b]:
                continue
            n = int(self.n[b])
            if samples is not None:
                s = np.array(samples[b], float)
                assert s[39 + 2 * nj] == n, (b, s[39 + 2 * nj], n)
            else:
                s = sample(self.m, x_opt[b], rbd[b], None if t is None else t[b], None if safe is None else safe[b], None if mode is None else mode[b], n)
            e, ej = errors(s, nj)
            not_finite = not np.all(np.isfinite(s[:36 + 2 * nj]))
            unsafe = safe is not None and safe[b] == 0
            trigger = unsafe or not_finite
            freezing = self.freeze and trigger
            row = self.stats[b]
            if np.all(np.isfinite(e)) and np.all(np.isfinite(ej)):
                for k in range(GROUPS):
                    row[3 * k] += e[k] * e[k]
                    if e[k] > row[3 * k + 1]:
                        row[3 * k + 1], row[3 * k + 2] = e[k], n
                row[JOINT_MAX:JOINT_MAX + nj] = np.maximum(row[JOINT_MAX:JOINT_MAX + nj], ej)
                row[SAMPLES] += 1
            if trigger and row[FIRST_UNSAFE] < 0:
                row[FIRST_UNSAFE] = n
            self.last[b] = s
            if self.L > 0 and (freezing or n % self.every == 0):
                self.rings[b, self.rec[b] % self.L] = s
                self.rec[b] += 1
            self.n[b] += 1
            if freezing:
                self.frozen[b] = 1

    def ring(self, b):
        have = min(int(self.rec[b]), self.L)
        first = 0 if self.rec[b] <= self.L else int(self.rec[b]) % self.L
        return np.array([self.rings[b, (first + k) % self.L] for k in range(have)]).reshape(have, stride(self.nj))

    def summary(self):
        g = self.stats[:, :21].reshape(self.B, GROUPS, 3)
        return {"rms": np.sqrt(g[:, :, 0] / np.maximum(self.stats[:, SAMPLES], 1.0)[:, None]), "max": g[:, :, 1], "max_at": g[:, :, 2].astype(int),
                "samples": self.stats[:, SAMPLES].astype(int), "first_unsafe": self.stats[:, FIRST_UNSAFE].astype(int),
                "joint_max": self.stats[:, JOINT_MAX:JOINT_MAX + self.nj], "frozen": self.frozen.copy()}
