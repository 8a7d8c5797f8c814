"""A numpy restatement of the supervisor's rules, written from the header comment (include/bpmpc.h "Supervisor", items 1 to 5 of
bpmpc_supervisor_update and bpmpc_supervisor_request), for a batch of robots held in plain arrays.  No fused operations: s = elapsed / ramp_time
and q_latch + s (q_init - q_latch) round once per operation, as the header states."""
import numpy as np

INIT, RUN, STOPPED = 0, 1, 2
ROLL, PITCH, HEIGHT, MEASUREMENT, COMMAND, REQUEST = 1, 2, 4, 8, 16, 64
PARAM_STRIDE = 8
TILT_LIMIT, MIN_BASE_HEIGHT, RAMP_TIME, SETTLE_POS_TOL, SETTLE_VEL_TOL, SETTLE_TIME, STOP_KD = range(7)
DEFAULT_PARAMS = np.array([np.pi / 3.0, 0, 0, 0, 0, 0, 0, 0], float)
JOINT_ROWS = ("q_init", "kp_init", "kd_init", "lower", "upper")
COMMAND_ROWS = ("pos_des", "vel_des", "tau_ff", "kp", "kd")


def default_gains(nj):
    """the start-up values of the reference's reconfigure server for InitialJointPositionController: 80 / 5 per leg motor, kd 3 for the sixth
    motor of a six-motor leg"""
    kd = np.full(nj, 5.0)
    if nj == 12:
        kd[5::6] = 3.0
    return np.full(nj, 80.0), kd


class Supervisor:
    """The state of `max_batch` robots after create: every robot in INIT with its latch pending"""

    def __init__(self, max_batch, nj, q_init, params=None, lower=None, upper=None):
        B = max_batch
        self.B, self.nj = B, nj
        self.params = np.tile(DEFAULT_PARAMS if params is None else np.asarray(params, float), (B, 1))
        kp, kd = default_gains(nj)
        self.rows = {"q_init": np.tile(np.asarray(q_init, float), (B, 1)), "kp_init": np.tile(kp, (B, 1)), "kd_init": np.tile(kd, (B, 1)),
                     "lower": np.tile(np.full(nj, -np.inf) if lower is None else np.asarray(lower, float), (B, 1)),
                     "upper": np.tile(np.full(nj, np.inf) if upper is None else np.asarray(upper, float), (B, 1))}
        self.state, self.cause, self.unsafe, self.ready = (np.zeros(B, np.int32) for _ in range(4))
        self.latch = np.ones(B, np.int32)
        self.elapsed, self.settled = np.zeros(B), np.zeros(B)
        self.q_latch = np.zeros((B, nj))
        self.cmd = {k: np.zeros((B, nj)) for k in COMMAND_ROWS}
        self.counts = np.zeros(8, np.int32)

    def request(self, target, mask=None, only_ready=False, batch=None):
        B = self.B if batch is None else batch
        for b in range(B):
            if mask is not None and not mask[b]:
                continue
            if target == RUN and (self.state[b] != INIT or (only_ready and self.ready[b] != 1)):
                continue
            self.state[b] = target
            self.elapsed[b] = self.settled[b] = 0.0
            self.ready[b] = 0
            if target in (INIT, RUN):
                self.cause[b] = 0
            if target == INIT:
                self.latch[b] = 1
            if target == STOPPED:
                self.cause[b] = REQUEST

    def update(self, rbd, run_cmd=None, period=0.002):
        """rbd [B, 2 (6 + nj)]; run_cmd None or five [B, nj] arrays in the order of COMMAND_ROWS"""
        rbd = np.asarray(rbd, float)
        B, nj = rbd.shape[0], self.nj
        nv = 6 + nj
        for b in range(B):
            p = self.params[b]
            zyx, pos, q, v = rbd[b, 0:3], rbd[b, 3:6], rbd[b, 6:nv], rbd[b, nv + 6:]
            # 1
            unsafe = 0
            if abs(zyx[2]) > p[TILT_LIMIT]:
                unsafe |= ROLL
            if abs(zyx[1]) > p[TILT_LIMIT]:
                unsafe |= PITCH
            if p[MIN_BASE_HEIGHT] > 0 and pos[2] < p[MIN_BASE_HEIGHT]:
                unsafe |= HEIGHT
            if not np.all(np.isfinite(rbd[b])):
                unsafe |= MEASUREMENT
            if self.state[b] == RUN and (run_cmd is None or not all(np.all(np.isfinite(np.asarray(a)[b])) for a in run_cmd)):
                unsafe |= COMMAND
            self.unsafe[b] = unsafe
            # 2
            if self.state[b] == RUN and unsafe:
                self.state[b], self.cause[b] = STOPPED, unsafe
                self.elapsed[b] = self.settled[b] = 0.0
                self.ready[b] = 0
            # 3
            self.elapsed[b] = self.elapsed[b] + period
            # 4
            if self.state[b] == RUN:
                for k, a in zip(COMMAND_ROWS, run_cmd):
                    self.cmd[k][b] = np.asarray(a)[b]
            elif self.state[b] == INIT:
                q_init = self.rows["q_init"][b]
                if self.latch[b]:
                    self.q_latch[b] = np.where(np.isfinite(q), q, q_init)
                    self.latch[b] = 0
                T = p[RAMP_TIME]
                s = 1.0 if (T == 0 or self.elapsed[b] >= T) else self.elapsed[b] / T
                target = q_init.copy() if s == 1.0 else self.q_latch[b] + s * (q_init - self.q_latch[b])
                lo, up = self.rows["lower"][b], self.rows["upper"][b]
                pos_des = np.where(target > up, up, np.where(target < lo, lo, target))
                self.cmd["pos_des"][b], self.cmd["vel_des"][b], self.cmd["tau_ff"][b] = pos_des, 0.0, 0.0
                self.cmd["kp"][b], self.cmd["kd"][b] = self.rows["kp_init"][b], self.rows["kd_init"][b]
                with np.errstate(invalid="ignore"):
                    holds = bool(s == 1.0 and unsafe == 0 and np.all(np.abs(q - pos_des) <= p[SETTLE_POS_TOL]) and np.all(np.abs(v) <= p[SETTLE_VEL_TOL]))
                self.settled[b] = self.settled[b] + period if holds else 0.0
                self.ready[b] = 1 if (holds and self.settled[b] >= p[SETTLE_TIME]) else 0
            else:
                self.cmd["pos_des"][b] = np.where(np.isfinite(q), q, 0.0)
                self.cmd["vel_des"][b], self.cmd["tau_ff"][b], self.cmd["kp"][b] = 0.0, 0.0, 0.0
                self.cmd["kd"][b] = p[STOP_KD]
                self.ready[b] = 0
        # 5
        st = self.state[:B]
        self.counts[:] = [np.sum(st == INIT), np.sum(st == RUN), np.sum(st == STOPPED), np.sum(self.ready[:B] != 0), np.sum(self.unsafe[:B] != 0), 0, 0, 0]
