"""numpy restatement of the batched state estimator (include/bpmpc.h "State estimation"; kernels/estimator.h): the front end of
StateEstimateBase (bipedal_estimation/src/StateEstimateBase.cpp:34-63, quatToZyx of StateEstimateBase.h:70-79), FromTopicStateEstimate::update
(FromTopicEstimate.cpp:28-47) and the linear Kalman filter the reference declares in LinearKalmanFilter.h and does not implement (the filter of the
project that header cites, recalled and unpinned; the specification is the comment in include/bpmpc.h).  Written with dense matrices - C, A, B, Q, R
are formed and S is solved by LAPACK - so that it shares no arithmetic with the kernel, and with the kinematics of oracle/wbc_py.py."""
import numpy as np

from oracle import wbc_py as wp

GRAVITY = 9.81
NC, N, M = 4, 18, 28
PARAM_NAMES = ("footRadius", "imuProcessNoisePosition", "imuProcessNoiseVelocity", "footProcessNoisePosition", "footSensorNoisePosition",
               "footSensorNoiseVelocity", "footHeightSensorNoise")
DEFAULT_ROW = np.array([0.02, 0.02, 0.02, 0.002, 0.005, 0.1, 0.01, 0.0])      # LinearKalmanFilter.h:45-51
XY_RESET_DET = 1e-6


def quat_to_zyx(q):
    """q = (x, y, z, w).  The clamp is one-sided, as in the header."""
    x, y, z, w = (float(v) for v in q)
    s = min(-2.0 * (x * z - w * y), .99999)
    return np.array([np.arctan2(2 * (x * y + w * z), w * w + x * x - y * y - z * z), np.arcsin(s),
                     np.arctan2(2 * (y * z + w * x), w * w - x * x - y * y + z * z)])


def quat_from_zyx(zyx):
    """(x, y, z, w) of Rz(zyx[0]) Ry(zyx[1]) Rx(zyx[2])."""
    cz, sz = np.cos(zyx[0] / 2), np.sin(zyx[0] / 2)
    cy, sy = np.cos(zyx[1] / 2), np.sin(zyx[1] / 2)
    cx, sx = np.cos(zyx[2] / 2), np.sin(zyx[2] / 2)
    return np.array([cz * cy * sx - sz * sy * cx, cz * sy * cx + sz * cy * sx, sz * cy * cx - cz * sy * sx, cz * cy * cx + sz * sy * sx])


def euler_rates_from_local(zyx, w_local):
    """thetadot with R(zyx) w_local = E(zyx) thetadot."""
    return np.linalg.solve(wp.euler_rate_map(zyx), wp.rot_zyx(zyx) @ np.asarray(w_local, float))


def mode_flags(mode):
    return np.array(wp.mode_flags(mode))


def observation_matrix():
    C = np.zeros((M, N))
    for i in range(NC):
        C[3 * i:3 * i + 3, 0:3] = np.eye(3)
        C[3 * i:3 * i + 3, 6 + 3 * i:9 + 3 * i] = -np.eye(3)
        C[12 + 3 * i:15 + 3 * i, 3:6] = np.eye(3)
        C[24 + i, 6 + 3 * i + 2] = 1.0
    return C


def front_end(m, joint_pos, joint_vel, quat, w_local):
    """rbd with its angular and joint parts filled (updateJointStates, updateImu); also zyx and the Euler rates."""
    nj = m["nj"]
    nv = 6 + nj
    rbd = np.zeros(2 * nv)
    zyx = quat_to_zyx(quat)
    rates = euler_rates_from_local(zyx, w_local)
    rbd[0:3] = zyx
    rbd[nv:nv + 3] = wp.euler_rate_map(zyx) @ rates
    rbd[6:6 + nj] = joint_pos
    rbd[nv + 6:nv + 6 + nj] = joint_vel
    return rbd, zyx, rates


def from_topic(m, joint_pos, joint_vel, odom_pos, odom_quat, odom_lin, odom_ang):
    nj = m["nj"]
    nv = 6 + nj
    rbd = np.zeros(2 * nv)
    rbd[0:3] = quat_to_zyx(odom_quat)
    rbd[3:6] = odom_pos
    rbd[6:6 + nj] = joint_pos
    rbd[nv:nv + 3] = odom_ang
    rbd[nv + 3:nv + 6] = odom_lin
    rbd[nv + 6:] = joint_vel
    return rbd


def contact_kinematics(m, zyx, rates, joint_pos, joint_vel):
    """Contact positions and velocities (12 each) with the base at the origin."""
    q = np.concatenate([np.zeros(3), zyx, joint_pos])
    v = np.concatenate([np.zeros(3), rates, joint_vel])
    R, o, _ = wp.fk(m, q)
    return np.concatenate(wp.contact_points(m, R, o)), wp.contact_jacobian(m, q) @ v


class KalmanFilter:
    """One robot's filter.  params: a row of 8 (PARAM_NAMES + a reserved entry)."""

    def __init__(self, m, params=None):
        self.m = m
        self.params = np.array(DEFAULT_ROW if params is None else params, float)
        self.C = observation_matrix()
        self.reset()

    def reset(self):
        self.x = np.zeros(N)
        self.P = 100.0 * np.eye(N)

    def update(self, joint_pos, joint_vel, quat, w_local, a_local, flags, dt, feet_heights=None, solve=np.linalg.solve):
        """Returns (rbd, xy_reset, det / 1e-6 of the xy block before the reset, cond S)."""
        m, par = self.m, self.params
        nv = 6 + m["nj"]
        flags = np.asarray(flags).astype(bool)
        rbd, zyx, rates = front_end(m, joint_pos, joint_vel, quat, w_local)
        A = np.eye(N)
        A[0:3, 3:6] = dt * np.eye(3)
        B = np.zeros((N, 3))
        B[0:3] = 0.5 * dt * dt * np.eye(3)
        B[3:6] = dt * np.eye(3)
        qd = np.concatenate([np.full(3, dt / 20.0 * par[1]), np.full(3, dt * GRAVITY / 20.0 * par[2]), np.full(12, dt * par[3])])
        rd = np.concatenate([np.full(12, par[4]), np.full(12, par[5]), np.full(4, par[6])])
        for i in range(NC):
            if not flags[i]:
                qd[6 + 3 * i:9 + 3 * i] *= 100.0
                rd[12 + 3 * i:15 + 3 * i] *= 100.0
                rd[24 + i] *= 100.0
        p, v = contact_kinematics(m, zyx, rates, np.asarray(joint_pos, float), np.asarray(joint_vel, float))
        ps = -p
        ps[2::3] += par[0]
        y = np.concatenate([ps, -v, np.zeros(NC) if feet_heights is None else np.asarray(feet_heights, float)])
        accel = wp.rot_zyx(zyx) @ np.asarray(a_local, float) + np.array([0.0, 0.0, -GRAVITY])
        xm = A @ self.x + B @ accel
        Pm = A @ self.P @ A.T + np.diag(qd)
        C = self.C
        S = C @ Pm @ C.T + np.diag(rd)
        PCt = Pm @ C.T
        self.x = xm + PCt @ solve(S, y - C @ xm)
        P = (np.eye(N) - PCt @ solve(S, C)) @ Pm
        P = 0.5 * (P + P.T)
        det = P[0, 0] * P[1, 1] - P[0, 1] * P[1, 0]
        fired = det > XY_RESET_DET
        if fired:
            P[0:2, 2:] = 0.0
            P[2:, 0:2] = 0.0
            P[0:2, 0:2] /= 10.0
        self.P = P
        rbd[3:6] = self.x[0:3]
        rbd[nv + 3:nv + 6] = self.x[3:6]
        return rbd, int(fired), det / XY_RESET_DET, np.linalg.cond(S)


# ---------------------------------------------------------------------------------------------------------------------
# smooth per-robot sensor trajectories for the sequence tests (deterministic in seed, robot index and tick)
# ---------------------------------------------------------------------------------------------------------------------
class SensorTrajectories:
    """B robots: joints oscillate about the default joint state, the base orientation about a per-robot yaw; the IMU acceleration is gravity in the
    base frame plus a small oscillation.  contact(k) switches pattern every `switch` seconds; robots of the second half report it as a mode number."""

    def __init__(self, m, B, seed, dt=0.0025, switch=0.3):
        rng = np.random.default_rng(seed)
        self.m, self.B, self.dt, self.switch = m, B, dt, switch
        nj = m["nj"]
        self.q0 = np.asarray(m["default_joint_state"], float)
        self.ja = rng.uniform(0.02, 0.12, (B, nj))
        self.jf = rng.uniform(0.5, 2.0, (B, nj))
        self.jp = rng.uniform(0.0, 2 * np.pi, (B, nj))
        self.yaw0 = rng.uniform(-1.0, 1.0, B)
        self.ea = rng.uniform(0.02, 0.15, (B, 3))
        self.ef = rng.uniform(0.3, 1.5, (B, 3))
        self.ep = rng.uniform(0.0, 2 * np.pi, (B, 3))
        self.aa = rng.uniform(0.0, 0.5, (B, 3))
        self.af = rng.uniform(0.5, 3.0, (B, 3))
        self.fh = rng.uniform(-0.005, 0.005, (B, 4))
        self.mode_offset = rng.integers(0, 4, B)

    def at(self, k):
        """dict of [B, ...] arrays at tick k: joint_pos, joint_vel, quat, angular_vel_local, linear_accel_local, flags, mode, feet_heights."""
        t = k * self.dt
        B = self.B
        jp = self.q0 + self.ja * np.sin(2 * np.pi * self.jf * t + self.jp)
        jv = self.ja * 2 * np.pi * self.jf * np.cos(2 * np.pi * self.jf * t + self.jp)
        zyx = self.ea * np.sin(2 * np.pi * self.ef * t + self.ep)
        zyx[:, 0] += self.yaw0
        zd = self.ea * 2 * np.pi * self.ef * np.cos(2 * np.pi * self.ef * t + self.ep)
        quat = np.array([quat_from_zyx(z) for z in zyx])
        wl = np.array([wp.rot_zyx(zyx[b]).T @ (wp.euler_rate_map(zyx[b]) @ zd[b]) for b in range(B)])
        al = np.array([wp.rot_zyx(zyx[b]).T @ (np.array([0.0, 0.0, GRAVITY]) + self.aa[b] * np.sin(2 * np.pi * self.af[b] * t)) for b in range(B)])
        mode = (np.array([3, 1, 3, 2])[(int(t / self.switch + 1e-9) + self.mode_offset) % 4]).astype(np.int32)
        flags = np.array([mode_flags(mo) for mo in mode], np.int32)
        return dict(joint_pos=jp, joint_vel=jv, quat=quat, angular_vel_local=wl, linear_accel_local=al, flags=flags, mode=mode, feet_heights=self.fh)
