"""numpy restatement of the plant's sensor model, written from the "sensors" paragraph of the Plant comment of include/bpmpc.h and from nothing
else: Philox4x32-10 on uint64 arithmetic, the draw table, seeding, and one measurement with bias walk, quantisation, dropout, ring and delay.
tests/test_plant_sensor_reference.py checks it on its own; tests/test_plant_sensor_capi.py and tests/test_gpu_plant_sensors.py hold the library to it."""
import numpy as np

STRIDE = 16
FIELDS = ("gyro_noise", "gyro_bias_walk", "gyro_bias_init", "accel_noise", "accel_bias_walk", "accel_bias_init", "orientation_noise", "joint_pos_noise",
          "joint_pos_resolution", "joint_vel_noise", "contact_dropout", "delay_steps")
RING = 9
CHANNELS = ("joint_pos", "joint_vel", "quat", "angular_vel_local", "linear_accel_local", "contact")
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
TURN_ON = 0xFFFFFFFFFFFFFFFF


def row(**fields):
    r = np.zeros(STRIDE)
    for k, v in fields.items():
        r[FIELDS.index(k)] = v
    return r


def philox4x32_10(counter, key):
    """counter: four words, key: two words, each a Python int or an array of them (broadcast against each other) -> the four output words as
    uint64 arrays"""
    m = np.uint64(MASK)
    c = [np.asarray(x, np.uint64) & m for x in counter]
    k = [np.asarray(x, np.uint64) & m for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]      # 32 x 32 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m, p1 >> np.uint64(32), p1 & m
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & m, (k[1] + np.uint64(W1)) & m]
    return c


def _key(seed):
    s = int(seed) & TURN_ON      # the seed reinterpreted as unsigned
    return s & MASK, s >> 32


def blocks(seed, robot, tick, index):
    """the words [4, len(index)] of the blocks `index` at (seed, robot, tick); tick = -1: the tick with all 64 bits set"""
    t = TURN_ON if tick < 0 else int(tick)
    index = np.asarray(index, np.uint64)
    return np.array(np.broadcast_arrays(*philox4x32_10((t & MASK, t >> 32, robot, index), _key(seed)), index)[:4])


def uniform(w):
    return (np.asarray(w, np.uint64).astype(np.float64) + 0.5) * 2.0 ** -32


def draw(seed, robot, tick):
    """(z[64], u[4]) at (seed, robot, tick); tick = -1: the turn-on draw"""
    w = blocks(seed, robot, tick, np.arange(32))                 # [4, 32]
    u1 = uniform(np.stack([w[0], w[2]], axis=1).reshape(-1))     # z[g]: block g >> 1, words (0, 1) for even g, (2, 3) for odd g
    u2 = uniform(np.stack([w[1], w[3]], axis=1).reshape(-1))
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return z, uniform(blocks(seed, robot, tick, [32])[:, 0])


def quat_mul(a, b):
    """Hamilton product of two quaternions x y z w"""
    av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
    return np.r_[aw * bv + bw * av + np.cross(av, bv), aw * bw - av @ bv]


class Sensors:
    """The sensor model's state of one robot (index `robot` in its batch) and its calls"""

    def __init__(self, robot, params=None, seed=0):
        self.robot, self.params = robot, np.zeros(STRIDE) if params is None else np.array(params, float)
        self.seed, self.t, self.n = seed, 0, 0
        self.bg, self.ba = np.zeros(3), np.zeros(3)
        self.ring = [None] * RING

    def seed_sensors(self, seed):
        p = dict(zip(FIELDS, self.params))
        self.seed, self.t, self.n = seed, 0, 0
        z0, _ = draw(seed, self.robot, -1)
        self.bg, self.ba = p["gyro_bias_init"] * z0[0:3], p["accel_bias_init"] * z0[3:6]

    def set_state(self):
        self.n = 0

    def pre_rounding_joint_pos(self, truth):
        """joint_pos + noise at the current tick, before quantisation (what the quantisation test inspects)"""
        z, _ = draw(self.seed, self.robot, self.t)
        nj = len(truth["joint_pos"])
        return np.asarray(truth["joint_pos"], float) + self.params[FIELDS.index("joint_pos_noise")] * z[16:16 + nj]

    def sense(self, truth, period):
        """One measurement of `truth` (a dict with the six CHANNELS) after a control step of `period`; returns the sensed sample"""
        p = dict(zip(FIELDS, self.params))
        nj = len(truth["joint_pos"])
        z, u = draw(self.seed, self.robot, self.t)
        self.bg = self.bg + p["gyro_bias_walk"] * np.sqrt(period) * z[3:6]
        self.ba = self.ba + p["accel_bias_walk"] * np.sqrt(period) * z[9:12]
        s = {}
        s["angular_vel_local"] = np.asarray(truth["angular_vel_local"], float) + self.bg + p["gyro_noise"] * z[0:3]
        s["linear_accel_local"] = np.asarray(truth["linear_accel_local"], float) + self.ba + p["accel_noise"] * z[6:9]
        quat = np.asarray(truth["quat"], float)
        if p["orientation_noise"] > 0:
            delta = p["orientation_noise"] * z[12:15]
            a = np.linalg.norm(delta)
            q = quat_mul(quat, np.r_[delta * (np.sin(a / 2) / a), np.cos(a / 2)])
            quat = q / np.linalg.norm(q)
        s["quat"] = quat
        jp = np.asarray(truth["joint_pos"], float) + p["joint_pos_noise"] * z[16:16 + nj]
        if p["joint_pos_resolution"] > 0:
            jp = np.rint(jp / p["joint_pos_resolution"]) * p["joint_pos_resolution"]
        s["joint_pos"] = jp
        s["joint_vel"] = np.asarray(truth["joint_vel"], float) + p["joint_vel_noise"] * z[32:32 + nj]
        s["contact"] = ((np.asarray(truth["contact"]) != 0) & ~(u < p["contact_dropout"])).astype(np.int32)
        self.ring[self.n % RING] = s
        d = int(min(max(p["delay_steps"], 0), RING - 1))
        out = self.ring[max(self.n - d, 0) % RING]
        self.t += 1
        self.n += 1
        return out
