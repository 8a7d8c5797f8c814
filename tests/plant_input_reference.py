"""numpy restatement of the plant's input model, written from the "inputs" paragraph of the Plant comment of include/bpmpc.h and from nothing else:
integer nanoseconds, the loss, the ring and the delay, the push windows.  The generator is the sensors' (tests/plant_sensor_reference.py) with the
blocks 64 and 65.  tests/test_plant_input_reference.py checks it on its own; tests/test_plant_input_capi.py and tests/test_gpu_plant_inputs.py hold
the library to it."""
import numpy as np

from tests.plant_sensor_reference import blocks, philox4x32_10, uniform  # noqa: F401

STRIDE = 8
FIELDS = ("delay", "dropout", "push_force", "push_interval", "push_duration")
RING = 16
ROWS = ("pos_des", "vel_des", "tau_ff", "kp", "kd")
LOSS_BLOCK, PUSH_BLOCK = 64, 65
MAX_NS = 1 << 62


def row(**fields):
    r = np.zeros(STRIDE)
    for k, v in fields.items():
        r[FIELDS.index(k)] = v
    return r


def clamp(x):
    """not a number, or negative: 0"""
    return float(x) if x > 0.0 else 0.0


def ns(x):
    """integer nanoseconds of a clamped time: llrint(x 1e9), ties to even; 2^62 ns or more: 2^62 ns"""
    v = clamp(x) * 1e9
    return MAX_NS if v >= float(MAX_NS) else int(np.rint(v))


def period_ns(period):
    return max(1, ns(period))


def delay_steps(delay, period):
    return min(RING - 1, ns(delay) // period_ns(period))


def push_windows(push_force, push_interval, push_duration, period):
    """(W, D), or None when the pushes are off"""
    P = period_ns(period)
    if not clamp(push_force) > 0.0 or ns(push_interval) <= 0:
        return None
    W = max(1, ns(push_interval) // P)
    return W, min(W, max(1, ns(push_duration) // P))


def draw(seed, robot, counter):
    """(u_drop of block 64, u_s and u_dir of block 65) of (seed, robot) at `counter`"""
    w = blocks(seed, robot, counter, [LOSS_BLOCK, PUSH_BLOCK])      # [4, 2]
    u = uniform(w)
    return float(u[0, 0]), float(u[0, 1]), float(u[1, 1])


class Inputs:
    """The input model's state of one robot (index `robot` in its batch) and its calls"""

    def __init__(self, robot, params=None, seed=0):
        self.robot, self.params = robot, np.zeros(STRIDE) if params is None else np.array(params, float)
        self.seed, self.t, self.n = seed, 0, 0
        self.ring = [None] * RING

    def seed_inputs(self, seed):
        self.seed, self.t, self.n = seed, 0, 0

    def set_state(self):
        self.n = 0

    def step(self, command, force, period):
        """One control step: `command` (anything; the five rows as one object or array) and the caller's base force [3] (None: 0) ->
        (applied command, applied force [3], lost, pushing, delay_steps)"""
        p = dict(zip(FIELDS, self.params))
        u_drop = draw(self.seed, self.robot, self.t)[0]
        lost = self.n > 0 and u_drop < min(clamp(p["dropout"]), 1.0)
        arrived = self.ring[(self.n - 1) % RING] if lost else command
        self.ring[self.n % RING] = arrived
        k = delay_steps(p["delay"], period)
        applied = self.ring[max(self.n - k, 0) % RING]
        f = np.zeros(3) if force is None else np.array(force, float)
        pushing = False
        windows = push_windows(p["push_force"], p["push_interval"], p["push_duration"], period)
        if windows:
            W, D = windows
            w, o = self.t // W, self.t % W
            _, u_s, u_dir = draw(self.seed, self.robot, w)
            s = min(W - D, int(np.floor(u_s * (W - D + 1))))
            pushing = s <= o < s + D
            if pushing:
                f = f + clamp(p["push_force"]) * np.array([np.cos(2.0 * np.pi * u_dir), np.sin(2.0 * np.pi * u_dir), 0.0])
        self.t += 1
        self.n += 1
        return applied, f, int(lost), int(pushing), k
