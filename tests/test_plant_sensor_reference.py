"""CPU tier: the numpy restatement of the plant's sensor model (tests/plant_sensor_reference.py) on its own - the generator's known answers, the
statistics of its Gaussian stream, the zero row, the delay rule.  Nothing here touches the library."""
import numpy as np
import pytest

from tests import plant_sensor_reference as sr

NJ = 10


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("counter, key, answer", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, answer):
    assert _hex(sr.philox4x32_10(counter, key)) == answer


def test_counter_and_key_layout():
    """counter = (tick low, tick high, robot, block), key = (seed low, seed high); the turn-on draw is the tick with all 64 bits set; a negative
    seed is reinterpreted as unsigned"""
    tick, seed = (5 << 32) | 9, (3 << 32) | 4
    assert _hex(sr.blocks(seed, 2, tick, [7])[:, 0]) == _hex(sr.philox4x32_10((9, 5, 2, 7), (4, 3)))
    assert _hex(sr.blocks(-1, 2, -1, [7])[:, 0]) == _hex(sr.philox4x32_10((0xFFFFFFFF, 0xFFFFFFFF, 2, 7), (0xFFFFFFFF, 0xFFFFFFFF)))
    z, u = sr.draw(seed, 2, tick)
    w = sr.blocks(seed, 2, tick, [3, 32])
    assert z[6] == np.sqrt(-2.0 * np.log(sr.uniform(w[0, 0]))) * np.cos(2.0 * np.pi * sr.uniform(w[1, 0]))      # even g: words (0, 1) of block g >> 1
    assert z[7] == np.sqrt(-2.0 * np.log(sr.uniform(w[2, 0]))) * np.cos(2.0 * np.pi * sr.uniform(w[3, 0]))      # odd g: words (2, 3)
    assert np.array_equal(u, sr.uniform(w[:, 1]))
    assert sr.uniform(0) == 2.0 ** -33 and sr.uniform(0xFFFFFFFF) == 1.0 - 2.0 ** -33


def test_gaussian_stream_statistics():
    """200 000 draws of (seed 7, robot 3), z[0] and z[1] of the ticks 0..99 999: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N) (measured: -5.5e-4
    and 0.99947 against 0.0112 and 0.0158); no draw beyond sqrt(2 ln 2^33) = 6.76.  The first ticks are the draws of sr.draw itself."""
    N = 200000
    w = sr.philox4x32_10((np.arange(N // 2), 0, 3, 0), (7, 0))      # block 0 of every tick
    z = np.stack([np.sqrt(-2.0 * np.log(sr.uniform(w[0]))) * np.cos(2.0 * np.pi * sr.uniform(w[1])),
                  np.sqrt(-2.0 * np.log(sr.uniform(w[2]))) * np.cos(2.0 * np.pi * sr.uniform(w[3]))], axis=1)
    for t in (0, 1, 77):
        assert np.array_equal(z[t], sr.draw(7, 3, t)[0][:2])
    z = z.reshape(-1)
    assert z.size == N
    mean, var = z.mean(), z.var()
    print("gaussian stream: mean %.3e (bound %.3e), var %.6f (bound %.3e), max |z| %.3f" % (mean, 5 / np.sqrt(N), var, 5 * np.sqrt(2 / N), np.abs(z).max()))
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1.0) <= 5 * np.sqrt(2.0 / N)
    assert np.abs(z).max() <= np.sqrt(2.0 * np.log(2.0 ** 33))
    # the uniforms of the same ticks lie inside (0, 1)
    u = np.concatenate([sr.draw(7, 3, t)[1] for t in range(64)])
    assert u.min() > 0.0 and u.max() < 1.0


def _truth(rng, k):
    q = rng.standard_normal(4)
    return {"joint_pos": rng.standard_normal(NJ), "joint_vel": rng.standard_normal(NJ), "quat": q / np.linalg.norm(q), "angular_vel_local": rng.standard_normal(3),
            "linear_accel_local": rng.standard_normal(3) + [0, 0, 9.81], "contact": np.array([1, k % 2, 1, (k // 2) % 2], np.int32)}


def test_zero_row_is_the_identity():
    rng = np.random.default_rng(0)
    s = sr.Sensors(robot=4, seed=11)
    s.seed_sensors(11)
    assert not s.bg.any() and not s.ba.any()
    for k in range(12):
        truth = _truth(rng, k)
        out = s.sense(truth, 0.002)
        for c in sr.CHANNELS:
            assert np.array_equal(out[c], truth[c]), c
    assert s.t == 12 and s.n == 12


@pytest.mark.parametrize("delay", [0, 1, 3, 8])
def test_delay_index_rule(delay):
    """the sensed sample at step n is the measured sample max(n - d, 0), over 12 samples (the ring of 9 wraps); a twin without delay measures the
    same samples"""
    rng = np.random.default_rng(1)
    noisy = dict(gyro_noise=0.01, gyro_bias_walk=0.001, accel_noise=0.1, joint_pos_noise=0.001, joint_vel_noise=0.01, orientation_noise=0.01, contact_dropout=0.3)
    late, twin = sr.Sensors(1, sr.row(delay_steps=delay, **noisy), seed=5), sr.Sensors(1, sr.row(**noisy), seed=5)
    samples = []
    for n in range(12):
        truth = _truth(rng, n)
        samples.append(twin.sense(truth, 0.002))
        out = late.sense(truth, 0.002)
        for c in sr.CHANNELS:
            assert np.array_equal(out[c], samples[max(n - delay, 0)][c]), (n, c)
    assert any(not np.array_equal(samples[0]["angular_vel_local"], s["angular_vel_local"]) for s in samples[1:])
    # set_state forgets the history: the next sensed sample is the next measured one
    late.set_state()
    twin.set_state()
    truth = _truth(rng, 12)
    fresh = twin.sense(truth, 0.002)
    assert np.array_equal(late.sense(truth, 0.002)["joint_vel"], fresh["joint_vel"]) and late.n == 1 and late.t == 13


def test_seed_bias_quantisation_and_dropout():
    s = sr.Sensors(2, sr.row(gyro_bias_init=0.02, accel_bias_init=0.3))
    s.seed_sensors(9)
    z0, _ = sr.draw(9, 2, -1)
    assert np.array_equal(s.bg, 0.02 * z0[0:3]) and np.array_equal(s.ba, 0.3 * z0[3:6]) and s.bg.any()
    rng = np.random.default_rng(2)
    truth = _truth(rng, 3)
    res = 2 * np.pi / 2 ** 14
    q = sr.Sensors(0, sr.row(joint_pos_resolution=res)).sense(truth, 0.002)["joint_pos"]
    assert np.array_equal(q, np.rint(truth["joint_pos"] / res) * res) and np.abs(q - truth["joint_pos"]).max() <= res / 2
    truth["contact"][:] = 1
    assert sr.Sensors(0, sr.row(contact_dropout=1.0)).sense(truth, 0.002)["contact"].tolist() == [0, 0, 0, 0]
    assert sr.Sensors(0, sr.row(contact_dropout=0.0)).sense(truth, 0.002)["contact"].tolist() == [1, 1, 1, 1]
