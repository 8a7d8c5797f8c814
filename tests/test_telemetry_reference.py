"""CPU tier of the tracking telemetry: the numpy restatement tests/telemetry_reference.py against closed forms - equal configurations, a pure base
translation, the yaw wrap, one joint offset, the contact points of the standing state against oracle/wbc_py.py - and its record keeping: ring
wrap-around, decimation, the freeze, a sample that is not finite."""
import math

import numpy as np
import pytest

from oracle import wbc_py as wp
from tests import oracle_bridge as ob
from tests import telemetry_reference as tr
from tests.test_plant_reference import standing_state


def _pair(m, q_des, q_meas):
    """(x_opt, rbd) rows whose configurations are q_des and q_meas"""
    nj = m["nj"]
    x = np.r_[np.zeros(6), q_des]
    rbd = wp.rbd_from(m, np.asarray(q_meas, float), np.zeros(6 + nj))
    return x, rbd


def _q(m, rng, spread=0.3):
    q = np.array(m["initial_state"], float)[6:].copy()
    q[6:] += spread * rng.standard_normal(m["nj"])
    q[3:6] = rng.uniform(-0.5, 0.5, 3)
    return q


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_layout_and_equal_configurations(robot):
    m = ob.model(robot)
    nj = m["nj"]
    assert tr.stride(nj) == {10: 60, 12: 64}[nj]
    q = _q(m, np.random.default_rng(0))
    x, rbd = _pair(m, q, q)
    s = tr.sample(m, x, rbd, t=1.5, safe=1, mode=3, n=7)
    assert np.array_equal(s[0:6], q[:6]) and np.array_equal(s[6:12], q[:6])
    assert np.array_equal(s[36:36 + nj], q[6:]) and np.array_equal(s[36 + nj:36 + 2 * nj], q[6:])
    assert s[36 + 2 * nj:].tolist() == [1.5, 1.0, 3.0, 7.0]
    assert np.array_equal(s[12:24], s[24:36])
    e, ej = tr.errors(s, nj)
    assert np.all(e == 0.0) and np.all(ej == 0.0)


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_pure_base_translation(robot):
    m = ob.model(robot)
    q = _q(m, np.random.default_rng(1))
    d = np.array([0.03, -0.04, 0.12])
    qm = q.copy()
    qm[0:3] -= d
    e, ej = tr.errors(tr.sample(m, *_pair(m, q, qm)), m["nj"])
    nd = np.linalg.norm(d)
    assert abs(e[0] - nd) < 1e-15 and e[1] == 0.0 and e[6] == 0.0 and np.all(ej == 0.0)
    assert np.abs(e[2:6] - nd).max() < 1e-14


def test_yaw_wrap():
    m = ob.model("h1")
    q = _q(m, np.random.default_rng(2))
    qd, qm = q.copy(), q.copy()
    qd[3], qm[3] = 3.1, -3.1
    e, _ = tr.errors(tr.sample(m, *_pair(m, qd, qm)), m["nj"])
    assert abs(e[1] - (2.0 * math.pi - 6.2)) < 1e-14 and abs(e[1] - 0.083) < 2e-4
    qd[3], qm[3] = -3.1, 3.1
    e2, _ = tr.errors(tr.sample(m, *_pair(m, qd, qm)), m["nj"])
    assert abs(e2[1] - e[1]) < 1e-14
    assert tr.normalize_angle(np.array([math.pi]))[0] == math.pi and tr.normalize_angle(np.array([-math.pi]))[0] == math.pi


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_single_joint_offset(robot):
    m = ob.model(robot)
    nj = m["nj"]
    q = _q(m, np.random.default_rng(3))
    for j, delta in ((2, 0.07), (nj - 1, -0.2)):
        qm = q.copy()
        qm[6 + j] -= delta
        t = tr.Telemetry(m, 1)
        x, rbd = _pair(m, q, qm)
        t.update([x], [rbd])
        s = t.summary()
        assert abs(s["max"][0, 6] - abs(delta)) < 1e-15 and s["max"][0, 0] == 0.0 and s["max"][0, 1] == 0.0
        jm = s["joint_max"][0]
        assert abs(jm[j] - abs(delta)) < 1e-15 and np.all(np.delete(jm, j) == 0.0)
        assert abs(s["rms"][0, 6] - abs(delta)) < 1e-15 and s["samples"][0] == 1 and s["first_unsafe"][0] == -1


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_contact_points_of_the_standing_state(robot):
    """the sample's contact points are those of oracle/wbc_py.py that the plant's reference stands the robot on: the lowest ones `depth` in the ground"""
    m = ob.model(robot)
    q, v, _ = standing_state(m, depth=0.005)
    s = tr.sample(m, *_pair(m, q, q))
    R, o, _ = wp.fk(m, q)
    pts = np.array(wp.contact_points(m, R, o))
    assert np.array_equal(s[12:24].reshape(4, 3), pts) and np.array_equal(s[24:36].reshape(4, 3), pts)
    assert abs(s[12:24].reshape(4, 3)[:, 2].min() + 0.005) < 1e-15


def _episode(m, updates, seed=4):
    rng = np.random.default_rng(seed)
    return [_pair(m, _q(m, rng), _q(m, rng)) for _ in range(updates)]


def test_ring_wraps_and_decimates():
    m = ob.model("h1")
    nj = m["nj"]
    ep = _episode(m, 12)
    full = tr.Telemetry(m, 1, ring_len=4)
    half = tr.Telemetry(m, 1, ring_len=4, every=2)
    none = tr.Telemetry(m, 1, ring_len=0)
    for k, (x, rbd) in enumerate(ep):
        for t in (full, half, none):
            t.update([x], [rbd], t=[0.002 * k])
        if k == 2:
            assert half.ring(0)[:, 39 + 2 * nj].tolist() == [0.0, 2.0] and full.ring(0)[:, 39 + 2 * nj].tolist() == [0.0, 1.0, 2.0]
    assert full.ring(0)[:, 39 + 2 * nj].tolist() == [8.0, 9.0, 10.0, 11.0]
    assert half.ring(0)[:, 39 + 2 * nj].tolist() == [4.0, 6.0, 8.0, 10.0]
    assert np.array_equal(half.ring(0)[-1], tr.sample(m, *ep[10], t=0.02, n=10))
    assert none.ring(0).shape == (0, tr.stride(nj)) and none.summary()["samples"][0] == 12
    assert np.array_equal(none.stats, full.stats) and np.array_equal(half.stats, full.stats)


def test_freeze_and_not_finite():
    m = ob.model("h1")
    nj = m["nj"]
    ep = _episode(m, 10)
    B = 3
    frozen = tr.Telemetry(m, B, ring_len=4, every=2)
    free = tr.Telemetry(m, B, ring_len=4, every=2, freeze_on_unsafe=False)
    for k, (x, rbd) in enumerate(ep):
        xs, rs = [x.copy() for _ in range(B)], [rbd.copy() for _ in range(B)]
        safe = [1, 0 if k == 5 else 1, 1]
        if k == 7:
            rs[2][6 + 3] = np.nan
        for t in (frozen, free):
            t.update(xs, rs, safe=safe)
    s, f = frozen.summary(), free.summary()
    assert s["frozen"].tolist() == [0, 1, 1] and f["frozen"].tolist() == [0, 0, 0]
    assert s["first_unsafe"].tolist() == [-1, 5, 7] and f["first_unsafe"].tolist() == [-1, 5, 7]
    # the unsafe sample is finite and accumulated; the one that is not finite is recorded and not accumulated
    assert s["samples"].tolist() == [10, 6, 7] and f["samples"].tolist() == [10, 10, 9]
    assert frozen.n.tolist() == [10, 6, 8] and free.n.tolist() == [10, 10, 10]
    # a frozen ring ends with the freezing sample, at an odd n too
    assert frozen.ring(1)[:, 39 + 2 * nj].tolist() == [0.0, 2.0, 4.0, 5.0] and frozen.ring(2)[:, 39 + 2 * nj].tolist() == [2.0, 4.0, 6.0, 7.0]
    assert np.isnan(frozen.ring(2)[-1][36 + nj + 3]) and frozen.ring(1)[-1][37 + 2 * nj] == 0.0
    assert free.ring(2)[:, 39 + 2 * nj].tolist() == [2.0, 4.0, 6.0, 8.0] and np.all(np.isfinite(f["max"]))
    # a masked reset starts robot 1 over and leaves the others alone
    before = (frozen.stats.copy(), frozen.n.copy())
    frozen.reset(np.array([0, 1, 0]))
    assert frozen.n.tolist() == [10, 0, 8] and frozen.frozen.tolist() == [0, 0, 1] and frozen.ring(1).shape[0] == 0
    assert np.array_equal(frozen.stats[[0, 2]], before[0][[0, 2]]) and frozen.stats[1, tr.FIRST_UNSAFE] == -1.0
