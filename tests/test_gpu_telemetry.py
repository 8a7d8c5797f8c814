"""GPU tier: the tracking telemetry (include/bpmpc.h "Tracking telemetry"; kernels/telemetry.h k_telemetry) against the numpy restatement
tests/telemetry_reference.py, whose kinematics are oracle/wbc_py.py fk / contact_points.
  samples      H1 batch 5 in a handle of 8 (the last wavefront holds one robot of four), G1 batch 3 (one of two), batch 1; joints within 0.5 rad of
               the default joint state, base height 0.6 .. 1.1, pitch and roll up to 1.2, yaws within 0.05 of +-pi with desired and measured on
               opposite sides; three updates; 1e-12 absolute - the bound tests/test_gpu_plant_sensors.py holds FP64 compositions of a few rotations
               on values of order 1 to (tests/tolerances.py has no entry for the WBC's kinematic quantities)
  statistics   twelve updates at batch 5 against the restatement fed the kernel's own samples: sums 1e-12 relative (twelve sequential accumulations
               differ by a few ulp under multiply-add contraction: a factor above 100), maxima, max_at, samples, first_unsafe and joint_max exactly
  freeze       safe = 0 at update 5, a NaN joint at update 7; a device-mask reset of one robot at update 9 against a handle that saw no reset
  ring         ring_len 4, every 2; a frozen ring; robots = [3, 0]; ring_len 0
  host arrays and device pointers the same bits
  attached     the tick's outputs bit-identical to a detached tick; the attached sample bit for bit bpmpc_telemetry_update of the tick's outputs;
               the same with a policy buffer; detached, the counter stops
  the loop     step_controlled -> update_from_plant -> tick_estimated, 20 ticks, no host synchronise inside
Every comparison prints its maximum before it asserts (pytest -s)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

from oracle import wbc_py as wp
from tests import oracle_bridge as ob
from tests import telemetry_reference as tr

pytestmark = pytest.mark.gpu
TOL = 1e-12
INVALID, CAPACITY = -1, -6


def _itf(robot):
    from bipedal_control_amd import scenarios as sc
    return sc.interface(robot)


def _handle(robot, max_batch, ring_len=0):
    import bipedal_control_amd as bp
    return bp.BatchedTelemetry(_itf(robot), max_batch, ring_len=ring_len)


def _episode(robot, B, updates, seed=0):
    """updates x (x_opt [B, 12 + nj], rbd [B, 2 (6 + nj)], t [B], safe [B], mode [B]) in the ranges of the module docstring"""
    m = ob.model(robot)
    nj = m["nj"]
    rng = np.random.default_rng(seed)
    q0 = np.array(m["initial_state"], float)[12:]
    out = []
    for k in range(updates):
        xs, rs = np.zeros((B, 12 + nj)), np.zeros((B, 2 * (6 + nj)))
        for b in range(B):
            qs = []
            for side in (1.0, -1.0):
                q = np.zeros(6 + nj)
                q[0:2] = rng.uniform(-2.0, 2.0, 2)
                q[2] = rng.uniform(0.6, 1.1)
                q[3] = rng.uniform(-3.0, 3.0)
                q[4:6] = rng.uniform(-1.2, 1.2, 2)
                q[6:] = q0 + rng.uniform(-0.5, 0.5, nj)
                qs.append(q)
            if (b + k) % 2 == 0:                                    # desired and measured yaw on opposite sides of +-pi
                sign = 1.0 if b % 4 < 2 else -1.0
                qs[0][3] = sign * (math.pi - rng.uniform(0.0, 0.05))
                qs[1][3] = -sign * (math.pi - rng.uniform(0.0, 0.05))
            xs[b] = np.r_[rng.standard_normal(6), qs[0]]
            rs[b] = wp.rbd_from(m, qs[1], rng.standard_normal(6 + nj))
        out.append((xs, rs, np.full(B, 0.002 * k), np.ones(B, np.int32), rng.integers(0, 4, B).astype(np.int32)))
    return m, out


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _last(tel, B):
    torch.cuda.synchronize()
    return tel.outputs()["sample"].torch().cpu().numpy()[:B]


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("robot,B,max_batch", [("h1", 5, 8), ("g1", 3, 3), ("h1", 1, 1), ("g1", 1, 2)])
def test_samples_against_restatement(robot, B, max_batch):
    m, ep = _episode(robot, B, 3, seed=B)
    nj = m["nj"]
    tel = _handle(robot, max_batch, ring_len=4)
    assert (tel.sample_stride, tel.stats_stride) == (tr.stride(nj), 40)
    ref = tr.Telemetry(m, B, ring_len=4)
    worst, wraps = 0.0, 0
    for x, rbd, t, safe, mode in ep:
        tel.update(x, rbd, t=t, safe=safe, planned_mode=mode)
        ref.update(x, rbd, t=t, safe=safe, mode=mode)
        got = _last(tel, B)
        worst = max(worst, np.abs(got - ref.last).max())
        wraps += int((np.abs(x[:, 9] - rbd[:, 0]) > 6.0).sum())
    ring = tel.ring()
    assert ring["count"].tolist() == [3] * B and wraps >= B
    for b in range(B):
        worst = max(worst, np.abs(ring["samples"][b, :3] - ref.ring(b)).max())
    # the entries that are copies are the inputs' bits
    x, rbd = ep[-1][0], ep[-1][1]
    assert _same(got[:, 0:6], x[:, 6:12]) and _same(got[:, 6:9], rbd[:, 3:6]) and _same(got[:, 9:12], rbd[:, 0:3])
    assert _same(got[:, 36:36 + nj], x[:, 12:]) and _same(got[:, 36 + nj:36 + 2 * nj], rbd[:, 6:6 + nj])
    assert _same(got[:, 36 + 2 * nj:], np.c_[ep[-1][2], ep[-1][3], ep[-1][4], np.full(B, 2.0)])
    s = tel.stats()
    print("telemetry samples %s batch %d: max |kernel - restatement| %.3e; yaw error max %.4f" % (robot, B, worst, s["max"][:, 1].max()))
    assert worst <= TOL
    assert s["max"][:, 1].max() <= math.sqrt(3.0) * math.pi and s["samples"].tolist() == [3] * B and not s["frozen"].any()
    assert np.array_equal(ring["n"][:, :3], np.tile(np.arange(3.0), (B, 1))) and np.all(ring["samples"][:, 3] == 0.0)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_statistics_against_restatement_of_the_kernels_samples(robot):
    B, N = 5, 12
    m, ep = _episode(robot, B, N, seed=21)
    nj = m["nj"]
    tel = _handle(robot, 8, ring_len=N)
    for x, rbd, t, safe, mode in ep:
        tel.update(x, rbd, t=t, safe=safe, planned_mode=mode)
    ring = tel.ring()
    assert ring["count"].tolist() == [N] * B
    ref = tr.Telemetry(m, B)
    for k in range(N):
        ref.update(None, None, safe=ep[k][3], samples=ring["samples"][:, k])
    got, want = tel.stats(), ref.summary()
    rows = got["rows"]
    sums, sums_ref = rows[:, 0:21:3], ref.stats[:, 0:21:3]
    rel = np.abs(sums - sums_ref) / sums_ref
    print("telemetry statistics %s: sums max relative difference %.3e; max e" % (robot, rel.max()), got["max"].max(axis=0))
    assert rel.max() <= 1e-12
    for key in ("max", "max_at", "samples", "first_unsafe", "joint_max", "frozen"):
        assert np.array_equal(got[key], want[key]), key
    assert got["samples"].tolist() == [N] * B and got["first_unsafe"].tolist() == [-1] * B
    assert np.all(rows[:, 23 + nj:] == 0.0) and np.abs(got["rms"] - want["rms"]).max() <= 1e-12 * want["rms"].max()


# ---------------------------------------------------------------------------------------------------------------- 3
def _unsafe_episode(robot="h1", B=5, N=12):
    m, ep = _episode(robot, B, N, seed=33)
    ep[5][3][2] = 0                                   # robot 2 is unsafe at update 5
    ep[7][1][4, 6 + 3] = np.nan                       # robot 4 measures a NaN joint at update 7
    return m, ep


def _state(tel, B):
    s = tel.stats(B)
    return s["rows"].copy(), s["frozen"].copy(), tel.ring(batch=B)["samples"].copy(), tel.ring(batch=B)["count"].copy(), _last(tel, B).copy()


def test_freeze_and_masked_reset():
    B, N = 5, 12
    m, ep = _unsafe_episode()
    nj = m["nj"]
    a, plain, free = _handle("h1", 8, ring_len=4), _handle("h1", 8, ring_len=4), _handle("h1", 8, ring_len=4)
    free.configure(every=1, freeze_on_unsafe=False)
    mask = torch.tensor([0, 0, 1, 0, 0], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    at_freeze = {}
    for k, (x, rbd, t, safe, mode) in enumerate(ep):
        if k == 9:
            for b in (2, 4):                          # unchanged by the updates since they froze, bit for bit
                rows, frozen, rings, counts, last = _state(a, B)
                assert frozen[b] == 1 and _same(rows[b], at_freeze[b][0]) and _same(rings[b], at_freeze[b][1]) and _same(last[b], at_freeze[b][2])
            a.reset(mask)                             # the (safe == 0) mask of a restart, on the device: only enqueued
        for tel in (a, plain, free):
            tel.update(x, rbd, t=t, safe=safe, planned_mode=mode)
        if k in (5, 7):
            b = 2 if k == 5 else 4
            rows, frozen, rings, counts, last = _state(a, B)
            assert frozen.tolist() == ([0, 0, 1, 0, 0] if k == 5 else [0, 0, 1, 0, 1])
            at_freeze[b] = (rows[b].copy(), rings[b].copy(), last[b].copy())
            assert rows[b, tr.FIRST_UNSAFE] == k and last[b, 39 + 2 * nj] == k and rings[b, counts[b] - 1, 39 + 2 * nj] == k
    ra, rp = _state(a, B), _state(plain, B)
    others = [0, 1, 3, 4]
    for got, want in zip(ra, rp):
        assert _same(got[others], want[others])
    assert rp[1].tolist() == [0, 0, 1, 0, 1] and ra[1].tolist() == [0, 0, 0, 0, 1]
    sa = a.stats(B)
    assert sa["samples"].tolist() == [12, 12, 3, 12, 7] and sa["first_unsafe"].tolist() == [-1, -1, -1, -1, 7]
    assert ra[4][2, 39 + 2 * nj] == 2.0 and a.ring([2], batch=B)["n"][0, :3].tolist() == [0.0, 1.0, 2.0] and ra[3][2] == 3      # robot 2 counts from 0
    assert _same(rp[0][2], at_freeze[2][0]) and np.isnan(at_freeze[4][2][36 + nj + 3])
    assert at_freeze[2][0][tr.SAMPLES] == 6 and at_freeze[4][0][tr.SAMPLES] == 7      # the unsafe sample is accumulated, the NaN one is not
    sf = free.stats(B)
    assert not sf["frozen"].any() and sf["first_unsafe"].tolist() == [-1, -1, 5, -1, 7] and sf["samples"].tolist() == [12, 12, 12, 12, 11]
    assert np.all(np.isfinite(sf["rows"])) and free.ring(batch=B)["n"][:, -1].tolist() == [11.0] * B


# ---------------------------------------------------------------------------------------------------------------- 4
def test_ring():
    B, N = 5, 12
    m, ep = _episode("h1", B, N, seed=44)
    nj = m["nj"]
    ep[5][3][1] = 0                                   # robot 1 falls at an odd n
    tel, none = _handle("h1", 8, ring_len=4), _handle("h1", 8, ring_len=0)
    tel.configure(every=2)
    ref = tr.Telemetry(m, B, ring_len=4, every=2)
    for k, (x, rbd, t, safe, mode) in enumerate(ep):
        tel.update(x, rbd, t=t, safe=safe, planned_mode=mode)
        none.update(x, rbd, t=t, safe=safe, planned_mode=mode)
        ref.update(x, rbd, t=t, safe=safe, mode=mode)
        if k == 2:
            early = tel.ring()
            assert early["count"].tolist() == [2] * B and early["n"][:, :2].tolist() == [[0.0, 2.0]] * B
    ring = tel.ring()
    assert ring["count"].tolist() == [4] * B
    for b in range(B):
        assert ring["n"][b].tolist() == ([0.0, 2.0, 4.0, 5.0] if b == 1 else [4.0, 6.0, 8.0, 10.0])
        assert np.abs(ring["samples"][b] - ref.ring(b)).max() <= TOL
    assert ring["safe"][1, -1] == 0.0 and np.array_equal(ring["t"][0], 0.002 * np.array([4.0, 6.0, 8.0, 10.0]))
    two = tel.ring(robots=[3, 0])
    assert two["count"].tolist() == [4, 4] and _same(two["samples"][0], ring["samples"][3]) and _same(two["samples"][1], ring["samples"][0])
    assert two["contact_pos_desired"].shape == (2, 4, 4, 3)
    empty = none.ring()
    assert empty["count"].tolist() == [0] * B and empty["samples"].shape == (B, 0, tr.stride(nj))
    assert none.stats()["samples"].tolist() == [12, 6, 12, 12, 12] and _same(none.stats()["rows"], tel.stats()["rows"])


# ---------------------------------------------------------------------------------------------------------------- 5
def test_host_arrays_and_device_pointers_give_the_same_bits():
    B = 5
    m, ep = _unsafe_episode()
    host, dev = _handle("h1", 8, ring_len=4), _handle("h1", 8, ring_len=4)
    on = [[torch.tensor(a, device="cuda") for a in step] for step in ep]
    torch.cuda.synchronize()
    for step, dstep in zip(ep, on):
        host.update(step[0], step[1], t=step[2], safe=step[3], planned_mode=step[4])
        dev.update(dstep[0], dstep[1], t=dstep[2], safe=dstep[3], planned_mode=dstep[4])      # only enqueued
    for got, want in zip(_state(dev, B), _state(host, B)):
        assert _same(got, want)
    # without t, safe and planned_mode the fields are 0 and nothing is unsafe
    bare = _handle("h1", 8)
    bare.update(ep[5][0], ep[5][1])
    nj = m["nj"]
    assert np.all(_last(bare, B)[:, 36 + 2 * nj:] == 0.0) and not bare.stats()["frozen"].any() and bare.stats()["first_unsafe"].tolist() == [-1] * B


# ---------------------------------------------------------------------------------------------------------------- 6
TICK = ("x_obs", "x_opt", "u_opt", "joint_cmd", "wbc_solution", "planned_mode", "wbc_status", "safe", "joint_torque", "joint_kp", "joint_kd")


def _standalone(robot, out, t, rbd):
    tel = _handle(robot, len(t))
    tel.update(out["x_opt"], rbd, t=t, safe=out["safe"], planned_mode=out["planned_mode"])
    return _last(tel, len(t))


def test_attached_to_a_controller():
    import bipedal_control_amd as bp
    from tests.test_gpu_controller_tick import _rbd, _solved
    itf = _itf("h1")
    m = ob.model("h1")
    prob, mpc, _ = _solved(itf, gaits=["trot"], commands=[(0.3, 0.0), (0.0, 0.1), (-0.2, 0.0)])
    B = prob["x0"].shape[0]
    assert B == 3
    rng = np.random.default_rng(9)
    rbd = np.array([_rbd(m, prob["x0"][b], rng, speed=0.05, consistent_mode=3)[0] for b in range(B)])
    t = np.array([0.01, 0.02, 0.03])
    detached, attached = (bp.BatchedController(mpc, bp.WeightedWbc(itf, max_batch=B)) for _ in range(2))      # fresh WBC state each
    tel = _handle("h1", 4, ring_len=2)
    attached.attachTelemetry(tel)
    want, got = detached.tick(t, rbd), attached.tick(t, rbd)
    for k in TICK:
        assert _same(got[k], want[k]), k
    sample = _last(tel, B)
    assert _same(sample, _standalone("h1", got, t, rbd)) and tel.stats(B)["samples"].tolist() == [1] * B
    assert np.all(sample[:, 39 + 2 * m["nj"]] == 0.0) and _same(sample[:, 36:36 + m["nj"]], got["x_opt"][:, 12:])
    got2 = attached.tick(t + 0.002, rbd)
    second = _standalone("h1", got2, t + 0.002, rbd)                       # a fresh handle: its n is 0, the attached one's 1
    assert tel.stats(B)["samples"].tolist() == [2] * B and _same(_last(tel, B), np.c_[second[:, :-1], np.ones(B)])
    attached.attachTelemetry(None)                    # detached, the counter stops
    attached.tick(t + 0.004, rbd)
    assert tel.stats(B)["samples"].tolist() == [2] * B and _last(tel, B)[:, -1].tolist() == [1.0] * B


def test_attached_with_a_policy_buffer():
    from tests.test_gpu_policy_buffer import Rig
    r = Rig("h1", 3)
    want = r.reference("A")
    r.pol.publish()
    assert r.pol.update() is True
    tel = _handle("h1", 3, ring_len=2)
    r.buf.attachTelemetry(tel)
    got = r.tick(r.buf)                               # on the buffer's stream
    for k in TICK:
        assert _same(got[k], want[k]), k
    assert _same(_last(tel, 3), _standalone("h1", got, r.tq, r.rbd)) and tel.stats(3)["samples"].tolist() == [1, 1, 1]
    r.buf.attachTelemetry(None)
    r.tick(r.buf)
    assert tel.stats(3)["samples"].tolist() == [1, 1, 1]


# ---------------------------------------------------------------------------------------------------------------- 7
def test_the_loop_records_every_tick():
    from tests import test_gpu_plant as tp
    lp = tp._Loop()
    NB, TICKS = tp.NB, 20
    tel = _handle("h1", NB, ring_len=8)
    lp.plant.set_state(lp.rbd0)
    lp.arm(0.0, True)
    t = torch.zeros(NB, dtype=torch.float64, device="cuda")
    times = [torch.full((NB,), 0.002 * (k + 1), dtype=torch.float64, device="cuda") for k in range(TICKS)]
    torch.cuda.synchronize()
    lp.ctrl.tick(t, lp.plant.outputs()["rbd"].torch(), period=0.002, fetch=False)
    lp.ctrl.attachTelemetry(tel)
    for k in range(TICKS):                            # no host synchronise inside
        lp.plant.step_controlled(lp.ctrl, period=0.002, substeps=4)
        lp.est.update_from_plant(lp.plant, period=0.002, fetch=False)
        lp.ctrl.tick_estimated(times[k], lp.est, period=0.002, fetch=False)
        if k % tp.REARM == tp.REARM - 1:
            lp.arm(0.002 * (k + 1), False)
    s = tel.stats(NB)
    ring = tel.ring(batch=NB)
    print("telemetry loop: rms", s["rms"].max(axis=0), "joint_max", s["joint_max"].max(axis=0))
    assert s["samples"].tolist() == [TICKS] * NB and not s["frozen"].any() and s["first_unsafe"].tolist() == [-1] * NB
    assert np.all(np.isfinite(s["rows"])) and np.all(np.isfinite(ring["samples"])) and ring["count"].tolist() == [8] * NB
    assert np.array_equal(ring["n"], np.tile(np.arange(12.0, 20.0), (NB, 1))) and np.allclose(ring["t"][:, -1], 0.04)
    lp.ctrl.attachTelemetry(None)


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_handle_refusals(robot="h1"):
    """every < 1, a batch above max_batch, a robot index outside the batch: by name, with the right status, changing nothing"""
    import bipedal_control_amd as bp
    lib = bp.load_library()
    m, ep = _episode(robot, 5, 1, seed=5)
    tel = _handle(robot, 4, ring_len=2)
    tel.update(ep[0][0][:4], ep[0][1][:4])
    before = _state(tel, 4)

    def refused(call, status, *words):
        with pytest.raises(bp.BpmpcError) as err:
            call()
        msg = lib.bpmpc_last_error()
        assert err.value.status == status and all(w in msg for w in words), msg

    refused(lambda: tel.configure(every=0), INVALID, b"bpmpc_telemetry_configure", b"every")
    refused(lambda: tel.configure(every=-3), INVALID, b"every")
    refused(lambda: tel.update(ep[0][0], ep[0][1]), CAPACITY, b"bpmpc_telemetry_update", b"max_batch")
    refused(lambda: tel.reset(np.ones(5, np.int32)), CAPACITY, b"bpmpc_telemetry_reset", b"max_batch")
    refused(lambda: tel.stats(5), CAPACITY, b"bpmpc_telemetry_get_stats", b"max_batch")
    refused(lambda: tel.ring(batch=5), CAPACITY, b"bpmpc_telemetry_fetch_ring", b"max_batch")
    refused(lambda: tel.ring(robots=[0, 4], batch=4), INVALID, b"bpmpc_telemetry_fetch_ring", b"robots[1] = 4", b"outside the batch")
    refused(lambda: tel.ring(robots=[-1], batch=4), INVALID, b"robots[0] = -1")
    refused(lambda: tel.ring(robots=[3], batch=3), INVALID, b"robots[0] = 3")
    counts = (C.c_int * 4)()
    assert lib.bpmpc_telemetry_fetch_ring(tel._h, 4, None, 0, None, None) == INVALID and b"null" in lib.bpmpc_last_error()
    assert lib.bpmpc_telemetry_update(tel._h, 4, None, None, ep[0][1].ctypes.data_as(C.POINTER(C.c_double)), None, None, 0) == INVALID
    assert b"null" in lib.bpmpc_last_error() and lib.bpmpc_telemetry_fetch_ring(tel._h, 4, None, 0, None, counts) == 0 and list(counts) == [1] * 4
    for got, want in zip(_state(tel, 4), before):
        assert _same(got, want)
    tel.update(ep[0][0][:4], ep[0][1][:4])            # every is still 1
    assert tel.ring(batch=4)["count"].tolist() == [2] * 4


def test_refusals():
    import bipedal_control_amd as bp
    from tests.test_gpu_controller_tick import _rbd, _solved
    check_handle_refusals("h1")
    lib = bp.load_library()
    itf = _itf("h1")
    m = ob.model("h1")
    prob, mpc, _ = _solved(itf, gaits=["trot"], commands=[(0.3, 0.0), (0.0, 0.1), (-0.2, 0.0)])
    B = prob["x0"].shape[0]
    ctrl = bp.BatchedController(mpc, bp.WeightedWbc(itf, max_batch=B))
    with pytest.raises(bp.BpmpcError) as err:
        ctrl.attachTelemetry(_handle("g1", B))
    assert err.value.status == INVALID and b"bpmpc_controller_attach_telemetry" in lib.bpmpc_last_error() and b"different robots" in lib.bpmpc_last_error()
    small = _handle("h1", B - 1)
    ctrl.attachTelemetry(small)
    rng = np.random.default_rng(2)
    rbd = np.array([_rbd(m, prob["x0"][b], rng)[0] for b in range(B)])
    with pytest.raises(bp.BpmpcError) as err:
        ctrl.tick(np.zeros(B), rbd)
    assert err.value.status == CAPACITY and b"telemetry's max_batch" in lib.bpmpc_last_error() and small.stats(B - 1)["samples"].tolist() == [0] * (B - 1)
    ctrl.attachTelemetry(None)
    assert np.all(np.isfinite(ctrl.tick(np.zeros(B), rbd)["joint_cmd"]))
