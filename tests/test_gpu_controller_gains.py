"""GPU tier: per-robot joint gains and the full joint command of the tick (include/bpmpc.h "Run-time parameters"; the kp / kd of
HybridJointHandle::setCommand, BipedalController.cpp:250-254, set by dynamicReconfigCallback :423-472; the law of the hardware layer,
bipedal_gazebo/src/BipedalHWSim.cpp:174-175).
  zero gains      joint_torque equals the torque row of joint_cmd bit for bit and every other tick output equals a controller nothing was set on
  per-robot gains joint_torque against numpy from the tick's own joint_cmd and rbd: |diff| <= 1e-12 max(1, |kp e_q| + |kd e_v| + |tau|) (four
                  double operations, contraction allowed)
  masks           only masked robots are written; device tensors give the host path's bits; restarts and reset keep the gains
  leg gains       setLegMotorGains mirrors nj / 2 values onto both legs, H1 (5 + 5) and G1 (6 + 6)"""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

from tests.test_gpu_restart import NB, TICK, _rbd_rows, _same_tick
from tests.test_gpu_wbc_params import _fleet

pytestmark = pytest.mark.gpu
INVALID = -1


def _gains(h):
    o = h.ctrl.device_outputs()
    h.mpc.synchronize()
    return o["joint_kp"].torch().cpu().numpy(), o["joint_kd"].torch().cpu().numpy()


def _expected(out, rbd, kp, kd, nj):
    nv = 6 + nj
    pos, vel, tau = out["joint_cmd"][:, 0], out["joint_cmd"][:, 1], out["joint_cmd"][:, 2]
    e_q, e_v = pos - rbd[:, 6:6 + nj], vel - rbd[:, nv + 6:]
    return kp * e_q + kd * e_v + tau, 1e-12 * np.maximum(1.0, np.abs(kp * e_q) + np.abs(kd * e_v) + np.abs(tau))


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_joint_torque_and_gains(robot):
    import bipedal_control_amd as bp
    itf, m, H, x0, cmd, (h, twin) = _fleet(robot, 2)
    nj = m["nj"]
    for x in (h, twin):
        x.cycle(0.0, x0, cmd, H, False)
    rbd = _rbd_rows(m, x0, 71, speed=0.3)
    t = np.full(NB, 0.004)
    # ---- zero gains: after create, and set explicitly
    h.ctrl.setJointGains(np.zeros(nj), np.zeros(nj))
    o, o0 = h.ctrl.tick(t, rbd), twin.ctrl.tick(t, rbd)
    _same_tick(o, o0, range(NB))
    assert o["joint_torque"].shape == (NB, nj) and np.array_equal(o["joint_torque"], o["joint_cmd"][:, 2]) and np.abs(o["joint_torque"]).max() > 0.0
    assert o["joint_cmd"].shape == (NB, 3, nj)
    kp0, kd0 = _gains(twin)
    assert kp0.shape == (NB, nj) and not kp0.any() and not kd0.any()
    # ---- a gain row per robot
    rng = np.random.default_rng(3)
    kp, kd = rng.uniform(0.0, 200.0, (NB, nj)), rng.uniform(0.0, 10.0, (NB, nj))
    h.ctrl.setJointGains(kp, kd)
    g = _gains(h)
    assert np.array_equal(g[0], kp) and np.array_equal(g[1], kd)
    o = h.ctrl.tick(t, rbd)
    o0 = twin.ctrl.tick(t, rbd)
    for k in o0:
        if k not in bp.BatchedController.JOINT_NAMES:
            assert np.array_equal(o[k], o0[k]), k          # the gains touch nothing else
    assert np.array_equal(o["joint_kp"], kp) and np.array_equal(o["joint_kd"], kd)
    exp, bound = _expected(o, rbd, kp, kd, nj)
    print(robot, "joint_torque max |diff| / bound", float((np.abs(o["joint_torque"] - exp) / bound).max()))
    assert np.all(np.abs(o["joint_torque"] - exp) <= bound)
    assert np.abs(o["joint_torque"] - o["joint_cmd"][:, 2]).max() > 1e-3
    dev_t = h.ctrl.device_outputs()["joint_torque"].torch().cpu().numpy()
    assert np.array_equal(dev_t, o["joint_torque"])
    # ---- a mask: only its robots are written; one row for all of them
    mask = np.array([0, 1, 0, 0, 1, 1, 0, 1], np.int32)
    kp1, kd1 = rng.uniform(0.0, 200.0, nj), rng.uniform(0.0, 10.0, nj)
    h.ctrl.setJointGains(kp1, kd1, mask=mask)
    kp2, kd2 = np.where(mask[:, None] != 0, kp1, kp), np.where(mask[:, None] != 0, kd1, kd)
    g = _gains(h)
    assert np.array_equal(g[0], kp2) and np.array_equal(g[1], kd2)
    kp3, kd3 = rng.uniform(0.0, 200.0, (NB, nj)), rng.uniform(0.0, 10.0, (NB, nj))
    h.ctrl.setJointGains(kp3, kd3, mask=1 - mask)
    kp2, kd2 = np.where(mask[:, None] == 0, kp3, kp2), np.where(mask[:, None] == 0, kd3, kd2)
    g = _gains(h)
    assert np.array_equal(g[0], kp2) and np.array_equal(g[1], kd2)
    o = h.ctrl.tick(t, rbd)
    exp, bound = _expected(o, rbd, kp2, kd2, nj)
    assert np.all(np.abs(o["joint_torque"] - exp) <= bound)
    # ---- device tensors, enqueued only on the solver's stream, give the host path's bits
    import torch
    kp_d, kd_d = torch.tensor(kp, dtype=torch.float64, device="cuda"), torch.tensor(kd, dtype=torch.float64, device="cuda")
    mask_d = torch.tensor(mask, dtype=torch.int32, device="cuda")
    t_d, rbd_d = torch.full((NB,), 0.004, dtype=torch.float64, device="cuda"), torch.tensor(rbd, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    twin.ctrl.setJointGains(kp_d, kd_d, mask=mask_d)
    twin.ctrl.tick(t_d, rbd_d, fetch=False)
    h.ctrl.setJointGains(np.zeros(nj), np.zeros(nj))
    h.ctrl.setJointGains(kp, kd, mask=mask)
    o = h.ctrl.tick(t, rbd)
    twin.mpc.synchronize()
    assert np.array_equal(twin.ctrl.device_outputs()["joint_torque"].torch().cpu().numpy(), o["joint_torque"])
    g, g2 = _gains(h), _gains(twin)
    assert np.array_equal(g[0], g2[0]) and np.array_equal(g[1], g2[1]) and np.array_equal(g[0], kp * (mask[:, None] != 0))
    with pytest.raises(ValueError):
        h.ctrl.setJointGains(kp_d, kd)
    # ---- bad host gains are refused and change nothing; restarts and reset keep the gains
    for bad_kp, bad_kd in ((np.full(nj, -1.0), kd1), (kp1, np.full(nj, np.nan))):
        with pytest.raises(bp.BpmpcError) as e:
            h.ctrl.setJointGains(bad_kp, bad_kd)
        assert e.value.status == INVALID
    with pytest.raises(ValueError):
        h.ctrl.setJointGains(np.zeros(nj + 1), np.zeros(nj + 1))
    assert np.array_equal(_gains(h)[0], g[0])
    h.ctrl.reset()
    h.ctrl.restart(np.array([1, 0, 0, 1, 0, 0, 0, 1], np.int32), rbd)
    h.wbc.reset()
    g3 = _gains(h)
    assert np.array_equal(g3[0], g[0]) and np.array_equal(g3[1], g[1])
    h.cycle(TICK, None, cmd, H, True)
    o = h.ctrl.tick(t + TICK, rbd)
    exp, bound = _expected(o, rbd, g[0], g[1], nj)
    assert np.all(np.abs(o["joint_torque"] - exp) <= bound)
    # ---- leg gains: nj / 2 values mirrored onto both legs
    leg_kp, leg_kd = np.arange(1.0, 1.0 + nj // 2) * 10.0, np.arange(1.0, 1.0 + nj // 2)
    h.ctrl.setLegMotorGains(leg_kp, leg_kd)
    g = _gains(h)
    assert np.array_equal(g[0], np.tile(np.concatenate([leg_kp, leg_kp]), (NB, 1))) and np.array_equal(g[1], np.tile(np.concatenate([leg_kd, leg_kd]), (NB, 1)))
    per = rng.uniform(0.0, 100.0, (NB, nj // 2))
    h.ctrl.setLegMotorGains(per, 0.1 * per, mask=mask)
    g2 = _gains(h)
    assert np.array_equal(g2[0][mask != 0], np.concatenate([per, per], axis=1)[mask != 0]) and np.array_equal(g2[0][mask == 0], g[0][mask == 0])
    assert np.array_equal(g2[1][mask != 0], np.concatenate([0.1 * per, 0.1 * per], axis=1)[mask != 0])
    h.ctrl.setLegMotorGains(np.full(nj // 2, bp.WbcParams.RECONFIGURE_MOTOR_KP), np.full(nj // 2, bp.WbcParams.RECONFIGURE_MOTOR_KD))
    g = _gains(h)
    assert np.all(g[0] == 80.0) and np.all(g[1] == 5.0)
    with pytest.raises(ValueError):
        h.ctrl.setLegMotorGains(np.zeros(nj), np.zeros(nj))
    del kp_d, kd_d, mask_d
