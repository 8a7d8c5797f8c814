"""GPU tier: the masked per-robot row write that the WBC's parameter rows, the estimator's parameter rows and the controller's joint gains share
(csrc/device_handle.hip), through its three entry points: bpmpc_wbc_set_params, bpmpc_estimator_set_params, bpmpc_controller_set_joint_gains.
  shape        H1 (nj 10) and G1 (nj 12) with max_batch = 9: the 32-wide WBC rows are 288 entries, a full workgroup of 256 and a partial one;
               the 8-wide estimator rows and the nj-wide gain rows end inside the first workgroup
  cases        host arrays and device tensors x no mask and the mask [1,0,1,1,0,0,1,0,1] x one row and nine rows
  statements   every robot starts from a row of its own; a robot outside the mask keeps its bits; a written robot holds the bits of its
               source row (row 0 of a single row); the reserved entries (WBC entries 25.., estimator entry 7) read back as exactly 0.0, also
               where a device source row holds NaN there.  The kernel copies: every comparison is bit for bit."""
import itertools
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

pytestmark = pytest.mark.gpu

B = 9
MASK = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], np.int32)


def _macro(name):
    """the integer value of a macro of include/bpmpc.h: the row layouts are read from the header, not copied"""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bpmpc.h")).read()
    return int(re.search(r"^#define %s (\d+)\s*$" % name, header, re.M).group(1))


WBC_WIDTH, WBC_USED = _macro("BPMPC_WBC_PARAM_STRIDE"), _macro("BPMPC_WBC_PARAM_RESERVED")      # 32 and 25: entries from RESERVED on are written as 0
EST_WIDTH = _macro("BPMPC_EST_PARAM_STRIDE")                                                    # 8: the last entry is the reserved one
EST_USED = EST_WIDTH - 1
CASES = list(itertools.product(("host", "device"), (False, True), (1, B)))       # (where, masked, n_rows)


def _rows(rng, n, width, used):
    """valid host rows (finite, positive), the reserved entries 0"""
    r = np.zeros((n, width))
    r[:, :used] = rng.uniform(0.5, 50.0, (n, used))
    return r


def _check_write(name, case, used, set_rows, get_rows, before, src):
    """one masked write of `src` ([n, width] host rows; `used` leading entries are taken) and every statement on what is read back"""
    where, masked, n_rows = case
    rows = src[0] if n_rows == 1 else src
    mask = MASK if masked else None
    if where == "device":
        rows = rows.copy()
        rows[..., used:] = np.nan                  # reserved entries of a device source are not read: written as 0
        keep = [torch.tensor(rows, dtype=torch.float64, device="cuda")] + ([torch.tensor(MASK, dtype=torch.int32, device="cuda")] if masked else [])
        torch.cuda.synchronize()
        set_rows(keep[0], keep[1] if masked else None)
    else:
        set_rows(rows, mask)
    after = get_rows()
    for b in range(B):
        if masked and not MASK[b]:
            assert np.array_equal(after[b], before[b]), (name, case, b, "a robot outside the mask changed")
            continue
        want = src[0 if n_rows == 1 else b]
        assert np.array_equal(after[b][:used], want[:used]), (name, case, b, "source row")
        assert after[b][used:].tobytes() == np.zeros(after.shape[1] - used).tobytes(), (name, case, b, "reserved entries", after[b][used:])
    return after


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_masked_row_writes_of_the_three_entry_points(robot):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    from bipedal_control_amd.api import _check, _d, load_library
    itf = sc.interface(robot)
    nj = itf.actuatedDofNum
    assert nj == {"h1": 10, "g1": 12}[robot]
    wbc = bp.WeightedWbc(itf, max_batch=B)
    est = bp.BatchedStateEstimate(itf, kind="kalman", max_batch=B)
    mpc = bp.BatchedSqpMpc(itf, max_batch=1, max_nodes=sc.max_nodes_for(30, 30 * sc.DT))      # the controller needs a solver; it is never set up
    ctrl = bp.BatchedController(mpc, wbc)
    assert ctrl.max_batch == B
    rng = np.random.default_rng({"h1": 101, "g1": 121}[robot])

    def gains():
        kp, kd = np.full((B, nj), -1.0), np.full((B, nj), -1.0)
        _check(load_library().bpmpc_controller_joint_outputs(ctrl._h, B, None, _d(kp), _d(kd), None, None, None))
        return np.concatenate([kp, kd], axis=1)          # [B, 2 nj]: one "row" per robot for the shared statements

    held = []                                            # device halves of the last gain rows: alive until the read that follows their write

    def set_gains(rows, mask):
        if hasattr(rows, "data_ptr"):
            held[:] = [rows[..., :nj].contiguous(), rows[..., nj:].contiguous()]
            torch.cuda.synchronize()
        else:
            held[:] = [np.ascontiguousarray(rows[..., :nj]), np.ascontiguousarray(rows[..., nj:])]
        ctrl.setJointGains(held[0], held[1], mask=mask)

    targets = [("wbc", WBC_WIDTH, WBC_USED, lambda r, m: wbc.setParams(r, mask=m), lambda: np.array([wbc.getParams(b) for b in range(B)])),
               ("estimator", EST_WIDTH, EST_USED, lambda r, m: est.setParams(r, mask=m), lambda: np.array([est.getParams(b) for b in range(B)])),
               ("gains", 2 * nj, 2 * nj, set_gains, gains)]
    for name, width, used, set_rows, get_rows in targets:
        # distinct rows first (a row per robot, no mask, from the host), read back bit for bit
        first = _rows(rng, B, width, used)
        set_rows(first, None)
        before = get_rows()
        assert np.array_equal(before, first), name
        assert len({before[b].tobytes() for b in range(B)}) == B
        for case in CASES:
            src = _rows(rng, B, width, used)
            before = _check_write(name, case, used, set_rows, get_rows, before, src)


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_masked_row_writes_of_the_supervisor_and_plant_tables(robot):
    """The same statements for the six row tables the test above does not reach: the supervisor's parameter rows and the plant's parameter,
    sensor, input, joint and body rows.  At 9 robots the 160-wide body rows are 1440 entries, five full workgroups and a partial one; the 64-wide
    joint rows straddle one workgroup boundary; the 8- and 16-wide rows end inside the first workgroup.  Every row passes the host validation of
    its table and differs from robot to robot.  A body row has no reserved entries: what reads back as 0.0 are the slots of the bodies the robot
    does not have (bpmpc_plant_get_body_params), so the body rows are compared with those slots moved behind the others, and a device source holds
    its NaN there.  Nothing is stepped: that the sensor and input writes switch the plant's models on changes nothing that is read here."""
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    itf = sc.interface(robot)
    nj = itf.actuatedDofNum
    sup = bp.BatchedSupervisor(itf, max_batch=B)
    plant = bp.BatchedPlant(itf, max_batch=B)
    rng = np.random.default_rng({"h1": 103, "g1": 123}[robot])
    Sp, Ip, Jp, Bp = bp.SensorParams, bp.InputParams, bp.JointParams, bp.BodyParams
    assert (_macro("BPMPC_SUP_PARAM_STRIDE"), _macro("BPMPC_PLANT_PARAM_STRIDE")) == (bp.SupervisorParams.STRIDE, bp.PlantParams.STRIDE)
    assert [_macro("BPMPC_PLANT_%s_PARAM_STRIDE" % t) for t in ("SENSOR", "INPUT", "JOINT", "BODY")] == [Sp.STRIDE, Ip.STRIDE, Jp.STRIDE, Bp.STRIDE]

    def sensor_rows(n):
        r = np.zeros((n, Sp.STRIDE))
        r[:, :11] = rng.uniform(0.0, 1.0, (n, 11))
        r[:, 11] = rng.integers(0, 9, n)                  # delay_steps
        return r

    def input_rows(n):
        r = np.zeros((n, Ip.STRIDE))
        r[:, :len(Ip.FIELDS)] = rng.uniform(0.0, 1.0, (n, len(Ip.FIELDS)))
        return r

    def joint_rows(n):
        def draw():
            return rng.uniform(0.5, 50.0, nj)
        rows = []
        for _ in range(n):
            x = draw()
            rows.append(Jp(nj, armature=draw(), damping=draw(), friction_loss=draw(), lower=-x, upper=x).toRow())
        return np.array(rows)

    # body rows with the slots of the robot's nj + 1 bodies first and the slots of the bodies it does not have behind them
    order = np.array([e for e in range(Bp.STRIDE) if e % Bp.SLOTS <= nj] + [e for e in range(Bp.STRIDE) if e % Bp.SLOTS > nj])
    back = np.argsort(order)
    body_used = (Bp.STRIDE // Bp.SLOTS) * (nj + 1)
    model_row = Bp.model(itf)

    def body_rows(n):
        r = np.array([model_row.scaled(s).row for s in rng.uniform(0.5, 2.0, n)])[:, order]
        assert not r[:, body_used:].any()
        return r

    held = []                                            # the device rows in the layout of the library: alive until the read that follows their write

    def set_body_rows(rows, mask):
        if hasattr(rows, "data_ptr"):
            held[:] = [rows[..., torch.tensor(back, device="cuda")].contiguous()]
            torch.cuda.synchronize()
        else:
            held[:] = [np.ascontiguousarray(rows[..., back])]
        plant.setBodyParams(held[0], mask=mask)

    def reader(get):
        return lambda: np.array([get(b) for b in range(B)])

    positive = lambda width, used: lambda n: _rows(rng, n, width, used)      # noqa: E731
    targets = [("supervisor", len(bp.SupervisorParams.FIELDS), positive(bp.SupervisorParams.STRIDE, len(bp.SupervisorParams.FIELDS)),
                lambda r, m: sup.setParams(r, mask=m), reader(sup.getParams)),
               ("plant", len(bp.PlantParams.FIELDS), positive(bp.PlantParams.STRIDE, len(bp.PlantParams.FIELDS)),
                lambda r, m: plant.setParams(r, mask=m), reader(plant.getParams)),
               ("sensors", len(Sp.FIELDS), sensor_rows, lambda r, m: plant.setSensorParams(r, mask=m), reader(plant.getSensorParams)),
               ("inputs", len(Ip.FIELDS), input_rows, lambda r, m: plant.setInputParams(r, mask=m), reader(plant.getInputParams)),
               ("joints", Jp.STRIDE - 1, joint_rows, lambda r, m: plant.setJointParams(r, mask=m), reader(plant.getJointParams)),
               ("bodies", body_used, body_rows, set_body_rows, lambda: np.array([plant.getBodyParams(b)[order] for b in range(B)]))]
    for name, used, draw_rows, set_rows, get_rows in targets:
        first = draw_rows(B)
        set_rows(first, None)
        before = get_rows()
        assert np.array_equal(before, first), name
        assert len({before[b].tobytes() for b in range(B)}) == B
        for case in CASES:
            before = _check_write(name, case, used, set_rows, get_rows, before, draw_rows(B))
