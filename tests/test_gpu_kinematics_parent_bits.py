"""The five chain-walk kernels and the plan geometry's host twin give the bits they gave before their forward kinematics moved into
csrc/kernels/kinematics.h.  tests/golden/kinematics_parent_bits.npz (written on an MI355X by tests/golden/make_kinematics_parent_bits.py from the
parent of that change, through the `record_*` functions below) holds, at batch 5 - the last wave of the four-robots-per-wave kernels is partly empty:
  h1 (nj = 10), g1 (nj = 12)   every output of one WBC update, one Kalman estimator tick, one controller tick, one telemetry update with ring and
                               statistics, one plan-geometry update over plans of 21 nodes (two tiles, the second partial) through both launch modes
  h1                           bpmpc_plan_rows_host on robot 0's plan
  W12, L46                     (tests/tree_variants.py) the WBC update and the estimator tick - the two kernels tests/test_gpu_tree_variants.py runs there
The inputs are those of the handles' own GPU tests, off the nominal pose (tests/test_wbc.py _case, tests/estimator_reference.py SensorTrajectories,
tests/test_gpu_controller_tick.py _rbd, tests/test_gpu_telemetry.py _episode, tests/test_plan_geometry_reference.py random_plan).  Every comparison is
tobytes() equality.  The plant's kernels are pinned by tests/test_gpu_plant_stiction.py::test_parent_bits and the test_untouched_handles_keep_the_parent_bits
tests."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

pytestmark = pytest.mark.gpu

B5 = 5
MODES5 = [3, 1, 2, 0, 3]
PLAN_NODES, PLAN_CAP = 21, 24
PLAN_EVENTS = ((3, 9), (4, 5, 12), (), (6, 18, 19), (2,))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kinematics_parent_bits.npz")
STOCK, TREES = ("h1", "g1"), ("W12", "L46")


def record_wbc(itf, m, consistent=True):
    import bipedal_control_amd as bp
    from tests.test_wbc import _case
    rng = np.random.default_rng(11)
    cases = [_case(m, md, rng, speed=0.4, consistent=consistent) for md in MODES5]
    wbc = bp.WeightedWbc(itf, max_batch=B5)
    sol, status, dbg = wbc.update([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], MODES5, debug=True)
    nv = 6 + m["nj"]
    written = nv * nv + nv + 12 * nv + 24      # M, nle, J, Jdot v, the base task's right-hand side, the six counters: what every robot's block holds
    return {"wbc_solution": sol, "wbc_status": status, "wbc_debug": dbg[:, :written].copy()}


def record_estimator(itf, m):
    import bipedal_control_amd as bp
    from tests import estimator_reference as er
    from tests.test_gpu_estimator import _update
    rng = np.random.default_rng(17)
    s = er.SensorTrajectories(m, B5, seed=5).at(37)
    s["mode"] = np.array(MODES5, np.int32)
    s["flags"] = np.array([er.mode_flags(mo) for mo in s["mode"]], np.int32)
    x0 = rng.standard_normal((B5, 18))
    P0 = np.zeros((B5, 18, 18))
    for b in range(B5):
        A = rng.standard_normal((18, 18))
        P0[b] = (A @ A.T + np.eye(18)) * (1e-5 if b >= 3 else 1.0)      # as test_one_tick_matches_restatement: some stay below the xy reset's threshold
    est = bp.BatchedStateEstimate(itf, kind="kalman", max_batch=B5)
    est.setState(x0, P0)
    rbd = _update(est, s, source="mode")
    x, P = est.getState()
    return {"est_rbd": rbd, "est_x_hat": x, "est_cov": P, "est_xy_reset": est.device_outputs()["xy_reset"].torch().cpu().numpy()}


def record_tick(itf, m):
    import bipedal_control_amd as bp
    from tests.test_gpu_controller_tick import _rbd, _solved
    from tests.test_gpu_telemetry import TICK
    prob, mpc, _ = _solved(itf, gaits=["stance", "trot", "flying_trot", "trot", "stance"], commands=[(0.3, 0.1)])
    assert prob["x0"].shape[0] == B5
    rng = np.random.default_rng(5)
    rbd = np.array([_rbd(m, prob["x0"][b], rng, speed=0.3 if b == 0 else 0.05, consistent_mode=None if b == 0 else 3)[0] for b in range(B5)])
    ctrl = bp.BatchedController(mpc, bp.WeightedWbc(itf, max_batch=B5))
    o = ctrl.tick(np.full(B5, 0.0025), rbd)
    return {"tick_" + k: np.asarray(o[k]) for k in TICK}


def record_telemetry(robot):
    from tests.test_gpu_telemetry import _episode, _handle, _last
    m, ep = _episode(robot, B5, 1, seed=B5)
    tel = _handle(robot, 8, ring_len=4)
    x, rbd, t, safe, mode = ep[0]
    tel.update(x, rbd, t=t, safe=safe, planned_mode=mode)
    ring, stats = tel.ring(), tel.stats()
    return {"tel_sample": _last(tel, B5), "tel_ring": ring["samples"], "tel_ring_count": ring["count"], "tel_stats": stats["rows"], "tel_frozen": stats["frozen"]}


def _plans(robot):
    from tests.test_gpu_plan_geometry import _arrays
    return _arrays(robot, PLAN_CAP, (PLAN_NODES,) * B5, PLAN_EVENTS, 1, seed=3)


def record_plan(robot):
    from tests.test_gpu_plan_geometry import OUTPUTS, _fill, _handle, _read
    _, a, _ = _plans(robot)
    out = {}
    for launches in (1, 2):
        plan = _handle(robot, B5, PLAN_CAP, launches)
        _fill(plan)
        plan.update_arrays(**a)
        got = _read(plan)
        for k in OUTPUTS + ("count",):
            out["plan%d_%s" % (launches, k)] = got[k]
    return out


def record_plan_host(robot):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    _, _, plans = _plans(robot)
    t, x, mode, kind, u, _ = plans[0]
    rows, foot, count, summ = bp.PlanGeometry.rows_host(sc.interface(robot), t, x, mode, kind, u)
    return {"host_rows": rows, "host_footholds": foot, "host_count": np.array([count], np.int32), "host_summary": summ}


def record_stock(robot, what):
    from bipedal_control_amd import scenarios as sc
    from tests import oracle_bridge as ob
    if what == "wbc":
        return record_wbc(sc.interface(robot), ob.model(robot))
    if what == "estimator":
        return record_estimator(sc.interface(robot), ob.model(robot))
    if what == "tick":
        return record_tick(sc.interface(robot), ob.model(robot))
    if what == "telemetry":
        return record_telemetry(robot)
    if what == "plan":
        return record_plan(robot)
    assert what == "plan_host" and robot == "h1"
    return record_plan_host(robot)


def record_tree(name, what, directory):
    from tests import oracle_bridge as ob
    from tests import tree_variants as tv
    itf = tv.interface(tv.register(name, directory))
    return record_wbc(itf, ob.model(name), consistent=False) if what == "wbc" else record_estimator(itf, ob.model(name))


CASES = [(r, w) for r in STOCK for w in ("wbc", "estimator", "tick", "telemetry", "plan")] + [("h1", "plan_host")] + [(r, w) for r in TREES for w in ("wbc", "estimator")]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("robot,what", CASES)
def test_parent_bits(golden, robot, what, tmp_path):
    got = record_stock(robot, what) if robot in STOCK else record_tree(robot, what, tmp_path)
    assert got
    for k, v in got.items():
        want = golden["%s_%s" % (robot, k)]
        v = np.asarray(v)
        assert v.dtype == want.dtype and v.shape == want.shape, (robot, k, v.dtype, want.dtype, v.shape, want.shape)
        assert v.tobytes() == want.tobytes(), (robot, k, int((v != want).sum()), "entries differ")
