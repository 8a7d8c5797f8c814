"""CPU tier of the far-iterate tests (tests/far_iterates.py): the reference kernel bodies (tests/hostemu) against the oracle at states and inputs far
from the nominal pose, and the conditions that tests/test_gpu_far_iterates.py relies on - checked here, with the oracle alone, so that no GPU test has to
skip or filter a case: the oracle succeeds on every case of the GPU tier, and no decision of its line search is close to its threshold."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import far_iterates as fi
from tests import oracle_bridge as ob
from tests.test_hostemu_kernels import d, ip

LQ_NAMES = ("A", "B", "b", "Q", "R", "P", "q", "r", "c", "C", "D", "e", "perf")
# what the GPU tier runs (tests/test_gpu_far_iterates.py imports these lists)
GPU_LQ_CASES = [(r, s, a) for r in fi.ROBOTS for s in ("single", "sweep") for a in (0.6, 1.0)]
GPU_QP_CASES = [(r, s, 1.0) for r in ("h1", "g1") for s in ("single", "sweep")]
GPU_SOLVE_CASES = [(r, s, a) for r in fi.ROBOTS for s, a in (("single", 1.0), ("sweep", 0.6))]
SOLVE_ITERATIONS = (1, 2)
DECISION_MARGIN = 1e-6


def _emu_model(lib, robot):
    A = os.path.join(ob.ROOT, "assets", robot)
    h = lib.emu_model_create(os.path.join(A, ob._URDF[robot]).encode(), os.path.join(A, "task.info").encode(), os.path.join(A, "reference.info").encode())
    assert h
    return C.c_void_p(h)


def _emu_lq(lib, h, nx, c):
    nu = nx
    o = dict(A=np.zeros((nx, nx)), B=np.zeros((nx, nu)), b=np.zeros(nx), Q=np.zeros((nx, nx)), R=np.zeros((nu, nu)), P=np.zeros((nu, nx)),
             q=np.zeros(nx), r=np.zeros(nu), c=np.zeros(1), C=np.zeros((16, nx)), D=np.zeros((16, nu)), e=np.zeros(16), perf=np.zeros(3))
    nc = C.c_int(0)
    rc = lib.emu_linearize_node(h, int(c["kind"]), int(c["mode"]), C.c_double(c["dt"]), d(c["x"]), d(c["u"]), d(c["xn"]), d(c["xr"]), d(c["zr"]), d(c["zd"]),
                                d(o["A"]), d(o["B"]), d(o["b"]), d(o["Q"]), d(o["R"]), d(o["P"]), d(o["q"]), d(o["r"]), d(o["c"]), d(o["C"]), d(o["D"]),
                                d(o["e"]), C.byref(nc), d(o["perf"]))
    assert rc == 0
    o["nc"], o["c"] = nc.value, float(o["c"][0])
    return o


@pytest.mark.parametrize("robot,nx", [("h1", 22), ("openloong", 24)])
def test_far_node_lq_model(hostemu_lib, robot, nx):
    """48 nodes per robot, all four contact modes and event nodes, unwrapped yaw, pitch up to 1.2, straight knees, pulling contacts: the tolerance of
    test_node_linearization_all_modes (measured: 4e-15)."""
    h, om = _emu_model(hostemu_lib, robot), ob.oracle(robot)
    cases = fi.node_cases(robot, 48, seed=1)
    assert {c["mode"] for c in cases if c["kind"] == 0} == {0, 1, 2, 3} and any(c["kind"] == 1 for c in cases)
    assert max(c["x"][9] for c in cases) > np.pi and min(c["x"][9] for c in cases) < -np.pi and max(abs(c["x"][10]) for c in cases) > 1.0
    assert any(c["x"][j] == 0.0 for c in cases for j in fi.knee_indices(ob.model(robot)))
    assert sum(1 for c in cases for k in range(4) if c["u"][3 * k + 2] == -20.0) >= 5
    worst = {}
    for c in cases:
        a = om.node_lq(c["kind"], c["dt"], c["x"], c["u"], c["xn"], c["xr"], c["mode"], c["zr"], c["zd"])
        b = _emu_lq(hostemu_lib, h, nx, c)
        assert a["nc"] == b["nc"]
        for k in LQ_NAMES:
            err = float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max() / max(1.0, np.abs(np.asarray(a[k])).max()))
            worst[k] = max(worst.get(k, 0.0), err)
    print("far node LQ", robot, worst)
    assert max(worst.values()) < 1e-13, worst


@pytest.mark.parametrize("robot,amp", [("h1", a) for a in fi.AMPLITUDES] + [("g1", 1.0)])
def test_far_qp_step_pipeline(hostemu_lib, robot, amp):
    """linearize -> project -> Riccati through the emulated kernel bodies against oracle.qp_step at the far iterates of the flying trot (five
    problems, 27 nodes, modes {0, 1, 2}; H1, and G1 for the robots of six joints per leg): the tolerances of test_qp_step_pipeline.  At amp 1 the step
    reaches |dx| = 3.4, |du| = 320.  (Before far_iterates.pivot_margin kept the pivot ties out, one problem in five missed by 1e-2: see there.)"""
    h = _emu_model(hostemu_lib, robot)
    steps = []
    for (nodes, x, u, x0), (dx, du, K) in zip(fi.batch_iterates(robot, "single", amp), fi.oracle_qp_steps(robot, "single", amp)):
        N = nodes["N"]
        dx2, du2, K2, summ, ps = np.zeros_like(dx), np.zeros_like(du), np.zeros_like(K), np.zeros(4), np.zeros(3)
        kind, mode = np.ascontiguousarray(nodes["kind"], np.int32), np.ascontiguousarray(nodes["mode"], np.int32)
        hostemu_lib.emu_qp_step(h, N, kind.ctypes.data_as(ip), d(nodes["dt"]), mode.ctypes.data_as(ip), d(nodes["zref"]), d(nodes["zdref"]), d(nodes["xref"]),
                                d(x0), d(x), d(u), d(dx2), d(du2), d(K2), d(summ), d(ps))
        assert summ[3] == 0
        errs = [np.abs(a - b).max() / max(1, np.abs(a).max()) for a, b in ((dx, dx2), (du, du2), (K, K2))]
        steps.append((np.abs(dx).max(), np.abs(du).max()))
        print("far qp step amp", amp, errs)
        assert errs[0] < 1e-11 and errs[1] < 1e-11 and errs[2] < 1e-10
    assert max(s[0] for s in steps) > amp and max(s[1] for s in steps) > 100.0 * amp      # the step really is far


@pytest.mark.parametrize("robot,shape,amp", sorted(set(GPU_LQ_CASES + GPU_QP_CASES + GPU_SOLVE_CASES)))
def test_generator_conditions_and_oracle_status(robot, shape, amp):
    """Every batch of the GPU tier: the generator's conditions hold for every problem, the batch covers the contact modes of its shape with event nodes,
    and the oracle's QP step succeeds (status 0: every reduced Hessian positive definite) at every iterate."""
    m = ob.model(robot)
    its = fi.batch_iterates(robot, shape, amp)
    assert 5 <= len(its) <= 8 and all(n["N"] + 1 <= fi.MAX_NODES for n, _, _, _ in its)
    modes, grids, events = set(), set(), []
    for nodes, x, u, x0 in its:
        c = fi.conditions(robot, nodes, x, u, x0)
        assert c["negative_normal"] >= 1 and c["outside_cone"] >= 1 and c["log_branch"] >= 1, c
        assert c["pitch_max"] <= fi.PITCH_MAX and c["knee_min"] >= fi.KNEE_MIN and c["event_inputs"] == 0.0, c
        assert c["dx0"] > 0.1 * amp, c
        assert c["pivot_lead"] > fi.PIVOT_MARGIN and c["pivot_smallest"] > 1e-3, c       # the elimination's row choice and rank are not rounding's
        events.append(c["events"])
        modes |= c["modes"]
        grids.add(tuple(nodes["kind"]) + tuple(nodes["mode"]))
    assert modes == ({0, 1, 2} if shape == "single" else {0, 1, 2, 3})
    assert len(grids) == (1 if shape == "single" else 4)
    assert min(events) >= 1 if shape == "single" else sum(1 for n in events if n >= 1) >= 6          # event nodes (the sweep's stance gait may have none)
    yaw = np.concatenate([x[:, 9] for _, x, _, _ in its])
    assert np.abs(yaw).max() > np.pi and np.abs(yaw[np.abs(yaw) < np.pi]).max() > 0.8 * 3.0 * amp
    assert max(np.abs(x[:, 12:] - m["initial_state"][12:]).max() for _, x, _, _ in its) > 0.5 * amp
    steps = fi.oracle_qp_steps(robot, shape, amp)          # raises on a failed sweep
    assert all(np.isfinite(dx).all() and np.isfinite(du).all() and np.isfinite(K).all() for dx, du, K in steps)


@pytest.mark.parametrize("iterations", SOLVE_ITERATIONS)
@pytest.mark.parametrize("robot,shape,amp", GPU_SOLVE_CASES)
def test_oracle_solves_from_far_warm_starts_are_decisive(robot, shape, amp, iterations):
    """The whole solves of the GPU tier in the oracle: every iteration runs and accepts a step (status 0), and no comparison of the filter line search
    or of the convergence test lies within 1e-6 relative of its threshold (column 11 of the per-iteration record), so the device has to take the same
    decisions.  Some problem back-tracks in the second iteration (H1, Hunter), so the trial evaluation is exercised beyond the full step."""
    its = fi.batch_iterates(robot, shape, amp)
    for (nodes, _, _, _), (xo, uo, Ko, st) in zip(its, fi.oracle_solves(robot, shape, amp, iterations)):
        assert np.isfinite(xo).all() and np.isfinite(uo).all()
        assert all(r[10] >= 1 and r[3] > 0.0 for r in st), st[:, [3, 10]]
        assert min(r[11] for r in st) > DECISION_MARGIN, st[:, 11]
        if iterations < max(SOLVE_ITERATIONS):
            # the next iteration eliminates the constraints at this iterate: its row choices must not be rounding's either (far_iterates.SEEDS)
            lead, smallest = fi.iterate_pivot_margin(robot, nodes, xo, uo)
            assert lead > fi.PIVOT_MARGIN and smallest > 1e-3, (lead, smallest)


def test_reference_floor_of_the_far_solves():
    """Whole solves are compared at the robot's figures of the cold-start tests (1e-11 / 1e-11 / 1e-10 for x, u, K) unless the reference's own floor - the
    oracle against itself with the warm iterate moved by 1e-15 relative - lies above them; such a case gets 100 x its floor.  One does: Hunter, flying
    trot, amplitude 1, two iterations (2.4e-10 / 1.8e-10 / 5.0e-11; its first iteration alone 2e-14 / 2e-14 / 8e-14).  Every other case amplifies one
    rounding error to 4e-12 at most, and the floor case's tolerance stays below 1e-7."""
    floors = {(r, s, a, it): fi.oracle_solve_floor(r, s, a, it) for r, s, a in GPU_SOLVE_CASES for it in SOLVE_ITERATIONS}
    print("reference floors", floors)
    special = floors.pop(("hunter", "single", 1.0, 2))
    assert 1e-11 < special[0] < 1e-9 and 1e-11 < special[1] < 1e-9 and 1e-11 < special[2] < 1e-9, special
    assert max(max(f) for f in floors.values()) < 1e-11, floors
