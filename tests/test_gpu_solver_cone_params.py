"""GPU tier of the per-problem cone parameters (include/bpmpc.h "Per-problem cone parameters"): every problem of one solve under a cone row of its
own, against the oracle under that row (tests/cone_cases.py oracle_for) and against a product solver created from a task file with that row, which
runs the kernels of a handle that never had a row set.  Tolerances: the project's own for the same quantities (tests/tolerances.py, as
tests/test_gpu_solver_weights.py) - x and u 1e-11, gains 1e-10 per physical block, LQ blocks 1e-11.

Shapes (weight_cases.h1_problem): H1, batch 3, trot tiled from t = 0, 20 intervals plus event nodes, max_nodes 32 - two lineariser workgroups per
problem, the second partly filled, event nodes on workgroups of their own, and trial workgroups that straddle the problems."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

pytestmark = pytest.mark.gpu

from tests import cone_cases as cc  # noqa: E402
from tests import weight_cases as wc  # noqa: E402
from tests.tolerances import rel_K, rel_u, rel_x  # noqa: E402

ITERATIONS = 2        # the second iteration linearises and searches at an iterate that already differs between the rows
H1_ROWS = ("model", "mu03", "all")
CLASSES = ("linearize", "linesearch", "project")


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


@pytest.fixture(scope="module")
def ctx():
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    from tests import oracle_bridge as ob
    itf = sc.interface("h1")
    prob = wc.h1_problem(itf)
    oracle = [cc.solve(prob, b, cc.row("h1", n), ITERATIONS) for b, n in enumerate(H1_ROWS)]      # computed once, shared, never modified
    return dict(bp=bp, sc=sc, ob=ob, itf=itf, prob=prob, oracle=oracle)


def _solver(ctx, itf=None, **kw):
    kw.setdefault("sqp_iterations", ITERATIONS)
    kw.setdefault("return_gains", True)
    return ctx["bp"].BatchedSqpMpc(itf or ctx["itf"], max_batch=kw.pop("max_batch", wc.BATCH), max_nodes=wc.MAX_NODES, **kw)


def _setup(mpc, prob, warm=(None, None)):
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], warm_x=warm[0], warm_u=warm[1])


def _solve(mpc, prob, cone=None, mask=None, warm=(None, None), weights=None):
    _setup(mpc, prob, warm)
    if weights is not None:
        mpc.setWeights(weights)
    if cone is not None:
        mpc.setConeParams(cone, mask)
    mpc.enqueue()
    mpc.synchronize()
    return mpc.fetch(gains=mpc.return_gains)


def _same_bits(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a[:4], b[:4]) if p is not None)


def _rows(names, robot="h1"):
    return np.stack([cc.row(robot, n) for n in names])


def _against_oracle(label, got, oracle, gains=True):
    """x, u (and K) of every problem against its oracle solve; iteration count and accepted steps equal."""
    t, x, u, K, st = got
    for b, (xo, uo, Ko, so) in enumerate(oracle):
        n = st[b].n_nodes
        steps = cc.steps(so)
        assert st[b].status == 0 and st[b].iterations == len(steps) and st[b].step_size == steps[-1], (label, b, st[b].status, st[b].iterations, st[b].step_size, steps)
        err = (rel_x(x[b, :n + 1], xo), rel_u(u[b, :n], uo), rel_K(K[b, :n], Ko) if gains else 0.0)
        print("%s problem %d: x %.2e u %.2e K %.2e, steps %s" % (label, b, *err, steps))
        assert err[0] < 1e-11 and err[1] < 1e-11 and err[2] < 1e-10, (label, b, err)


def test_solve_parity_per_row_in_both_modes(ctx, tmp_path):
    """Item 1: one run, each problem against the oracle of its own cone row; materialised and fused mode bit-identical; problem 1 against a product
    solver created from the task file of its row.  Fails on a tree without the entry point."""
    bp, prob = ctx["bp"], ctx["prob"]
    got = {mat: _solve(_solver(ctx, materialize_lq=mat), prob, _rows(H1_ROWS)) for mat in (True, False)}
    assert _same_bits(got[True], got[False])
    for mat in (True, False):
        _against_oracle("mat=%d" % mat, got[mat], ctx["oracle"])
    for b in (1, 2):      # the rows must matter: the oracle solutions differ far beyond the tolerances
        assert _rel(ctx["oracle"][b][1], ctx["oracle"][0][1]) > 1e-6
    f = cc.write_variant("h1", "mu03", tmp_path)
    tp, xp, up, Kp, sp = _solve(_solver(ctx, itf=bp.BipedalRobotInterface(f["task"], f["urdf"], f["reference"])), prob)      # the default kernels under friction 0.3
    t, x, u, K, st = got[False]
    n = st[1].n_nodes
    err = (rel_x(x[1, :n + 1], xp[1, :n + 1]), rel_u(u[1, :n], up[1, :n]), rel_K(K[1, :n], Kp[1, :n]))
    print("problem 1 against a solver created from the mu03 task file: x %.2e u %.2e K %.2e" % err)
    assert sp[1].step_size == st[1].step_size and err[0] < 1e-11 and err[1] < 1e-11 and err[2] < 1e-10, err


def test_lq_blocks_of_a_problem_under_its_row(ctx):
    """Item 2: the staged R, r, c (and Q, q) of the `all` problem at an intermediate node and at the node behind an event, against the oracle's
    node_lq under `all`; R is not the model's."""
    ob, prob, itf = ctx["ob"], ctx["prob"], ctx["itf"]
    mpc = _solver(ctx, materialize_lq=True, sqp_iterations=1)
    B, N, nx = wc.BATCH, wc.MAX_NODES, itf.stateDim
    _solve(mpc, prob, _rows(H1_ROWS))          # one accepted step: a generic iterate
    mpc.stage("linearize")
    mpc.synchronize()
    x = mpc.read("x").reshape(B, N + 1, nx)
    u = mpc.read("u").reshape(B, N, nx)
    shapes = dict(Q=(nx, nx), R=(nx, nx), q=(nx,), r=(nx,), c=())
    dev = {k: mpc.read(k).reshape(B, N, *s) for k, s in shapes.items()}
    b = H1_ROWS.index("all")
    nodes = ob.oracle_nodes(prob, b)
    kind = np.asarray(nodes["kind"])[:nodes["N"]]
    events = np.flatnonzero(kind == 1)
    assert len(events) >= 1 and events[0] + 1 < nodes["N"]
    picked = [int(np.flatnonzero(kind == 0)[3]), int(events[0]) + 1]
    assert kind[picked[1]] == 0
    worst = {}
    for name in ("all", "model"):
        om = cc.oracle_for("h1", cc.row("h1", name))
        for k in picked:
            o = om.node_lq(nodes["kind"][k], nodes["dt"][k], x[b, k], u[b, k], x[b, k + 1], nodes["xref"][k], nodes["mode"][k], nodes["zref"][k], nodes["zdref"][k])
            for q in shapes:
                worst[name, q] = max(worst.get((name, q), 0.0), _rel(dev[q][b, k], o[q]))
    own = {q: worst["all", q] for q in shapes}
    print("LQ blocks of problem %d at nodes %s: %s; R against the model's cone: %.2e" % (b, picked, own, worst["model", "R"]))
    assert max(own.values()) < 1e-11, own
    assert worst["model", "R"] > 1e-3      # ... and not the model's cone


def test_back_tracking_under_a_problems_own_cone(ctx):
    """Item 3: cone_cases.BACKTRACK three times over under the rows (model, mu03, bar1), warm-started from the far iterate, one iteration: accepted
    steps exactly [1.0, 0.5, 1.0] - the per-slot cone scalars of the trial kernel, whose workgroups straddle the problems, and the tail."""
    itf = ctx["itf"]
    prob, xi, ui = cc.backtrack_problem(itf)
    B, N, nx = wc.BATCH, wc.MAX_NODES, itf.stateDim
    wx, wu = np.zeros((B, N + 1, nx)), np.zeros((B, N, nx))
    wx[:, :xi.shape[0]], wu[:, :ui.shape[0]] = xi, ui
    names = cc.BACKTRACK["rows"]
    mpc = _solver(ctx, sqp_iterations=1)
    got = _solve(mpc, prob, _rows(names), warm=(wx, wu))
    steps = [s.step_size for s in got[4]]
    print("accepted step lengths:", steps)
    assert steps == [1.0, 0.5, 1.0]
    oracle = [cc.solve(prob, b, cc.row("h1", n), 1, xi, ui) for b, n in enumerate(names)]
    _against_oracle("far iterate", got, oracle, gains=False)
    assert not np.array_equal(oracle[0][1], oracle[2][1])
    assert not (np.array_equal(got[1][0], got[1][2]) and np.array_equal(got[2][0], got[2][2]))      # rows model and bar1: the same step, not the same problem


def test_weight_rows_and_cone_rows_together(ctx, tmp_path):
    """Item 4: problem 1 carries weight row pose4_force025 AND cone row `all`; problem 0 a weight row alone, problem 2 a cone row alone.  Each against
    the oracle of its weight variant's task file with the cone entries overwritten."""
    bp, prob, itf = ctx["bp"], ctx["prob"], ctx["itf"]
    weights, cones = ("joints01_vel3", "pose4_force025", "base"), ("model", "all", "mu03")
    files = {v: wc.write_variant("h1", v, tmp_path) for v in weights}
    W = np.stack([wc.row_of(bp, itf, files[v]).row for v in weights])
    got = _solve(_solver(ctx), prob, _rows(cones), weights=W)
    oracle = [cc.solve(prob, b, cc.row(files[w]["name"], c), ITERATIONS, robot=files[w]["name"]) for b, (w, c) in enumerate(zip(weights, cones))]
    _against_oracle("weights + cone", got, oracle)
    assert _rel(oracle[1][1], ctx["oracle"][2][1]) > 1e-6      # (cone `all` under the model's weights is another solution)


def test_per_grid_mapping_two_gaits(ctx):
    """Item 5: two gaits, hence two grids and the lineariser's per-grid mapping; a cone row per problem, both against the oracle."""
    sc, itf = ctx["sc"], ctx["itf"]
    prob = sc.gait_sweep_problem(itf, ["trot", "standing_trot"], [(0.3, 0.0)], n_intervals=wc.N_INTERVALS)
    names = ("all", "mu03")
    mpc = _solver(ctx, max_batch=2)
    got = _solve(mpc, prob, _rows(names))
    assert mpc.layout()["n_grids"] == 2
    _against_oracle("two grids", got, [cc.solve(prob, b, cc.row("h1", n), ITERATIONS) for b, n in enumerate(names)])


def test_isolation_and_plumbing(ctx):
    """Item 6."""
    bp, prob = ctx["bp"], ctx["prob"]
    base, row1 = cc.row("h1", "model"), cc.row("h1", "all")
    mpc = _solver(ctx)
    assert np.array_equal(mpc.getConeParams(1).row, base)                         # a handle that never had a row set: the start row
    ref = _solve(mpc, prob, base)                                                 # n_rows = 1: every row the model's, the per-problem kernels active
    three = _solve(mpc, prob, np.stack([base] * 3))
    assert _same_bits(ref, three)                                                 # n_rows = 1 equals three equal rows
    masked = _solve(mpc, prob, row1, mask=np.array([0, 1, 0], np.int32))          # problem 1 alone, through a mask
    for b in (0, 2):
        assert all(np.array_equal(p[b], q[b]) for p, q in zip(masked[:4], ref[:4])), b      # the others keep every bit
    assert not np.array_equal(masked[1][1], ref[1][1])
    for robot, want in ((0, base), (1, row1), (2, base), (-1, base)):
        assert np.array_equal(mpc.getConeParams(robot).row, want), robot          # get returns what was set; robot < 0 the start row
    full = np.stack([base, row1, base])
    host = _solve(mpc, prob, full)
    assert _same_bits(host, masked)
    mpc.resetConeParams()
    assert np.array_equal(mpc.getConeParams(1).row, base)
    dev_rows = torch.from_numpy(full).cuda()
    torch.cuda.synchronize()
    device = _solve(mpc, prob, dev_rows)                                          # device-pointer rows equal host rows, bit for bit
    assert _same_bits(device, host)
    assert np.array_equal(mpc.getConeParams(1).row, row1)
    # a refused host row leaves the table and the next solve unchanged
    bad = full.copy()
    bad[2, cc.FRICTION] = -0.3                                                    # problem 2 alone; problems 0 and 1 would be fine
    _setup(mpc, prob)
    with pytest.raises(bp.BpmpcError) as e:
        mpc.setConeParams(bad)
    assert e.value.status == -1 and "row 2" in str(e.value) and "entry 0" in str(e.value), str(e.value)
    for robot, want in ((0, base), (1, row1), (2, base)):
        assert np.array_equal(mpc.getConeParams(robot).row, want), robot
    mpc.enqueue()
    mpc.synchronize()
    assert _same_bits(mpc.fetch(gains=True), host)
    # reset and the restarts keep the rows
    mpc.restart(np.array([0, 1, 0], np.int32))
    assert np.array_equal(mpc.getConeParams(1).row, row1)
    mpc.reset()
    for robot, want in ((0, base), (1, row1), (2, base)):
        assert np.array_equal(mpc.getConeParams(robot).row, want), robot
    assert _same_bits(_solve(mpc, prob), host)                                    # a cold solve after the reset, no set in between


def test_switching_between_the_kernel_sets(ctx):
    """Item 7: one switch for both tables."""
    bp, prob, itf = ctx["bp"], ctx["prob"], ctx["itf"]
    row1 = cc.row("h1", "all")

    def launches(mpc):
        return {c: mpc.kernel_time(c)[1] for c in CLASSES + tuple(c + "_w" for c in CLASSES)}

    def default_only(n):
        return all(n[c] > 0 for c in CLASSES) and all(n[c + "_w"] == 0 for c in CLASSES)

    def per_problem_only(n):
        return all(n[c + "_w"] > 0 for c in CLASSES) and all(n[c] == 0 for c in CLASSES)
    fresh_mpc = _solver(ctx, profile=True)
    fresh = _solve(fresh_mpc, prob)
    n = launches(fresh_mpc)
    assert default_only(n), n

    mpc = _solver(ctx, profile=True)
    changed = _solve(mpc, prob, row1, mask=np.array([0, 1, 0], np.int32))
    n = launches(mpc)
    assert per_problem_only(n), n                                                 # the per-problem kernels after a set
    assert not _same_bits(changed, fresh)
    mpc.resetConeParams()
    again = _solve(mpc, prob)
    n = launches(mpc)
    assert default_only(n), n
    assert _same_bits(again, fresh)                                               # after reset_cone_params: the fresh handle's bits
    # with a weight row set, resetConeParams stays on the per-problem kernels; resetWeights then returns to the default ones
    base_w = bp.MpcWeights.from_model(itf).row
    _solve(mpc, prob, row1, weights=base_w)
    assert per_problem_only(launches(mpc))
    mpc.resetConeParams()
    under_w = _solve(mpc, prob)
    n = launches(mpc)
    assert per_problem_only(n), n
    mpc.resetWeights()
    last = _solve(mpc, prob)
    n = launches(mpc)
    assert default_only(n), n
    assert _same_bits(last, fresh)
    _against_oracle("model rows on the per-problem kernels", under_w, [ctx["oracle"][0]] + [cc.solve(prob, b, cc.row("h1", "model"), ITERATIONS) for b in (1, 2)])


def test_g1_two_problems_materialised(ctx):
    """Item 8: nj = 12 (the lineariser's packed lanes, another trial instantiation), batch 2, materialised mode, rows (model, friction 0.3)."""
    bp, sc = ctx["bp"], ctx["sc"]
    itf = sc.interface("g1")
    names = ("model", "mu03")
    prob = sc.trot_problem(itf, batch=2, n_intervals=wc.N_INTERVALS, gait_start=wc.GAIT_START)
    mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=wc.MAX_NODES, sqp_iterations=ITERATIONS, return_gains=True, materialize_lq=True)
    got = _solve(mpc, prob, _rows(names, "g1"))
    oracle = [cc.solve(prob, b, cc.row("g1", n), ITERATIONS, robot="g1") for b, n in enumerate(names)]
    assert all(cc.steps(o[3]) == [1.0, 1.0] for o in oracle)
    _against_oracle("g1", got, oracle)
    assert _rel(oracle[1][1], cc.solve(prob, 1, cc.row("g1", "model"), ITERATIONS, robot="g1")[1]) > 1e-6


def test_hard_cone(ctx):
    """Item 9: H1 with useHardFrictionConeConstraint, batch 3, cold start, rows: the start row; friction 0.3; mu 1.0 in entry 4 - against the oracle
    of "h1:hard" with friction_coefficient / ineq_mu overwritten.  A row with a shift is refused on this model."""
    bp, sc = ctx["bp"], ctx["sc"]
    robot = "h1:hard"
    itf = sc.interface(robot)
    names = ("model", "mu03", "bar1")
    prob = wc.h1_problem(itf)
    mpc = _solver(ctx, itf=itf)
    assert np.array_equal(mpc.getConeParams().row, cc.start_row(robot)) and mpc.getConeParams().hessianShift == 0.0
    got = _solve(mpc, prob, _rows(names, robot))
    oracle = [cc.solve(prob, b, cc.row(robot, n), ITERATIONS, robot=robot) for b, n in enumerate(names)]
    _against_oracle("hard cone", got, oracle)
    for b in (1, 2):
        own_model = cc.solve(prob, b, cc.row(robot, "model"), ITERATIONS, robot=robot)
        change = _rel(oracle[b][1], own_model[1])
        print("hard cone, row %s changes u of problem %d by %.2e" % (names[b], b, change))
        assert change > 1e-6
    shifted = cc.row(robot, "model")
    shifted[cc.HESSIAN_SHIFT] = 1e-6
    with pytest.raises(bp.BpmpcError) as e:
        mpc.setConeParams(shifted)
    assert e.value.status == -1 and "entry 3" in str(e.value) and "hard" in str(e.value), str(e.value)
    assert np.array_equal(mpc.getConeParams(1).row, cc.row(robot, "mu03"))


def test_refusals(ctx):
    """Item 10: each with its status and a message."""
    bp, prob = ctx["bp"], ctx["prob"]
    base = cc.row("h1", "model")

    def refused(call, status):
        with pytest.raises(bp.BpmpcError) as e:
            call()
        assert e.value.status == status and len(str(e.value)) > 30, str(e.value)
        return str(e.value)
    UNSUPPORTED, INVALID = -3, -1      # BPMPC_ERR_UNSUPPORTED, BPMPC_ERR_INVALID_ARGUMENT
    ddp = bp.BatchedDdpMpc(ctx["itf"], max_batch=wc.BATCH, max_nodes=wc.MAX_NODES)
    _setup(ddp, prob)
    assert "DDP" in refused(lambda: ddp.setConeParams(base), UNSUPPORTED)
    ref = _solver(ctx, reference_kernels=True)
    _setup(ref, prob)
    assert "reference_kernels" in refused(lambda: ref.setConeParams(base), UNSUPPORTED)
    mpc = _solver(ctx, max_batch=4)
    refused(lambda: mpc.setConeParams(base), INVALID)                                           # before any setup
    _setup(mpc, prob)
    assert "batch" in refused(lambda: mpc.setConeParams(np.stack([base] * 4)), INVALID)         # batch 4 after a setup of 3
    two = np.stack([base] * 2)                                                                  # n_rows of 2 with batch 3: straight through the C ABI
    assert "n_rows" in refused(lambda: mpc._call("bpmpc_solver_set_cone_params", 3, None, two.ctypes.data_as(C.POINTER(C.c_double)), 2, 0), INVALID)
    assert np.array_equal(mpc.getConeParams(0).row, base)
