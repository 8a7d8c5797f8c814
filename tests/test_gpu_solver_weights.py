"""GPU tier of the per-problem cost weights (include/bpmpc.h "Per-problem cost weights"): every problem of one solve under a weight row of its own,
against the oracle built from a task file with those weights (tests/weight_cases.py) and against a product solver created from that file, which runs
the kernels of a handle that never had a row set.  Tolerances: the project's own for the same quantities (tests/test_gpu_parity.py) - LQ blocks 1e-11,
x and u 1e-11, gains 1e-10 per physical block (tests/tolerances.py).

Shapes (weight_cases.h1_problem): H1, batch 3, trot tiled from t = 0, 20 intervals plus event nodes - two lineariser workgroups per problem, the second
partly filled, event nodes on workgroups of their own; in launch order 16-slot workgroups would straddle the problems."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

pytestmark = pytest.mark.gpu

from tests import weight_cases as wc  # noqa: E402
from tests.tolerances import rel_K, rel_u, rel_x  # noqa: E402

ITERATIONS = 2        # the second iteration linearises and searches at an iterate that already differs between the rows
H1_ROWS = ("base", "pose4_force025", "joints01_vel3")      # problem 0: the model's row; 1: base pose of Q x 4, forces of R x 0.25; 2: joints of Q x 0.1, R_task velocities x 3


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    from tests import oracle_bridge as ob
    d = tmp_path_factory.mktemp("weight_variants")
    itf = sc.interface("h1")
    files = {v: wc.write_variant("h1", v, d) for v in wc.VARIANTS}
    rows = {v: wc.row_of(bp, itf, f).row for v, f in files.items()}      # through bpmpc_model_compose_weights
    prob = wc.h1_problem(itf)
    oracle = [ob.oracle_solve_like(prob, b, iterations=ITERATIONS, robot=files[v]["name"]) for b, v in enumerate(H1_ROWS)]      # computed once, shared, never modified
    return dict(bp=bp, sc=sc, ob=ob, itf=itf, files=files, rows=rows, prob=prob, oracle=oracle, dir=d)


def _solver(ctx, itf=None, **kw):
    kw.setdefault("sqp_iterations", ITERATIONS)
    kw.setdefault("return_gains", True)
    return ctx["bp"].BatchedSqpMpc(itf or ctx["itf"], max_batch=kw.pop("max_batch", wc.BATCH), max_nodes=wc.MAX_NODES, **kw)


def _solve(mpc, prob, rows=None, mask=None, warm=(None, None)):
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], warm_x=warm[0], warm_u=warm[1])
    if rows is not None:
        mpc.setWeights(rows, mask)
    mpc.enqueue()
    mpc.synchronize()
    return mpc.fetch(gains=mpc.return_gains)


def _same_bits(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a[:4], b[:4]) if p is not None)


def _h1_rows(ctx):
    return np.stack([ctx["rows"][v] for v in H1_ROWS])


def test_solve_parity_per_row_in_both_modes(ctx):
    """Item 1: one run, each problem against the oracle of its own weights and against a product solver created from its task file; materialised and
    fused mode bit-identical.  Fails on a tree without the entry point."""
    bp, prob = ctx["bp"], ctx["prob"]
    got = {mat: _solve(_solver(ctx, materialize_lq=mat), prob, _h1_rows(ctx)) for mat in (True, False)}
    assert _same_bits(got[True], got[False])
    for mat in (True, False):
        t, x, u, K, st = got[mat]
        for b, variant in enumerate(H1_ROWS):
            xo, uo, Ko, so = ctx["oracle"][b]
            n = st[b].n_nodes
            its = int(sum(1 for r in so if r[10] > 0))
            assert st[b].status == 0 and st[b].iterations == its and st[b].step_size == so[its - 1][3]
            err = (rel_x(x[b, :n + 1], xo), rel_u(u[b, :n], uo), rel_K(K[b, :n], Ko))
            print("mat=%d problem %d (%s): x %.2e u %.2e K %.2e" % (mat, b, variant, *err))
            assert err[0] < 1e-11 and err[1] < 1e-11 and err[2] < 1e-10, (mat, b, err)
    # the rows must matter: the three oracle solutions differ far beyond the tolerances
    assert _rel(ctx["oracle"][1][1], ctx["oracle"][0][1]) > 1e-6 or _rel(ctx["oracle"][1][0], ctx["oracle"][0][0]) > 1e-6
    t, x, u, K, st = got[False]
    for b, variant in enumerate(H1_ROWS):
        f = ctx["files"][variant]
        itv = bp.BipedalRobotInterface(f["task"], f["urdf"], f["reference"])
        tp, xp, up, Kp, sp = _solve(_solver(ctx, itf=itv), prob)          # the present kernels under the variant's weights
        n = st[b].n_nodes
        err = (rel_x(x[b, :n + 1], xp[b, :n + 1]), rel_u(u[b, :n], up[b, :n]), rel_K(K[b, :n], Kp[b, :n]))
        print("problem %d (%s) against a solver created from its task file: x %.2e u %.2e K %.2e, bits equal: %s"
              % (b, variant, *err, np.array_equal(x[b], xp[b]) and np.array_equal(u[b], up[b]) and np.array_equal(K[b], Kp[b])))
        assert err[0] < 1e-11 and err[1] < 1e-11 and err[2] < 1e-10, (b, err)


def test_lq_blocks_of_a_problem_under_its_row(ctx):
    """Item 2: the staged Q, R, q, r, c of problem 1 at an intermediate node and at the node after an event, against the oracle of its weights."""
    ob, prob, itf = ctx["ob"], ctx["prob"], ctx["itf"]
    mpc = _solver(ctx, materialize_lq=True, sqp_iterations=1)
    B, N, nx = wc.BATCH, wc.MAX_NODES, itf.stateDim
    _solve(mpc, prob, _h1_rows(ctx))          # one accepted step: a generic iterate
    mpc.stage("linearize")
    mpc.synchronize()
    x = mpc.read("x").reshape(B, N + 1, nx)
    u = mpc.read("u").reshape(B, N, nx)
    shapes = dict(Q=(nx, nx), R=(nx, nx), q=(nx,), r=(nx,), c=())
    dev = {k: mpc.read(k).reshape(B, N, *s) for k, s in shapes.items()}
    b = 1
    nodes = ob.oracle_nodes(prob, b)
    kind = np.asarray(nodes["kind"])[:nodes["N"]]
    events = np.flatnonzero(kind == 1)
    assert len(events) >= 1 and events[0] + 1 < nodes["N"]
    picked = [int(np.flatnonzero(kind == 0)[3]), int(events[0]) + 1]
    assert kind[picked[1]] == 0
    worst = {}
    for name in (ctx["files"]["pose4_force025"]["name"], ctx["files"]["base"]["name"]):
        om = ob.oracle(name)
        for k in picked:
            o = om.node_lq(nodes["kind"][k], nodes["dt"][k], x[b, k], u[b, k], x[b, k + 1], nodes["xref"][k], nodes["mode"][k], nodes["zref"][k], nodes["zdref"][k])
            for q in shapes:
                worst[name, q] = max(worst.get((name, q), 0.0), _rel(dev[q][b, k], o[q]))
    own = {q: worst[ctx["files"]["pose4_force025"]["name"], q] for q in shapes}
    print("LQ blocks of problem 1 at nodes %s: %s" % (picked, own))
    assert max(own.values()) < 1e-11, own
    assert worst[ctx["files"]["base"]["name"], "Q"] > 1e-3      # ... and not the model's weights


def test_per_grid_mapping_two_gaits(ctx):
    """Item 3: two gaits, hence two grids and the lineariser's per-grid mapping; a row per problem, both against the oracle."""
    sc, ob, itf = ctx["sc"], ctx["ob"], ctx["itf"]
    prob = sc.gait_sweep_problem(itf, ["trot", "standing_trot"], [(0.3, 0.0)], n_intervals=wc.N_INTERVALS)
    variants = ("pose4_force025", "joints01_vel3")
    mpc = _solver(ctx, max_batch=2)
    t, x, u, K, st = _solve(mpc, prob, np.stack([ctx["rows"][v] for v in variants]))
    assert mpc.layout()["n_grids"] == 2
    for b, v in enumerate(variants):
        xo, uo, Ko, so = ob.oracle_solve_like(prob, b, iterations=ITERATIONS, robot=ctx["files"][v]["name"])
        n = st[b].n_nodes
        err = (rel_x(x[b, :n + 1], xo), rel_u(u[b, :n], uo), rel_K(K[b, :n], Ko))
        print("two grids, problem %d (%s): x %.2e u %.2e K %.2e" % (b, v, *err))
        assert st[b].status == 0 and err[0] < 1e-11 and err[1] < 1e-11 and err[2] < 1e-10, (b, err)


def test_back_tracking_under_a_problems_own_weights(ctx):
    """Item 4: from the iterate weight_cases.BACKTRACK the oracle takes the full step under the model's row and alpha = 0.5 under row 1; the three
    problems here are that one problem under the rows (model, row 1, model), so the trial kernels and the back-tracking tail must sum each problem's own row."""
    ob, itf = ctx["ob"], ctx["itf"]
    prob, xi, ui = wc.backtrack_problem(itf)
    B, N, nx = wc.BATCH, wc.MAX_NODES, itf.stateDim
    wx, wu = np.zeros((B, N + 1, nx)), np.zeros((B, N, nx))
    wx[:, :xi.shape[0]], wu[:, :ui.shape[0]] = xi, ui
    variants = ("base", wc.BACKTRACK["variant"], "base")
    mpc = _solver(ctx, sqp_iterations=1)
    t, x, u, K, st = _solve(mpc, prob, np.stack([ctx["rows"][v] for v in variants]), warm=(wx, wu))
    steps = [s.step_size for s in st]
    print("accepted step lengths:", steps)
    assert steps == [1.0, wc.BACKTRACK["alpha"], 1.0]
    for b, v in enumerate(variants):
        xo, uo, Ko, so = ob.oracle_solve_like(prob, b, iterations=1, x_init=xi, u_init=ui, robot=ctx["files"][v]["name"])
        n = st[b].n_nodes
        assert so[0][3] == steps[b]
        err = (rel_x(x[b, :n + 1], xo), rel_u(u[b, :n], uo))
        print("far iterate, problem %d (%s): x %.2e u %.2e" % (b, v, *err))
        assert err[0] < 1e-11 and err[1] < 1e-11, (b, err)
    assert np.array_equal(x[0], x[2]) and np.array_equal(u[0], u[2])


def test_isolation_and_plumbing(ctx):
    """Item 5."""
    bp, prob = ctx["bp"], ctx["prob"]
    base, row1 = ctx["rows"]["base"], ctx["rows"]["pose4_force025"]
    mpc = _solver(ctx)
    ref = _solve(mpc, prob, base)                                                 # n_rows = 1: every row the model's, the per-problem kernels active
    three = _solve(mpc, prob, np.stack([base] * 3))
    assert _same_bits(ref, three)                                                 # n_rows = 1 equals three equal rows
    masked = _solve(mpc, prob, row1, mask=np.array([0, 1, 0], np.int32))          # problem 1 alone, through a mask
    for b in (0, 2):
        assert all(np.array_equal(p[b], q[b]) for p, q in zip(masked[:4], ref[:4])), b      # the others keep every bit
    assert not np.array_equal(masked[1][1], ref[1][1])
    for robot, want in ((0, base), (1, row1), (2, base), (-1, base)):
        assert np.array_equal(mpc.getWeights(robot).row, want), robot             # get returns what was set; robot < 0 the start row
    full = np.stack([base, row1, base])
    host = _solve(mpc, prob, full)
    assert _same_bits(host, masked)
    mpc.resetWeights()
    dev_rows = torch.from_numpy(full).cuda()
    torch.cuda.synchronize()
    device = _solve(mpc, prob, dev_rows)                                          # device-pointer rows equal host rows, bit for bit
    assert _same_bits(device, host)
    assert np.array_equal(mpc.getWeights(1).row, row1)
    # a refused host row leaves the table and the next solve unchanged
    bad = full.copy()
    bad[2, 0] = -1.0                                                              # Q[0][0] of problem 2 negative; problems 0 and 1 would be fine
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    with pytest.raises(bp.BpmpcError) as e:
        mpc.setWeights(bad)
    assert e.value.status == -1 and "row 2" in str(e.value) and "Q[0][0]" in str(e.value)
    for robot, want in ((0, base), (1, row1), (2, base)):
        assert np.array_equal(mpc.getWeights(robot).row, want), robot
    mpc.enqueue()
    mpc.synchronize()
    assert _same_bits(mpc.fetch(gains=True), host)


def test_switching_between_the_kernel_sets(ctx):
    """Item 6: a fresh handle, a handle after reset_weights, after only get / check calls and after a refused call solve bit-identically and launch the
    present kernels; after a set the per-problem kernels run."""
    bp, prob = ctx["bp"], ctx["prob"]
    base, row1 = ctx["rows"]["base"], ctx["rows"]["pose4_force025"]
    classes = ("linearize", "linesearch", "project")

    def launches(mpc):
        return {c: mpc.kernel_time(c)[1] for c in classes + tuple(c + "_w" for c in classes)}
    fresh_mpc = _solver(ctx, profile=True)
    fresh = _solve(fresh_mpc, prob)
    n = launches(fresh_mpc)
    assert all(n[c] > 0 for c in classes) and all(n[c + "_w"] == 0 for c in classes), n

    mpc = _solver(ctx, profile=True)
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert np.array_equal(mpc.getWeights(1).row, base) and np.array_equal(mpc.getWeights().row, base)
    mpc.checkWeights(row1)
    bad = row1.copy()
    bad[1] = 1.0                                                                  # Q[0][1]: off the pattern, and Q no longer symmetric
    with pytest.raises(bp.BpmpcError) as e:
        mpc.checkWeights(bad)
    assert e.value.status == -1 and "Q[0][1]" in str(e.value)
    with pytest.raises(bp.BpmpcError):
        mpc.setWeights(bad)
    mpc.enqueue()
    mpc.synchronize()
    assert _same_bits(mpc.fetch(gains=True), fresh)                               # only get / check calls and a refused call
    n = launches(mpc)
    assert all(n[c] > 0 for c in classes) and all(n[c + "_w"] == 0 for c in classes), n

    changed = _solve(mpc, prob, row1, mask=np.array([0, 1, 0], np.int32))
    n = launches(mpc)
    assert all(n[c + "_w"] > 0 for c in classes) and all(n[c] == 0 for c in classes), n      # the new kernels after a set
    assert not _same_bits(changed, fresh)
    mpc.resetWeights()
    again = _solve(mpc, prob)
    n = launches(mpc)
    assert all(n[c] > 0 for c in classes) and all(n[c + "_w"] == 0 for c in classes), n
    assert _same_bits(again, fresh)                                               # after reset_weights
    assert np.array_equal(mpc.getWeights(1).row, base)


def test_g1_two_problems_materialised(ctx):
    """Item 7: nj = 12 (nx = 24: a row without padding, the lineariser's packed lanes), batch 2, materialised mode."""
    bp, sc, ob = ctx["bp"], ctx["sc"], ctx["ob"]
    itf = sc.interface("g1")
    variants = ("base", "pose4_force025")
    files = {v: wc.write_variant("g1", v, ctx["dir"]) for v in variants}
    rows = np.stack([wc.row_of(bp, itf, files[v]).row for v in variants])
    prob = sc.trot_problem(itf, batch=2, n_intervals=wc.N_INTERVALS, gait_start=wc.GAIT_START)
    mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=wc.MAX_NODES, sqp_iterations=ITERATIONS, return_gains=True, materialize_lq=True)
    t, x, u, K, st = _solve(mpc, prob, rows)
    for b, v in enumerate(variants):
        xo, uo, Ko, so = ob.oracle_solve_like(prob, b, iterations=ITERATIONS, robot=files[v]["name"])
        n = st[b].n_nodes
        err = (rel_x(x[b, :n + 1], xo), rel_u(u[b, :n], uo), rel_K(K[b, :n], Ko))
        print("g1 problem %d (%s): x %.2e u %.2e K %.2e" % (b, v, *err))
        assert st[b].status == 0 and err[0] < 1e-11 and err[1] < 1e-11 and err[2] < 1e-10, (b, err)


def test_refusals(ctx):
    """Item 8: each with its status and a message."""
    bp, prob = ctx["bp"], ctx["prob"]
    base = ctx["rows"]["base"]

    def refused(call, status):
        with pytest.raises(bp.BpmpcError) as e:
            call()
        assert e.value.status == status and len(str(e.value)) > 30, str(e.value)
        return str(e.value)
    UNSUPPORTED, INVALID = -3, -1      # BPMPC_ERR_UNSUPPORTED, BPMPC_ERR_INVALID_ARGUMENT
    ddp = bp.BatchedDdpMpc(ctx["itf"], max_batch=wc.BATCH, max_nodes=wc.MAX_NODES)
    ddp.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert "DDP" in refused(lambda: ddp.setWeights(base), UNSUPPORTED)
    ref = _solver(ctx, reference_kernels=True)
    ref.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert "reference_kernels" in refused(lambda: ref.setWeights(base), UNSUPPORTED)
    mpc = _solver(ctx, max_batch=4)
    refused(lambda: mpc.setWeights(base), INVALID)                                               # before any setup
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert "batch" in refused(lambda: mpc.setWeights(np.stack([base] * 4)), INVALID)            # batch 4 after a setup of 3
    two = np.stack([base] * 2)                                                                  # n_rows of 2 with batch 3: straight through the C ABI
    assert "n_rows" in refused(lambda: mpc._call("bpmpc_solver_set_weights", 3, None, two.ctypes.data_as(C.POINTER(C.c_double)), 2, 0), INVALID)
    assert np.array_equal(mpc.getWeights(0).row, base)
