"""GPU tier of the dual solution (include/bpmpc.h "Dual solution"): the kernels of k_dual.hip against the numpy restatement
(tests/dual_solution_reference.py, held to the oracle's QP on the CPU tier), the certificates, the minimum-norm property, stationarity in x where
it holds, layout and untouched rows, the query, what the feature leaves alone, and the refusals.

Shapes: as tests/test_gpu_value_function.py - batch 2 to 4, 20 intervals plus event nodes, max_nodes 32, a perturbed warm iterate with x[0] != x0 - on
four scenes: h1 and g1 (single stance: 14 rows of rank 13; nx = 22 and 24), two_grids (trot and flying trot: flight nodes with 16 rows of rank 16,
two grid lengths in one batch), stance_start (trot from gait_start = 0.1: double stance, 12 rows of rank 10).

Tolerance of the kernels: with r the distance of the restatement in double from the same text in np.longdouble (per node, relative to the node's
largest entry, per quantity), the device must lie within 100 r of the extended result.  The factor is the margin for the matrix instruction's
accumulation order, FMA contraction and the Gram route's squared condition number at cond(D) <= 17 on these robots."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

pytestmark = pytest.mark.gpu

from tests import dual_solution_reference as ds  # noqa: E402
from tests import value_function_reference as vf  # noqa: E402
from tests import weight_cases as wc  # noqa: E402

MAX_NODES, ITERATIONS, MARGIN, ROWS = 32, 2, 100.0, 16
CERTIFICATE_CAP, NULL_CAP, X_STATIONARITY_CAP = 1e-10, 1e-10, 1e-11
SCENES = ("h1", "g1", "two_grids", "stance_start")
CLASS_OF = {"h1": (14, 13), "g1": (14, 13), "two_grids": (16, 16), "stance_start": (12, 10)}
QUANTITIES = ("lambda", "nu", "nu0", "nu_gain")
SENTINEL = -7.25


def _bp():
    import bipedal_control_amd as bp
    return bp


@functools.lru_cache(maxsize=None)
def _scene(name):
    from bipedal_control_amd import scenarios as sc
    if name == "h1":
        itf = sc.interface("h1")
        prob = wc.h1_problem(itf)
    elif name == "g1":
        itf = sc.interface("g1")
        prob = sc.trot_problem(itf, batch=wc.BATCH, n_intervals=wc.N_INTERVALS, gait_start=wc.GAIT_START)
    elif name == "two_grids":
        itf = sc.interface("h1")
        prob = sc.gait_sweep_problem(itf, ["trot", "flying_trot"], [(0.3, 0.0), (0.0, 0.2)], n_intervals=wc.N_INTERVALS)
    else:
        itf = sc.interface("h1")
        prob = sc.trot_problem(itf, batch=2, n_intervals=wc.N_INTERVALS, gait_start=0.1)
    return itf, prob, prob["x0"].shape[0]


def _solver(name, **kw):
    itf, _, B = _scene(name)
    kw.setdefault("sqp_iterations", ITERATIONS)
    return _bp().BatchedSqpMpc(itf, max_batch=B, max_nodes=MAX_NODES, return_gains=True, **kw)


def _setup(mpc, prob, warm=(None, None), x0=None):
    mpc.setup(prob["t0"], prob["x0"] if x0 is None else x0, prob["schedule"], prob["targets"], horizon=prob["horizon"], warm_x=warm[0], warm_u=warm[1])


def _read_problem_tables(mpc, B):
    N = MAX_NODES
    g_nodes, p_grid = mpc.read("g_nodes").astype(int), mpc.read("p_grid").astype(int)[:B]
    g_kind = mpc.read("g_kind").astype(int).reshape(-1, N)
    g_time = mpc.read("g_time").reshape(-1, N + 1)
    n = g_nodes[p_grid]
    return n, [g_kind[p_grid[b], :n[b]] for b in range(B)], [g_time[p_grid[b], :n[b] + 1] for b in range(B)]


def _read_model(mpc, B, nx):
    N = MAX_NODES
    shapes = dict(A=(N, nx, nx), B=(N, nx, nx), b=(N, nx), Q=(N, nx, nx), R=(N, nx, nx), P=(N, nx, nx), q=(N, nx), r=(N, nx), c=(N,), K=(N, nx, nx),
                  dx=(N + 1, nx), du=(N, nx), x=(N + 1, nx), u=(N, nx), C=(N, ROWS, nx), D=(N, ROWS, nx))
    m = {k: mpc.read(k).reshape(B, *s) for k, s in shapes.items()}
    m["nc"] = mpc.read("nc").astype(int).reshape(B, N)
    return m


def _restate(m, kind, S, s, b, dtype):
    n = len(kind[b])
    lq = {k: m[k][b][:n] for k in vf.LQ_NAMES}
    return ds.dual_solution(lq, m["D"][b][:n], m["nc"][b][:n], m["K"][b][:n], m["dx"][b][:n + 1], m["du"][b][:n], kind[b], S[b], s[b], dtype)


def _device(dual, b, n):
    return {"lambda": dual.costate[b, :n + 1], "nu": dual.nu[b, :n], "nu0": dual.nu0[b, :n], "nu_gain": dual.nu_gain[b, :n]}


class Staged:
    """A scene staged once: an iterate off the cold start with x[0] != x0, one backward pass stage by stage with the value function and the dual
    solution behind it, the buffers read back, and the restatement in double and in np.longdouble.  Shared by the tests; nothing modifies it."""

    def __init__(self, name):
        itf, prob, B = _scene(name)
        self.name, self.B, self.nx, self.prob = name, B, itf.stateDim, prob
        mpc = self.mpc = _solver(name)
        mpc.enableDualSolution()
        _setup(mpc, prob)
        rng = np.random.default_rng(3)
        x, u = mpc.read("x").reshape(B, MAX_NODES + 1, -1), mpc.read("u").reshape(B, MAX_NODES, -1)
        self.warm = (x + 0.01 * rng.uniform(-1, 1, x.shape), u + 0.5 * rng.uniform(-1, 1, u.shape))
        _setup(mpc, prob, self.warm)
        for stage in ("linearize", "project", "riccati", "value", "dual"):
            mpc.stage(stage)
        mpc.synchronize()
        self.n, self.kind, self.times = _read_problem_tables(mpc, B)
        self.m = _read_model(mpc, B, self.nx)
        self.S, self.s, self.v, self.x_lin, self.value_status = mpc.valueFunction()
        self.dual = mpc.dualSolution()
        self.dbl = [_restate(self.m, self.kind, self.S, self.s, b, np.float64) for b in range(B)]
        self.ext = [_restate(self.m, self.kind, self.S, self.s, b, np.longdouble) for b in range(B)]
        self.r = {q: max(vf.relative_distance(self.dbl[b][q], self.ext[b][q]) for b in range(B)) for q in QUANTITIES}
        self.inter = [[k for k in range(self.n[b]) if self.kind[b][k] != 1] for b in range(B)]
        self.classes = set()
        for b in range(B):
            g_mode = np.zeros(self.n[b], int)
            self.classes |= {c[1:] for c in ds.rank_classes(self.m["D"][b][:self.n[b]], self.m["nc"][b][:self.n[b]], g_mode, self.kind[b])[0]}


@functools.lru_cache(maxsize=None)
def _staged(name):
    return Staged(name)


@pytest.mark.parametrize("scene", SCENES)
def test_kernels_against_the_restatement(scene):
    """Item 1.  lambda: the restatement's adjoint recursion (neither S nor s) against the device's s + S dx.  On the machine this was written on r
    was, for lambda / nu / nu0 / nu_gain: h1 5.3e-16 / 1.8e-15 / 1.7e-15 / 6.2e-16, g1 2.0e-15 / 2.9e-14 / 9.9e-15 / 1.2e-14, two_grids 4.6e-16 /
    2.1e-15 / 1.8e-15 / 1.4e-15, stance_start 4.4e-16 / 3.4e-15 / 9.3e-16 / 7.5e-16; the device lay within 1.3e-15 .. 7.2e-14 (at most 23 r:
    lambda of stance_start)."""
    c = _staged(scene)
    assert (c.dual.status == 1).all() and (c.value_status == 1).all()
    assert np.abs(c.m["dx"][:, 0]).max() > 1e-3 and all((k == 1).any() for k in c.kind)
    assert CLASS_OF[scene] in c.classes, c.classes                      # the node class the scene is there for
    assert all(rank == {14: 13, 12: 10, 16: 16}[nc] for nc, rank in c.classes)
    failures = []
    for q in QUANTITIES:
        d = max(vf.relative_distance(_device(c.dual, b, c.n[b])[q], c.ext[b][q]) for b in range(c.B))
        print("%s %s: restatement in double from extended r = %.2e, device from extended %.2e (bound %.2e)" % (scene, q, c.r[q], d, MARGIN * c.r[q]))
        if not d <= MARGIN * c.r[q]:
            failures.append((q, d, c.r[q]))
    assert not failures, failures


@pytest.mark.parametrize("scene", SCENES)
def test_certificates(scene):
    """Item 2: both residuals relative to the problem's largest |g_u| and |Hux| under an absolute cap (a wrong solve gives O(1)); they are what numpy
    computes from the fetched arrays; the summary is the maxima of the per-node arrays, bit for bit."""
    c = _staged(scene)
    d = c.dual
    for b in range(c.B):
        n = c.n[b]
        ref = c.dbl[b]
        gnorm, hux = ref["gnorm"].max(), ref["hux"].max()
        print("%s problem %d: residual %.2e of %.2e, gain residual %.2e of %.2e" % (scene, b, d.residual[b, :n].max(), gnorm, d.gain_residual[b, :n].max(), hux))
        assert d.residual[b, :n].max() <= CERTIFICATE_CAP * d.summary[b, 1]
        assert d.gain_residual[b, :n].max() <= CERTIFICATE_CAP * d.summary[b, 3]
        lq = {k: c.m[k][b][:n] for k in vf.LQ_NAMES}
        for k in c.inter[b]:
            nc = c.m["nc"][b, k]
            Hux, g0, _, _ = ds.node_dual(lq, c.m["D"][b], nc, c.m["K"][b], c.m["dx"][b], c.m["du"][b], c.S[b], c.s[b], k)
            D = c.m["D"][b, k][:nc]
            res = np.abs(Hux @ c.m["dx"][b, k] + g0 + D.T @ d.nu[b, k, :nc]).max()
            gres = np.abs(Hux + D.T @ d.nu_gain[b, k, :nc]).max()
            assert res <= CERTIFICATE_CAP * gnorm and abs(res - d.residual[b, k]) <= 1e-12 * gnorm, (b, k, res, d.residual[b, k])
            assert gres <= CERTIFICATE_CAP * hux and abs(gres - d.gain_residual[b, k]) <= 1e-12 * hux, (b, k, gres, d.gain_residual[b, k])
        assert d.summary[b, 0] == d.residual[b, :n].max() and d.summary[b, 2] == d.gain_residual[b, :n].max()
        assert d.summary[b, 4] == np.abs(d.nu[b, :n]).max() and d.summary[b, 5] == np.abs(d.costate[b, :n + 1]).max()
        assert abs(d.summary[b, 1] - gnorm) <= 1e-12 * gnorm and abs(d.summary[b, 3] - hux) <= 1e-12 * hux


@pytest.mark.parametrize("scene", SCENES)
def test_minimum_norm(scene):
    """Item 3: no component in null(D') - the test a basic, non-canonical solution fails."""
    c = _staged(scene)
    worst, deficient = 0.0, 0
    for b in range(c.B):
        for k in c.inter[b]:
            nc = c.m["nc"][b, k]
            U, sv, _ = np.linalg.svd(c.m["D"][b, k][:nc])
            Z = U[:, (sv > ds.RCOND * sv[0]).sum():]
            deficient += Z.shape[1] > 0
            for col in [c.dual.nu[b, k, :nc], c.dual.nu0[b, k, :nc]] + list(c.dual.nu_gain[b, k, :nc].T):
                if Z.shape[1] and col.any():
                    worst = max(worst, np.abs(Z.T @ col).max() / np.linalg.norm(col))
                    assert np.abs(Z.T @ col).max() <= NULL_CAP * np.linalg.norm(col), (b, k, np.abs(Z.T @ col).max(), np.linalg.norm(col))
    print("%s: %d rank-deficient nodes, largest component in null(D') %.2e" % (scene, deficient, worst))
    assert deficient > 0


def test_x_stationarity_at_the_full_rank_nodes():
    """Item 4, on the batch with flight nodes: lambda_k = q + Q dx + P'du + A'lambda+ + C'nu where D has full row rank."""
    c = _staged("two_grids")
    seen = 0
    for b in range(c.B):
        n = c.n[b]
        lq = {k: c.m[k][b][:n] for k in vf.LQ_NAMES}
        for k in c.inter[b]:
            if c.m["nc"][b, k] != 16:
                continue
            seen += 1
            r = ds.x_stationarity(lq, c.m["C"][b], c.m["K"][b], c.m["dx"][b], c.m["du"][b], c.kind[b], c.dual.costate[b], c.dual.nu[b], k)
            assert np.abs(r).max() <= X_STATIONARITY_CAP * np.abs(c.dual.costate[b, k]).max(), (b, k, np.abs(r).max())
    assert seen > 0


def test_layout_and_rows_beyond_the_grid():
    """Item 5, on the batch with two grids: a full run; rows >= nc are exact zeros, event nodes are zero, the terminal costate is zero, and what lies
    beyond a problem's grid keeps a sentinel written through the device pointers before the run."""
    _, prob, B = _scene("two_grids")
    mpc = _solver("two_grids")
    mpc.enableDualSolution()
    dev = mpc.dualSolutionDevice()
    per_node = ("lambda", "nu", "nu0", "nu_gain", "residual", "gain_residual")
    for k in per_node:
        dev[k].torch().fill_(SENTINEL)
    torch.cuda.synchronize()
    _setup(mpc, prob)
    mpc.enqueue()
    mpc.synchronize()
    n, kind, _ = _read_problem_tables(mpc, B)
    nc = mpc.read("nc").astype(int).reshape(B, MAX_NODES)
    assert len(set(n.tolist())) > 1 and n.max() < MAX_NODES
    d = mpc.dualSolution()
    assert (d.status == 1).all()
    for b in range(B):
        assert not d.costate[b, n[b]].any() and (d.costate[b, n[b] + 1:] == SENTINEL).all() and not (d.costate[b, :n[b]] == SENTINEL).any()
        for a in (d.nu, d.nu0, d.nu_gain, d.residual, d.gain_residual):
            assert (a[b, n[b]:] == SENTINEL).all() and not (a[b, :n[b]] == SENTINEL).any()
        events = np.flatnonzero(kind[b] == 1)
        assert len(events) >= 1
        for k in range(n[b]):
            rows = 0 if kind[b][k] == 1 else nc[b, k]
            assert rows > 0 or k in events
            assert not d.nu[b, k, rows:].any() and not d.nu0[b, k, rows:].any() and not d.nu_gain[b, k, rows:].any()
            if rows:
                assert d.nu[b, k, :rows].any() and d.nu_gain[b, k, :rows].any()


@pytest.mark.parametrize("scene", ("h1", "g1"))
def test_query(scene):
    """Item 6: at a node time, mid-interval, before the first node, behind the last one and exactly on an event time, against the restatement's query
    on the fetched rows within item 1's bound; host and device inputs give the same bits; the costate is evaluateValue's dfdx, bit for bit."""
    c = _staged(scene)
    mpc, B, nx = c.mpc, c.B, c.nx
    _setup(mpc, c.prob, c.warm)                    # evaluate_dual asks for a completed run since the last setup
    with pytest.raises(_bp().BpmpcError) as e:
        mpc.evaluateDual(np.zeros(B), np.zeros((B, nx)))
    assert e.value.status == -1
    mpc.enqueue()
    mpc.synchronize()
    d = mpc.dualSolution()
    x_lin = mpc.valueFunction()[3]
    n, kind, times = _read_problem_tables(mpc, B)
    nc = mpc.read("nc").astype(int).reshape(B, MAX_NODES)
    rng = np.random.default_rng(5)
    tol = MARGIN * max(c.r.values())
    for which in ("node", "mid", "before", "after", "event"):
        t = np.zeros(B)
        events = [int(np.flatnonzero(kind[b] == 1)[-1]) for b in range(B)]      # the last event of the grid (a grid may begin with its only one)
        for b in range(B):
            tb, ev = times[b], events[b]
            t[b] = dict(node=tb[3 + b], mid=0.5 * (tb[5] + tb[6]), before=tb[0] - 0.1, after=tb[-1] + 0.1, event=tb[ev])[which]
        x = x_lin[:, 2] + 0.03 * rng.uniform(-1, 1, (B, nx))
        lam, nu, rows = mpc.evaluateDual(t, x)
        for b in range(B):
            rows_b = np.where(kind[b] == 1, 0, nc[b, :n[b]])
            nur, rr = ds.query(times[b], d.nu0[b], d.nu_gain[b], rows_b, x_lin[b], t[b], x[b])
            err = np.abs(nu[b] - nur).max() / np.abs(d.nu[b, :n[b]]).max()
            print("%s %s problem %d: rows %d nu %.2e (bound %.2e)" % (scene, which, b, rows[b], err, tol))
            assert rows[b] == rr and err <= tol, (which, b, err)
            if which == "event":
                ends = max(events[b] - 1, 0)           # the interval that ends at the event time (the first node for an event at the grid's start)
                assert rr == rows_b[ends] and (rr > 0 or kind[b][ends] == 1)
            if which == "before":
                assert rr == rows_b[0]                 # (a grid that starts on a mode switch begins with an event node: no rows)
            if which == "after":
                assert rows[b] == rows_b[n[b] - 1] and not lam[b].any()
        assert np.array_equal(lam, mpc.evaluateValue(t, x, hessian=False)[1])
        lam_d, nu_d, rows_d = mpc.evaluateDual(torch.as_tensor(t, device="cuda"), torch.as_tensor(x, device="cuda"))
        mpc.synchronize()
        assert np.array_equal(lam_d.torch().cpu().numpy(), lam) and np.array_equal(nu_d.torch().cpu().numpy(), nu)
        assert np.array_equal(rows_d.torch().cpu().numpy(), rows)


def _stats_tuple(st):
    return [tuple(getattr(s, f) for f, _ in s._fields_) for s in st]


def test_off_is_off_and_on_changes_nothing_else():
    """Item 7: with the feature on, x, u, K, the statistics and the value function's arrays are the bits of a handle with the value function alone;
    after enableDualSolution(False) the buffers keep the last run."""
    _, prob, B = _scene("h1")
    plain = _solver("h1")
    plain.enableValueFunction()
    _setup(plain, prob)
    plain.enqueue()
    plain.synchronize()
    ref, ref_value = plain.fetch(gains=True), plain.valueFunction()
    bare = _solver("h1")
    _setup(bare, prob)
    bare.enqueue()
    bare.synchronize()
    assert all(np.array_equal(p, q) for p, q in zip(bare.fetch(gains=True)[:4], ref[:4]))
    mpc = _solver("h1")
    mpc.enableDualSolution()
    _setup(mpc, prob)
    mpc.enqueue()
    mpc.synchronize()
    got = mpc.fetch(gains=True)
    assert all(np.array_equal(p, q) for p, q in zip(got[:4], ref[:4]))
    assert _stats_tuple(got[4]) == _stats_tuple(ref[4])
    assert all(np.array_equal(p, q) for p, q in zip(mpc.valueFunction(), ref_value))
    before = mpc.dualSolution()
    assert (before.status == 1).all()
    mpc.enableDualSolution(False)
    _setup(mpc, prob, x0=prob["x0"] + 0.01)
    mpc.enqueue()
    mpc.synchronize()
    assert not all(np.array_equal(p, q) for p, q in zip(mpc.fetch()[1:3], got[1:3]))      # another solve ...
    assert all(np.array_equal(p, q) for p, q in zip(mpc.dualSolution(), before))         # ... and the buffers as they were
    assert all(np.array_equal(p, q) for p, q in zip(mpc.valueFunction(), ref_value))     # the value function went off with it
    mpc.enableValueFunction()                      # the caller's own choice outlives the dual solution's
    mpc.enableDualSolution()
    mpc.enableDualSolution(False)
    _setup(mpc, prob, x0=prob["x0"] + 0.01)
    mpc.enqueue()
    mpc.synchronize()
    assert not all(np.array_equal(p, q) for p, q in zip(mpc.valueFunction(), ref_value))
    assert all(np.array_equal(p, q) for p, q in zip(mpc.dualSolution(), before))


def test_pipelined_backward_computes_it_behind_the_last_chunk():
    """pipeline_chunks = 3: the kernels run once, behind the last chunk's sweep and the value function's.  One iteration from the cold setup: the
    model, gains and step of that iteration are still in the buffers after the run."""
    _, prob, B = _scene("two_grids")
    mpc = _solver("two_grids", sqp_iterations=1, pipeline_chunks=3)
    mpc.enableDualSolution()
    _setup(mpc, prob)
    mpc.enqueue()
    mpc.synchronize()
    d = mpc.dualSolution()
    S, s = mpc.valueFunction()[:2]
    assert (d.status == 1).all()
    n, kind, _ = _read_problem_tables(mpc, B)
    m = _read_model(mpc, B, mpc.nx)
    for b in range(B):
        dbl, ext = _restate(m, kind, S, s, b, np.float64), _restate(m, kind, S, s, b, np.longdouble)
        dev = _device(d, b, n[b])
        for q in QUANTITIES:
            r, dist = vf.relative_distance(dbl[q], ext[q]), vf.relative_distance(dev[q], ext[q])
            print("chunked problem %d %s: r %.2e device %.2e" % (b, q, r, dist))
            assert dist <= MARGIN * r
        assert d.residual[b, :n[b]].max() <= CERTIFICATE_CAP * d.summary[b, 1]


def test_refusals():
    """Item 8."""
    bp = _bp()
    itf, prob, B = _scene("h1")

    def status_of(call):
        with pytest.raises(bp.BpmpcError) as e:
            call()
        return e.value.status

    ddp = bp.BatchedDdpMpc(itf, max_batch=1, max_nodes=MAX_NODES)
    assert status_of(ddp.enableDualSolution) == -3
    never = _solver("h1")
    _setup(never, prob)
    never.enqueue()
    never.synchronize()
    t, x = np.zeros(B), prob["x0"]
    assert status_of(never.dualSolution) == -1
    assert status_of(never.dualSolutionDevice) == -1
    assert status_of(lambda: never.evaluateDual(t, x)) == -1
    assert status_of(lambda: never.stage("dual")) == -1
    never.enableValueFunction()                    # the value function alone is not the dual solution
    assert status_of(never.dualSolution) == -1 and status_of(lambda: never.stage("dual")) == -1
    mpc = _solver("h1")
    mpc.enableDualSolution()
    mpc.batch = B
    assert status_of(lambda: mpc.evaluateDual(t, x)) == -1                    # before any setup and run
    _setup(mpc, prob)
    assert status_of(lambda: mpc.evaluateDual(t, x)) == -1                    # a setup, no run
    mpc.enqueue()
    mpc.synchronize()
    mpc.evaluateDual(t, x)
    mpc.batch = B - 1
    assert status_of(lambda: mpc.evaluateDual(t[:B - 1], x[:B - 1])) == -1    # a batch other than the setup's
