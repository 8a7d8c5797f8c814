"""The fast kernels at iterates far from the nominal pose (tests/far_iterates.py): yaw up to 3 rad and a node a whole turn on, pitch and roll up to 1 and
0.7 rad, joints 0.6 rad off the default pose, contact forces that pull on the ground or leave the friction cone, joint velocities of 2 rad/s.  The far
iterates reach the device as warm_x / warm_u.  tests/test_far_iterate_cases.py (CPU) asserts what these tests rely on: the oracle succeeds on every case,
no decision of its line search and no pivot choice of its elimination is rounding's, and the reference kernel bodies agree with it at 1e-13.  No case
is skipped or filtered here.

  (a) LQ model of the lineariser against the oracle            1e-11 relative to max(1, |oracle|_max) per quantity (test_gpu_parity.py)
  (b) the same iterate through the other paths                 fused / in-line lane map: bit for bit; table walks 1e-12; reference kernels 1e-11
  (c) QP step dx, du, K against the oracle                     1e-9 per physical block; both eliminations, every sweep a small batch can run
  (d) whole solves from the far warm start                     status, iterations and step size equal; merit 1e-9; x, u, K at the robot's figures

Achieved figures: written beside those of test_gpu_parity.py (its _write_report) under the keys far_*, committed copy profiles/far_iterate_parity.json."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import far_iterates as fi  # noqa: E402
from tests.test_far_iterate_cases import GPU_LQ_CASES, GPU_QP_CASES, GPU_SOLVE_CASES, SOLVE_ITERATIONS  # noqa: E402
from tests.test_gpu_parity import _rel, _write_report  # noqa: E402
from tests.tolerances import rel_K, rel_u, rel_x  # noqa: E402

NN = fi.MAX_NODES
LQ_NAMES = ("A", "B", "b", "Q", "R", "P", "q", "r", "c", "C", "D", "e", "perf")
# x, u, K of a whole solve (test_gpu_parity.py): the OpenLoong figures are those of its cold start with the semi-definite input cost
SOLVE_TOL = {"h1": (1e-11, 1e-11, 1e-10), "hunter": (1e-11, 1e-11, 1e-10), "g1": (1e-11, 1e-11, 1e-10), "openloong": (1e-9, 1e-9, 1e-8)}
# ... but for the cases whose reference floor lies above them (far_iterates.oracle_solve_floor: the oracle against itself with the warm iterate moved by
# 1e-15 relative): they get 100 x that floor, the margin of the plant tests over a restatement's floor.  Hunter, flying trot, amplitude 1, two iterations:
# floor 2.4e-10 / 1.8e-10 / 5.0e-11 for x / u / K (the second iteration's QP is that ill conditioned at the iterate the first one accepts; one iteration
# 2e-14), achieved on the MI355X 1.7e-10 / 1.6e-10 / 5.8e-11 - inside the floor itself.  Every other case of (d) holds the robot's figures.
FLOOR_CASES = {("hunter", "single", 1.0, 2)}


def _lq_shapes(nx):
    nu = nx
    return dict(A=(nx, nx), B=(nx, nu), b=(nx,), Q=(nx, nx), R=(nu, nu), P=(nu, nx), q=(nx,), r=(nu,), c=(), C=(16, nx), D=(16, nu), e=(16,), perf=(3,))


def _handle(robot, shape, amp, **settings):
    """A solver set up on the problem with the far iterate as its warm start; the grid is the oracle's."""
    import bipedal_control_amd as bp
    itf, prob = fi.problem(robot, shape)
    B = prob["x0"].shape[0]
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=NN, **settings)
    wx, wu = fi.padded(robot, shape, amp)
    lay = mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], warm_x=wx, warm_u=wu)
    its = fi.batch_iterates(robot, shape, amp)
    assert lay["batch"] == B and lay["n_nodes_max"] == max(n["N"] for n, _, _, _ in its)
    assert lay["n_grids"] == (1 if shape == "single" else 4)
    assert np.array_equal(mpc.read("x").reshape(B, NN + 1, -1), wx) and np.array_equal(mpc.read("u").reshape(B, NN, -1), wu)
    return mpc, prob, its


def _lq_model(mpc, nx, names=LQ_NAMES + ("nc",)):
    mpc.stage("linearize"); mpc.synchronize()
    shapes = dict(_lq_shapes(nx), nc=())
    return {k: mpc.read(k).reshape(mpc.max_batch, NN, *shapes[k]) for k in names}


def _valid(its, events=True):
    """Boolean mask [B, NN] of the nodes that exist (and, events=False, are no event nodes)."""
    m = np.zeros((len(its), NN), bool)
    for b, (nodes, _, _, _) in enumerate(its):
        m[b, :nodes["N"]] = True if events else (np.asarray(nodes["kind"]) == 0)
    return m


@pytest.mark.parametrize("robot,shape,amp", GPU_LQ_CASES)
def test_far_lq_model_matches_oracle(robot, shape, amp):
    """(a) every quantity of the materialised LQ model and the number of constraint rows, node by node against the oracle."""
    from tests import oracle_bridge as ob
    mpc, prob, its = _handle(robot, shape, amp, materialize_lq=True)
    nx = ob.model(robot)["nx"]
    dev = _lq_model(mpc, nx)
    om = ob.oracle(robot)
    worst = {}
    for b, (nodes, x, u, _) in enumerate(its):
        for k in range(nodes["N"]):
            o = om.node_lq(nodes["kind"][k], nodes["dt"][k], x[k], u[k], x[k + 1], nodes["xref"][k], nodes["mode"][k], nodes["zref"][k], nodes["zdref"][k])
            assert int(dev["nc"][b, k]) == o["nc"], (b, k)
            for name in LQ_NAMES:
                worst[name] = max(worst.get(name, 0.0), _rel(dev[name][b, k], o[name]))
    print("far LQ model", robot, shape, amp, worst)
    _write_report("far_lq_%s_%s_%.1f" % (robot, shape, amp), worst)
    assert max(worst.values()) < 1e-11, worst


@pytest.mark.parametrize("robot,shape", [(r, s) for r in fi.ROBOTS for s in ("single", "sweep")])
def test_far_iterates_through_the_other_paths(robot, shape, monkeypatch):
    """(b) amplitude 1: the fused handle and the in-line lane map (BPMPC_LIN_COMPACT=0) bit for bit against the materialised default; the table walks
    (BPMPC_LIN_TABLES=1) at 1e-12; the reference kernels - the bodies the CPU tier clears against the oracle - at 1e-11, which says whether a miss in
    (a) lies in the fast lineariser or in what both share."""
    from tests import oracle_bridge as ob
    amp = 1.0
    nx = ob.model(robot)["nx"]
    wp = ((2 * nx + 1 + 15) // 16) * 16
    mat, prob, its = _handle(robot, shape, amp, materialize_lq=True)
    base = _lq_model(mat, nx)
    inter, every = _valid(its, events=False), _valid(its)
    B = len(its)

    def projected(mpc):
        mpc.stage("linearize"); mpc.stage("project"); mpc.synchronize()
        out = {k: mpc.read(k).reshape(B, NN, -1) for k in ("b", "q", "r", "perf", "nc", "Vt", "Pe", "nut", "Wt", "Qp", "Mt")}
        out["A_dense_rows"] = mpc.read("A").reshape(B, NN, nx, nx)[:, :, 3:12].reshape(B, NN, -1)
        return out
    pm = projected(mat)
    fused, _, _ = _handle(robot, shape, amp)
    pf = projected(fused)
    for k in pm:
        # the cost gradient of an event node is zero by definition: only the materialised mode stores those zeros; A's dense rows likewise
        mask = inter if k in ("q", "r", "A_dense_rows") else every
        assert np.array_equal(pm[k][mask], pf[k][mask]), ("fused", k)
    assert wp * (nx - 12) == pm["Vt"].shape[2]

    monkeypatch.setenv("BPMPC_LIN_COMPACT", "0")
    inline, _, _ = _handle(robot, shape, amp, materialize_lq=True)
    monkeypatch.delenv("BPMPC_LIN_COMPACT")
    got = _lq_model(inline, nx)
    for k in base:
        assert np.array_equal(base[k][every], got[k][every]), ("in-line lane map", k)

    monkeypatch.setenv("BPMPC_LIN_TABLES", "1")
    tables, _, _ = _handle(robot, shape, amp, materialize_lq=True)
    monkeypatch.delenv("BPMPC_LIN_TABLES")
    got = _lq_model(tables, nx)
    worst_t = {k: _worst_per_node(got[k], base[k], every) for k in LQ_NAMES}
    assert np.array_equal(got["nc"][every], base["nc"][every])

    ref, _, _ = _handle(robot, shape, amp, materialize_lq=True, reference_kernels=True)
    got = _lq_model(ref, nx)
    worst_r = {k: _worst_per_node(base[k], got[k], every) for k in LQ_NAMES}
    assert np.array_equal(got["nc"][every], base["nc"][every])
    print("far other paths", robot, shape, "tables", worst_t, "reference", worst_r)
    _write_report("far_paths_%s_%s" % (robot, shape), dict(tables=worst_t, reference_kernels=worst_r))
    assert max(worst_t.values()) < 1e-12, worst_t
    assert max(worst_r.values()) < 1e-11, worst_r


def _worst_per_node(a, b, mask):
    """max over the nodes of |a - b|_max / max(1, |b|_max), node by node like (a)."""
    a, b = a[mask].reshape(int(mask.sum()), -1), b[mask].reshape(int(mask.sum()), -1)
    return float((np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(b).max(axis=1))).max())


@pytest.mark.parametrize("wave", ["0", "2", "4"])
@pytest.mark.parametrize("dense", ["0", "1"])
@pytest.mark.parametrize("robot,shape,amp", GPU_QP_CASES)
def test_far_qp_step_matches_oracle(robot, shape, amp, dense, wave, monkeypatch):
    """(c) linearize, project, riccati at the far iterate: dx, du, K per physical block against the oracle, with the structured and the dense elimination
    and the eight-wave sweep ("0" at this batch), riccati_wave.h ("2") and riccati_wave2.h ("4"); and the size-independent properties of
    test_full_size_properties: the step satisfies the linearised dynamics, the eliminated equality rows hold but for the nc - rank rows the rank
    decision leaves out, D Pu = 0."""
    from tests import oracle_bridge as ob
    from oracle import reference_py as rp
    monkeypatch.setenv("BPMPC_DENSE_PROJECT", dense)
    monkeypatch.setenv("BPMPC_RICCATI_WAVE", wave)
    mpc, prob, its = _handle(robot, shape, amp, materialize_lq=True, return_gains=True)
    for st in ("linearize", "project", "riccati"):
        mpc.stage(st)
    mpc.synchronize()
    nx = nu = ob.model(robot)["nx"]
    wp = ((2 * nx + 1 + 15) // 16) * 16
    B = len(its)
    assert not mpc.read("summary").reshape(B, 4)[:, 3].any()               # no sweep reports a numerical failure
    dx = mpc.read("dx").reshape(B, NN + 1, nx); du = mpc.read("du").reshape(B, NN, nu); K = mpc.read("K").reshape(B, NN, nu, nx)
    lq = {k: mpc.read(k).reshape(B, NN, *s) for k, s in _lq_shapes(nx).items() if k in ("A", "B", "b", "C", "D", "e")}
    nc = mpc.read("nc").reshape(B, NN).astype(int); nut = mpc.read("nut").reshape(B, NN).astype(int)
    Vt = mpc.read("Vt").reshape(B, NN, nu - 12, wp) if dense == "0" else None
    Pu_full = mpc.read("Pu").reshape(B, NN, nu, nu) if dense == "1" else None
    report, props, worst, rows = {}, dict(dynamics=0.0, D_Pu=0.0, equality_rows_kept=0.0), 0.0, []
    for b, ((nodes, x, u, x0), (odx, odu, oK)) in enumerate(zip(its, fi.oracle_qp_steps(robot, shape, amp))):
        N = nodes["N"]
        ex, eu, eK = rel_x(dx[b, :N + 1], odx, report), rel_u(du[b, :N], odu, report), rel_K(K[b, :N], oK, report)
        for k in range(N):
            res = lq["A"][b, k] @ dx[b, k] + lq["B"][b, k] @ du[b, k] + lq["b"][b, k] - dx[b, k + 1]
            props["dynamics"] = max(props["dynamics"], float(np.abs(res).max()))
            if nodes["kind"][k] != 0:
                continue
            mode, nt = int(nodes["mode"][k]), nut[b, k]
            req = lq["C"][b, k, :nc[b, k]] @ dx[b, k] + lq["D"][b, k, :nc[b, k]] @ du[b, k] + lq["e"][b, k, :nc[b, k]]
            dropped = nc[b, k] - (nu - nt)
            if not (0 <= dropped <= 2 and int((np.abs(req) > 1e-8).sum()) <= dropped):
                rows.append((b, k, int(dropped), np.abs(req).round(10).tolist()))
            props["equality_rows_kept"] = max(props["equality_rows_kept"], float(np.sort(np.abs(req))[:nc[b, k] - dropped].max()))
            if Vt is not None:          # joint rows packed by the elimination, force rows single ones in the columns of the stance components
                Pu = np.zeros((nu, nu))
                first, count = (6 if mode == 2 else 0), 3 * sum(rp.mode_flags(mode))
                Pu[first + np.arange(count), np.arange(count)] = 1.0
                Pu[12:, :nt] = Vt[b, k, :, nx + 1:nx + 1 + nt]
            else:
                Pu = Pu_full[b, k]
            props["D_Pu"] = max(props["D_Pu"], float(np.abs(lq["D"][b, k, :nc[b, k]] @ Pu[:, :nt]).max()))
        worst = max(worst, ex, eu, eK)
    print("far QP step", robot, shape, amp, "dense", dense, "wave", wave, report, props)
    _write_report("far_qp_%s_%s_%.1f_dense%s_wave%s" % (robot, shape, amp, dense, wave), dict(report, **props))
    assert worst < 1e-9, report
    assert not rows, rows
    assert props["dynamics"] < 1e-9 and props["D_Pu"] < 1e-10, props


@pytest.mark.parametrize("iterations", SOLVE_ITERATIONS)
@pytest.mark.parametrize("robot,shape,amp", GPU_SOLVE_CASES)
def test_far_warm_start_solve_matches_oracle(robot, shape, amp, iterations):
    """(d) run(..., warm_x, warm_u) against the oracle's solve from the same iterate: here the trial evaluation and the filter line search see far states
    (H1 and Hunter back-track in the second iteration).  Status, iteration count and accepted step size are equal - the CPU tier asserts that none of the
    oracle's decisions is within 1e-6 of its threshold -, the merit agrees at 1e-9, and x, u, K per physical block at the figures of the cold-start solve
    tests (1e-11 / 1e-11 / 1e-10; OpenLoong 1e-9 / 1e-9 / 1e-8) - except FLOOR_CASES above, which get 100 x the reference's own floor."""
    import bipedal_control_amd as bp
    itf, prob = fi.problem(robot, shape)
    its = fi.batch_iterates(robot, shape, amp)
    B = len(its)
    wx, wu = fi.padded(robot, shape, amp)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=NN, sqp_iterations=iterations, return_gains=True)
    t, x, u, K, stats = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], warm_x=wx, warm_u=wu, gains=True)
    tx, tu, tK = SOLVE_TOL[robot]
    floor = None
    if (robot, shape, amp, iterations) in FLOOR_CASES:
        floor = fi.oracle_solve_floor(robot, shape, amp, iterations)
        tx, tu, tK = (100.0 * f for f in floor)
    report, worst_merit, missed = {}, 0.0, []
    for b, (xo, uo, Ko, st) in enumerate(fi.oracle_solves(robot, shape, amp, iterations)):
        n = stats[b].n_nodes
        assert n == its[b][0]["N"] and stats[b].status == 0
        ran = int(sum(1 for r in st if r[10] > 0))
        assert stats[b].iterations == ran
        assert stats[b].step_size == st[ran - 1][3], (b, stats[b].step_size, st[ran - 1][3])
        worst_merit = max(worst_merit, _rel(stats[b].merit_after, st[ran - 1][4]))
        ex, eu, eK = rel_x(x[b, :n + 1], xo, report), rel_u(u[b, :n], uo, report), rel_K(K[b, :n], Ko, report)
        if not (ex < tx and eu < tu and eK < tK):
            missed.append((b, ex, eu, eK))
    print("far solve", robot, shape, amp, iterations, report, "merit", worst_merit, "reference floor", floor, "tolerances", (tx, tu, tK))
    _write_report("far_solve_%s_%s_%.1f_%d_iterations" % (robot, shape, amp, iterations),
                  dict(report, merit=worst_merit, **(dict(reference_floor_x_u_K=list(floor)) if floor else {})))
    assert not missed, missed
    assert worst_merit < 1e-9
