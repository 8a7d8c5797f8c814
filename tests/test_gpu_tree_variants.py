"""GPU tier for robots that are not two serial legs (tests/tree_variants.py: L46, U10, W12).  On them DeviceModel::serial_legs is 0, so every per-node kernel of
the solve runs its CHAIN = false form - tree walks over the LDS tables path / depth / subtree / contact_path - on tables that hold a real tree: a leg deeper
than nj / 2, feet at unequal depths, a third chain on the base, joints that move no contact.  tests/test_tree_variants.py (CPU) clears the tables themselves
and the reference kernel bodies against the oracle on the same robots.

Problems: tree_variants.SHAPES, three problems of 30 intervals each.  "walk": one schedule (STANCE, LF; one event node; 31 nodes) = one grid; "mixed": a
schedule per problem, two of them with a flight phase (all four contact modes, four event nodes, 34 nodes) = a grid per distinct schedule.  93 resp. 99 nodes: the last
wave of the kernels that take four nodes per wave is partly empty.  Every node of every problem is compared; nothing is filtered or skipped.

Each tolerance is the one the named existing test uses for the same comparison:
  LQ model against the oracle        1e-11 per quantity                         test_gpu_parity.py::test_linearize_matches_oracle
  fused / materialised               bit for bit                                test_gpu_parity.py::test_fused_and_materialised_modes_are_bit_identical
  fast / reference kernels           1e-9, equal step sizes                     test_gpu_parity.py::test_reference_and_fast_kernels_agree
  solves against the oracle          x, u 1e-11, K 1e-10 per physical block,    test_gpu_parity.py::test_solve_matches_oracle
                                     merit 1e-9, iterations and step size equal
  wave-per-problem sweeps            the same, against the oracle               test_gpu_parity.py::test_wave_per_problem_sweep_matches_the_workgroup_sweep
  constraint values                  1e-10                                      test_gpu_api.py::test_constraint_values_at_the_solution_match_oracle
  policy roll-out                    end state 1e-9, policy 1e-8, equal steps   test_gpu_rollout.py::test_rollout_matches_oracle
  DDP                                policy 1e-8, trajectories 1e-7 / 1e-6      test_gpu_ddp.py::_check
  WBC rigid-body quantities          M, nle, Jdot v 1e-10, J 1e-12              test_wbc.py::test_hip_wbc_matches_oracle
  Kalman estimator tick              1e-9, angular and joint part 1e-12         test_gpu_estimator.py::test_one_tick_matches_restatement
Every comparison prints its maximum before it asserts (pytest -s) and leaves it beside those of test_gpu_parity.py (its _write_report) under the keys tree_*.

Where the reference itself is decided by rounding.  Near its nominal pose L46 meets an exact tie in the complete pivoting of D at every node where both
feet stand (a rigid foot's x rows of heel and toe are equal once its other four rows are eliminated; pivot lead <= 4.4e-16 at nodes 0 .. 9 of the "walk"
grid), and U10's first flight problem meets one at nodes 23 .. 25 of the iterate its first iteration accepts.  Which of the two rows the elimination leaves
out is then rounding's choice - on the device, in the reference bodies and in the oracle alike - and shows in everything behind the elimination: the oracle's own
solve moves by 4e-5 .. 2e-3 (x, u) and up to 0.2 (K) when its cold start moves by 1e-15 relative (tree_variants.oracle_solve_floor; the CPU tier,
test_tree_variants.py::test_where_the_oracle_itself_is_decided_by_rounding, pins which cases these are and that everywhere else the floor is ~1e-13), and
the reference bodies differ from it by 1.7e-3 / 1.3e-3 / 1.3e-2 (dx / du / K) in one QP step on L46 (test_tree_variants.py::test_qp_step_pipeline).  A
comparison behind the elimination is therefore held, in the cases named by tree_variants.FLOOR_CASES and only there, to the inherited tolerance or to ten times
the reference's own floor for that problem, whichever is larger; W12, U10's "walk" batch and U10's other problems are held to the inherited tolerance.  The step lengths are stable under the perturbation and are compared
exactly everywhere.  What does not depend on the pivot choice is held to the inherited figures on every robot: the LQ model, the modes bit for bit, the
constraint values, the roll-out, and the properties of the QP step (dynamics, D Pu = 0, the eliminated rows) in test_qp_step_matches_oracle.

Measured on the MI355X (the maximum each test prints, over both batches and all problems):
                                          L46                          U10                                    W12
  LQ model, nominal / far                 4.9e-15 / 2.5e-15            2.0e-15 / 1.5e-15                      3.5e-15 / 1.9e-15
  QP step dx, du, K                       4.6e-4, 7.1e-4, 3.3e-2 (*)   4.7e-3, 1.0e-2, 8.5e-3 (*, problem 0)  2.5e-14, 1.3e-13, 1.9e-13
    dynamics / D Pu / rows kept           2.2e-16 / 9.7e-17 / 6.5e-15  6.2e-17 / 8.4e-17 / 9.6e-16            1.7e-16 / 1.4e-16 / 5.4e-15
  fast / reference kernels x, u           6.8e-4, 2.0e-3 (*)           "walk" 6.2e-16, 2.0e-14;               4.4e-14, 7.7e-14
                                                                       "mixed" 3.2e-3, 4.0e-3 (*, problem 0)
  solve, 1 iteration x, u, K, merit       7.3e-4, 7.9e-4, 0.18,        6.7e-16, 1.1e-14, 1.8e-14, 1.0e-15     1.1e-13, 2.5e-13, 2.4e-13, 1.3e-15
                                          5.7e-5 (*)
  solve, 3 iterations                     5.9e-4, 1.7e-3, 1.8e-2,      "walk" 7.8e-16, 1.6e-14, 1.7e-14,      4.4e-14, 1.2e-13, 2.5e-13, 3.5e-15
                                          6.8e-5 (*)                   5.7e-16; "mixed" 9.0e-4, 2.2e-3,
                                                                       3.4e-3, 6.3e-5 (*, problem 0)
  wave sweeps "2" / "4", 3 iterations     6.0e-4, 2.1e-3, 1.8e-2 (*)   "walk" 1.6e-15, 3.2e-14, 1.5e-14       3.6e-14, 8.2e-14, 1.4e-13
  constraint values                       4.9e-15                      2.0e-15                                3.5e-15
  roll-out end state / policy             2.6e-13 / 5.1e-13            3.1e-15 / 5.3e-15                      1.2e-11 / 3.5e-11
  DDP K, lff, merit, t, x, u              -                            1.1e-15, 1.9e-15, 5.8e-14, 8.2e-14,    -
                                                                       2.8e-13, 3.5e-13
  WBC M, nle, J, Jdot v                   5.6e-16, 3.6e-16, 3.3e-16,   4.3e-16, 3.4e-16, 2.1e-16, 2.0e-15     2.1e-16, 3.4e-16, 2.1e-16, 1.8e-15
                                          2.7e-15
  estimator x, P, lin, ang                5.0e-14, 4.8e-14, 3.3e-14,   4.1e-14, 4.8e-14, 3.9e-14, 1.1e-16     5.9e-14, 4.8e-14, 4.7e-14, 1.1e-16
                                          1.1e-16
(*) a comparison whose reference has a pivot tie: within ten times the oracle's own floor (printed per problem with the error); every other figure is held to the
inherited tolerance.  Step lengths, statuses and iteration counts are equal in every case, L46's back-trackers (0.5 and 0.25) included."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises: tests/test_gpu_estimator.py)

pytestmark = pytest.mark.gpu

from tests import tree_variants as tv  # noqa: E402
from tests.test_gpu_parity import _rel, _write_report  # noqa: E402
from tests.tolerances import rel_K, rel_u, rel_x  # noqa: E402

NN = tv.MAX_NODES
B = tv.BATCH
LQ_NAMES = ("A", "B", "b", "Q", "R", "P", "q", "r", "c", "C", "D", "e", "perf")


def _lq_shapes(nx):
    nu = nx
    return dict(A=(nx, nx), B=(nx, nu), b=(nx,), Q=(nx, nx), R=(nu, nu), P=(nu, nx), q=(nx,), r=(nu,), c=(), C=(16, nx), D=(16, nu), e=(16,), perf=(3,))


@pytest.fixture(scope="module")
def robots(tmp_path_factory):
    """name -> (interface, {shape: problem}); the variants' files are written into a temporary directory and registered with tests/oracle_bridge.py."""
    directory = tmp_path_factory.mktemp("tree_variants")
    out = {}
    for name in tv.NAMES:
        itf = tv.interface(tv.register(name, directory))
        out[name] = (itf, {shape: tv.problem(itf, shape) for shape in tv.SHAPES})
    return out


def _problem(robots, name, shape):
    itf, probs = robots[name]
    return itf, probs[shape]


_CACHE = {}      # (what, name, shape, iterations) -> oracle results: computed once, shared among the tests, not to be modified


def _oracle_solves(name, shape, iterations, prob):
    """The oracle's (x, u, K, per-iteration record) per problem of the batch `prob` = tree_variants.problem(interface of `name`, shape)."""
    from tests import oracle_bridge as ob
    key = ("solve", name, shape, iterations)
    if key not in _CACHE:
        _CACHE[key] = [ob.oracle_solve_like(prob, b, iterations=iterations, robot=name) for b in range(B)]
    return _CACHE[key]


def _solve_floor(name, shape, iterations, b, prob):
    """((x, u, K), merit) of tree_variants.oracle_solve_floor for problem b: the oracle's solve against itself with the cold start moved by 1e-15 relative."""
    key = ("floor", name, shape, iterations, b)
    if key not in _CACHE:
        floor, merit, stable = tv.oracle_solve_floor(name, prob, b, iterations)
        assert stable, key          # every sample accepts the same step lengths: they can be compared exactly
        _CACHE[key] = (floor, merit)
    return _CACHE[key]


def _tolerances(name, shape, iterations, b, prob, inherited, merit=1e-9, floor=None):
    """The inherited tolerances; for the cases of tree_variants.FLOOR_CASES - and only for them - ten times the reference's own floor for this problem where that
    is larger (module docstring).  Everywhere else a floor that rose would fail here as it does in the CPU tier.  floor(b): the floor of another reference
    than the cold-start solve under the model."""
    if (name, shape, b, iterations) not in tv.FLOOR_CASES:
        return tuple(inherited), merit
    floor, fm = floor(b) if floor is not None else _solve_floor(name, shape, iterations, b, prob)
    return tuple(max(t, tv.FLOOR_FACTOR * f) for t, f in zip(inherited, floor)), max(merit, tv.FLOOR_FACTOR * fm)


def _nodes(name, prob):
    from tests import oracle_bridge as ob
    return [ob.oracle_nodes(prob, b, robot=name) for b in range(B)]


def _run(itf, prob, **settings):
    import bipedal_control_amd as bp
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=NN, **settings)
    out = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=bool(settings.get("return_gains")))
    return mpc, out


def _compare_lq(name, mpc, nodes_of, x, u, key):
    """Every quantity of the materialised LQ model and the number of constraint rows, node by node against the oracle at the device's own iterate."""
    from tests import oracle_bridge as ob
    om = ob.oracle(name)
    nx = ob.model(name)["nx"]
    shapes = _lq_shapes(nx)
    dev = {k: mpc.read(k).reshape(B, NN, *s) for k, s in shapes.items()}
    nc = mpc.read("nc").reshape(B, NN)
    worst, modes, events = {}, set(), 0
    for b, nodes in enumerate(nodes_of):
        for k in range(nodes["N"]):
            o = om.node_lq(nodes["kind"][k], nodes["dt"][k], x[b, k], u[b, k], x[b, k + 1], nodes["xref"][k], nodes["mode"][k], nodes["zref"][k], nodes["zdref"][k])
            assert int(nc[b, k]) == o["nc"], (b, k)
            for q in LQ_NAMES:
                worst[q] = max(worst.get(q, 0.0), _rel(dev[q][b, k], o[q]))
            if nodes["kind"][k] == 0:
                modes.add(int(nodes["mode"][k]))
            events += int(nodes["kind"][k] == 1)
    print(key, worst)
    _write_report(key, worst)
    return worst, modes, events


@pytest.mark.parametrize("shape", list(tv.SHAPES))
@pytest.mark.parametrize("name", tv.NAMES)
def test_lq_model_matches_oracle(robots, name, shape):
    """1. As test_gpu_parity.py::test_linearize_matches_oracle: materialised mode, one accepted step away from the cold start, every node."""
    import bipedal_control_amd as bp
    itf, prob = _problem(robots, name, shape)
    nx = itf.stateDim
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=NN, materialize_lq=True)
    lay = mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    nodes_of = _nodes(name, prob)
    assert lay["n_nodes_max"] == max(n["N"] for n in nodes_of) and lay["n_grids"] == len({g for g, _ in tv.SHAPES[shape]})      # a grid per distinct schedule
    assert [n["N"] for n in nodes_of] == [tv.N_NODES[g] for g, _ in tv.SHAPES[shape]]
    mpc.enqueue(); mpc.synchronize()
    mpc.stage("linearize"); mpc.synchronize()
    x = mpc.read("x").reshape(B, NN + 1, nx); u = mpc.read("u").reshape(B, NN, nx)
    worst, modes, events = _compare_lq(name, mpc, nodes_of, x, u, "tree_lq_%s_%s" % (name, shape))
    assert (modes, events) == (({1, 3}, 3) if shape == "walk" else ({0, 1, 2, 3}, 9))
    assert max(worst.values()) < 1e-11, worst


@pytest.mark.parametrize("name", tv.NAMES)
def test_far_lq_model_matches_oracle(robots, name):
    """1. ... and on iterates far from the nominal pose: tests/far_iterates.py far_iterate at amplitude 1 (yaw a whole turn on, pitch and roll up to 1 and 0.7 rad,
    joints 0.6 rad off, forces outside the cone, joint velocities of 2 rad/s) on the grids of the "mixed" batch, handed over as the warm start - as
    test_gpu_far_iterates.py::test_far_lq_model_matches_oracle.  far_iterate is generic in the model; its redraw of nodes with a pivot tie concerns the
    elimination only, which this test does not run."""
    import bipedal_control_amd as bp
    from tests import far_iterates as fi
    itf, prob = _problem(robots, name, "mixed")
    nx = itf.stateDim
    nodes_of = _nodes(name, prob)
    wx, wu = np.zeros((B, NN + 1, nx)), np.zeros((B, NN, nx))
    for b, nodes in enumerate(nodes_of):
        x, u, _ = fi.far_iterate(name, nodes, prob["x0"][b], 1.0, seed=b)
        wx[b, :x.shape[0]], wu[b, :u.shape[0]] = x, u
        c = fi.conditions(name, nodes, x, u, prob["x0"][b])
        assert max(abs(c["yaw_range"][0]), abs(c["yaw_range"][1])) > np.pi and c["event_inputs"] == 0.0 and c["dx0"] > 0.0
        assert c["modes"] == ({1, 3} if tv.SHAPES["mixed"][b][0] == "walk" else {0, 1, 2, 3})
        assert c["negative_normal"] >= 1 and c["outside_cone"] >= 1
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=NN, materialize_lq=True)
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], warm_x=wx, warm_u=wu)
    assert np.array_equal(mpc.read("x").reshape(B, NN + 1, nx), wx) and np.array_equal(mpc.read("u").reshape(B, NN, nx), wu)
    mpc.stage("linearize"); mpc.synchronize()
    worst, _, _ = _compare_lq(name, mpc, nodes_of, wx, wu, "tree_far_lq_%s" % name)
    assert max(worst.values()) < 1e-11, worst


@pytest.mark.parametrize("name", tv.NAMES)
def test_fused_and_materialised_modes_are_bit_identical(robots, name):
    """2. As test_gpu_parity.py's test of the same name: x, u, K, the statistics and every buffer both modes write agree bit for bit, on a handle that has
    solved the other batch before, and a live handle switched to the materialised mode gives the materialised handle's complete model."""
    import bipedal_control_amd as bp
    itf, prob = _problem(robots, name, "mixed")
    _, other = _problem(robots, name, "walk")
    nx = itf.stateDim
    out = {}
    for mat in (True, False):
        mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=NN, sqp_iterations=3, return_gains=True, materialize_lq=mat)
        mpc.run(other["t0"], other["x0"], other["schedule"], other["targets"], horizon=other["horizon"])
        t, x, u, K, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
        mpc.stage("linearize"); mpc.stage("project"); mpc.synchronize()
        extra = {k: mpc.read(k) for k in ("b", "q", "r", "perf", "nc", "Vt", "Pe", "nut", "Wt", "Qp", "Mt")}
        A = mpc.read("A").reshape(B, NN, nx, nx)[:, :, 3:12].copy()          # the dense rows are written in both modes
        out[mat] = (x, u, K, [(s.step_size, s.merit_after, s.dynamics_sse_after, s.equality_sse_after, s.iterations, s.n_nodes) for s in st], extra, A, mpc)
    a, b = out[True], out[False]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    inter = np.zeros((B, NN), bool)          # the intermediate nodes that exist
    for p, nodes in enumerate(_nodes(name, prob)):
        inter[p, :nodes["N"]] = np.asarray(nodes["kind"]) == 0
    for k in a[4]:
        if k in ("q", "r"):      # the cost gradient of an event node is zero by definition: only the materialised mode stores those zeros
            assert np.array_equal(a[4][k].reshape(B, NN, nx)[inter], b[4][k].reshape(B, NN, nx)[inter]), k
        else:
            assert np.array_equal(a[4][k], b[4][k]), k
    assert np.array_equal(a[5][inter], b[5][inter])
    b[6].set_materialize(True)
    b[6].stage("linearize"); b[6].synchronize()
    for k in ("A", "B", "Q", "R", "C", "D", "e", "c"):
        assert np.array_equal(a[6].read(k), b[6].read(k)), k


@pytest.mark.parametrize("name", tv.NAMES)
def test_qp_step_matches_oracle(robots, name):
    """The QP step of the "mixed" batch one accepted step away from the cold start, as test_gpu_parity.py::test_qp_step_matches_oracle (dx, du, K per physical
    block at 1e-9, or ten times tree_variants.oracle_qp_floor where the pivot choice is rounding's), and what holds whichever row a tie leaves out, as
    test_gpu_far_iterates.py::test_far_qp_step_matches_oracle: the step satisfies the linearised dynamics (1e-9), the eliminated equality rows hold but for the
    nc - rank <= 2 rows the rank decision leaves out, D Pu = 0 (1e-10), no sweep reports a failure."""
    import bipedal_control_amd as bp
    from oracle import reference_py as rp
    from tests import oracle_bridge as ob
    itf, prob = _problem(robots, name, "mixed")
    nx = nu = itf.stateDim
    wp = ((2 * nx + 1 + 15) // 16) * 16
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=NN, materialize_lq=True, return_gains=True)
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    mpc.enqueue(); mpc.synchronize()
    for st in ("linearize", "project", "riccati"):
        mpc.stage(st)
    mpc.synchronize()
    assert not mpc.read("summary").reshape(B, 4)[:, 3].any()
    x = mpc.read("x").reshape(B, NN + 1, nx); u = mpc.read("u").reshape(B, NN, nu)
    dx = mpc.read("dx").reshape(B, NN + 1, nx); du = mpc.read("du").reshape(B, NN, nu); K = mpc.read("K").reshape(B, NN, nu, nx)
    lq = {k: mpc.read(k).reshape(B, NN, *s) for k, s in _lq_shapes(nx).items() if k in ("A", "B", "b", "C", "D", "e")}
    nc = mpc.read("nc").reshape(B, NN).astype(int); nut = mpc.read("nut").reshape(B, NN).astype(int)
    Vt = mpc.read("Vt").reshape(B, NN, nu - 12, wp)
    om = ob.oracle(name)
    report, props, rows, missed = {}, dict(dynamics=0.0, D_Pu=0.0, equality_rows_kept=0.0), [], []
    for b, nodes in enumerate(_nodes(name, prob)):
        N = nodes["N"]
        odx, odu, oK = om.qp_step(nodes, prob["x0"][b], x[b, :N + 1], u[b, :N])
        tol = (1e-9, 1e-9, 1e-9)
        if (name, "mixed", b, 2) in tv.FLOOR_CASES:          # the iterate is the one the first iteration accepts: what a second iteration linearises at
            floor = tv.oracle_qp_floor(name, nodes, prob["x0"][b], x[b, :N + 1], u[b, :N])["blocks"]
            tol = tuple(max(1e-9, tv.FLOOR_FACTOR * f) for f in floor)
        errs = (rel_x(dx[b, :N + 1], odx, report), rel_u(du[b, :N], odu, report), rel_K(K[b, :N], oK, report))
        report["tolerance_%d" % b], report["error_%d" % b] = tol, errs
        if not all(e < t for e, t in zip(errs, tol)):
            missed.append((b, errs, tol))
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
            Pu = np.zeros((nu, nu))       # joint rows packed by the elimination, force rows single ones in the columns of the stance components
            first, count = (6 if mode == 2 else 0), 3 * sum(rp.mode_flags(mode))
            Pu[first + np.arange(count), np.arange(count)] = 1.0
            Pu[12:, :nt] = Vt[b, k, :, nx + 1:nx + 1 + nt]
            props["D_Pu"] = max(props["D_Pu"], float(np.abs(lq["D"][b, k, :nc[b, k]] @ Pu[:, :nt]).max()))
    print("tree QP step", name, report, props)
    _write_report("tree_qp_%s" % name, dict(report, **props))
    assert not missed, missed
    assert not rows, rows
    assert props["dynamics"] < 1e-9 and props["D_Pu"] < 1e-10, props


@pytest.mark.parametrize("shape", list(tv.SHAPES))
@pytest.mark.parametrize("name", tv.NAMES)
def test_reference_and_fast_kernels_agree(robots, name, shape):
    """3. As test_gpu_parity.py's test of the same name: two iterations with the fast kernels (table walks) and with the reference kernels - the bodies the CPU
    tier clears against the oracle on these trees."""
    itf, prob = _problem(robots, name, shape)
    _, ra = _run(itf, prob, sqp_iterations=2)
    _, rb = _run(itf, prob, sqp_iterations=2, reference_kernels=True)
    report, missed = {}, []
    for b in range(B):
        (tx, tu), _ = _tolerances(name, shape, 2, b, prob, (1e-9, 1e-9))
        n = ra[4][b].n_nodes
        ex, eu = rel_x(ra[1][b, :n + 1], rb[1][b, :n + 1], report), rel_u(ra[2][b, :n], rb[2][b, :n], report)
        report["tolerance_%d" % b], report["error_%d" % b] = (tx, tu), (ex, eu)
        if not (ex < tx and eu < tu):
            missed.append((b, ex, eu, tx, tu))
    print("tree fast / reference", name, shape, report, [s.step_size for s in ra[4]], [s.step_size for s in rb[4]])
    _write_report("tree_reference_kernels_%s_%s" % (name, shape), report)
    assert not missed, missed
    assert np.isfinite(ra[1]).all() and np.isfinite(ra[2]).all()
    assert [s.step_size for s in ra[4]] == [s.step_size for s in rb[4]]
    assert [(s.status, s.n_nodes, s.iterations) for s in ra[4]] == [(s.status, s.n_nodes, s.iterations) for s in rb[4]]


def _compare_solve(name, shape, iterations, prob, out, key, oracle=None, floor=None):
    """oracle: the solves to compare with instead of the cold-start solves under the model (tests/test_gpu_row_kernel_edges.py: under a cone row per
    problem); floor(b) -> ((x, u, K), merit): the reference floor of THAT oracle for the cases of tree_variants.FLOOR_CASES."""
    t, x, u, K, stats = out
    report, steps, missed = {}, [], []
    for b, (xo, uo, Ko, st) in enumerate(oracle if oracle is not None else _oracle_solves(name, shape, iterations, prob)):
        n = stats[b].n_nodes
        assert n == xo.shape[0] - 1 and stats[b].status == 0
        its = int(sum(1 for r in st if r[10] > 0))
        assert its == iterations and stats[b].iterations == its
        steps.append((stats[b].step_size, float(st[its - 1][3])))
        (tx, tu, tK), tm = _tolerances(name, shape, iterations, b, prob, (1e-11, 1e-11, 1e-10), floor=floor)
        ex, eu, eK = rel_x(x[b, :n + 1], xo, report), rel_u(u[b, :n], uo, report), rel_K(K[b, :n], Ko, report)
        em = _rel(stats[b].merit_after, st[its - 1][4])
        report["merit"] = max(report.get("merit", 0.0), em)
        report["tolerance_%d" % b], report["error_%d" % b] = (tx, tu, tK, tm), (ex, eu, eK, em)
        if not (ex < tx and eu < tu and eK < tK and em < tm):
            missed.append((b, (ex, eu, eK, em), (tx, tu, tK, tm)))
    print(key, report, "steps (device, oracle)", steps)
    _write_report(key, report)
    assert all(a == o for a, o in steps), steps
    assert not missed, missed


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("shape", list(tv.SHAPES))
@pytest.mark.parametrize("name", tv.NAMES)
def test_solve_matches_oracle(robots, name, shape, iterations):
    """4. As test_gpu_parity.py::test_solve_matches_oracle: status, iteration count and accepted step size equal, merit 1e-9, x, u 1e-11 and K 1e-10 per
    physical block - or ten times the reference's own floor for the problem where that is larger (module docstring: every solve of L46, U10's first flight
    problem at three iterations).  L46 back-tracks: problem 0 of its "walk" batch takes 0.5 in the first iteration (asserted on the oracle's record first, so that the
    comparison of the step sizes cannot pass without a back-tracker)."""
    itf, prob = _problem(robots, name, shape)
    if name == "L46" and shape == "walk":
        first = [float(_oracle_solves(name, shape, iterations, prob)[b][3][0][3]) for b in range(B)]
        assert first[0] == 0.5 and 1.0 in first, first
    _, out = _run(itf, prob, sqp_iterations=iterations, return_gains=True)
    _compare_solve(name, shape, iterations, prob, out, "tree_solve_%s_%s_%d_iterations" % (name, shape, iterations))


@pytest.mark.parametrize("variant", ["2", "4"])
@pytest.mark.parametrize("name,shape", [("U10", "walk"), ("W12", "mixed"), ("L46", "mixed")])
def test_wave_per_problem_sweeps_match_oracle(robots, name, shape, variant, monkeypatch):
    """4. ... and under BPMPC_RICCATI_WAVE=2 (riccati_wave.h) and =4 (riccati_wave2.h), forced at this small batch: three iterations against the oracle at the
    same tolerances.  A variant per nx whose reference has no pivot tie, so that the sweeps are held to the inherited 1e-11 / 1e-10: U10 "walk" (22) and W12
    "mixed" (24); L46 "mixed" beside them for the deep leg and its repeated back-tracking, at its floor."""
    itf, prob = _problem(robots, name, shape)
    assert not any((name, shape, b, 3) in tv.FLOOR_CASES for b in range(B)) or name == "L46"
    monkeypatch.setenv("BPMPC_RICCATI_WAVE", variant)
    _, out = _run(itf, prob, sqp_iterations=3, return_gains=True)
    _compare_solve(name, shape, 3, prob, out, "tree_solve_%s_%s_3_iterations_wave%s" % (name, shape, variant))


@pytest.mark.parametrize("name", tv.NAMES)
def test_constraint_values_at_the_solution_match_oracle(robots, name):
    """5. As test_gpu_api.py's test of the same name (k_constraint_values in its table form), on the "mixed" batch: all four contact modes."""
    from tests import oracle_bridge as ob
    itf, prob = _problem(robots, name, "mixed")
    mpc, (t, x, u, _, st) = _run(itf, prob)
    v, rows, modes = mpc.constraint_values()
    om = ob.oracle(name)
    seen, worst = set(), 0.0
    for b, nodes in enumerate(_nodes(name, prob)):
        n = st[b].n_nodes
        assert n == nodes["N"]
        for k in range(n):
            if nodes["kind"][k] != 0:
                assert rows[b, k] == 0 and modes[b, k] == -1
                continue
            lq = om.node_lq(0, nodes["dt"][k], x[b, k], u[b, k], x[b, k + 1], nodes["xref"][k], nodes["mode"][k], nodes["zref"][k], nodes["zdref"][k])
            assert rows[b, k] == lq["nc"] and modes[b, k] == nodes["mode"][k]
            worst = max(worst, float(np.abs(v[b, k, :lq["nc"]] - np.asarray(lq["e"])[:lq["nc"]]).max()))
            seen.add(int(modes[b, k]))
        assert np.all(rows[b, n:] == 0)
    print("tree constraint values", name, worst)
    _write_report("tree_constraint_values_%s" % name, dict(e=worst))
    assert seen == {0, 1, 2, 3}
    assert worst < 1e-10


@pytest.mark.parametrize("name", tv.NAMES)
def test_rollout_matches_oracle(robots, name):
    """6. As test_gpu_rollout.py::test_rollout_matches_oracle (k_rollout<NJ, false> on a real tree): the same accepted / rejected step counts, end state 1e-9,
    policy at the end point 1e-8; the long window crosses the events of the "mixed" batch."""
    from oracle import reference_py as rp
    from tests import oracle_bridge as ob
    from tests.test_gpu_rollout import _oracle_rollout
    itf, prob = _problem(robots, name, "mixed")
    mpc, (t, x, u, K, st) = _run(itf, prob, return_gains=True)
    rng = np.random.default_rng(5)
    worst = dict(x=0.0, u=0.0)
    for duration, t_start in ((0.0025, 0.0), (0.02, 0.013), (0.25, 0.0)):
        xs = prob["x0"] + 2e-3 * rng.standard_normal(prob["x0"].shape)
        x_end, u_end, steps = mpc.rollout(duration, t_start=t_start, x_start=xs)
        crossed = 0
        for b in range(B):
            r = _oracle_rollout(ob, rp, prob, b, x, u, K, st[b].n_nodes, t_start, xs[b], duration, robot=name)
            assert (int(steps[b, 0]), int(steps[b, 1])) == (r["accepted"], r["rejected"]), (duration, b, steps[b], r["accepted"], r["rejected"])
            worst["x"] = max(worst["x"], float(np.abs(x_end[b] - r["states"][-1]).max()))
            worst["u"] = max(worst["u"], float(np.abs(u_end[b] - r["inputs"][-1]).max() / max(1.0, np.abs(r["inputs"][-1]).max())))
            crossed += len(r["post_event_indices"]) > 0
        assert crossed == (B if duration >= 0.25 else 0)
    print("tree rollout", name, worst)
    _write_report("tree_rollout_%s" % name, worst)
    assert worst["x"] < 1e-9 and worst["u"] < 1e-8


@pytest.mark.parametrize("name", tv.NAMES)
def test_table_switch_changes_no_bit(robots, name, monkeypatch):
    """7. BPMPC_LIN_TABLES=1 asks a robot of two serial legs for the table walks; a robot that is none already runs them, so the switch changes no bit of the LQ
    model, of a solve or of a roll-out.  This pins the dispatch on DeviceModel::serial_legs."""
    itf, prob = _problem(robots, name, "mixed")
    nx = itf.stateDim
    out = []
    for tables in (None, "1"):
        if tables:
            monkeypatch.setenv("BPMPC_LIN_TABLES", tables)
        mpc, (t, x, u, K, st) = _run(itf, prob, sqp_iterations=2, return_gains=True, materialize_lq=True)
        ro = mpc.rollout(0.25, t_start=0.01, x_start=prob["x0"] + 1e-3)
        v = mpc.constraint_values()
        mpc.stage("linearize"); mpc.synchronize()
        lq = {k: mpc.read(k) for k in LQ_NAMES + ("nc",)}
        out.append((x, u, K, [(s.step_size, s.merit_after, s.status) for s in st], ro, v, lq))
    a, b = out
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert all(np.array_equal(p, q) for p, q in zip(a[4], b[4])) and all(np.array_equal(p, q) for p, q in zip(a[5], b[5]))
    for k in a[6]:
        assert np.array_equal(a[6][k], b[6][k]), k
    assert np.isfinite(a[0]).all() and a[4][2][:, 0].min() >= 1 and nx == 12 + len(tv.VARIANTS[name]["joints"])


def test_ddp_on_u10_matches_its_restatement(robots):
    """8. One ILQR iteration on U10 against oracle/ddp_py.py, as test_gpu_ddp.py::_check (policy 1e-8, merit 1e-8, times and states 1e-7, inputs 1e-6, equal
    status and step size).  On a robot that is not two serial legs the DDP solver runs the reference bodies (solver.hip, the DDP handle's kernel choice)
    without saying so: this pins that what it then computes is the restatement's policy."""
    import bipedal_control_amd as bp
    from oracle import ddp_py, reference_py as rp
    from tests import oracle_bridge as ob
    name, cap = "U10", 60
    itf, prob = _problem(robots, name, "walk")
    m, om = ob.model(name), ob.oracle(name)
    mpc = bp.BatchedDdpMpc(itf, B, cap)
    t, x, u, K, stats = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    lff = mpc.read("ddp_lff").reshape(B, cap, itf.inputDim)
    upd = mpc.read("ddp_update_is")
    sched = prob["schedule"]
    ev, ms = list(map(float, sched.eventTimes)), list(map(int, sched.modeSequence))
    worst = dict(K=0.0, lff=0.0, update=0.0, merit=0.0, t=0.0, x=0.0, u=0.0)
    got, want = [], []
    for b in range(B):
        nodes = ob.oracle_nodes(prob, b, robot=name)
        x_nom, u_nom = rp.cold_start(m, nodes, prob["x0"][b])
        tt = prob["targets"][b]
        ref = ddp_py.ilqr_iteration(om, m, nodes, prob["x0"][b], x_nom, u_nom, ev, ms, np.asarray(tt.timeTrajectory), np.asarray(tt.stateTrajectory), m["ddp"], m["rollout"])
        N, n, st = int(nodes["N"]), len(ref["times"]), stats[b]
        got.append((st.status, st.step_size, st.n_nodes)); want.append((0 if ref["alpha"] > 0 else 1, ref["alpha"], n - 1))
        if got[-1] != want[-1]:
            continue
        worst["K"] = max(worst["K"], float(np.abs(K[b, :N] - ref["K"]).max() / max(1.0, np.abs(ref["K"]).max())))
        worst["lff"] = max(worst["lff"], float(np.abs(lff[b, :N] - ref["lff"]).max() / max(1.0, np.abs(ref["lff"]).max())))
        worst["update"] = max(worst["update"], float(abs(upd[b] - ref["update_is"]) / max(1.0, ref["update_is"])))
        worst["merit"] = max(worst["merit"], float(abs(st.merit_before - ref["merit0"]) / max(1.0, abs(ref["merit0"]))))
        worst["t"] = max(worst["t"], float(np.abs(t[b, :n] - ref["times"]).max()))
        worst["x"] = max(worst["x"], float(np.abs(x[b, :n] - ref["states"]).max()))
        worst["u"] = max(worst["u"], float(np.abs(u[b, :n - 1] - ref["inputs"][:n - 1]).max() / max(1.0, np.abs(ref["inputs"]).max())))
    print("tree ddp", name, worst, got, want)
    _write_report("tree_ddp_%s" % name, worst)
    assert got == want
    assert any(w[1] > 0 for w in want)
    assert worst["K"] < 1e-8 and worst["lff"] < 1e-8 and worst["update"] < 1e-8 and worst["merit"] < 1e-8
    assert worst["t"] < 1e-7 and worst["x"] < 1e-7 and worst["u"] < 1e-6


MODES16 = [0, 1, 2, 3] * 4


@pytest.mark.parametrize("name", tv.NAMES)
def test_wbc_rigid_body_quantities_match_oracle(robots, name):
    """9. One WBC tick against oracle/wbc_py.py, as test_wbc.py::test_hip_wbc_matches_oracle, on the rigid-body pass of kernels/wbc.h (CRBA, RNEA, contact
    Jacobians and Jdot v over path / subtree): mass matrix, nonlinear effects and Jdot v at 1e-10, J at 1e-12; all four contact modes in the batch.
    The comparison stops there on purpose: the WBC's task builder assumes nj / 2 joints per leg by construction - torqueLimitsTask holds nj / 2 entries and
    joint j takes entry j % (nj / 2) (kernels/wbc.h, wbc.hip load of the settings; oracle/wbc_py.py load_settings likewise) - so on these trees its QP is
    not the reference's QP of any robot, and the builder is not bent to them."""
    import bipedal_control_amd as bp
    from oracle import wbc_py as wp
    from tests import oracle_bridge as ob
    from tests.test_wbc import _case
    itf, _ = robots[name]
    m = ob.model(name)
    nv = 6 + m["nj"]
    rng = np.random.default_rng(11)
    cases = [_case(m, md, rng, speed=0.4, consistent=False) for md in MODES16[:8]]
    wbc = bp.WeightedWbc(itf, max_batch=len(cases))
    assert wbc.numDecisionVars == nv + 12 + m["nj"]
    _, _, dbg = wbc.update([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], MODES16[:8], debug=True)
    worst = dict(M=0.0, nle=0.0, J=0.0, djv=0.0)
    for b, (x, u, rbd, q, v) in enumerate(cases):
        d = dbg[b]
        M = d[:nv * nv].reshape(nv, nv); nle = d[nv * nv:nv * nv + nv]; J = d[nv * nv + nv:nv * nv + nv + 12 * nv].reshape(12, nv)
        djv = d[nv * nv + nv + 12 * nv:nv * nv + nv + 12 * nv + 12]
        ref = dict(M=wp.mass_matrix(m, q), nle=wp.nonlinear_effects(m, q, v), J=wp.contact_jacobian(m, q), djv=wp.jdot_v(wp.contact_jacobian, m, q, v))
        for k, got in (("M", M), ("nle", nle), ("J", J), ("djv", djv)):
            worst[k] = max(worst[k], _rel(got, ref[k]))
        # the tree shows in J: the columns of the joints off a contact's path are exactly zero, on both sides
        cp = tv.tables(m["parent"], m["contact_body"])["contact_path"]
        for i in range(4):
            off = np.array([not (cp[i] >> (j + 1) & 1) for j in range(m["nj"])])
            assert not J[3 * i:3 * i + 3, 6:][:, off].any() and not ref["J"][3 * i:3 * i + 3, 6:][:, off].any()
    print("tree wbc", name, worst)
    _write_report("tree_wbc_%s" % name, worst)
    assert worst["M"] < 1e-10 and worst["nle"] < 1e-10 and worst["J"] < 1e-12 and worst["djv"] < 1e-10, worst


@pytest.mark.parametrize("name", tv.NAMES)
def test_estimator_one_tick_matches_restatement(robots, name):
    """9. One Kalman estimator tick against tests/estimator_reference.py, as test_gpu_estimator.py::test_one_tick_matches_restatement (the contact kinematics
    of kernels/estimator.h over path): sixteen robots, every contact mode four times, through `mode` and through `contact`; x_hat, P and the filter part
    of rbd at 1e-9, the angular and joint part at 1e-12, the same xy resets."""
    import torch  # noqa: F401  (as tests/test_gpu_estimator.py: torch's HIP runtime first)
    import bipedal_control_amd as bp
    from tests import estimator_reference as er
    from tests import oracle_bridge as ob
    from tests.test_gpu_estimator import TOL, TOL_ANGULAR, _ref_update, _rel as rel_each, _split, _update
    itf, _ = robots[name]
    m = ob.model(name)
    nb = 16
    rng = np.random.default_rng(17)
    s = er.SensorTrajectories(m, nb, seed=5).at(37)
    s["mode"] = np.array(MODES16, np.int32)
    s["flags"] = np.array([er.mode_flags(mo) for mo in s["mode"]], np.int32)
    x0 = rng.standard_normal((nb, 18))
    P0 = np.zeros((nb, 18, 18))
    for b in range(nb):
        A = rng.standard_normal((18, 18))
        P0[b] = (A @ A.T + np.eye(18)) * (1e-5 if b >= 8 else 1.0)      # the second half stays below the xy reset's threshold
    worst = dict(x=0.0, P=0.0, lin=0.0, ang=0.0)
    for source in ("mode", "contact"):
        est = bp.BatchedStateEstimate(itf, kind="kalman", max_batch=nb)
        est.setState(x0, P0)
        rbd = _update(est, s, source=source)
        x, P = est.getState()
        xy = est.device_outputs()["xy_reset"].torch().cpu().numpy()
        for b in range(nb):
            f = er.KalmanFilter(m)
            f.x, f.P = x0[b].copy(), P0[b].copy()
            r, fired, margin, cond = _ref_update(f, s, b)
            assert abs(margin - 1.0) >= 1e-8
            assert xy[b] == fired, (name, source, b)
            lin, ang = _split(m, rbd[b])
            rl, ra = _split(m, r)
            worst = dict(x=max(worst["x"], rel_each(x[b], f.x)), P=max(worst["P"], rel_each(P[b], f.P)), lin=max(worst["lin"], rel_each(lin, rl)),
                         ang=max(worst["ang"], rel_each(ang, ra)))
            assert np.array_equal(P[b], P[b].T)
        assert set(xy.tolist()) == {0, 1}
    print("tree estimator", name, worst)
    _write_report("tree_estimator_%s" % name, worst)
    assert worst["x"] < TOL and worst["P"] < TOL and worst["lin"] < TOL and worst["ang"] < TOL_ANGULAR, worst
