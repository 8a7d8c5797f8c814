"""GPU parity tests (through the C ABI): HIP path vs the CPU oracle on the same seeded inputs.
Tolerances (FP64 both sides; different summation order and analytic-vs-AD derivatives):
  LQ model entries                 1e-11 relative to max(1, |oracle|_max) per quantity
  QP step dx, du, K                1e-9  relative, PER PHYSICAL BLOCK (tests/tolerances.py: momentum / base pose / joints of a state,
                                         contact forces / joint velocities of an input, the six row x column blocks of a gain)
  solve output x, u                1e-11 relative per block; K 1e-10 (measured on MI355X: 4e-14 / 5e-15, profiles/r03_parity_blocks.json;
                                         the OpenLoong cold start with its semi-definite input cost: 1e-9 / 1e-8)
The worst value per block that the hardware achieved is written to gpurun_out/parity_blocks.json by test_solve_matches_oracle
(committed copy: profiles/r03_parity_blocks.json).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.tolerances import rel_K, rel_u, rel_x  # noqa: E402  (per physical block: forces vs joint velocities, ...)


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


@pytest.fixture(scope="module")
def ctx():
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios
    from tests import oracle_bridge as ob
    itf = scenarios.h1_interface()
    return dict(bp=bp, sc=scenarios, ob=ob, itf=itf)


def _write_report(key, report):
    """Achieved per-block errors, for the record (never fails a test)."""
    import json
    import os
    try:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_blocks.json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = report
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except Exception:
        pass


def _views(mpc, name, per_node):
    raw = mpc.read(name)
    return raw.reshape(mpc.max_batch, mpc.max_nodes, *per_node) if per_node is not None else raw


def test_linearize_matches_oracle(ctx):
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    prob = sc.trot_problem(itf, batch=3, n_intervals=30)
    mpc = bp.BatchedSqpMpc(itf, max_batch=3, max_nodes=48, materialize_lq=True)     # the complete LQ model is compared, not only what the solve reads
    lay = mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    # move away from the cold start so that every term is exercised: one accepted step first
    mpc.enqueue(); mpc.synchronize()
    mpc.stage("linearize"); mpc.synchronize()
    nx = nu = itf.stateDim
    x = mpc.read("x").reshape(3, 49, nx); u = mpc.read("u").reshape(3, 48, nu)
    shapes = dict(A=(nx, nx), B=(nx, nu), b=(nx,), Q=(nx, nx), R=(nu, nu), P=(nu, nx), q=(nx,), r=(nu,), c=(), C=(16, nx), D=(16, nu), e=(16,), perf=(3,))
    dev = {k: _views(mpc, k, s) for k, s in shapes.items()}
    nc = mpc.read("nc").reshape(3, 48)
    om = ob.h1_oracle()
    worst = {}
    for b in range(3):
        nodes = ob.oracle_nodes(prob, b)
        assert nodes["N"] == lay["n_nodes_max"]
        for k in range(nodes["N"]):
            o = om.node_lq(nodes["kind"][k], nodes["dt"][k], x[b, k], u[b, k], x[b, k + 1], nodes["xref"][k], nodes["mode"][k], nodes["zref"][k], nodes["zdref"][k])
            assert int(nc[b, k]) == o["nc"]
            for name in shapes:
                worst[name] = max(worst.get(name, 0.0), _rel(dev[name][b, k], o[name]))
    assert max(worst.values()) < 1e-11, worst


def test_qp_step_matches_oracle(ctx):
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    prob = sc.trot_problem(itf, batch=2, n_intervals=40)
    mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=56, return_gains=True)
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    mpc.enqueue(); mpc.synchronize()      # generic iterate
    for st in ("linearize", "project", "riccati"):
        mpc.stage(st)
    mpc.synchronize()
    nx = nu = itf.stateDim
    x = mpc.read("x").reshape(2, 57, nx); u = mpc.read("u").reshape(2, 56, nu)
    dx = mpc.read("dx").reshape(2, 57, nx); du = mpc.read("du").reshape(2, 56, nu); K = mpc.read("K").reshape(2, 56, nu, nx)
    om = ob.h1_oracle()
    for b in range(2):
        nodes = ob.oracle_nodes(prob, b)
        N = nodes["N"]
        odx, odu, oK = om.qp_step(nodes, prob["x0"][b], x[b, :N + 1], u[b, :N])
        assert rel_x(dx[b, :N + 1], odx) < 1e-9
        assert rel_u(du[b, :N], odu) < 1e-9
        assert rel_K(K[b, :N], oK) < 1e-9


@pytest.mark.parametrize("iterations", [1, 3])
def test_solve_matches_oracle(ctx, iterations):
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    prob = sc.trot_problem(itf, batch=4, n_intervals=50)
    mpc = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=64, sqp_iterations=iterations, return_gains=True)
    t, x, u, K, stats = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    report = {}
    for b in range(4):
        xo, uo, Ko, st = ob.oracle_solve_like(prob, b, iterations=iterations)
        n = stats[b].n_nodes
        its = int(sum(1 for r in st if r[10] > 0))
        assert stats[b].iterations == its
        assert abs(stats[b].step_size - st[its - 1][3]) == 0.0
        assert rel_x(x[b, :n + 1], xo, report) < 1e-11
        assert rel_u(u[b, :n], uo, report) < 1e-11
        assert rel_K(K[b, :n], Ko, report) < 1e-10
        assert _rel(stats[b].merit_after, st[its - 1][4]) < 1e-9
    _write_report("solve_%d_iterations" % iterations, report)


def test_stance_config1(ctx):
    """BASELINE.json configs[0]: H1 stance, N = 20, single problem, cold start."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    prob = sc.stance_problem(itf, 20)
    mpc = bp.BatchedSqpMpc(itf, max_batch=1, max_nodes=24)
    t, x, u, K, stats = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    xo, uo, Ko, st = ob.oracle_solve_like(prob, 0)
    assert stats[0].n_nodes == 20
    assert np.allclose(t[0, :21], np.arange(21) * 0.015, atol=1e-12)
    assert rel_x(x[0, :21], xo) < 1e-11 and rel_u(u[0, :20], uo) < 1e-11
    # stance: joint velocities are pinned by the zero-velocity constraints
    assert np.abs(u[0, 0, 12:]).max() < 1e-9


def test_full_size_properties(ctx):
    """BASELINE.json configs[1] size: batch 256, N = 100.  Size-independent properties instead of the slow oracle:
    (a) a problem's solution does not depend on its batch neighbours or position (bitwise),
    (b) the linearised equality constraints hold for the QP step: C dx + D du + e = 0,
    (c) the QP step satisfies the linearised dynamics dx+ = A dx + B du + b,
    (d) three SQP iterations drive the constraint violation down."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    B, N = 256, 100
    prob = sc.trot_problem(itf, batch=B, n_intervals=N)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=112, sqp_iterations=3, materialize_lq=True)
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    for st in ("linearize", "project", "riccati"):
        mpc.stage(st)
    mpc.synchronize()
    nx = nu = itf.stateDim
    n = mpc.layout()["n_nodes_max"]
    dx = mpc.read("dx").reshape(B, 113, nx); du = mpc.read("du").reshape(B, 112, nu)
    A = mpc.read("A").reshape(B, 112, nx, nx); Bm = mpc.read("B").reshape(B, 112, nx, nu); bv = mpc.read("b").reshape(B, 112, nx)
    C = mpc.read("C").reshape(B, 112, 16, nx); D = mpc.read("D").reshape(B, 112, 16, nu); e = mpc.read("e").reshape(B, 112, 16)
    kind = mpc.read("g_kind")[:n]
    inter = kind == 0
    res_dyn = np.einsum("bkij,bkj->bki", A[:, :n], dx[:, :n]) + np.einsum("bkij,bkj->bki", Bm[:, :n], du[:, :n]) + bv[:, :n] - dx[:, 1:n + 1]
    assert np.abs(res_dyn).max() < 1e-9
    res_eq = np.einsum("bkij,bkj->bki", C[:, :n], dx[:, :n]) + np.einsum("bkij,bkj->bki", D[:, :n], du[:, :n]) + e[:, :n]
    # D is rank deficient (two contact points per rigid foot): exactly rank(D) rows are eliminated, the nc - rank rows
    # left out by the FullPivLU rank decision hold only to first order (|violation| * |step|).
    nc = mpc.read("nc").reshape(B, 112)[:, :n]
    nut = mpc.read("nut").reshape(B, 112)[:, :n]
    violated = (np.abs(res_eq) > 1e-8).sum(axis=2)
    dropped = nc - (nu - nut)
    assert np.all(violated[:, inter] <= dropped[:, inter]) and dropped[:, inter].max() <= 2
    # null-space basis of the projection: its joint rows come packed from the elimination kernel (Vt = joint rows of [Px | Pe | Pu], row
    # stride 48), its force rows are single ones in the columns of the stance components (generated by every reader from the contact mode)
    Vt = mpc.read("Vt").reshape(B, 112, nu - 12, 48)[:, :n]
    mode = mpc.read("g_mode")[:n].astype(int) & 3
    Pu = np.zeros((B, n, nu, nu))
    for k in range(n):
        if kind[k] != 0:
            continue
        first, count = (6 if mode[k] == 2 else 0), {0: 0, 1: 6, 2: 6, 3: 12}[mode[k]]
        for b_ in range(B):
            nt = int(nut[b_, k])
            Pu[b_, k, first + np.arange(count), np.arange(count)] = 1.0
            Pu[b_, k, 12:, :nt] = Vt[b_, k, :, nx + 1:nx + 1 + nt]
    DPu = np.einsum("bkij,bkjl->bkil", D[:, :n], Pu)
    assert np.abs(DPu[:, inter]).max() < 1e-10
    mpc.reset(); mpc.enqueue(); mpc.synchronize()
    t, x, u, K, stats = mpc.fetch()
    assert all(s.status == 0 for s in stats)
    viol0 = np.array([np.sqrt(s.dynamics_sse_before + s.equality_sse_before) for s in stats])
    viol1 = np.array([np.sqrt(s.dynamics_sse_after + s.equality_sse_after) for s in stats])
    # cold-start violation is O(0.1 .. 1); three filter-line-search iterations must bring every problem far below that
    assert np.all(viol1 < 5e-2) and np.median(viol1) < 5e-3 and np.all(viol1 <= viol0 + 1e-12)
    # (a) permutation / sub-batch invariance, bitwise
    sub = [200, 3, 77]
    prob2 = dict(prob, x0=prob["x0"][sub], targets=[prob["targets"][i] for i in sub])
    mpc2 = bp.BatchedSqpMpc(itf, max_batch=3, max_nodes=112, sqp_iterations=3)      # ... and of the solve mode: this handle runs fused
    t2, x2, u2, _, _ = mpc2.run(prob2["t0"], prob2["x0"], prob2["schedule"], prob2["targets"], horizon=prob2["horizon"])
    for j, i in enumerate(sub):
        assert np.array_equal(x2[j], x[i]) and np.array_equal(u2[j], u[i])


def test_openloong_24_dof_class(ctx):
    """nx = nu = 24 (12 leg joints): the reference's OpenLoong configuration, the dimension class of BASELINE.json
    configs[3].  Same tolerances as H1."""
    bp, sc, ob = ctx["bp"], ctx["sc"], ctx["ob"]
    itf = sc.interface("openloong")
    assert itf.stateDim == 24
    prob = sc.trot_problem(itf, batch=3, n_intervals=40, gait="standing_trot")
    mpc = bp.BatchedSqpMpc(itf, max_batch=3, max_nodes=64, return_gains=True)
    t, x, u, K, stats = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    for b in range(3):
        xo, uo, Ko, st = ob.oracle_solve_like(prob, b, robot="openloong")
        n = stats[b].n_nodes
        assert stats[b].step_size == st[0][3]
        # looser than H1's 1e-11: with six joints per leg the input cost J'RJ is only positive SEMI-definite (two contact points per rigid
        # foot), the cold-start step moves a swing-leg joint by ~10 rad and the stage Hessians are ill conditioned (measured 1.6e-11)
        assert rel_x(x[b, :n + 1], xo) < 1e-9 and rel_u(u[b, :n], uo) < 1e-9 and rel_K(K[b, :n], Ko) < 1e-8
    # reference kernels (lane-emulation verified) and fast kernels agree
    ref = bp.BatchedSqpMpc(itf, max_batch=3, max_nodes=64, reference_kernels=True)
    t2, x2, u2, _, _ = ref.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert rel_x(x2, x) < 1e-9 and rel_u(u2, u) < 1e-9


def test_per_problem_schedules_gait_sweep(ctx):
    """BASELINE.json configs[4] in miniature: every problem carries its own gait (mode schedule, swing references, grid)."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    gaits = ["stance", "trot", "standing_trot", "flying_trot"]
    prob = sc.gait_sweep_problem(itf, gaits, [(0.3, 0.0), (-0.2, 0.3)], n_intervals=60)
    nb = 8
    mpc = bp.BatchedSqpMpc(itf, max_batch=nb, max_nodes=96)
    t, x, u, K, stats = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert mpc.layout()["n_grids"] == len(gaits)      # identical (t0, schedule) pairs share one grid
    counts = set()
    for b in range(nb):
        xo, uo, _, st = ob.oracle_solve_like(prob, b)
        n = stats[b].n_nodes
        counts.add(n)
        assert n == xo.shape[0] - 1
        assert rel_x(x[b, :n + 1], xo) < 1e-11 and rel_u(u[b, :n], uo) < 1e-11
    assert len(counts) >= 3      # different gaits => different numbers of event nodes


def test_reference_and_fast_kernels_agree(ctx):
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    prob = sc.trot_problem(itf, batch=6, n_intervals=50, gait="flying_trot")
    a = bp.BatchedSqpMpc(itf, max_batch=6, max_nodes=72, sqp_iterations=2)
    b = bp.BatchedSqpMpc(itf, max_batch=6, max_nodes=72, sqp_iterations=2, reference_kernels=True)
    ra = a.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    rb = b.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert _rel(ra[1], rb[1]) < 1e-9 and _rel(ra[2], rb[2]) < 1e-9
    assert [s.step_size for s in ra[4]] == [s.step_size for s in rb[4]]


def test_pipelined_horizon_chunks_are_bit_identical(ctx):
    """The chunked horizon pipeline (Riccati sweep of the late stages overlapping with the linearisation / projection of the
    early ones) only reorders launches: every chunk count must give the same bits, also with grids of different lengths."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    gaits = ["stance", "trot", "standing_trot", "flying_trot"]
    prob = sc.gait_sweep_problem(itf, gaits, [(0.3, 0.0), (-0.2, 0.3)], n_intervals=60)
    results = []
    for chunks in (1, 2, 4, 7, 16):
        mpc = bp.BatchedSqpMpc(itf, max_batch=8, max_nodes=96, sqp_iterations=2, return_gains=True, pipeline_chunks=chunks)
        results.append(mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"]))
    for r in results[1:]:
        assert np.array_equal(r[1], results[0][1]) and np.array_equal(r[2], results[0][2]) and np.array_equal(r[3], results[0][3])
        assert [s.step_size for s in r[4]] == [s.step_size for s in results[0][4]]


def test_solver_reuse_across_gaits_matches_fresh_solver(ctx):
    """A solver handle that has projected wider reduced inputs at a node before (double stance, nut = 10) must give the same
    bits afterwards on a narrower problem (single support, nut = 9) as a fresh handle: the projection does not write the block columns
    and rows beyond nx + 1 + nut of the packed model (project_node.h, PackedLq), the sweep's staging masks them by nut."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    trot = sc.trot_problem(itf, batch=4, n_intervals=60)
    stance = sc.trot_problem(itf, batch=4, n_intervals=60, gait="stance")
    reused = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=80, sqp_iterations=2, return_gains=True)
    for prob in (trot, stance, trot):
        last = reused.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    fresh = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=80, sqp_iterations=2, return_gains=True)
    ref = fresh.run(trot["t0"], trot["x0"], trot["schedule"], trot["targets"], horizon=trot["horizon"])
    assert np.array_equal(last[1], ref[1]) and np.array_equal(last[2], ref[2]) and np.array_equal(last[3], ref[3])


# 300 > number of CUs: the eight-wave sweep in two rounds (the default of the 22-state robots since round 6) or, BPMPC_R8_ROUNDS=1, the four-wave workgroups
# (two per CU; what nx = 24 runs at that batch)
@pytest.mark.parametrize("batch,r8_rounds", [(48, None), (300, None), (300, "1"), (600, None),
                                              # the boundaries of the eight-wave sweep in rounds (nx = 22: three rounds of 256): the end of the second round, the full third
                                              # round, and the first batch on a wave per problem
                                              (512, None), (768, None), (769, None)])
def test_repeated_solves_are_bit_identical(ctx, batch, r8_rounds, monkeypatch):
    """Races, stale LDS or stale HBM scratch would show up as run-to-run differences; also checks the larger-batch Riccati variants
    against the oracle."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    if r8_rounds: monkeypatch.setenv("BPMPC_R8_ROUNDS", r8_rounds)
    prob = sc.trot_problem(itf, batch=batch, n_intervals=30, gait="flying_trot")
    mpc = bp.BatchedSqpMpc(itf, max_batch=batch, max_nodes=48, sqp_iterations=2, return_gains=True)
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    ref = None
    for i in range(12):
        mpc.reset(); mpc.enqueue()
        t, x, u, K, st = mpc.fetch(gains=True)
        if ref is None:
            ref = (x.copy(), u.copy(), K.copy())
        else:
            assert np.array_equal(x, ref[0]) and np.array_equal(u, ref[1]) and np.array_equal(K, ref[2])
    for b in (0, batch - 1):
        xo, uo, Ko, _ = ob.oracle_solve_like(prob, b, iterations=2)
        n = st[b].n_nodes
        assert rel_x(x[b, :n + 1], xo) < 1e-11 and rel_u(u[b, :n], uo) < 1e-11 and rel_K(K[b, :n], Ko) < 1e-10


@pytest.mark.parametrize("n_intervals,max_nodes", [(1, 8), (2, 8), (3, 8), (450, 512)])
def test_shortest_and_longest_horizons(ctx, n_intervals, max_nodes):
    """One to three intervals, and a horizon that fills the solver's maximum of 512 stages (482 nodes with the gait events)."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    prob = sc.trot_problem(itf, batch=2, n_intervals=n_intervals)
    mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=max_nodes, return_gains=True)
    t, x, u, K, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    n = st[0].n_nodes
    assert n >= n_intervals and all(s.status == 0 for s in st)
    xo, uo, Ko, so = ob.oracle_solve_like(prob, 1)
    assert xo.shape[0] == n + 1 and st[1].step_size == so[0][3]
    assert rel_x(x[1, :n + 1], xo) < 1e-11 and rel_u(u[1, :n], uo) < 1e-11 and rel_K(K[1, :n], Ko) < 1e-10


@pytest.mark.parametrize("t0", [0.175, 0.175 - 30 * 0.015])
def test_gait_event_on_the_window_boundaries(ctx, t0):
    """A mode switch exactly at the initial time resp. exactly at the final time of the horizon (events at -1.225 + 0.35 k)."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    horizon = 30 * sc.DT
    sched = sc.gait_schedule(itf, "trot", t0, horizon)
    ev = np.asarray(sched.eventTimes)
    assert np.any(np.abs(ev - t0) < 1e-12) or np.any(np.abs(ev - (t0 + horizon)) < 1e-12)
    x0 = sc.perturbed_initial_states(itf, 1)
    tg = [itf.cmdVelToTargetTrajectories((0.3, 0.0, 0.0, 0.0), t0, x0[0], horizon)]
    prob = dict(t0=t0, x0=x0, schedule=sched, targets=tg, horizon=horizon)
    mpc = bp.BatchedSqpMpc(itf, max_batch=1, max_nodes=48)
    t, x, u, _, st = mpc.run(t0, x0, sched, tg, horizon=horizon)
    n = st[0].n_nodes
    xo, uo, _, _ = ob.oracle_solve_like(prob, 0)
    assert xo.shape[0] == n + 1 and rel_x(x[0, :n + 1], xo) < 1e-11 and rel_u(u[0, :n], uo) < 1e-11


@pytest.mark.parametrize("robot,gait", [("h1", "trot"), ("h1", "flying_trot"), ("g1", "standing_trot")])
def test_fused_and_materialised_modes_are_bit_identical(ctx, robot, gait):
    """settings.materialize_lq only decides what the lineariser leaves in HBM (the complete LQ model of the reference, or just what the
    rest of the solve reads): x, u, K, the statistics and every buffer both modes write must agree bit for bit - also after the
    handle has switched modes, and on a handle that is reused for another gait (stale rows / stale padding must never be read)."""
    bp, sc = ctx["bp"], ctx["sc"]
    itf = sc.interface(robot)
    nx = itf.stateDim
    prob = sc.trot_problem(itf, batch=5, n_intervals=45, gait=gait)
    other = sc.trot_problem(itf, batch=5, n_intervals=45, gait="stance")
    out = {}
    for mat in (True, False):
        mpc = bp.BatchedSqpMpc(itf, max_batch=5, max_nodes=72, sqp_iterations=3, return_gains=True, materialize_lq=mat)
        mpc.run(other["t0"], other["x0"], other["schedule"], other["targets"], horizon=other["horizon"])     # leaves 12-row nodes with other contents behind
        t, x, u, K, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
        n = st[0].n_nodes
        mpc.stage("linearize"); mpc.stage("project"); mpc.synchronize()
        extra = {k: mpc.read(k) for k in ("b", "q", "r", "perf", "nc", "Vt", "Pe", "nut", "Wt", "Qp", "Mt")}      # the projected model in the packed layout of the fast kernels
        A = mpc.read("A").reshape(5, 72, nx, nx)[:, :n, 3:12].copy()          # the dense rows are written in both modes
        out[mat] = (x, u, K, [(s.step_size, s.merit_after, s.dynamics_sse_after, s.equality_sse_after, s.iterations) for s in st], extra, A, mpc)
    a, b = out[True], out[False]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    kinds = a[6].read("g_kind").reshape(5, 72)[0, :a[5].shape[1]]
    for k in a[4]:
        if k in ("q", "r"):      # the cost gradient of an event node is zero by definition: only the materialised mode stores those zeros
            va, vb = (v[k].reshape(5, 72, nx)[:, :len(kinds)][:, kinds == 0] for v in (a[4], b[4]))
            assert np.array_equal(va, vb), k
        else:
            assert np.array_equal(a[4][k], b[4][k]), k
    assert np.array_equal(a[5][:, kinds == 0], b[5][:, kinds == 0])
    # switching a live handle: fused -> materialised gives the materialised handle's complete model
    b[6].set_materialize(True)
    b[6].stage("linearize"); b[6].synchronize()
    for k in ("A", "B", "Q", "R", "C", "D", "e", "c"):
        assert np.array_equal(a[6].read(k), b[6].read(k)), k


def test_reg_prim_setting_matches_oracle(ctx):
    """settings.reg_prim = 1e-12 (HPIPM's primal regularisation, off by default): the HIP path and the oracle apply it identically (QP step
    1e-9), and its effect on the step is the measured ~1e-9..1e-8 - visible, below the solve tolerance."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    prob = sc.trot_problem(itf, batch=2, n_intervals=40)
    outs = []
    for reg in (0.0, 1e-12, 1e-6):
        mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=56, return_gains=True, reg_prim=reg)
        mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
        for st in ("linearize", "project", "riccati"):
            mpc.stage(st)
        mpc.synchronize()
        nx = itf.stateDim
        x = mpc.read("x").reshape(2, 57, nx); u = mpc.read("u").reshape(2, 56, nx)
        dx = mpc.read("dx").reshape(2, 57, nx); du = mpc.read("du").reshape(2, 56, nx); K = mpc.read("K").reshape(2, 56, nx, nx)
        om = ob.h1_oracle()
        for b in range(2):
            nodes = ob.oracle_nodes(prob, b)
            N = nodes["N"]
            odx, odu, oK = om.qp_step(nodes, prob["x0"][b], x[b, :N + 1], u[b, :N], reg_prim=reg)
            assert rel_x(dx[b, :N + 1], odx) < 1e-9 and rel_u(du[b, :N], odu) < 1e-9 and rel_K(K[b, :N], oK) < 1e-9
        outs.append(du.copy())
    assert 0.0 < _rel(outs[1], outs[0]) < 1e-7 < _rel(outs[2], outs[0])
    with pytest.raises(bp.BpmpcError):
        bp.BatchedSqpMpc(itf, max_batch=1, max_nodes=8, reg_prim=1e-12, reference_kernels=True)


def _modes_seen(got, n):
    kind = got["g_kind"][:n].astype(int)
    return set(got["g_mode"][:n].astype(int)[kind == 0] & 3)


def _structured_against_dense(structured, dense, B, N, n, nx):
    """The packed projected model Wt, Qp, Mt of the first n nodes in the region the sweep reads, a handle on the structured path against one under
    BPMPC_DENSE_PROJECT=1 (each the dict of buffers test_structured_and_dense_change_of_variables_agree reads): the worst relative difference.
    Also used by tests/test_gpu_row_kernel_edges.py."""
    wp = ((2 * nx + 1 + 15) // 16) * 16
    got = {"0": structured, "1": dense}
    nut = got["0"]["nut"].reshape(B, N)[:, :n].astype(int)
    assert np.array_equal(nut, got["1"]["nut"].reshape(B, N)[:, :n])
    kind = got["0"]["g_kind"][:n].astype(int)
    W = {d: got[d]["Wt"].reshape(B, N, nx, wp)[:, :n] for d in got}
    Q = {d: got[d]["Qp"].reshape(B, N, nx, 32)[:, :n] for d in got}
    M = {d: got[d]["Mt"].reshape(B, N, nx, wp)[:, :n] for d in got}
    Vt = got["0"]["Vt"].reshape(B, N, nx - 12, wp)[:, :n]
    bb = got["0"]["b"].reshape(B, N, nx)[:, :n]
    dt = got["0"]["g_dt"][:n]
    worst = 0.0
    for other in ("0",):
        for b in range(B):
            for k in range(n):
                nt = nut[b, k]
                cend = 16 * ((nx + 1 + nt + 15) // 16) if kind[k] == 0 else 32
                # the structured path leaves the joint rows of Wt to the sweep (round 4, every regime but the four-wave kernel): rows 0..11 are compared
                # as written, the joint rows of the dense path against what the sweep's loaders complete: [I | b | 0] + dt x (joint rows of [Px | Pe | Pu]) = Vt
                done = dt[k] * Vt[b, k, :, :cend]
                done[:, 12:nx] += np.eye(nx - 12); done[:, nx] += bb[b, k, 12:]
                pairs = [(W[other][b, k, :12, :cend], W["1"][b, k, :12, :cend]), (done, W["1"][b, k, 12:, :cend]), (Q[other][b, k, :, :nx + 1], Q["1"][b, k, :, :nx + 1])]
                if kind[k] == 0:
                    pairs.append((M[other][b, k, :nt, :cend], M["1"][b, k, :nt, :cend]))
                for a, d in pairs:
                    worst = max(worst, _rel(a, d))
    return worst


@pytest.mark.parametrize("robot,gait", [("h1", "trot"), ("h1", "standing_trot"), ("h1", "flying_trot"), ("hunter", "trot"), ("g1", "standing_trot"),
                                         ("openloong", "flying_trot")])
def test_structured_and_dense_change_of_variables_agree(ctx, robot, gait, monkeypatch):
    """The change of variables behind the structured elimination (packed joint rows Vt, force rows generated in registers) against the
    same kernel behind the general elimination outputs (Px, Pu, Pe written in full, BPMPC_DENSE_PROJECT=1): the packed projected model Wt = [At | bt | Bt], Qp = [Qt | qt], Mt = [Pt | rt | Rt] of every node, in
    the region the sweep reads (block columns < nbc, rows < nut of Mt), on all four contact modes, after one accepted step."""
    bp, sc = ctx["bp"], ctx["sc"]
    itf = sc.interface(robot)
    nx = itf.stateDim
    wp = ((2 * nx + 1 + 15) // 16) * 16
    B, N = 3, 64
    prob = sc.trot_problem(itf, batch=B, n_intervals=45, gait=gait)
    got = {}
    # "1": elimination outputs Px, Pu, Pe in full + k_project_fast<.., false>;  "0" (default): packed joint rows + k_project_fast<.., true>
    for dense in ("0", "1"):
        monkeypatch.setenv("BPMPC_DENSE_PROJECT", dense)
        mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=N)
        lay = mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
        mpc.enqueue(); mpc.synchronize()                                  # away from the cold start
        mpc.stage("linearize"); mpc.stage("project"); mpc.synchronize()
        got[dense] = {k: mpc.read(k) for k in ("Wt", "Qp", "Mt", "nut", "g_kind", "g_mode", "Vt", "b", "g_dt")}
        n = lay["n_nodes_max"]
    modes = _modes_seen(got["0"], n)
    assert modes >= ({0, 1, 2} if "flying" in gait else ({1, 2} if gait == "trot" else {1, 2, 3}))
    worst = _structured_against_dense(got["0"], got["1"], B, N, n, nx)
    assert worst < 1e-12, worst


@pytest.mark.parametrize("robot,gait", [("h1", "trot"), ("h1", "standing_trot"), ("h1", "flying_trot"), ("g1", "standing_trot"), ("hunter", "trot")])
@pytest.mark.parametrize("variant", ["2", "4"])
def test_wave_per_problem_sweep_matches_the_workgroup_sweep(ctx, robot, gait, variant, monkeypatch):
    """riccati_wave.h (one wavefront owns a problem: batches larger than the chip) against the workgroup-per-problem sweep of the same
    solver, same solves to rounding (the wave kernel reads S transposed instead of symmetrising it), and against the oracle at the
    tolerance of the other solve tests.  All contact modes incl. event nodes; two iterations so that the second starts from the first's step."""
    bp, sc, ob = ctx["bp"], ctx["sc"], ctx["ob"]
    itf = sc.interface(robot)
    prob = sc.trot_problem(itf, batch=5, n_intervals=45, gait=gait)
    out = {}
    for wave in ("0", variant):              # "2": riccati_wave.h (one wave per SIMD), "4": riccati_wave2.h (two) - forced at this small batch
        monkeypatch.setenv("BPMPC_RICCATI_WAVE", wave)
        mpc = bp.BatchedSqpMpc(itf, max_batch=5, max_nodes=72, sqp_iterations=2, return_gains=True)
        out[wave] = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    (t, x, u, K, st), (_, x1, u1, K1, st1) = out["0"], out[variant]
    n = st[0].n_nodes
    assert all(s.status == 0 for s in st1)
    assert [s.step_size for s in st] == [s.step_size for s in st1]
    assert rel_x(x1[:, :n + 1], x[:, :n + 1]) < 1e-11 and rel_u(u1[:, :n], u[:, :n]) < 1e-11 and rel_K(K1[:, :n], K[:, :n]) < 1e-10
    if robot == "h1":
        for b in (0, 4):
            xo, uo, Ko, _ = ob.oracle_solve_like(prob, b, iterations=2)
            assert rel_x(x1[b, :n + 1], xo) < 1e-11 and rel_u(u1[b, :n], uo) < 1e-11 and rel_K(K1[b, :n], Ko) < 1e-10


def test_config2_with_the_template_tiled_from_zero(ctx):
    """SURVEY.md section 8(d) config 2 to the letter: the trot template is inserted at t = 0, so the solve starts ON a mode switch (the
    scenarios default inserts it 3.5 half periods earlier, t0 mid-swing).  Same comparison as the other solve tests."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    prob = sc.trot_problem(itf, batch=4, n_intervals=60, gait_start=0.0)
    assert abs(prob["schedule"].eventTimes[np.searchsorted(prob["schedule"].eventTimes, -1e-9)]) < 1e-12      # a switch at t0 = 0
    mpc = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=80, sqp_iterations=2, return_gains=True)
    t, x, u, K, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    n = st[0].n_nodes
    for b in (0, 3):
        xo, uo, Ko, _ = ob.oracle_solve_like(prob, b, iterations=2)
        assert rel_x(x[b, :n + 1], xo) < 1e-11 and rel_u(u[b, :n], uo) < 1e-11 and rel_K(K[b, :n], Ko) < 1e-10


def test_h1_batch_beyond_four_problems_per_cu_matches_oracle(ctx):
    """Batch 1100 on the 256-CU chip: the sweep runs riccati_wave2.h (two wavefronts per SIMD, one per problem).  First, middle and last
    problem against the oracle; every problem reports success."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    B = 1100
    prob = sc.trot_problem(itf, batch=B, n_intervals=45)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=72, sqp_iterations=2, return_gains=True)
    t, x, u, K, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    n = st[0].n_nodes
    assert all(s.status == 0 for s in st)
    for b in (0, 550, B - 1):
        xo, uo, Ko, _ = ob.oracle_solve_like(prob, b, iterations=2)
        assert rel_x(x[b, :n + 1], xo) < 1e-11 and rel_u(u[b, :n], uo) < 1e-11 and rel_K(K[b, :n], Ko) < 1e-10


def test_batch_4096_full_size_matches_small_batches_and_oracle(ctx):
    """configs[2] on one GPU at its full size (4096 problems, horizon 100): the sweep runs riccati_wave2.h, sixteen problems per CU.  A
    problem's solution does not depend on its batch: first, middle and last problem against the same three solved as a batch of their own
    (eight-wave sweep, one problem per CU) to rounding, one of them against the oracle; every problem reports success and the
    violation of every problem goes down."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    B, N, NN = 4096, 100, 116
    prob = sc.trot_problem(itf, batch=B, n_intervals=N)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=NN, sqp_iterations=2)
    t, x, u, _, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert all(s.status == 0 for s in st)
    v0 = np.array([np.sqrt(s.dynamics_sse_before + s.equality_sse_before) for s in st])
    v1 = np.array([np.sqrt(s.dynamics_sse_after + s.equality_sse_after) for s in st])
    assert np.all(v1 <= v0 + 1e-12) and np.median(v1) < 0.2 * np.median(v0)
    sub = [0, 2047, 4095]
    prob2 = dict(prob, x0=prob["x0"][sub], targets=[prob["targets"][i] for i in sub])
    mpc2 = bp.BatchedSqpMpc(itf, max_batch=3, max_nodes=NN, sqp_iterations=2)
    _, x2, u2, _, st2 = mpc2.run(prob2["t0"], prob2["x0"], prob2["schedule"], prob2["targets"], horizon=prob2["horizon"])
    n = st2[0].n_nodes
    for j, i in enumerate(sub):
        assert st[i].step_size == st2[j].step_size
        assert rel_x(x[i, :n + 1], x2[j, :n + 1]) < 1e-10 and rel_u(u[i, :n], u2[j, :n]) < 1e-10
    xo, uo, _, _ = ob.oracle_solve_like(prob2, 2, iterations=2)
    assert rel_x(x[4095, :n + 1], xo) < 1e-11 and rel_u(u[4095, :n], uo) < 1e-11
    # (round 5) sixteen more problems spread over the batch - every CU position of the sixteen-per-CU sweep is hit - against the oracle
    for i in np.linspace(1, B - 2, 16).astype(int):
        xo, uo, _, _ = ob.oracle_solve_like(prob, int(i), iterations=2)
        assert rel_x(x[i, :n + 1], xo) < 1e-11 and rel_u(u[i, :n], uo) < 1e-11, i


def test_batch_4096_tiled_from_zero_back_tracking_problems_match_oracle(ctx):
    """configs[2] as bench.py times it since round 5 (template tiled from t = 0: the solve starts on a mode switch): a handful of the 4096 problems
    reject the full step and take alpha = 0.5 in the second, batch-wide line-search round.  Every one of them, and as many that accept at once,
    against the oracle: iterate, step size and merit; the others are untouched by the second round (their step size is 1)."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    B, N, NN = 4096, 100, 116
    prob = sc.trot_problem(itf, batch=B, n_intervals=N, gait_start=0.0)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=NN)
    t, x, u, _, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert all(s.status == 0 for s in st)
    steps = np.array([s.step_size for s in st])
    back = np.flatnonzero(steps < 1.0)
    assert 1 <= len(back) <= 64 and np.all(steps[back] == 0.5), (len(back), np.unique(steps))
    n = st[0].n_nodes
    others = [int(i) for i in np.linspace(0, B - 1, len(back) + 2).astype(int) if steps[i] == 1.0][:len(back)]
    for i in list(back) + others:
        xo, uo, _, so = ob.oracle_solve_like(prob, int(i), iterations=1)
        assert rel_x(x[i, :n + 1], xo) < 1e-11 and rel_u(u[i, :n], uo) < 1e-11, i
        assert so[0][3] == steps[i], (i, so[0][3], steps[i])              # column 3 of the oracle's per-iteration record: the accepted step size


@pytest.mark.parametrize("variant", ["2", "4"])
def test_wave_sweeps_chunked_horizon_and_handle_reuse(ctx, variant, monkeypatch):
    """The sweeps that give a problem one or two wavefronts of its own (riccati_wave.h "2", riccati_wave2.h "4", forced at
    this small batch): (1) the chunked horizon pipeline hands [S | s] and the status from launch to launch through the carry record -
    every chunk count gives the same bits, also with grids of different lengths; (2) a handle that has seen wider reduced inputs at a node
    gives the same bits on a narrower problem as a fresh one (block columns and rows beyond nx + 1 + nut are neither loaded nor used)."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    monkeypatch.setenv("BPMPC_RICCATI_WAVE", variant)
    gaits = ["stance", "trot", "standing_trot", "flying_trot"]
    prob = sc.gait_sweep_problem(itf, gaits, [(0.3, 0.0), (-0.2, 0.3)], n_intervals=60)
    results = []
    for chunks in (1, 3, 7):
        mpc = bp.BatchedSqpMpc(itf, max_batch=8, max_nodes=96, sqp_iterations=2, return_gains=True, pipeline_chunks=chunks)
        results.append(mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"]))
    for r in results[1:]:
        assert np.array_equal(r[1], results[0][1]) and np.array_equal(r[2], results[0][2]) and np.array_equal(r[3], results[0][3])
        assert [s.step_size for s in r[4]] == [s.step_size for s in results[0][4]]
    trot = sc.trot_problem(itf, batch=4, n_intervals=60)
    stance = sc.trot_problem(itf, batch=4, n_intervals=60, gait="stance")
    reused = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=80, sqp_iterations=2, return_gains=True)
    for p in (trot, stance, trot):
        last = reused.run(p["t0"], p["x0"], p["schedule"], p["targets"], horizon=p["horizon"])
    fresh = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=80, sqp_iterations=2, return_gains=True)
    ref = fresh.run(trot["t0"], trot["x0"], trot["schedule"], trot["targets"], horizon=trot["horizon"])
    assert np.array_equal(last[1], ref[1]) and np.array_equal(last[2], ref[2]) and np.array_equal(last[3], ref[3])


@pytest.mark.parametrize("variant", ["0", "2", "4"])
def test_indefinite_hessian_is_reported_by_every_sweep(ctx, variant, monkeypatch, tmp_path):
    """Fail loudly: with a NEGATIVE input weight the reduced Hessian of a stage has a non-positive pivot; every sweep kernel has to report
    the numerical failure (status 2, bpmpc.h) for the problem instead of returning numbers - the eight-wave sweep ("0" at this batch) and
    the sweeps with one or two wavefronts per problem, forced."""
    bp, sc = ctx["bp"], ctx["sc"]
    monkeypatch.setenv("BPMPC_RICCATI_WAVE", variant)
    text = open(sc.H1["task"]).read()
    a = text.index("\nR\n{")
    bad = tmp_path / "task_negative_R.info"
    bad.write_text(text[:a] + text[a:].replace("scaling 1e-3", "scaling -1e-3", 1))
    itf = bp.BipedalRobotInterface(str(bad), sc.H1["urdf"], sc.H1["reference"])
    itf.gaitFile = sc.H1["gait"]
    prob = sc.trot_problem(itf, batch=3, n_intervals=30)
    mpc = bp.BatchedSqpMpc(itf, max_batch=3, max_nodes=48, sqp_iterations=1)
    t, x, u, _, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert all(s.status == 2 for s in st), [s.status for s in st]




def test_lineariser_with_the_event_nodes_out_of_the_way_is_bit_identical(ctx, monkeypatch):
    """Round 6: when the batch lies on one grid the lineariser maps its lane groups onto the intermediate nodes first (closed-form slot -> node map) and
    the event nodes onto workgroups of their own (Launch::lin_ev; BPMPC_LIN_COMPACT=0 keeps them in line): the same LQ model, bit for bit, in both
    output modes - and a batch on several grids (different gait phases) takes the in-line map and still matches itself."""
    bp, sc, itf = ctx["bp"], ctx["sc"], ctx["itf"]
    prob = sc.trot_problem(itf, batch=21, n_intervals=60, gait_start=0.0)          # 21 x 64 node slots: a last workgroup that is partly empty
    out = {}
    for compact in ("1", "0"):
        monkeypatch.setenv("BPMPC_LIN_COMPACT", compact)
        for mat in (True, False):
            mpc = bp.BatchedSqpMpc(itf, max_batch=21, max_nodes=72, materialize_lq=mat)
            lay = mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
            assert lay["n_grids"] == 1
            kinds = mpc.read("g_kind").reshape(21, 72)[0, :lay["n_nodes_max"]]
            assert 1 <= int((kinds == 1).sum()) <= 8
            mpc.stage("linearize"); mpc.synchronize()
            names = ("A", "B", "b", "Q", "R", "q", "r", "c", "C", "D", "e", "perf", "qrd", "nc") if mat else ("b", "q", "r", "e", "perf", "qrd", "nc")
            out[(compact, mat)] = {k: mpc.read(k).copy() for k in names}
            t, x, u, _, st = (mpc.enqueue(), mpc.synchronize(), mpc.fetch())[2]
            out[(compact, mat)]["x"] = x.copy(); out[(compact, mat)]["u"] = u.copy()
    for mat in (True, False):
        for k, v in out[("1", mat)].items():
            assert np.array_equal(v, out[("0", mat)][k]), (mat, k)


@pytest.mark.parametrize("batch,n_intervals,cap,min_nodes", [(2, 440, 500, 400), (258, 225, 250, 216), (2, 171, 200, 0), (2, 173, 200, 0), (2, 176, 200, 0)])
def test_horizons_beyond_the_roll_outs_lds_history_match_oracle(ctx, batch, n_intervals, cap, min_nodes, monkeypatch):
    """The roll-out behind the workgroup sweeps keeps its state history in LDS and walks a longer horizon in several passes.  Eight-wave kernel
    (riccati_rollout_ring, round 6: one wave computes, six stream chunks of four stages into a ring in LDS): 184 stages per pass - ~460 nodes are three
    passes, the horizons of 171 .. 176 intervals put the node count at and next to the pass length (a last chunk that is partly beyond the horizon, a second
    pass of a few stages).  Four-wave kernel (riccati_rollout_deep, batch > number of CUs): ~216 stages per pass, ~236 nodes.  Against the oracle."""
    bp, sc, ob, itf = ctx["bp"], ctx["sc"], ctx["ob"], ctx["itf"]
    if batch > 256: monkeypatch.setenv("BPMPC_R8_ROUNDS", "1")       # the four-wave workgroups (by default this robot runs the eight-wave sweep in rounds up to batch 768)
    prob = sc.trot_problem(itf, batch=batch, n_intervals=n_intervals)
    mpc = bp.BatchedSqpMpc(itf, max_batch=batch, max_nodes=cap, return_gains=True)
    t, x, u, K, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    n = st[0].n_nodes
    assert n > min_nodes and all(s.status in (0, 1) for s in st)
    for b in (0, batch - 1):
        xo, uo, Ko, _ = ob.oracle_solve_like(prob, b)
        assert rel_x(x[b, :n + 1], xo) < 1e-10 and rel_u(u[b, :n], uo) < 1e-10 and rel_K(K[b, :n], Ko) < 1e-9, (b, rel_x(x[b, :n + 1], xo), rel_u(u[b, :n], uo))
