"""GPU tier: behaviour of the C ABI beyond the cold-start happy path - warm start, one-call entry point, capacity and
argument errors, multi-iteration convergence flags, and the bench.py output contract."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.tolerances import rel_K, rel_u, rel_x  # noqa: E402  (per physical block: forces vs joint velocities, ...)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


@pytest.fixture(scope="module")
def ctx():
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios
    from tests import oracle_bridge as ob
    return bp, scenarios, ob, scenarios.h1_interface()


def test_one_call_entry_point_and_warm_start(ctx):
    bp, sc, ob, itf = ctx
    prob = sc.trot_problem(itf, batch=3, n_intervals=30)
    mpc = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=40, return_gains=True)
    t, x, u, K, st = mpc.solve_batch(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    n = st[0].n_nodes
    for b in range(3):
        xo, uo, Ko, _ = ob.oracle_solve_like(prob, b)
        assert rel_x(x[b, :n + 1], xo) < 1e-11 and rel_u(u[b, :n], uo) < 1e-11 and rel_K(K[b, :n], Ko) < 1e-10
    # warm start: the previous solution is the initial iterate of the next solve (mpc.coldStart false, task.info:173);
    # the measured state differs from the first node of the iterate, so dx_0 != 0
    x0b = prob["x0"] + 1e-3
    t2, x2, u2, _, st2 = mpc.solve_batch(prob["t0"], x0b, prob["schedule"], [itf.cmdVelToTargetTrajectories((0.3, 0, 0, 0), 0.0, x0b[b], prob["horizon"]) for b in range(3)],
                                         horizon=prob["horizon"], warm_x=x, warm_u=u)
    for b in range(3):
        p2 = dict(prob, x0=x0b, targets=[itf.cmdVelToTargetTrajectories((0.3, 0, 0, 0), 0.0, x0b[b], prob["horizon"]) for b in range(3)])
        xo, uo, _, sto = ob.oracle_solve_like(p2, b, x_init=x[b, :n + 1], u_init=u[b, :n])
        assert st2[b].step_size == sto[0][3]
        assert rel_x(x2[b, :n + 1], xo) < 1e-11 and rel_u(u2[b, :n], uo) < 1e-11
        assert np.abs(x2[b, 0] - x0b[b]).max() < 1e-12 or st2[b].step_size < 1.0    # full step lands on the measured state


def test_capacity_and_argument_errors(ctx):
    bp, sc, ob, itf = ctx
    prob = sc.trot_problem(itf, batch=4, n_intervals=30)
    mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=40)
    with pytest.raises(bp.BpmpcError) as e:
        mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert e.value.status == -6                                      # BPMPC_ERR_CAPACITY: batch > max_batch
    small = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=16)
    with pytest.raises(bp.BpmpcError) as e:
        small.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert e.value.status == -6 and "max_nodes" in str(e.value)       # grid longer than max_nodes
    with pytest.raises(bp.BpmpcError) as e:
        small.enqueue()                                               # run before any successful setup
    assert e.value.status == -1
    with pytest.raises(bp.BpmpcError):                                # shared schedule with different t0
        bp.BatchedSqpMpc(itf, 4, 64).setup(np.array([0.0, 0.1, 0.0, 0.0]), prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    # a schedule whose first swing has no lift-off inside the window is rejected like SwingTrajectoryPlanner does
    bad = bp.ModeSchedule(np.array([5.0]), np.array([1, 3], np.int32))
    with pytest.raises(bp.BpmpcError):
        bp.BatchedSqpMpc(itf, 4, 64).setup(prob["t0"], prob["x0"], bad, prob["targets"], horizon=prob["horizon"])


def test_iterations_and_convergence_flags(ctx):
    bp, sc, ob, itf = ctx
    prob = sc.stance_problem(itf, 20)
    mpc = bp.BatchedSqpMpc(itf, max_batch=1, max_nodes=24, sqp_iterations=10)
    t, x, u, _, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    xo, uo, _, sto = ob.oracle_solve_like(prob, 0, iterations=10)
    its = int(sum(1 for r in sto if r[10] > 0))
    assert st[0].iterations == its and 1 < its <= 10                  # converged before the iteration cap, like the oracle
    assert rel_x(x[0, :21], xo) < 1e-7 and st[0].dynamics_sse_after + st[0].equality_sse_after < 1e-8


def test_bench_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "32", "--intervals", "40",
                          "--cpu-sample", "4", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["dtype"] == "f64" and d["vs_baseline"] is None and d["scaling"] == "weak" and d["n_gpus"] == 1 and d["steps"] == 3
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(d["roofline"]) and d["roofline"]["bound"] in ("hbm", "fp64-issue", "mfma", "latency")
    assert set(("linearize", "riccati")) <= set(d["roofline_all"]) and any(v.get("dominant") for v in d["roofline_all"].values() if isinstance(v, dict))
    for cls, v in d["roofline_all"].items():
        if not isinstance(v, dict):
            continue
        assert set(("frac", "frac_basis", "hbm_util", "packed_bytes_per_unit", "algorithmic_bytes_per_unit", "bound")) <= set(v), cls
        if v["traffic_ratio"] is not None and v["traffic_ratio"] < 1.0:       # packed operands: the fraction is counted on the bytes the kernel moves
            assert v["frac_basis"].startswith("counter") and abs(v["frac"] - v["hbm_util"]) < 1e-3 and v["packed_bytes_per_unit"] < v["algorithmic_bytes_per_unit"]
        if v["hbm_util"] is not None and v["hbm_util"] < 0.5 and max(v["bound_fracs"].values()) < 0.5:
            assert v["bound"] == "latency", cls
    ts = d["timing_spread"]
    assert ts["regions"] == 5 and ts["ms_per_step_min"] <= ts["ms_per_step_median"] <= ts["ms_per_step_max"] and ts["ms_per_step_min"] > 0
    assert d["cpu_baseline_analytic"]["max_abs_x_diff_vs_gpu"] < 1e-8 and d["cpu_baseline_analytic"]["failures"] == 0
    assert abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-4
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["max_abs_x_diff_vs_gpu"] < 1e-8
    assert "workload" in d["config"] and d["value"] > 0


def test_bench_plain_line_and_dumped_outputs(ctx, tmp_path):
    """Without --full the line carries the headline figure of exactly --steps timed steps and nothing measured beside it; --dump-outputs
    writes the solution of the last timed step: the same numbers from run to run, and what the solver returns for the same problems."""
    bp, sc, _, _ = ctx
    itf = sc.interface("h1")            # as bench.py builds it

    def bench(d):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--batch", "32", "--intervals", "40",
                              "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    a, b = bench(tmp_path / "a"), bench(tmp_path / "b")
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(a) and a["steps"] == 4 and a["dtype"] == "f64"
    assert not {"roofline", "roofline_all", "cpu_baseline", "fused", "kernel_ms_per_step", "timing_spread"} & set(a)
    assert abs(a["value"] - 32 * 1e3 / a["ms_per_step"]) <= 1e-3 * a["value"]
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert {"t.npy", "x.npy", "u.npy", "stats_n_nodes.npy", "stats_status.npy"} <= set(names) and names == sorted(p.name for p in (tmp_path / "b").iterdir())
    for n in names:
        da, db = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert da.dtype == np.float64 and np.array_equal(da, db), n
    prob = sc.trot_problem(itf, batch=32, n_intervals=40, gait_start=0.0)
    _, x, u, _, st = bp.BatchedSqpMpc(itf, max_batch=32, max_nodes=56).run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    xd, ud, nd = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "u.npy"), np.load(tmp_path / "a" / "stats_n_nodes.npy")
    assert xd.shape == x.shape and np.array_equal(nd, [s.n_nodes for s in st])
    for k in range(32):
        n = st[k].n_nodes
        assert rel_x(xd[k, :n + 1], x[k, :n + 1]) < 1e-12 and rel_u(ud[k, :n], u[k, :n]) < 1e-12 and not xd[k, n + 1:].any()


@pytest.mark.parametrize("feedback", [True, False])
def test_receding_horizon_loop_matches_oracle(ctx, feedback, tmp_path):
    """the MPC loop (BipedalController.cpp:332-350) with warm starts shifted on the device
    (bpmpc_solver_setup_from_previous) against the oracle's restatement of SqpSolver::initializeStateInputTrajectories
    (oracle/reference_py.py warm_start_from_previous).  The tick period (0.02 s) is not a multiple of dt (0.015 s) and the
    horizon contains gait events, so inputs, gains and states are all interpolated.  feedback False: a task.info with
    sqp.useFeedbackPolicy false - the previous solution is evaluated as a FeedforwardController."""
    import numpy as np
    from oracle import reference_py as rp
    bp, sc, ob, itf = ctx
    if not feedback:
        text = open(sc.H1["task"]).read()
        assert text.index("useFeedbackPolicy true") > text.index("\nsqp")
        task = tmp_path / "task_feedforward.info"
        task.write_text(text.replace("useFeedbackPolicy true", "useFeedbackPolicy false", 1))     # the sqp block is the first with this key
        itf = bp.BipedalRobotInterface(str(task), sc.H1["urdf"], sc.H1["reference"])
        itf.gaitFile = sc.H1["gait"]
        assert itf.sqpSettings()["useFeedbackPolicy"] is False
    B, NI, tick = 3, 40, 0.02
    horizon = NI * sc.DT
    x_meas = sc.perturbed_initial_states(itf, B)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=64, return_gains=True)
    m, om = ob.model("h1"), ob.oracle("h1")
    sq = m["sqp"]
    prev = [None] * B
    worst = 0.0
    for it in range(4):
        t0 = it * tick
        sched = sc.gait_schedule(itf, "trot", t0, horizon)
        targets = [itf.cmdVelToTargetTrajectories((0.3, 0.0, 0.0, 0.1), t0, x_meas[b], horizon) for b in range(B)]
        prob = dict(t0=t0, x0=x_meas, schedule=sched, targets=targets, horizon=horizon)
        if it == 0:
            t, x, u, K, stats = mpc.run(t0, x_meas, sched, targets, horizon=horizon, gains=True)
        else:
            t, x, u, K, stats = mpc.advance(t0, x_meas, sched, targets, horizon=horizon, gains=True)
        nxt = np.zeros_like(x_meas)
        for b in range(B):
            nodes = ob.oracle_nodes(prob, b)
            if prev[b] is None:
                xi, ui = rp.cold_start(m, nodes, x_meas[b])
            else:
                xi, ui = rp.warm_start_from_previous(m, nodes, x_meas[b], *prev[b], feedback=feedback)
            xo, uo, Ko, st = om.solve(nodes, x_meas[b], xi, ui, iterations=1, g_max=sq["g_max"], g_min=sq["g_min"], delta_tol=sq["deltaTol"])
            n = stats[b].n_nodes
            assert n == nodes["N"]
            ex = np.max(np.abs(x[b, :n + 1] - xo)) / max(1.0, np.max(np.abs(xo)))
            eu = np.max(np.abs(u[b, :n] - uo)) / max(1.0, np.max(np.abs(uo)))
            worst = max(worst, ex, eu)
            assert ex < 1e-8 and eu < 1e-8, (it, b, ex, eu)
            prev[b] = (nodes, xo, uo, Ko)
            # "measurement" of the next tick: the planned state at t0 + tick plus a small deterministic disturbance
            j, a = rp.time_segment(nodes["times"], t0 + tick)
            nxt[b] = a * xo[j] + (1.0 - a) * xo[j + 1] + 1e-3 * np.sin(np.arange(xo.shape[1]) + b + it)
        x_meas = nxt
    assert worst < 1e-8


def test_backtracking_rounds_on_device_match_oracle(ctx):
    """Several back-tracking rounds of the filter line search (alpha = 1/2, 1/4, ...): after the first trial they run inside k_ls_tail,
    one workgroup per problem, without the host.  A converged iterate re-used as the warm start for a far-away measured state makes
    the full step unacceptable; step sizes, merit and the accepted iterate must equal the oracle's."""
    bp, sc, ob, itf = ctx
    B = 6
    prob = sc.trot_problem(itf, batch=B, n_intervals=40)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=64)
    t, x, u, _, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    n = st[0].n_nodes
    seen = set()
    for d in (0.5, 1.0):
        x0b = prob["x0"] + d * np.sin(np.arange(prob["x0"].size).reshape(prob["x0"].shape))
        t2, x2, u2, _, st2 = mpc.run(prob["t0"], x0b, prob["schedule"], prob["targets"], horizon=prob["horizon"], warm_x=x, warm_u=u)
        p2 = dict(prob, x0=x0b)
        for b in range(B):
            xo, uo, _, sto = ob.oracle_solve_like(p2, b, x_init=x[b, :n + 1], u_init=u[b, :n])
            assert st2[b].step_size == sto[0][3], (d, b, st2[b].step_size, sto[0][3])
            assert rel_x(x2[b, :n + 1], xo) < 1e-11 and rel_u(u2[b, :n], uo) < 1e-11
            seen.add(st2[b].step_size)
    assert min(seen) <= 0.25 and len(seen) >= 2, seen      # the device-side rounds were really exercised


def test_profile_levels(ctx):
    """settings.profile: 0 nothing is timed, 1 every kernel class, 2 the linearisation kernel only; switchable on a live solver."""
    bp, sc, ob, itf = ctx
    prob = sc.trot_problem(itf, batch=4, n_intervals=20)
    mpc = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=32, profile=2)
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    mpc.enqueue(); mpc.synchronize()
    assert mpc.kernel_time("linearize")[1] == 1 and mpc.kernel_time("riccati")[1] == 0
    mpc.set_profile(1)
    mpc.reset(); mpc.enqueue(); mpc.synchronize()
    t_lin, n_lin = mpc.kernel_time("linearize")
    t_ric, n_ric = mpc.kernel_time("riccati")
    assert n_lin == 1 and n_ric == 1 and 0.0 < t_lin < 50.0 and 0.0 < t_ric < 50.0
    mpc.set_profile(0)
    mpc.reset(); mpc.enqueue(); mpc.synchronize()
    assert mpc.kernel_time("linearize")[1] == 0
    with pytest.raises(bp.BpmpcError):
        mpc.set_profile(7)


def test_long_target_trajectories_are_cropped_exactly(ctx):
    """The ROS reference manager hands its TargetTrajectories over verbatim (integration/HipSqpSolver.h); one with more than the
    device's 8 points used to be a runtime error that stopped the controller.  Only the points the piecewise-linear
    interpolation can touch inside [t0, t0 + horizon] are kept - same reference bits - and a rejected setup leaves the handle usable."""
    bp, sc, ob, itf = ctx
    nx = itf.stateDim
    horizon, t0 = 30 * sc.DT, 0.2
    x0 = sc.perturbed_initial_states(itf, 2)
    sched = sc.gait_schedule(itf, "trot", t0, horizon)
    rng = np.random.default_rng(5)
    times = np.concatenate([np.linspace(-3.0, 0.1, 9), [0.31, 0.47], np.linspace(0.7, 6.0, 11)])       # 22 points, 2 strictly inside the window
    base = itf.cmdVelToTargetTrajectories((0.3, 0.0, 0.0, 0.1), t0, x0[0], horizon).stateTrajectory[0]
    states = base[None, :] + 0.02 * rng.standard_normal((len(times), nx))
    tt = bp.TargetTrajectories(times, states)
    prob = dict(t0=t0, x0=x0, schedule=sched, targets=[tt, tt], horizon=horizon)
    mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=48)
    t, x, u, _, st = mpc.run(t0, x0, sched, [tt, tt], horizon=horizon)
    n = st[0].n_nodes
    xref = mpc.read("xref").reshape(2, 48, nx)[:, :n].copy()
    # the same bits as handing over just the four points that matter (last before the window, two inside, first behind it) ...
    keep = slice(8, 12)
    assert times[8] < t0 <= times[9] and times[10] < t0 + horizon <= times[11]
    four = bp.TargetTrajectories(times[keep], states[keep])
    t4, x4, u4, _, _ = mpc.run(t0, x0, sched, [four, four], horizon=horizon)
    assert np.array_equal(mpc.read("xref").reshape(2, 48, nx)[:, :n], xref) and np.array_equal(x4, x) and np.array_equal(u4, u)
    t, x, u, _, st = mpc.run(t0, x0, sched, [tt, tt], horizon=horizon)
    for b in range(2):
        nodes = ob.oracle_nodes(prob, b)                                # ... and what the oracle interpolates from the full 22-point trajectory
        assert np.abs(xref[b] - np.asarray(nodes["xref"])[:n]).max() < 1e-14
        xo, uo, _, _ = ob.oracle_solve_like(prob, b)
        assert rel_x(x[b, :n + 1], xo) < 1e-11 and rel_u(u[b, :n], uo) < 1e-11
    # more than 8 points inside the window: a clear error, and the handle keeps its previous setup (node times included)
    dense = bp.TargetTrajectories(np.linspace(t0, t0 + horizon, 12), base[None, :] + np.zeros((12, 1)))
    with pytest.raises(bp.BpmpcError) as e:
        mpc.setup(t0 + 0.1, x0, sc.gait_schedule(itf, "trot", t0 + 0.1, horizon), [dense, dense], horizon=horizon)
    assert "inside the horizon" in str(e.value)
    t2, x2, u2, _, st2 = mpc.fetch()
    assert np.array_equal(t2, t) and np.array_equal(x2, x) and np.array_equal(u2, u)


def test_constraint_values_at_the_solution_match_oracle(ctx):
    """bpmpc_solver_constraint_values (solution metrics for solver observers, BipedalRobotSqpMpcNode.cpp:74-86): the active equality rows of
    every intermediate node at the accepted iterate against the oracle's constraint evaluation there; rows / modes bookkeeping; event nodes."""
    bp, sc, ob, itf = ctx
    prob = sc.trot_problem(itf, batch=2, n_intervals=40, gait="flying_trot")
    mpc = bp.BatchedSqpMpc(itf, max_batch=2, max_nodes=56)
    t, x, u, _, st = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    v, rows, modes = mpc.constraint_values()
    om = ob.h1_oracle()
    n = st[0].n_nodes
    seen = set()
    for b in range(2):
        nodes = ob.oracle_nodes(prob, b)
        for k in range(n):
            if nodes["kind"][k] != 0:
                assert rows[b, k] == 0 and modes[b, k] == -1
                continue
            lq = om.node_lq(0, nodes["dt"][k], x[b, k], u[b, k], x[b, k + 1], nodes["xref"][k], nodes["mode"][k], nodes["zref"][k], nodes["zdref"][k])
            assert rows[b, k] == lq["nc"] and modes[b, k] == nodes["mode"][k]
            assert np.abs(v[b, k, :lq["nc"]] - np.asarray(lq["e"])[:lq["nc"]]).max() < 1e-10
            seen.add(int(modes[b, k]))
    assert seen >= {0, 1, 2} and np.all(rows[:, n:] == 0)


def test_setups_of_different_shape_on_one_handle_match_a_fresh_handle(ctx):
    """What a launch reads of the handle is put together once per setup.  A handle that has solved a larger batch on a shorter, event-free grid
    from a cold start, then takes a setup with another batch, another longest grid, a gait event inside the horizon and the caller's warm-start
    arrays, then a receding-horizon step - and computes bit for bit what a handle that has only seen the last two does."""
    bp, sc, ob, itf = ctx
    N = 48

    def targets(t0, x0, horizon):
        return [itf.cmdVelToTargetTrajectories((0.3, 0.0, 0.0, 0.1), t0, x, horizon) for x in x0]

    def second_and_third(mpc):
        out = []
        x0 = sc.perturbed_initial_states(itf, 2)
        step = bp.ModeSchedule(np.array([0.3, 0.9]), np.array([3, 1, 3], np.int32))      # stance, one lift-off inside the horizon, touch-down behind it
        warm_x, warm_u = np.repeat(x0[:, None, :], N + 1, axis=1), np.zeros((2, N, itf.inputDim))
        warm_u[:, :, [2, 5, 8, 11]] = 9.81 * itf.robotMass() / 4.0
        lay = mpc.setup(0.0, x0, step, targets(0.0, x0, 0.6), horizon=0.6, warm_x=warm_x, warm_u=warm_u)
        assert lay["batch"] == 2 and lay["n_grids"] == 1 and 40 < lay["n_nodes_max"] <= N
        mpc.enqueue()
        out.append(mpc.fetch())
        x1 = x0 + 1e-3 * np.sin(np.arange(x0.size)).reshape(x0.shape)
        mpc.setup_from_previous(0.015, x1, step, targets(0.015, x1, 0.6), horizon=0.6)
        mpc.enqueue()
        out.append(mpc.fetch())
        return out

    P = bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=N, sqp_iterations=2)
    prob = sc.trot_problem(itf, batch=4, n_intervals=20, gait="stance")
    lay = P.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"])
    assert lay["batch"] == 4 and lay["n_nodes_max"] == 20
    P.enqueue()
    P.fetch()
    got = second_and_third(P)
    want = second_and_third(bp.BatchedSqpMpc(itf, max_batch=4, max_nodes=N, sqp_iterations=2))
    for (_, x, u, _, st), (_, xf, uf, _, stf) in zip(got, want):
        assert np.isfinite(x).all() and np.isfinite(u).all() and np.abs(u).max() > 0
        assert np.array_equal(x, xf) and np.array_equal(u, uf)
        assert [(s.iterations, s.status) for s in st] == [(s.iterations, s.status) for s in stf]
