"""The value-only kernels (line-search trials, constraint values, DDP roll-out costs) sum the cost gradient over the non-zero lists of Q and R
(csrc/weight_structure.h) and the change of variables takes a diagonal Q as its diagonal; the dense paths stay behind BPMPC_DENSE_WEIGHTS=1.  A skipped term is a product with an exact zero and the remaining terms keep their order, so every output must
be the SAME BITS on both paths: each case runs the default and the dense handle on the same problem and compares with np.array_equal.  The cases with
changed weights (an off-diagonal pair in Q; a row of nine non-zeros in R, which must select the dense path unasked) are also held against the oracle
at the parity tests' 1e-11."""
import os
import shutil

import numpy as np
import pytest

import bipedal_control_amd as bp
from bipedal_control_amd import scenarios
from tests.tolerances import rel_u, rel_x

pytestmark = pytest.mark.gpu

LQ = ("Q", "R", "q", "r", "c", "b", "perf", "qrd")                # what the lineariser leaves (the materialised mode: all of it)
PROJECTED = ("Wt", "Qp", "Mt")                                    # what the change of variables leaves


def _stats(stats):
    """every field of the solver's statistics, n_nodes first"""
    return [(s.n_nodes,) + tuple(getattr(s, name) for name, _ in type(s)._fields_) for s in stats]


def _sqp_outputs(itf, prob, monkeypatch, dense, max_nodes, materialize, iterations=2):
    """One handle, created with BPMPC_DENSE_WEIGHTS as asked: the solve, then the LQ model and the projected model at the solution"""
    monkeypatch.setenv("BPMPC_DENSE_WEIGHTS", "1" if dense else "0")
    B = prob["x0"].shape[0]
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=max_nodes, sqp_iterations=iterations, return_gains=True, materialize_lq=materialize)
    t, x, u, K, stats = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
    mpc.stage("linearize"); mpc.stage("project"); mpc.synchronize()
    out = dict(x=x, u=u, K=K, stats=_stats(stats), compact=int(mpc.read("weights_compact")[0]))
    out.update({k: mpc.read(k) for k in LQ + PROJECTED + ("g_kind", "g_mode")})
    return out


def _assert_same_bits(a, b, names):
    assert a["stats"] == b["stats"]
    for k in names:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("materialize", [True, False])
def test_h1_trot_through_a_mode_switch_and_an_event_node(monkeypatch, materialize):
    """(a) H1 trot, batch 4, 24 intervals, the gait template tiled from t = 0, two SQP iterations, both formulations"""
    itf = scenarios.h1_interface()
    prob = scenarios.trot_problem(itf, batch=4, n_intervals=24, gait_start=0.0)
    got = {dense: _sqp_outputs(itf, prob, monkeypatch, dense, 40, materialize) for dense in (False, True)}
    assert (got[False]["compact"], got[True]["compact"]) == (1, 0)
    n = got[False]["stats"][0][0]
    kind, mode = got[False]["g_kind"][:n].astype(int), got[False]["g_mode"][:n].astype(int)
    assert (kind == 1).any() and len(set(mode[kind == 0] & 3)) >= 2, "the horizon holds an event node and a mode switch"
    _assert_same_bits(got[False], got[True], ("x", "u", "K") + LQ + PROJECTED)
    nx = itf.stateDim
    q = got[False]["q"].reshape(4, 40, nx)[:, :n][:, kind == 0]
    assert np.abs(q).max() > 0.0
    if materialize:                                               # the materialised Q of this model is diagonal: exact zeros elsewhere, something on the diagonal
        Q = got[False]["Q"].reshape(4, 40, nx, nx)[:, :n][:, kind == 0]
        off = Q.copy(); off[..., np.arange(nx), np.arange(nx)] = 0.0
        assert not off.any() and (Q[..., np.arange(nx), np.arange(nx)] > 0.0).all()


def test_g1_packed_lanes(monkeypatch):
    """(b) nx = 24: the packed lane layout (lanes 0..2 also own the base translations), six terms per row of R"""
    itf = scenarios.interface("g1")
    prob = scenarios.trot_problem(itf, batch=2, n_intervals=24, gait="standing_trot", gait_start=0.0)
    got = {dense: _sqp_outputs(itf, prob, monkeypatch, dense, 40, True) for dense in (False, True)}
    assert (got[False]["compact"], got[True]["compact"]) == (1, 0)
    _assert_same_bits(got[False], got[True], ("x", "u", "K") + LQ + PROJECTED)


def test_ddp_on_h1(monkeypatch):
    """(c) the DDP solver: the costs of its roll-outs run the value-only sums, its backward pass the change of variables"""
    itf = scenarios.h1_interface()
    prob = scenarios.trot_problem(itf, batch=2, n_intervals=24, gait_start=0.0)
    got = {}
    for dense in (False, True):
        monkeypatch.setenv("BPMPC_DENSE_WEIGHTS", "1" if dense else "0")
        mpc = bp.BatchedDdpMpc(itf, 2, 48, materialize_lq=True)
        t, x, u, K, stats = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], gains=True)
        got[dense] = dict(t=t, x=x, u=u, K=K, stats=_stats(stats), compact=int(mpc.read("weights_compact")[0]))
        got[dense].update({k: mpc.read(k) for k in ("Q", "R", "q", "r", "qrd", "ddp_lff", "ddp_update_is")})
    assert (got[False]["compact"], got[True]["compact"]) == (1, 0)
    assert np.abs(got[False]["q"]).max() > 0.0
    _assert_same_bits(got[False], got[True], ("t", "x", "u", "K", "Q", "R", "q", "r", "qrd", "ddp_lff", "ddp_update_is"))


# ---- changed weights: a temporary copy of the H1 asset files

def _h1_copy(tmp_path, edit):
    """edit: (unique line of task.info, lines inserted behind it)"""
    paths = {}
    for key in ("task", "urdf", "reference", "gait"):
        paths[key] = str(tmp_path / os.path.basename(scenarios.H1[key]))
        shutil.copy(scenarios.H1[key], paths[key])
    text = open(paths["task"]).read()
    anchor, extra = edit
    assert text.count(anchor) == 1
    open(paths["task"], "w").write(text.replace(anchor, anchor + extra))
    return paths


def _oracle_solution(paths, prob, b, iterations):
    """tests/oracle_bridge.oracle_solve_like on the model of the copied files"""
    from oracle import ingest, oracle_py, reference_py as rp
    m = _oracle_solution.models.get(paths["task"])
    if m is None:
        model = ingest.build_model(paths["urdf"], paths["task"], paths["reference"])
        m = _oracle_solution.models[paths["task"]] = (model, oracle_py.OracleModel(ingest.model_blob(model)))
    model, om = m
    sched = prob["schedule"]
    ev, ms = list(map(float, sched.eventTimes)), list(map(int, sched.modeSequence))
    planner = rp.SwingTrajectoryPlanner(model["swing"])
    planner.update(ev, ms)
    tt = prob["targets"][b]
    nodes = rp.node_arrays(model, 0.0, prob["horizon"], 0.015, ev, ms, np.asarray(tt.timeTrajectory), np.asarray(tt.stateTrajectory), planner)
    x0 = prob["x0"][b]
    x_init, u_init = rp.cold_start(model, nodes, x0)
    s = model["sqp"]
    xo, uo, _, _ = om.solve(nodes, x0, x_init, u_init, iterations=iterations, g_max=s["g_max"], g_min=s["g_min"], delta_tol=s["deltaTol"])
    return model, xo, uo


_oracle_solution.models = {}


def _changed_weights_case(tmp_path, monkeypatch, edit, expect_compact, pattern):
    paths = _h1_copy(tmp_path, edit)
    itf = bp.BipedalRobotInterface(paths["task"], paths["urdf"], paths["reference"])
    itf.gaitFile = paths["gait"]
    prob = scenarios.trot_problem(itf, batch=2, n_intervals=24, gait_start=0.0)
    got = {dense: _sqp_outputs(itf, prob, monkeypatch, dense, 40, True, iterations=1) for dense in (False, True)}
    assert (got[False]["compact"], got[True]["compact"]) == (expect_compact, 0)
    _assert_same_bits(got[False], got[True], ("x", "u", "K") + LQ + PROJECTED)
    for b in range(2):
        model, xo, uo = _oracle_solution(paths, prob, b, 1)
        pattern(np.asarray(model["Q"]), np.asarray(model["R"]))
        n = got[False]["stats"][b][0]
        assert rel_x(got[False]["x"][b, :n + 1], xo) < 1e-11 and rel_u(got[False]["u"][b, :n], uo) < 1e-11


def test_off_diagonal_pair_in_Q(tmp_path, monkeypatch):
    """(d) Q with one symmetric off-diagonal pair (two terms per row at most), R as it is: the lists with q_diagonal false"""
    def pattern(Q, R):
        assert Q[12, 13] == 50.0 and Q[13, 12] == 50.0 and max(np.count_nonzero(Q, axis=1)) == 2 and max(np.count_nonzero(R, axis=1)) <= 8
    _changed_weights_case(tmp_path, monkeypatch, ("  (12,12) 800.0\n", "  (12,13) 50.0\n  (13,12) 50.0\n"), 1, pattern)


def test_row_of_nine_in_R_runs_dense_unasked(tmp_path, monkeypatch):
    """(e) a force row of R with nine non-zeros: no compact form, the handle says so and the dense path matches the oracle"""
    extra = "".join("  (0,%d) 0.5\n  (%d,0) 0.5\n" % (k, k) for k in range(1, 9))
    def pattern(Q, R):
        assert np.count_nonzero(R[0]) == 9 and max(np.count_nonzero(R, axis=1)) == 9
    _changed_weights_case(tmp_path, monkeypatch, ("  (0,0) 5.0\n", extra), 0, pattern)
