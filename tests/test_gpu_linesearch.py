"""GPU tier: every decision of the filter line search on the device against the oracle (cases: tests/linesearch_cases.py; what they rest on is asserted on
the CPU by tests/test_linesearch_cases.py - in particular that no decision of the oracle lies within 1e-6 of its threshold, so status, iteration count and
step size are compared for equality).

  branches      the three acceptance branches, up to 14 trials, a search that gives up, under three settings, two distances, 1 and 3 iterations
  launch        BPMPC_LS_WIDE_ROUNDS 1 .. 20 (which launch judges which round) against the default of 2: bit for bit
  stagger       problems of one batch that stop iterating at different SQP iterations
  horizons      121 and 290 nodes (the update's remainder loop, more nodes than summing lanes), 1 .. 3 intervals (fewer nodes than nx)
  nx = 24       G1 and OpenLoong
  reference     the host-driven round loop of the reference kernels against the fast path
  settings      sqp.gamma_c / alpha_decay / alpha_min / armijoFactor from task.info, among them the filter that rejects everything

Tolerances: merit, both SSEs and the descent 1e-9 relative; x, u per physical block (tests/tolerances.py) at the figures of the cold-start solve tests
(1e-11; OpenLoong 1e-9), unless the reference's own floor (the oracle against itself with the warm iterate moved by 1e-15 relative) lies above a hundredth of
that - then 100 x the floor (linesearch_cases.tolerance; G1 and OpenLoong).  Floors and achieved errors are written beside those of
test_gpu_parity.py (its _write_report) under the keys linesearch_*; committed copy of the measured run: profiles/linesearch_cases.json."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import linesearch_cases as lc  # noqa: E402
from tests.test_gpu_parity import _write_report  # noqa: E402
from tests.tolerances import rel_u, rel_x  # noqa: E402

FIELDS = ("n_nodes", "iterations", "status", "merit_before", "dynamics_sse_before", "equality_sse_before", "merit_after", "dynamics_sse_after",
          "equality_sse_after", "step_size", "armijo_descent", "dx_norm", "du_norm")


def _records(stats, B):
    return [tuple(getattr(stats[b], f) for f in FIELDS) for b in range(B)]


def _solve(name, tmp_path, iterations=None, only=None, **handle):
    """The case on the device: (x, u, K, stats records).  only = b: problem b in a batch of its own."""
    import bipedal_control_amd as bp
    c, prob, _ = lc.case_inputs(name)
    wx, wu = lc.padded_warm(name)
    if only is not None:
        prob, wx, wu = dict(prob, x0=prob["x0"][only:only + 1], targets=[prob["targets"][only]]), wx[only:only + 1], wu[only:only + 1]
    B = prob["x0"].shape[0]
    itf = lc.interface(c["robot"], lc.SETTINGS[c["settings"]], tmp_path)
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=c["max_nodes"], sqp_iterations=iterations or c["iterations"], return_gains=True, **handle)
    t, x, u, K, stats = mpc.run(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], warm_x=wx, warm_u=wu, gains=True)
    return np.array(x), np.array(u), np.array(K), _records(stats, B)


def _relative(a, b):
    return abs(a - b) / abs(b) if b != 0.0 else abs(a)


def _compare_with_oracle(name, x, u, records, record_figures=True, key=None):
    """Status, iteration count and step size equal; merit, SSEs and descent 1e-9 relative; x, u at the case's tolerance.  Returns the report."""
    (tx, tu), floor = lc.tolerance(name)
    report, figures, before, missed = {}, 0.0, 0.0, []
    for b, (xo, uo, _, rec) in enumerate(lc.oracle_solves(name)):
        rows = lc.ran(rec)
        last = rows[-1]
        r = dict(zip(FIELDS, records[b]))
        n = r["n_nodes"]
        assert n == xo.shape[0] - 1
        assert r["iterations"] == len(rows), (b, r["iterations"], len(rows))
        assert r["status"] == (0 if last[3] > 0.0 else 1), (b, r["status"], last[3])
        assert r["step_size"] == last[3], (b, r["step_size"], last[3])
        if record_figures:
            for got, ref in ((r["merit_after"], last[4]), (r["dynamics_sse_after"], last[5]), (r["equality_sse_after"], last[6]), (r["armijo_descent"], last[7])):
                figures = max(figures, _relative(got, ref))
            # the figures of the linearisation, which the warm start decides: the cold-start solution satisfies the equality constraints of a short
            # horizon to rounding (SSE 1e-33, the square of residuals of 1e-17), and a relative error of rounding is no figure - an SSE counts from
            # 1e-24 on, the square of a residual of a thousand roundings
            for got, ref in ((r["merit_before"], last[0]), (r["dynamics_sse_before"], last[1]), (r["equality_sse_before"], last[2])):
                before = max(before, abs(got - ref) / max(abs(ref), 1e-15))
        ex, eu = rel_x(x[b, :n + 1], xo, report), rel_u(u[b, :n], uo, report)
        if not (ex < tx and eu < tu):
            missed.append((b, ex, eu))
    report = dict(report, figures=float(figures), figures_before=float(before), reference_floor_x_u=list(floor), tolerance_x_u=[tx, tu], trials=[t[-1] for t in lc.trials(name)])
    print("line search", name, report)
    _write_report("linesearch_" + (key or name), report)
    assert not missed, (missed, tx, tu)
    assert figures < 1e-9 and before < 1e-9, (figures, before)
    return report


def _give_ups_return_the_previous_iterate(name, tmp_path, x, u):
    """A search that gives up takes no step: the problem returns, bit for bit, what the same settings return with one iteration fewer (the warm start itself
    when it gives up in the first iteration)."""
    fewer = {}
    wx, wu = lc.padded_warm(name)
    for b, (_, _, _, rec) in enumerate(lc.oracle_solves(name)):
        rows = lc.ran(rec)
        if rows[-1][3] != 0.0:
            continue
        k = len(rows)
        if k == 1:
            xp, up = wx, wu
        else:
            if k - 1 not in fewer:
                fewer[k - 1] = _solve(name, tmp_path, iterations=k - 1)
            xp, up = fewer[k - 1][0], fewer[k - 1][1]
        n = lc.oracle_solves(name)[b][0].shape[0] - 1
        assert np.array_equal(x[b, :n + 1], xp[b, :n + 1]) and np.array_equal(u[b, :n], up[b, :n]), (name, b, k)
    return len(fewer)


BRANCHES = sorted(n for n in lc.CASES if n.startswith("branches-"))
HORIZONS = sorted(n for n in lc.CASES if n.startswith(("horizon", "short")))


@pytest.mark.parametrize("name", BRANCHES)
def test_branches_match_oracle(name, tmp_path):
    """Defaults, g_max = g_min = 1e9 (every trial judged by Armijo) and g_max = 1e9 alone, measured state 0.5 and 1.0 away, one and three iterations: 2 .. 14
    trials per search, among them (Armijo, 1.0, problem 3) 8 trials, then an accepted step of 2^-12 at trial 13, then 14 rejected trials - that problem must
    return the iterate of two iterations."""
    x, u, _, records = _solve(name, tmp_path)
    _compare_with_oracle(name, x, u, records)
    reruns = _give_ups_return_the_previous_iterate(name, tmp_path, x, u)
    assert reruns == (1 if name == "branches-armijo-d1-it3" else 0)


@pytest.mark.parametrize("rounds", [1, 3, 5, 14, 20])
def test_launch_structure_does_not_change_a_bit(rounds, tmp_path, monkeypatch):
    """BPMPC_LS_WIDE_ROUNDS decides how many rounds run as launches over all nodes (judged by k_ls_decide, 256 lanes, update operands preloaded; the last of
    them by k_ls_tail) and how many inside k_ls_tail (512 lanes, update in place).  The Armijo batch at 1.0 with three iterations (up to 14 rounds) must not
    depend on it in any bit: x, u, K and the whole record.  20 > 14 trials: the cap by max_trials."""
    name = "branches-armijo-d1-it3"
    monkeypatch.setenv("BPMPC_LS_WIDE_ROUNDS", "2")
    x2, u2, K2, rec2 = _solve(name, tmp_path)
    monkeypatch.setenv("BPMPC_LS_WIDE_ROUNDS", str(rounds))
    x, u, K, rec = _solve(name, tmp_path)
    assert rec == rec2, [(a, b) for a, b in zip(rec, rec2) if a != b]
    assert max(r[FIELDS.index("iterations")] for r in rec) == 3 and min(r[FIELDS.index("step_size")] for r in rec) == 0.0
    for b, r in enumerate(rec):
        n = r[0]
        assert np.array_equal(x[b, :n + 1], x2[b, :n + 1]) and np.array_equal(u[b, :n], u2[b, :n]) and np.array_equal(K[b, :n], K2[b, :n]), (rounds, b)


def test_problems_that_stop_at_different_iterations(tmp_path):
    """deltaTol = 1: checkConvergence stops a problem as soon as its step is shorter than 1 in both norms - after 2 iterations for two problems of the batch,
    after 3 for the other four, of 5 allowed.  Counts, statuses and iterates against the oracle; and a problem that stopped early is not touched by the
    iterations the others go on with: bit for bit what it returns from a batch of its own."""
    name = "stagger"
    x, u, _, records = _solve(name, tmp_path)
    its = [r[1] for r in records]
    assert len(set(its)) >= 2 and its == [len(t) for t in lc.trials(name)], its
    _compare_with_oracle(name, x, u, records, record_figures=False)          # the SSEs of a converged iterate are rounding (1e-15 and below)
    for b in (b for b, k in enumerate(its) if k == min(its)):
        xs, us, _, rs = _solve(name, tmp_path, only=b)
        n = records[b][0]
        assert rs[0] == records[b], (b, rs[0], records[b])
        assert np.array_equal(xs[0, :n + 1], x[b, :n + 1]) and np.array_equal(us[0, :n], u[b, :n]), b


@pytest.mark.parametrize("name", HORIZONS)
def test_horizon_edges_match_oracle(name, tmp_path):
    """121 nodes (flying trot, batch 3) and 290 nodes (trot, batch 2): (n + 1) nx exceeds the 2400 preloaded entries of the update, and 290 nodes exceed the
    256 summing lanes; 3 .. 7 trials.  1, 2 and 3 intervals: fewer nodes than nx, so the lanes that are summed are chosen by the mismatch terms; the oracle
    back-tracks at every one of them (7, 7 and 8 trials under the Armijo settings at 0.5, 2 under the defaults at 1.0)."""
    x, u, _, records = _solve(name, tmp_path)
    _compare_with_oracle(name, x, u, records)


@pytest.mark.parametrize("name", ["g1", "openloong"])
def test_nx24_back_tracking_matches_oracle(name, tmp_path):
    """G1 standing trot and OpenLoong flying trot (nx = 24: the variant of k_ls_tail with the register-pressure work-arounds), Armijo settings, 0.5: up to 5
    resp. 7 trials.  OpenLoong at its own figures (1e-9); both above their reference floor (see the module's docstring)."""
    x, u, _, records = _solve(name, tmp_path)
    _compare_with_oracle(name, x, u, records)


def test_reference_kernels_take_the_same_decisions(tmp_path):
    """The host-driven round loop (one launch pair and one read-back of the `remaining` counter per round) against the fast path on the Armijo batch at 1.0,
    three iterations: statuses, iteration counts and step sizes equal, x and u to 1e-9 as in the other agreement tests of the two paths."""
    name = "branches-armijo-d1-it3"
    xf, uf, _, fast = _solve(name, tmp_path)
    xr, ur, _, ref = _solve(name, tmp_path, reference_kernels=True)
    _compare_with_oracle(name, xr, ur, ref, key=name + "-reference_kernels")
    for b, (a, r) in enumerate(zip(fast, ref)):
        n = a[0]
        assert a[:3] == r[:3] and a[FIELDS.index("step_size")] == r[FIELDS.index("step_size")], (b, a, r)
        assert rel_x(xr[b, :n + 1], xf[b, :n + 1]) < 1e-9 and rel_u(ur[b, :n], uf[b, :n]) < 1e-9


@pytest.mark.parametrize("name,trials", [("reject_all", 14), ("reject_all_9", 9), ("reject_all_9_edge", 10)])
def test_a_filter_that_rejects_everything_gives_up(name, trials, tmp_path):
    """gamma_c = 1 with g_max = g_min = -1 and deltaTol = 0: every trial is judged by `violation < 0`.  All 14 trials run (9 with alpha_decay 0.7 and
    alpha_min 0.05; 10 with alpha_min = 0.5 * 0.7^8, between the ninth and the tenth step size), every problem ends with status 1 and step 0, and x, u are
    the warm start, bit for bit.  The device reports the number of trials through the step size only: the count is the oracle's (CPU tier)."""
    assert lc.trials(name) == [[trials]] * 6
    x, u, _, records = _solve(name, tmp_path)
    _compare_with_oracle(name, x, u, records)
    wx, wu = lc.padded_warm(name)
    for b, r in enumerate(records):
        rec = dict(zip(FIELDS, r))
        n = rec["n_nodes"]
        assert rec["status"] == 1 and rec["step_size"] == 0.0 and rec["iterations"] == 1 and rec["dx_norm"] == 0.0 and rec["du_norm"] == 0.0
        assert rec["merit_after"] == rec["merit_before"] and rec["dynamics_sse_after"] == rec["dynamics_sse_before"]
        assert np.array_equal(x[b, :n + 1], wx[b, :n + 1]) and np.array_equal(u[b, :n], wu[b, :n]), b


def test_armijo_factor_from_task_info(tmp_path):
    """armijoFactor = 0.9 (upstream's default 1e-4) at 1.0: nine tenths of the predicted descent are demanded, 3 .. 12 trials (3 .. 9 at the default)."""
    x, u, _, records = _solve("armijo_0.9", tmp_path)
    _compare_with_oracle("armijo_0.9", x, u, records)
    default = lc.oracle_solves("branches-armijo-d1-it1")
    assert sum(1 for r, (_, _, _, rec) in zip(records, default) if r[FIELDS.index("step_size")] != rec[0][3]) >= 3
