"""GPU tier: the per-problem kernel family (csrc/k_weights.hip - what a handle launches once bpmpc_solver_set_weights or bpmpc_solver_set_cone_params has
set a row) at the edges the default family is held to by test_gpu_linesearch.py, test_gpu_tree_variants.py, test_gpu_parity.py and
test_gpu_weight_structure.py.  The twins restate the default kernels' mappings (csrc/node_kernels.h) and are correct only as far as they are tested
themselves.  Cases: tests/row_kernel_cases.py; what they rest on is asserted with the oracle alone by tests/test_row_kernel_cases.py.

"On the row kernels" is asserted where it is claimed, on one handle per test: under profile=True the launch counts of the classes linearize_w,
linesearch_w and project_w are positive and those of linearize, linesearch and project are zero (_on_the_row_kernels).  That is the evidence for
the family; the switch value and the robot are the evidence for the instantiation:

  k_ls_tail_w, its own trial rounds                      test_line_search_cases_on_the_row_kernels (up to 14 trials, 121 nodes = four chunks of 32 with a
                                                          remainder, nx = 24), test_*_rows_decide_in_the_tails_own_rounds (distinct rows),
                                                          BPMPC_LS_WIDE_ROUNDS = 1 (every round but the first in the tail) and 3
  k_trial_fast_w, a workgroup over >= 3 problems         short1-armijo, short3-defaults (max_nodes 8, batch 6)
  k_linearize_fast_w / k_trial_fast_w / k_ls_tail_w      BPMPC_LIN_TABLES=1 on H1 and G1 (test_table_walks_under_both_kinds_of_rows); W12 (nx = 24, two grids:
    <.., CHAIN = false>                                   the per-grid mapping), U10 (nx = 22, one grid: the compact mapping), L46 (6 .. 10 trials per
                                                          search: the table-walk tail) in test_trees_under_cone_rows
  k_project_fast_qd_w<NJ, false, true>                   BPMPC_DENSE_PROJECT=1        test_dense_project
  k_project_fast_qd_w<NJ, true, true>                    BPMPC_WT_JOINT_ROWS=1        test_joint_rows_of_wt
  k_project_fast_w<NJ, true, false>                      BPMPC_DENSE_WEIGHTS=1        test_dense_weights
  k_project_fast_w<NJ, false, true>, <NJ, true, true>    ... with one of the two above test_dense_weights
  k_linearize_fast_w, per-grid mapping, k0 > 0           pipeline_chunks 2, 3, 7      test_horizon_chunks (at 7 a chunk is 3 .. 4 nodes)
  k_linearize_fast_w, in-line lane map on one grid       BPMPC_LIN_COMPACT=0          test_inline_lane_map
NJ = 10 (H1, U10, L46) and 12 (G1, OpenLoong, W12) each.

Tolerances: the project's own for the same quantities - x, u 1e-11 and K 1e-10 per physical block (tests/tolerances.py), merit, both SSEs and the
descent 1e-9 relative, status, iteration count and step size equal; lc.tolerance(name) for the line-search cases (100 x the oracle's floor on G1 and
OpenLoong); the rule of tree_variants.FLOOR_CASES for L46 (ten times the floor of the oracle under the problem's own row).  The row kernels are not
held to the bits of the default kernels (they sum dense rows where those sum the non-zero lists); within the family, switches that only move work
between launches or skip exact zeros are.  Every maximum is printed before it is asserted and left beside those of test_gpu_parity.py (its
_write_report) under the keys rows_*; committed copy of the measured run: profiles/row_kernel_edges.json.

Measured on the MI355X (maxima over the problems of each case; every step size, status and iteration count equal, every bit comparison exact):
                                                     x         u         K         merit / SSEs / descent
  A  branches-armijo-d1-it3                          2.8e-15   7.0e-15   -         3.4e-12
     short1-armijo, short3-defaults                  5.9e-16   1.3e-15   -         2.1e-14
     horizon121-armijo                               4.8e-15   4.8e-15   -         3.8e-15
     stagger                                         5.1e-16   4.0e-15   -         -
     g1 (tolerance 2.9e-11)                          5.2e-13   5.2e-13   -         6.8e-14
     openloong (tolerance 1.1e-9)                    1.6e-11   1.5e-11   -         1.3e-11
     reject_all                                      0         0         -         1.2e-15
     branches-armijo-d1-it1 through the weight table 1.5e-15   2.8e-15   -         3.2e-15
  B  cone rows, 3 6 3 7 8 3 trials                   2.6e-15   2.7e-15   -         3.2e-15
     weight rows at d = 2.0, 4 7 3 9 3 3 trials      3.6e-15   2.6e-15   -         3.7e-15
  C1 H1 / G1 with BPMPC_LIN_TABLES=1                 3.3e-16 / 1.3e-13   9.5e-15 / 1.3e-13   7.6e-15 / 1.8e-13
     ... against the chain walks (1e-12)             2.2e-16 / 7.7e-14   5.4e-15 / 7.7e-14
  C2 W12 "mixed"                                     1.4e-14   4.0e-14   1.7e-13   3.7e-15
     U10 "walk"                                      7.8e-16   2.0e-14   2.4e-14   5.7e-16
  C3 L46 (tolerances 0.12 .. 0.15, 0.08 .. 0.13,     1.5e-2    1.3e-2    1.1e-2    1.3e-3
     0.03 .. 0.09, 1.4e-3 .. 6.8e-3: ten times the floor)
  D  H1 / G1 / two gaits, every switch and chunking  3.3e-16 / 2.1e-13 / 4.0e-16   7.6e-15 / 2.1e-13 / 2.0e-15   8.6e-15 / 2.4e-13 / 4.8e-15
     BPMPC_DENSE_PROJECT=1: Wt, Qp, Mt (1e-12)       1.1e-16 on both robots"""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's own HIP runtime sees the GPU only when it is loaded before the library's runtime initialises)

pytestmark = pytest.mark.gpu

from tests import cone_cases as cc  # noqa: E402
from tests import linesearch_cases as lc  # noqa: E402
from tests import row_kernel_cases as rk  # noqa: E402
from tests import tree_variants as tv  # noqa: E402
from tests import weight_cases as wc  # noqa: E402
from tests.test_gpu_linesearch import FIELDS, _compare_with_oracle, _records, _relative  # noqa: E402
from tests.test_gpu_parity import _structured_against_dense, _write_report  # noqa: E402
from tests.test_gpu_solver_cone_params import _against_oracle  # noqa: E402
from tests.test_gpu_tree_variants import _compare_solve  # noqa: E402
from tests.test_gpu_weight_structure import _stats  # noqa: E402
from tests.tolerances import rel_K, rel_u, rel_x  # noqa: E402

CLASSES = ("linearize", "linesearch", "project")
STAGED = ("b", "q", "r", "perf", "nc", "Vt", "Pe", "nut", "Wt", "Qp", "Mt")        # what the fused mode leaves behind stage("linearize"), stage("project")
DENSE = ("Wt", "Qp", "Mt", "nut", "g_kind", "g_mode", "Vt", "b", "g_dt")           # what _structured_against_dense reads
LQ = ("A", "B", "b", "Q", "R", "P", "q", "r", "c", "C", "D", "e", "perf", "nc")    # the materialised LQ model


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    return tmp_path_factory.mktemp("row_kernel_edges")


def _on_the_row_kernels(mpc):
    n = {c: mpc.kernel_time(c)[1] for c in CLASSES + tuple(c + "_w" for c in CLASSES)}
    assert all(n[c + "_w"] > 0 for c in CLASSES) and all(n[c] == 0 for c in CLASSES), n


def _solve(mpc, prob, cone=None, weights=None, warm=(None, None)):
    """setup / set rows / enqueue / fetch: (x, u, K, records, every field of the statistics)."""
    mpc.setup(prob["t0"], prob["x0"], prob["schedule"], prob["targets"], horizon=prob["horizon"], warm_x=warm[0], warm_u=warm[1])
    if weights is not None:
        mpc.setWeights(weights)
    if cone is not None:
        mpc.setConeParams(cone)
    mpc.enqueue()
    mpc.synchronize()
    t, x, u, K, st = mpc.fetch(gains=True)
    return dict(x=np.array(x), u=np.array(u), K=np.array(K), records=_records(st, len(st)), stats=_stats(st), raw=(t, x, u, K, st))


def _same_bits(a, b, names=("x", "u", "K")):
    assert a["stats"] == b["stats"], [(p, q) for p, q in zip(a["stats"], b["stats"]) if p != q]
    for k in names:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------- A
def _ls_solve(name, tmp_path, table="cone", only=None, **handle):
    """A case of tests/linesearch_cases.py as test_gpu_linesearch._solve runs it, on the row kernels: the model's row through the cone table (or the
    weight table) after setup."""
    import bipedal_control_amd as bp
    c, prob, _ = lc.case_inputs(name)
    wx, wu = lc.padded_warm(name)
    if only is not None:
        prob, wx, wu = dict(prob, x0=prob["x0"][only:only + 1], targets=[prob["targets"][only]]), wx[only:only + 1], wu[only:only + 1]
    itf = lc.interface(c["robot"], lc.SETTINGS[c["settings"]], tmp_path)
    mpc = bp.BatchedSqpMpc(itf, max_batch=prob["x0"].shape[0], max_nodes=c["max_nodes"], sqp_iterations=c["iterations"], return_gains=True, **handle)
    rows = dict(cone=cc.start_row(c["robot"])) if table == "cone" else dict(weights=bp.MpcWeights.from_model(itf).row)
    out = _solve(mpc, prob, warm=(wx, wu), **rows)
    if handle.get("profile"):
        _on_the_row_kernels(mpc)
    return out


@pytest.mark.parametrize("name", rk.LS_CASES)
def test_line_search_cases_on_the_row_kernels(name, tmp_path):
    """A: the default family's line-search cases with the model's row in the cone table, against the oracle exactly as test_gpu_linesearch.py compares
    them.  stagger: an early stopper returns the bits of a batch of its own; reject_all: the warm start comes back bit for bit."""
    got = _ls_solve(name, tmp_path, profile=True)
    report = _compare_with_oracle(name, got["x"], got["u"], got["records"], record_figures=name != "stagger", key="rows_" + name)
    _write_report("rows_ls_" + name, report)
    if name == "stagger":
        its = [r[1] for r in got["records"]]
        assert len(set(its)) >= 2 and its == [len(t) for t in lc.trials(name)], its
        for b in (b for b, k in enumerate(its) if k == min(its)):
            alone = _ls_solve(name, tmp_path, only=b)
            n = got["records"][b][0]
            assert alone["records"][0] == got["records"][b], (b, alone["records"][0], got["records"][b])
            assert np.array_equal(alone["x"][0, :n + 1], got["x"][b, :n + 1]) and np.array_equal(alone["u"][0, :n], got["u"][b, :n]), b
    if name == "reject_all":
        wx, wu = lc.padded_warm(name)
        for b, r in enumerate(got["records"]):
            rec = dict(zip(FIELDS, r))
            n = rec["n_nodes"]
            assert rec["status"] == 1 and rec["step_size"] == 0.0 and rec["iterations"] == 1 and rec["merit_after"] == rec["merit_before"]
            assert np.array_equal(got["x"][b, :n + 1], wx[b, :n + 1]) and np.array_equal(got["u"][b, :n], wu[b, :n]), b


def test_either_table_switches_to_one_family(tmp_path):
    """A: rk.FAMILY_CASE with the model's row set through the weight table instead: both tables then hold the model's rows and the family is one, so
    the result has the bits of the cone-switched run."""
    by_cone = _ls_solve(rk.FAMILY_CASE, tmp_path, profile=True)
    by_weights = _ls_solve(rk.FAMILY_CASE, tmp_path, table="weights", profile=True)
    _same_bits(by_cone, by_weights)
    report = _compare_with_oracle(rk.FAMILY_CASE, by_weights["x"], by_weights["u"], by_weights["records"], key="rows_weight_table_" + rk.FAMILY_CASE)
    _write_report("rows_ls_weight_table_" + rk.FAMILY_CASE, report)


_WIDE_TWO = {}


def _wide_rounds(name, rounds, tmp_path, monkeypatch, solve):
    """BPMPC_LS_WIDE_ROUNDS is read when the handle is created; the run at the default of 2 once per case."""
    if rounds == 2 and name in _WIDE_TWO:
        return _WIDE_TWO[name]
    monkeypatch.setenv("BPMPC_LS_WIDE_ROUNDS", str(rounds))
    out = solve()
    if rounds == 2:
        _WIDE_TWO[name] = out
    return out


@pytest.mark.parametrize("rounds", rk.WIDE_ROUNDS)
def test_launch_structure_does_not_change_a_bit_on_the_row_kernels(rounds, tmp_path, monkeypatch):
    """A: BPMPC_LS_WIDE_ROUNDS = 1 and 3 against 2 on rk.WIDE_ROUNDS_CASE (up to 14 trials, three iterations, a give-up): x, u, K and the whole
    statistics record bit for bit, as test_gpu_linesearch.py::test_launch_structure_does_not_change_a_bit holds the default family."""
    name = rk.WIDE_ROUNDS_CASE
    two = _wide_rounds(name, 2, tmp_path, monkeypatch, lambda: _ls_solve(name, tmp_path))
    got = _wide_rounds(name, rounds, tmp_path, monkeypatch, lambda: _ls_solve(name, tmp_path, profile=True))
    assert max(r[FIELDS.index("iterations")] for r in got["records"]) == 3 and min(r[FIELDS.index("step_size")] for r in got["records"]) == 0.0
    _same_bits(two, got)


# ---------------------------------------------------------------------------------------------------- B
def _compare_tail(key, got, oracle, tolerance):
    """Status, iteration count and step size equal; merit_after, both SSEs and the descent 1e-9 relative; x, u at `tolerance`."""
    tx, tu = tolerance
    report, figures, missed = {}, 0.0, []
    for b, (xo, uo, _, rec) in enumerate(oracle):
        (last,) = lc.ran(rec)
        r = dict(zip(FIELDS, got["records"][b]))
        n = r["n_nodes"]
        assert n == xo.shape[0] - 1
        assert (r["iterations"], r["status"], r["step_size"]) == (1, 0 if last[3] > 0.0 else 1, last[3]), (b, r["iterations"], r["status"], r["step_size"], last[3])
        for dev, ref in ((r["merit_after"], last[4]), (r["dynamics_sse_after"], last[5]), (r["equality_sse_after"], last[6]), (r["armijo_descent"], last[7])):
            figures = max(figures, _relative(dev, ref))
        ex, eu = rel_x(got["x"][b, :n + 1], xo, report), rel_u(got["u"][b, :n], uo, report)
        if not (ex < tx and eu < tu):
            missed.append((b, ex, eu))
    report = dict(report, figures=float(figures), tolerance_x_u=[tx, tu], trials=[t[0] for t in rk.trials_of(oracle)], steps=[float(lc.ran(o[3])[0][3]) for o in oracle])
    print(key, report)
    _write_report(key, report)
    assert not missed, (missed, tx, tu)
    assert figures < 1e-9, figures
    return report


def _tail_handle(tmp_path, **handle):
    import bipedal_control_amd as bp
    c = lc.CASES[rk.TAIL_CASE]
    itf = lc.interface(c["robot"], lc.SETTINGS[c["settings"]], tmp_path)
    return bp, itf, bp.BatchedSqpMpc(itf, max_batch=c["batch"], max_nodes=c["max_nodes"], sqp_iterations=1, return_gains=True, **handle)


def test_cone_rows_decide_in_the_tails_own_rounds(tmp_path, monkeypatch):
    """B: the inputs of rk.TAIL_CASE, a cone row per problem (rk.TAIL_CONE_ROWS), one iteration: every search takes 3 .. 8 trials, so from the third on
    the trial is evaluated by k_ls_tail_w under the row it overlays on the model block.  The CPU tier shows that each non-model row changes the
    accepted step or the merit after it by more than 1e-6, so a tail that read the model's row or a neighbour's cannot pass.  Once more at
    BPMPC_LS_WIDE_ROUNDS=1 (the tail evaluates from the second trial on): the same bits."""
    _, prob, _ = rk.tail_inputs(rk.TAIL_CONE_D)
    rows = np.stack([cc.row("h1", r) for r in rk.TAIL_CONE_ROWS])
    warm = rk.padded_tail_warm(rk.TAIL_CONE_D)

    def solve():
        _, _, mpc = _tail_handle(tmp_path, profile=True)
        out = _solve(mpc, prob, cone=rows, warm=warm)
        _on_the_row_kernels(mpc)
        return out
    got = _wide_rounds("tail_cone", 2, tmp_path, monkeypatch, solve)
    _compare_tail("rows_tail_cone", got, rk.tail_cone_solves(True), lc.tolerance(rk.TAIL_CASE)[0])
    _same_bits(got, _wide_rounds("tail_cone", 1, tmp_path, monkeypatch, solve))


def test_weight_rows_decide_in_the_tails_own_rounds(tmp_path, directory):
    """B: the same with a weight row per problem (rk.TAIL_WEIGHTS cycled), the measured state rk.TAIL_WEIGHT_D away: the tail's lane groups sum over
    the row of the workgroup's problem, whose pointer the tail forms from an opaque scalar."""
    bp, itf, mpc = _tail_handle(tmp_path, profile=True)
    files = rk.weight_files("h1", directory)
    _, prob, _ = rk.tail_inputs(rk.TAIL_WEIGHT_D)
    rows = np.stack([wc.row_of(bp, itf, files[rk.tail_weight_of(b)]).row for b in range(prob["x0"].shape[0])])
    got = _solve(mpc, prob, weights=rows, warm=rk.padded_tail_warm(rk.TAIL_WEIGHT_D))
    _on_the_row_kernels(mpc)
    _compare_tail("rows_tail_weights", got, rk.tail_weight_solves(directory, True), lc.tolerance(rk.TAIL_CASE)[0])


# ---------------------------------------------------------------------------------------------------- C1, D
def _both(which, directory, chunks=0, materialize=False, profile=False):
    """The problem `which` of rk.both_rows_problem under a weight row AND a cone row per problem, two iterations from the cold start, on a handle created
    under the present environment: the solve, then the staged buffers at the solution."""
    import bipedal_control_amd as bp
    from bipedal_control_amd import scenarios as sc
    robot = "g1" if which == "g1" else "h1"
    itf = sc.interface(robot)
    prob = rk.both_rows_problem(which, itf)
    files = rk.weight_files(robot, directory)
    weights, cones = rk.both_rows(which)
    B = prob["x0"].shape[0]
    mpc = bp.BatchedSqpMpc(itf, max_batch=B, max_nodes=wc.MAX_NODES, sqp_iterations=rk.ITERATIONS, return_gains=True, pipeline_chunks=chunks,
                           materialize_lq=materialize, profile=profile)
    out = _solve(mpc, prob, cone=np.stack([cc.row(robot, c) for c in cones]), weights=np.stack([wc.row_of(bp, itf, files[w]).row for w in weights]))
    if profile:
        _on_the_row_kernels(mpc)
    lay = mpc.layout()
    mpc.stage("linearize"); mpc.stage("project"); mpc.synchronize()
    out.update({k: mpc.read(k) for k in set(STAGED + DENSE + (LQ if materialize else ()))})
    out.update(prob=prob, n=lay["n_nodes_max"], n_grids=lay["n_grids"], nx=itf.stateDim, B=B, compact=int(mpc.read("weights_compact")[0]))
    return out


_DEFAULT = {}


def _default(which, directory):
    """The handle with every switch at its default (call before any setenv of the test): computed once, shared, never modified; on the row kernels, and
    against the oracle."""
    if which not in _DEFAULT:
        _DEFAULT[which] = _both(which, directory, profile=True)
        _against_both_oracle("rows_both_%s_default" % which, which, _DEFAULT[which], directory)
    return _DEFAULT[which]


def _against_both_oracle(key, which, got, directory):
    oracle = rk.both_rows_solves(which, got["prob"], directory)
    report = {}
    for b, (xo, uo, Ko, _) in enumerate(oracle):
        n = got["records"][b][0]
        rel_x(got["x"][b, :n + 1], xo, report), rel_u(got["u"][b, :n], uo, report), rel_K(got["K"][b, :n], Ko, report)
    print(key, report)
    _write_report(key, report)
    _against_oracle(key, got["raw"], oracle)      # x, u 1e-11, K 1e-10; status, iteration count and step size equal


@pytest.mark.parametrize("which", ["h1", "g1"])
def test_table_walks_under_both_kinds_of_rows(which, directory, monkeypatch):
    """C1: BPMPC_LIN_TABLES=1 asks a robot of two serial legs for the CHAIN = false form of the three node kernels.  Every problem against its oracle,
    and against the same handle without the switch at 1e-12 (x, u per physical block) with equal step sizes - the figure
    test_gpu_far_iterates.py::test_far_iterates_through_the_other_paths holds this switch to."""
    base = _default(which, directory)
    monkeypatch.setenv("BPMPC_LIN_TABLES", "1")
    got = _both(which, directory, profile=True)
    _against_both_oracle("rows_tables_%s" % which, which, got, directory)
    worst = [0.0, 0.0]
    for b in range(got["B"]):
        n = got["records"][b][0]
        worst = [max(worst[0], rel_x(got["x"][b, :n + 1], base["x"][b, :n + 1])), max(worst[1], rel_u(got["u"][b, :n], base["u"][b, :n]))]
    print("rows_tables_%s against the chain walks: x %.2e u %.2e" % (which, *worst))
    _write_report("rows_tables_%s_against_chain" % which, dict(x=worst[0], u=worst[1]))
    assert [r[FIELDS.index("step_size")] for r in got["records"]] == [r[FIELDS.index("step_size")] for r in base["records"]]
    assert worst[0] < 1e-12 and worst[1] < 1e-12, worst


@pytest.mark.parametrize("which", ["h1", "g1"])
def test_dense_project(which, directory, monkeypatch):
    """D: BPMPC_DENSE_PROJECT=1 (k_project_fast_qd_w<NJ, false, true> behind the general elimination outputs): against the oracle, and Wt, Qp, Mt at the
    solution in the region the sweep reads against the default-switch row handle at 1e-12, by the loop of
    test_gpu_parity.py::test_structured_and_dense_change_of_variables_agree."""
    base = _default(which, directory)
    monkeypatch.setenv("BPMPC_DENSE_PROJECT", "1")
    got = _both(which, directory, profile=True)
    _against_both_oracle("rows_dense_project_%s" % which, which, got, directory)
    # both handles stage at their own solution: the same iterate only to the rounding the two paths differ by, as in the default family's test
    worst = _structured_against_dense({k: base[k] for k in DENSE}, {k: got[k] for k in DENSE}, got["B"], wc.MAX_NODES, got["n"], got["nx"])
    print("rows_dense_project_%s projected model: %.2e" % (which, worst))
    _write_report("rows_dense_project_%s_projected" % which, dict(Wt_Qp_Mt=worst))
    assert worst < 1e-12, worst


@pytest.mark.parametrize("which", ["h1", "g1"])
def test_joint_rows_of_wt(which, directory, monkeypatch):
    """D: BPMPC_WT_JOINT_ROWS=1 (k_project_fast_qd_w<NJ, true, true>) only adds stores of the rows the sweep's loaders would otherwise complete: x, u, K
    and the statistics bit for bit equal to the default-switch row handle."""
    base = _default(which, directory)
    monkeypatch.setenv("BPMPC_WT_JOINT_ROWS", "1")
    got = _both(which, directory, profile=True)
    _against_both_oracle("rows_wt_joint_rows_%s" % which, which, got, directory)
    _same_bits(base, got)


@pytest.mark.parametrize("other", [None, "BPMPC_DENSE_PROJECT", "BPMPC_WT_JOINT_ROWS"])
@pytest.mark.parametrize("which", ["h1", "g1"])
def test_dense_weights(which, other, directory, monkeypatch):
    """D: BPMPC_DENSE_WEIGHTS=1: weights_compact reads 0 and k_project_fast_w runs in place of the diagonal-Q kernel - the same body, a skipped term is
    a product with an exact zero (test_gpu_weight_structure.py): x, u, K, Wt, Qp and Mt bit for bit.  Alone (<NJ, true, false>), and on top of each of
    the other two project switches (<NJ, false, true>, <NJ, true, true>) against that switch alone."""
    base = _default(which, directory)
    if other:
        monkeypatch.setenv(other, "1")
        base = _both(which, directory)
    monkeypatch.setenv("BPMPC_DENSE_WEIGHTS", "1")
    got = _both(which, directory, profile=True)
    assert (base["compact"], got["compact"]) == (1, 0)
    _against_both_oracle("rows_dense_weights_%s%s" % (which, "_" + other[6:].lower() if other else ""), which, got, directory)
    _same_bits(base, got, ("x", "u", "K", "Wt", "Qp", "Mt"))


@pytest.mark.parametrize("which", ["h1", "g1", "two_gaits"])
def test_horizon_chunks(which, directory):
    """D: pipeline_chunks 2, 3 and 7 against 1: the lineariser twin in its per-grid mapping with k0 > 0 (at 7 chunks 3 .. 4 nodes per launch, a partly
    filled single workgroup per problem), on one grid and on the two grids of the two-gait problem: x, u, K and the statistics bit for bit, as
    test_gpu_parity.py::test_pipelined_horizon_chunks_are_bit_identical holds the default family."""
    base = _default(which, directory)
    assert base["n_grids"] == (2 if which == "two_gaits" else 1)
    for chunks in rk.CHUNKS:
        got = _both(which, directory, chunks=chunks, profile=True)
        _against_both_oracle("rows_chunks%d_%s" % (chunks, which), which, got, directory)
        _same_bits(base, got)


@pytest.mark.parametrize("which", ["h1", "g1"])
def test_inline_lane_map(which, directory, monkeypatch):
    """D: BPMPC_LIN_COMPACT=0 on one grid (the lineariser twin's per-grid mapping with k0 = 0 over the whole horizon): the solve and what stage
    ("linearize") leaves - in fused mode, and the complete LQ model of the materialised mode - bit for bit equal to the compact mapping."""
    base = _default(which, directory)
    full = _both(which, directory, materialize=True)
    _same_bits(base, full)
    monkeypatch.setenv("BPMPC_LIN_COMPACT", "0")
    got = _both(which, directory, profile=True)
    _against_both_oracle("rows_lin_compact0_%s" % which, which, got, directory)
    _same_bits(base, got, ("x", "u", "K") + STAGED)
    _same_bits(full, _both(which, directory, materialize=True), ("x", "u", "K") + LQ)


# ---------------------------------------------------------------------------------------------------- C2, C3
@pytest.mark.parametrize("name", list(rk.TREE_CASES))
def test_trees_under_cone_rows(name, directory):
    """C2, C3: robots that are not two serial legs run the CHAIN = false form of the three node kernels; here under cone rows (model, mu03, all), three
    iterations, compared as test_gpu_tree_variants.py::_compare_solve compares.  W12 "mixed": nx = 24, two grids (a grid per distinct schedule), hence
    the per-grid lineariser mapping, four contact modes, problem 0 back-tracks in every iteration; U10 "walk": nx = 22, one grid, the compact
    mapping; L46 "walk": one problem three times over from a far iterate (rk.L46_BACKTRACK) - 6, 10 and 9 trials under every row, the table-walk
    tail - at ten times the floor of the oracle under each row (tree_variants.FLOOR_CASES), step lengths exact."""
    import bipedal_control_amd as bp
    shape = rk.TREE_CASES[name]
    itf = tv.interface(tv.register(name, directory))
    prob, start = rk.tree_problem(name, tv.problem(itf, shape))
    oracle = rk.tree_solves(name, prob, start)
    nx = itf.stateDim
    warm = (None, None)
    if start:
        warm = np.zeros((tv.BATCH, tv.MAX_NODES + 1, nx)), np.zeros((tv.BATCH, tv.MAX_NODES, nx))
        for b, (x, u) in enumerate(start):
            warm[0][b, :x.shape[0]], warm[1][b, :u.shape[0]] = x, u
    mpc = bp.BatchedSqpMpc(itf, max_batch=tv.BATCH, max_nodes=tv.MAX_NODES, sqp_iterations=rk.TREE_ITERATIONS, return_gains=True, profile=True)
    got = _solve(mpc, prob, cone=np.stack([cc.row(name, r) for r in rk.TREE_ROWS]), warm=warm)
    _on_the_row_kernels(mpc)
    assert mpc.layout()["n_grids"] == len({g for g, _ in tv.SHAPES[shape]}) and (nx, mpc.layout()["n_grids"]) == dict(W12=(24, 2), U10=(22, 1), L46=(22, 1))[name]

    def floor(b):
        fl, merit, stable = rk.tree_solve_floor(name, prob, start, b)
        assert stable, (name, b)          # every sample accepts the same step lengths: they can be compared exactly
        return fl, merit
    _compare_solve(name, shape, rk.TREE_ITERATIONS, prob, got["raw"], "rows_tree_%s_%s" % (name, shape), oracle=oracle, floor=floor)
