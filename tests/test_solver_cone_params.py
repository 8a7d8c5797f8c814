"""CPU tier of the per-problem cone parameters (include/bpmpc.h "Per-problem cone parameters"): the host check of a cone row
(bpmpc_model_check_cone_params), the ABI of the new entry points, and - with the oracle alone - the cases the GPU tier stands on
(tests/cone_cases.py).  No device."""
import ctypes as C

import numpy as np
import pytest

from tests import cone_cases as cc
from tests import weight_cases as wc

NEW_SYMBOLS = ("bpmpc_solver_set_cone_params", "bpmpc_solver_get_cone_params", "bpmpc_solver_reset_cone_params", "bpmpc_model_check_cone_params")


@pytest.fixture(scope="module")
def bp():
    import bipedal_control_amd as bp
    return bp


def test_host_check_accepts_the_rows_and_refuses_each_case(bp):
    """Item 1."""
    from bipedal_control_amd import scenarios as sc
    h1, g1, hard = sc.interface("h1"), sc.interface("g1"), sc.interface("h1:hard")
    for itf, robot in ((h1, "h1"), (g1, "g1"), (hard, "h1:hard")):
        start = bp.ConeParams.from_model(itf)
        assert np.array_equal(start.row, cc.start_row(robot)), robot      # the product's start row is the oracle model's
        itf.checkConeParams(start)
        itf.checkConeParams(start.row)
    for name in cc.ROWS:
        h1.checkConeParams(cc.row("h1", name))
    assert cc.row("h1:hard", "model")[cc.HESSIAN_SHIFT] == 0.0
    hard.checkConeParams(cc.row("h1:hard", "mu03"))
    hard.checkConeParams(cc.row("h1:hard", "bar1"))

    def changed(robot, **entries):
        r = cc.row(robot, "model")
        for i, v in entries.items():
            r[int(i[1:])] = v
        return r
    refusals = [      # (interface, row, entry named in the message, word of the reason)
        (h1, changed("h1", e0=np.nan), "entry 0", "finite"), (h1, changed("h1", e5=np.inf), "entry 5", "finite"), (h1, changed("h1", e7=np.nan), "entry 7", "finite"),
        (h1, changed("h1", e0=0.0), "entry 0", "positive"), (h1, changed("h1", e0=-0.5), "entry 0", "positive"),
        (h1, changed("h1", e1=0.0), "entry 1", "positive"), (h1, changed("h1", e1=-1.0), "entry 1", "positive"),
        (h1, changed("h1", e2=-1e-3), "entry 2", "negative"),
        (h1, changed("h1", e3=-1e-9), "entry 3", "negative"),
        (hard, changed("h1:hard", e3=1e-6), "entry 3", "hard"),
        (h1, changed("h1", e4=0.0), "entry 4", "positive"), (h1, changed("h1", e4=-0.1), "entry 4", "positive"),
        (h1, changed("h1", e5=0.0), "entry 5", "positive"), (h1, changed("h1", e5=-5.0), "entry 5", "positive"),
        (h1, changed("h1", e6=1.0), "entry 6", "must be 0"), (h1, changed("h1", e7=-1.0), "entry 7", "must be 0"),
    ]
    for itf, r, entry, reason in refusals:
        with pytest.raises(bp.BpmpcError) as e:
            itf.checkConeParams(r)
        assert e.value.status == -1 and entry in str(e.value) and reason in str(e.value), (entry, str(e.value))
    h1.checkConeParams(changed("h1", e2=0.0, e3=0.0))      # the bounds that include zero
    with pytest.raises(ValueError):
        h1.checkConeParams(np.zeros(6))


def test_cone_params_class(bp):
    from bipedal_control_amd import scenarios as sc
    p = bp.ConeParams.from_model(sc.interface("h1"))
    assert bp.ConeParams.STRIDE == 8 and p.row.shape == (8,) and not p.row[6:].any()
    q = p.replaced(frictionCoefficient=0.3)
    assert q.frictionCoefficient == 0.3 and p.frictionCoefficient == 0.5 and np.array_equal(q.row, cc.row("h1", "mu03"))
    assert np.array_equal(bp.ConeParams.fromRow(cc.row("h1", "all")).row, cc.row("h1", "all"))
    assert np.array_equal(p.replaced(frictionCoefficient=0.3, mu=0.5, delta=2.0, regularization=4.0, gripperForce=10.0, hessianShift=1e-4).row, cc.row("h1", "all"))
    with pytest.raises(ValueError):
        bp.ConeParams(friction=0.3)


def test_header_declares_and_library_exports_the_new_entry_points(bp):
    from bipedal_control_amd import abi
    protos = abi.prototypes()
    lib = bp.load_library()
    for name in NEW_SYMBOLS:
        assert name in protos, name
        assert getattr(lib, name).restype is C.c_int and len(getattr(lib, name).argtypes) == len(protos[name][1])
    assert protos["bpmpc_solver_set_cone_params"][1] == protos["bpmpc_solver_set_weights"][1]      # the contract of set_weights, argument for argument
    text = open(abi.HEADER).read()
    assert "#define BPMPC_SOLVER_CONE_STRIDE 8" in text
    for i, name in enumerate(("FRICTION", "REGULARIZATION", "GRIPPER_FORCE", "HESSIAN_SHIFT", "BARRIER_MU", "BARRIER_DELTA", "RESERVED")):
        assert "#define BPMPC_SOLVER_CONE_%s %d\n" % (name, i) in text, name
    assert "Not per problem: the cone parameters" not in text
    # the null-argument refusals need no device
    assert lib.bpmpc_model_check_cone_params(None, None) == -1
    assert lib.bpmpc_solver_set_cone_params(None, 1, None, None, 1, 0) == -1 and lib.bpmpc_solver_get_cone_params(None, 0, None) == -1
    assert lib.bpmpc_solver_reset_cone_params(None) == -1


def test_oracle_for_leaves_the_cached_model_alone():
    from tests import oracle_bridge as ob
    before = {k: ob.model("h1")[k] for k in ("friction_coefficient", "cone_regularization", "cone_gripper_force", "cone_hessian_shift", "barrier_mu", "barrier_delta")}
    m = cc.model_under("h1", cc.row("h1", "all"))
    assert m is not ob.model("h1") and m["friction_coefficient"] == 0.3 and m["cone_gripper_force"] == 10.0
    cc.oracle_for("h1", cc.row("h1", "all"))
    assert before == {k: ob.model("h1")[k] for k in before}
    assert ob.model("h1:hard")["ineq_mu"] == cc.start_row("h1:hard")[cc.BARRIER_MU]
    assert cc.model_under("h1:hard", cc.row("h1:hard", "bar1"))["ineq_mu"] == 1.0


def test_backtracking_case_is_what_it_says():
    """Item 2: the iterate the GPU tier warm-starts from (cone_cases.BACKTRACK): the oracle alone, one iteration under each cone row."""
    from bipedal_control_amd import scenarios as sc
    prob, x, u = cc.backtrack_problem(sc.interface("h1"))
    got = tuple(cc.steps(cc.solve(prob, 0, cc.row("h1", n), 1, x, u)[3])[0] for n in cc.BACKTRACK["rows"])
    assert cc.BACKTRACK["rows"] == ("model", "mu03", "bar1") and got == cc.BACKTRACK["alpha"] == (1.0, 0.5, 1.0), got


def test_the_rows_matter_to_the_oracle():
    """Item 3: each row changes u of the 2-iteration cold-start solve of problem 0 by more than 1e-6 relative; the model's row is the bridge's oracle."""
    from bipedal_control_amd import scenarios as sc
    from tests import oracle_bridge as ob
    prob = wc.h1_problem(sc.interface("h1"))
    base = cc.solve(prob, 0, cc.row("h1", "model"), 2)
    assert np.array_equal(base[1], ob.oracle_solve_like(prob, 0, iterations=2)[1])
    for name in ("mu03", "bar1", "all"):
        u = cc.solve(prob, 0, cc.row("h1", name), 2)[1]
        change = float(np.abs(u - base[1]).max() / max(1.0, np.abs(base[1]).max()))
        print("row %s changes u by %.2e" % (name, change))
        assert change > 1e-6, (name, change)
