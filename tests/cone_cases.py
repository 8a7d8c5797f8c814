"""Cone rows for the tests of the per-problem cone parameters (bpmpc_solver_set_cone_params), shared by tests/test_solver_cone_params.py (CPU) and
tests/test_gpu_solver_cone_params.py.  Host only: numpy, text editing and the oracle.

A cone row is eight doubles: friction coefficient, regularisation, gripper force, Hessian shift, barrier mu, barrier delta, 0, 0 (include/bpmpc.h
BPMPC_SOLVER_CONE_*).  The oracle under a row is the oracle of a COPY of the robot's model dictionary with those entries overwritten (oracle_for);
oracle/ stays as it is."""
import copy
import functools
import os
import re

import numpy as np

from oracle import ingest, oracle_py, reference_py as rp
from tests import oracle_bridge as ob
from tests import weight_cases as wc

STRIDE = 8
FRICTION, REGULARIZATION, GRIPPER_FORCE, HESSIAN_SHIFT, BARRIER_MU, BARRIER_DELTA = range(6)
# row name -> the entries that differ from the start row
ROWS = {
    "model": {},
    "mu03": {FRICTION: 0.3},
    "bar1": {BARRIER_MU: 1.0},
    "all": {FRICTION: 0.3, BARRIER_MU: 0.5, BARRIER_DELTA: 2.0, REGULARIZATION: 4.0, GRIPPER_FORCE: 10.0, HESSIAN_SHIFT: 1e-4},
}
# The back-tracking case: the iterate tests/far_iterates.far_iterate("h1", nodes of problem 1, x0 of problem 1, amp, seed) of weight_cases.h1_problem, under
# the model's weights.  The oracle's first iteration takes the step `alpha[row]` under each cone row: the full step under the model's cone and under
# barrier mu 1.0, half a step under friction 0.3 - the cone row alone decides.  Found by search_backtrack below (amplitudes, problems, seeds in that
# order; the first hit at the lowest amplitude that has one); tests/test_solver_cone_params.py asserts it with the oracle alone.
BACKTRACK = dict(problem=1, amp=1.5, seed=30, rows=("model", "mu03", "bar1"), alpha=(1.0, 0.5, 1.0))


def _hard(robot):
    return robot.endswith(":hard")


def start_row(robot):
    """What the solver's kernels read of the model (csrc/device_model.cpp): with the hard cone the SQP penalty's mu / delta and no shift."""
    m = ob.model(robot)
    row = np.zeros(STRIDE)
    row[:6] = [m["friction_coefficient"], m["cone_regularization"], m["cone_gripper_force"], m["cone_hessian_shift"], m["barrier_mu"], m["barrier_delta"]]
    if _hard(robot):
        row[HESSIAN_SHIFT], row[BARRIER_MU], row[BARRIER_DELTA] = 0.0, m["ineq_mu"], m["ineq_delta"]
    return row


def row(robot, name):
    r = start_row(robot)
    for i, v in ROWS[name].items():
        r[i] = v
    return r


def model_under(robot, cone_row):
    """A deep copy of oracle_bridge.model(robot) - the cached dictionary is not touched - with the cone entries of `cone_row`."""
    m = copy.deepcopy(ob.model(robot))
    r = np.asarray(cone_row, float)
    m["friction_coefficient"], m["cone_regularization"], m["cone_gripper_force"] = float(r[FRICTION]), float(r[REGULARIZATION]), float(r[GRIPPER_FORCE])
    if _hard(robot):
        assert r[HESSIAN_SHIFT] == 0.0
        m["ineq_mu"], m["ineq_delta"] = float(r[BARRIER_MU]), float(r[BARRIER_DELTA])
    else:
        m["cone_hessian_shift"], m["barrier_mu"], m["barrier_delta"] = float(r[HESSIAN_SHIFT]), float(r[BARRIER_MU]), float(r[BARRIER_DELTA])
    return m


@functools.lru_cache(maxsize=None)
def _oracle(robot, key):
    return oracle_py.OracleModel(ingest.model_blob(model_under(robot, np.array(key))))


def oracle_for(robot, cone_row):
    """The oracle of `robot` (a name oracle_bridge knows, ":hard" included) under `cone_row`; cached per (robot, row)."""
    return _oracle(robot, tuple(float(v) for v in np.asarray(cone_row, float).reshape(-1)))


def solve(prob, b, cone_row, iterations=1, x_init=None, u_init=None, robot="h1"):
    """oracle_bridge.oracle_solve_like under `cone_row`: (x, u, K, stats) of problem b."""
    m, om = ob.model(robot), oracle_for(robot, cone_row)
    nodes = ob.oracle_nodes(prob, b, robot=robot)
    x0 = prob["x0"][b]
    if x_init is None:
        x_init, u_init = rp.cold_start(m, nodes, x0)      # (the cold start reads no cone parameter: the nominal input is the robot's weight)
    s = m["sqp"]
    return om.solve(nodes, x0, x_init, u_init, iterations=iterations, g_max=s["g_max"], g_min=s["g_min"], delta_tol=s["deltaTol"])


def steps(stats):
    """The accepted step of every iteration that ran."""
    return [float(r[3]) for r in stats if r[10] > 0]


def write_variant(robot, name, directory):
    """Writes a copy of assets/<robot>/task.info whose frictionConeSoftConstraint.frictionCoefficient / mu / delta (hard cone: frictionCoefficient
    and sqp.inequalityConstraintMu / Delta) are those of row `name` - a row that changes nothing else, the other three entries are no task-file
    settings - and returns dict(task, urdf, reference): a product model of its own, whose default kernels solve under that row."""
    base = robot.partition(":")[0]
    r, s = row(robot, name), start_row(robot)
    assert all(r[i] == s[i] for i in (REGULARIZATION, GRIPPER_FORCE, HESSIAN_SHIFT)), name
    a = wc.assets(base)
    text = open(a["task"]).read()

    def put(text, block, key, value):
        m = re.search(r"^%s\s*\n\{\n(.*?)^\}" % block, text, flags=re.S | re.M)
        assert m, block
        body, n = re.subn(r"^(\s*%s\s+)\S+" % key, lambda e: e.group(1) + repr(float(value)), m.group(1), flags=re.M)
        assert n == 1, (block, key)
        return text[:m.start(1)] + body + text[m.end(1):]
    text = put(text, "frictionConeSoftConstraint", "frictionCoefficient", r[FRICTION])
    if _hard(robot):
        text = put(put(text, "sqp", "inequalityConstraintMu", r[BARRIER_MU]), "sqp", "inequalityConstraintDelta", r[BARRIER_DELTA])
    else:
        text = put(put(text, "frictionConeSoftConstraint", "mu", r[BARRIER_MU]), "frictionConeSoftConstraint", "delta", r[BARRIER_DELTA])
    path = os.path.join(str(directory), "task_%s_cone_%s.info" % (base, name))
    with open(path, "w") as f:
        f.write(text)
    return dict(task=path, urdf=a["urdf"], reference=a["reference"])


def backtrack_problem(itf):
    """(prob, x, u): problem BACKTRACK["problem"] of weight_cases.h1_problem three times over - the cone rows differ, nothing else - and its far iterate."""
    from tests import far_iterates as fi
    prob = wc.h1_problem(itf)
    b = BACKTRACK["problem"]
    nodes = ob.oracle_nodes(prob, b)
    x, u, _ = fi.far_iterate("h1", nodes, prob["x0"][b], BACKTRACK["amp"], BACKTRACK["seed"])
    same = dict(prob, x0=np.repeat(prob["x0"][b:b + 1], wc.BATCH, axis=0), targets=[prob["targets"][b]] * wc.BATCH)
    return same, x, u


def search_backtrack(itf, amps=(0.5, 1.0, 1.5, 2.0, 3.0), problems=range(3), seeds=range(40), want=(1.0, 0.5, 1.0)):
    """The search that found BACKTRACK: the first (amp, problem, seed), in that order, whose far iterate makes the oracle's first iteration accept
    `want` under the rows BACKTRACK["rows"].  Minutes on the CPU; no test runs it."""
    from tests import far_iterates as fi
    prob = wc.h1_problem(itf)
    for amp in amps:
        for b in problems:
            nodes = ob.oracle_nodes(prob, b)
            for seed in seeds:
                x, u, _ = fi.far_iterate("h1", nodes, prob["x0"][b], amp, seed)
                got = tuple(steps(solve(prob, b, row("h1", n), 1, x, u)[3])[0] for n in BACKTRACK["rows"])
                if got == tuple(want):
                    return dict(problem=b, amp=amp, seed=seed)
    return None
