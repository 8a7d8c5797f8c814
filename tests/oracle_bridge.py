"""Test-side glue: rebuild a product scenario (bipedal_control_amd.scenarios) with the ORACLE's own ingest and
reference pre-pass and solve it with the C++ oracle.  Used by the GPU parity tests and by __graft_entry__.smoke().

The mode schedule handed to the oracle's pre-pass (oracle_nodes below) is the PRODUCT's: scenarios.gait_schedule tiles the gait template with the
product's own GaitSchedule (C++), and the oracle starts from its event times and mode sequence.  The oracle's time grid, swing references and target
interpolation are its own; the tiling is not re-derived here.  It is checked independently on the CPU tier, against the oracle's own pure-Python
GaitSchedule and a hand-derived answer: tests/test_reference_prepass.py::test_gait_schedule_tiling and ::test_trot_tiling_known_answer."""
import functools
import os

import numpy as np

from oracle import ingest, oracle_py, reference_py as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets", "h1")


_URDF = {"h1": "h1_mpc.urdf", "openloong": "openloong_mpc.urdf", "g1": "g1_mpc.urdf", "hunter": "hunter_mpc.urdf"}


_REGISTERED = {}      # name -> (urdf, task, reference): robots that are not under assets/ (tests/tree_variants.py writes their files at test time)


def register(name, urdf, task, reference):
    """Makes model(name) / oracle(name) and everything that takes a robot name work on the given files.  The first registration of a name holds: the model is
    cached, and the files of a name are the same text wherever they were written."""
    assert name not in _URDF
    _REGISTERED.setdefault(name, (urdf, task, reference))


@functools.lru_cache(maxsize=None)
def model(robot="h1"):
    """robot name, optionally with the suffix ":hard" = BipedalRobotInterface(..., useHardFrictionConeConstraint = true)."""
    name, _, variant = robot.partition(":")
    if name in _REGISTERED:
        return ingest.build_model(*_REGISTERED[name], use_hard_friction_cone=(variant == "hard"))
    d = os.path.join(ROOT, "assets", name)
    return ingest.build_model(os.path.join(d, _URDF[name]), os.path.join(d, "task.info"), os.path.join(d, "reference.info"),
                              use_hard_friction_cone=(variant == "hard"))


@functools.lru_cache(maxsize=None)
def oracle(robot="h1"):
    return oracle_py.OracleModel(ingest.model_blob(model(robot)))


def h1_model():
    return model("h1")


def h1_oracle():
    return oracle("h1")


def oracle_nodes(prob, b, dt=0.015, robot="h1"):
    """Per-interval arrays of problem b computed by the oracle's own pre-pass from the scenario's schedule / targets."""
    m = model(robot)
    sched = prob["schedule"][b] if isinstance(prob["schedule"], list) else prob["schedule"]
    ev, ms = list(map(float, sched.eventTimes)), list(map(int, sched.modeSequence))
    planner = rp.SwingTrajectoryPlanner(m["swing"])
    planner.update(ev, ms)
    tt = prob["targets"][b if len(prob["targets"]) > 1 else 0]
    t0 = float(np.broadcast_to(prob["t0"], (prob["x0"].shape[0],))[b])
    return rp.node_arrays(m, t0, t0 + prob["horizon"], dt, ev, ms, np.asarray(tt.timeTrajectory), np.asarray(tt.stateTrajectory), planner)


def oracle_solve_like(prob, b, iterations=1, x_init=None, u_init=None, robot="h1"):
    m, om = model(robot), oracle(robot)
    nodes = oracle_nodes(prob, b, robot=robot)
    x0 = prob["x0"][b]
    if x_init is None:
        x_init, u_init = rp.cold_start(m, nodes, x0)
    s = m["sqp"]
    xo, uo, K, stats = om.solve(nodes, x0, x_init, u_init, iterations=iterations, g_max=s["g_max"], g_min=s["g_min"], delta_tol=s["deltaTol"])
    return xo, uo, K, stats
