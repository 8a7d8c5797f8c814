"""Robots whose kinematic tree is NOT two serial legs of nj / 2 joints, for the kernels that walk the tree through tables (DeviceModel::path, depth, subtree,
contact_path: the CHAIN = false form of the per-node kernels, the rigid-body pass of the WBC, the estimator's contact kinematics).  Every robot under
assets/ is two equal chains in body order, so on them the tables only ever hold chains.

A variant is a committed URDF with a task file whose model_settings.jointNames / contactNames3DoF are replaced by a text edit: joints that are not
named are welded at zero and their links merged into the parent body (oracle/ingest.py, robot_model.cpp), which changes the tree.  The files are written
at test time into a directory the caller gives (tmp_path); nothing is added to the tree.  Trees as oracle/ingest.py:build_model returns them (parent of
bodies 1 .. nj, body 0 = the base; joints depth-first with children in joint-name order):

  L46  nx 22  parent [0,1,2,3, 0,5,6,7,8,9]        contacts on bodies [4,4,10,10]   legs of 4 and 6 joints: depth 6 > nj / 2, feet at unequal depths
  U10  nx 22  parent [0,1,2,3, 0,5,6,7,8, 0]       contacts on bodies [4,4,9,9]     three chains on the base; the torso joint moves no contact
  W12  nx 24  parent [0,1,2,3,4, 0,6,7,8,9, 0,11]  contacts on bodies [5,5,10,10]   the packed 16-lane layout; a chain of two outside every contact path

The joint block of R (J' R_task J at the initial pose) is singular on all three, as it is on stock G1 and OpenLoong.

Plain module (no fixtures): CPU and GPU tiers import it."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_A = os.path.join(ROOT, "assets")
_H1_SOLE_URDF = os.path.join(ROOT, "tests", "golden", "reference", "bipedal_robot_example", "unitree_h1", "h1_description", "urdf", "h1_with_sole.urdf")
_H1_LEFT = ["left_hip_yaw_joint", "left_hip_roll_joint", "left_hip_pitch_joint", "left_knee_joint", "left_ankle_joint"]
_H1_RIGHT = [n.replace("left", "right") for n in _H1_LEFT]
_H1_SOLES = ["left_sole_1_link", "left_sole_2_link", "right_sole_1_link", "right_sole_2_link"]
_G1_SOLES = ["left_sole_front", "left_sole_back", "right_sole_front", "right_sole_back"]

VARIANTS = {
    "L46": dict(urdf=os.path.join(_A, "g1", "g1_mpc.urdf"), task=os.path.join(_A, "h1", "task.info"), reference=os.path.join(_A, "h1", "reference.info"),
                joints=["left_%s_joint" % j for j in ("hip_pitch", "hip_roll", "hip_yaw", "knee")]
                + ["right_%s_joint" % j for j in ("hip_pitch", "hip_roll", "hip_yaw", "knee", "ankle_pitch", "ankle_roll")],
                contacts=_G1_SOLES, parent=[0, 1, 2, 3, 0, 5, 6, 7, 8, 9], contact_body=[4, 4, 10, 10]),
    "U10": dict(urdf=_H1_SOLE_URDF, task=os.path.join(_A, "h1", "task.info"), reference=os.path.join(_A, "h1", "reference.info"),
                joints=_H1_LEFT[:4] + _H1_RIGHT + ["torso_joint"], contacts=_H1_SOLES,
                parent=[0, 1, 2, 3, 0, 5, 6, 7, 8, 0], contact_body=[4, 4, 9, 9]),
    "W12": dict(urdf=_H1_SOLE_URDF, task=os.path.join(_A, "g1", "task.info"), reference=os.path.join(_A, "g1", "reference.info"),
                joints=_H1_LEFT + _H1_RIGHT + ["torso_joint", "left_shoulder_pitch_joint"], contacts=_H1_SOLES,
                parent=[0, 1, 2, 3, 4, 0, 6, 7, 8, 9, 0, 11], contact_body=[5, 5, 10, 10]),
}
NAMES = tuple(VARIANTS)
STOCK = ("h1", "hunter", "g1", "openloong")

# ---- the problems (the smallest that still have a partly filled last wave in the kernels of four nodes per wave, event nodes, and a back-tracker)
# (event times, mode sequence).  The horizon of 0.45 s sees STANCE and LF of "walk" and one event node; "hop" is the schedule with a flight phase, its
# events drawn together so that all four contact modes and four event nodes lie inside the horizon
SCHEDULES = {"walk": ((0.15, 0.45, 0.60, 0.90), (3, 1, 3, 2, 3)),        # STANCE, LF, STANCE, RF, STANCE
             "hop": ((0.09, 0.21, 0.30, 0.39), (3, 1, 0, 2, 3))}         # STANCE, LF, FLY, RF, STANCE
# problem b of a batch: (mode sequence, seed of the perturbation of the initial state).  "walk": one schedule for the whole batch = one grid (the lineariser's
# compact lane map, event nodes in workgroups of their own); "mixed": a schedule per problem = a grid per distinct schedule, of 34 and 31 nodes (the in-line
# lane map).
SHAPES = {"walk": (("walk", 3), ("walk", 4), ("walk", 5)),
          "mixed": (("hop", 3), ("walk", 4), ("hop", 5))}
BATCH = 3
DT, N_INTERVALS = 0.015, 30
HORIZON = N_INTERVALS * DT
N_NODES = {"walk": 31, "hop": 34}        # 30 intervals and the event nodes inside the horizon ("walk": the event at 0.45 is the end of the horizon)
MAX_NODES = 40
COMMAND = (0.3, 0.0, 0.0, 0.1)
INPUT_BOUND = {"walk": 260.0, "mixed": 410.0}      # |u| of the oracle's solves of one and three iterations stays below this on all three variants


def _replace_list(text, key, names):
    """The block `key { [0] a [1] b ... }` of an INFO file with the given names."""
    pat = re.compile(r"(\n[ \t]*" + re.escape(key) + r"[ \t]*\n[ \t]*\{)[^}]*(\})")
    body = "".join("\n    [%d] %s" % (i, n) for i, n in enumerate(names)) + "\n  "
    out, n = pat.subn(lambda m: m.group(1) + body + m.group(2), text, count=1)
    assert n == 1, key
    return out


def write_files(name, directory):
    """Writes the variant's task file into `directory`; returns dict(urdf, task, reference) of paths (urdf and reference are committed files)."""
    v = VARIANTS[name]
    text = open(v["task"]).read()
    text = _replace_list(text, "jointNames", v["joints"])
    text = _replace_list(text, "contactNames3DoF", v["contacts"])
    path = os.path.join(str(directory), "task_%s.info" % name)
    with open(path, "w") as f:
        f.write(text)
    return dict(urdf=v["urdf"], task=path, reference=v["reference"])


def stock_files(robot):
    d = os.path.join(_A, robot)
    return dict(urdf=os.path.join(d, robot + "_mpc.urdf"), task=os.path.join(d, "task.info"), reference=os.path.join(d, "reference.info"))


def register(name, directory):
    """write_files + tests.oracle_bridge.register: afterwards oracle_bridge.model(name), .oracle(name), .oracle_nodes(..., robot=name) and
    tests/far_iterates.py work on the variant."""
    from tests import oracle_bridge as ob
    files = write_files(name, directory)
    ob.register(name, files["urdf"], files["task"], files["reference"])
    return files


def interface(files):
    import bipedal_control_amd as bp
    return bp.BipedalRobotInterface(files["task"], files["urdf"], files["reference"])


def initial_states(initial_state, shape):
    x0 = np.asarray(initial_state, float)
    return np.stack([x0 + 0.02 * np.random.default_rng(seed).standard_normal(len(x0)) for _, seed in SHAPES[shape]])


def problem(itf, shape):
    """The batch `shape` in the form of bipedal_control_amd.scenarios (t0, x0, schedule, targets, horizon), through the product's host API."""
    from bipedal_control_amd.api import ModeSchedule
    x0 = initial_states(itf.getInitialState(), shape)
    scheds = [ModeSchedule(np.array(SCHEDULES[g][0]), np.array(SCHEDULES[g][1], np.int32)) for g, _ in SHAPES[shape]]
    targets = [itf.cmdVelToTargetTrajectories(COMMAND, 0.0, x0[b], HORIZON) for b in range(BATCH)]
    return dict(t0=0.0, x0=x0, schedule=(scheds[0] if shape == "walk" else scheds), targets=targets, horizon=HORIZON)


# ---- the tables of DeviceModel from `parent` alone (parent[j] = parent body of body j + 1)
def tables(parent, contact_body):
    parent = [int(p) for p in parent]
    nj = len(parent)
    up = [0] + parent                                      # up[b] for bodies 0 .. nj
    path, depth = [[] for _ in range(nj + 1)], [0] * (nj + 1)
    for b in range(1, nj + 1):
        chain, c = [], b
        while c > 0:
            chain.append(c)
            c = up[c]
        path[b], depth[b] = chain[::-1], len(chain)
    subtree = [0] * (nj + 1)
    for b in range(nj + 1):
        for c in range(nj + 1):
            if b == 0 or b in path[c]:
                subtree[b] |= 1 << c
    contact_path = [sum(1 << k for k in path[int(cb)]) for cb in contact_body]
    half = nj // 2
    serial = int(nj % 2 == 0 and all(parent[b - 1] == (0 if b in (1, half + 1) else b - 1) for b in range(1, nj + 1)))
    return dict(parent=up, depth=depth, path=path, subtree=subtree, contact_path=contact_path, max_depth=max(depth), serial_legs=serial)


# ---- the reference's own floor where the complete pivoting of the elimination meets a tie
FLOOR_SAMPLES = 8
FLOOR_FACTOR = 10.0     # the project's usual distance between exact solvers and a kernel tolerance


# (robot, batch, problem, iterations) of the GPU tier's solves in which the oracle's own result moves by more than the inherited tolerances when its cold start
# moves by 1e-15 relative: every solve of L46 (ties from the cold start on), and U10's first flight problem from the second iteration on (a tie at the iterate
# the first iteration accepts)
FLOOR_CASES = {("L46", shape, b, it) for shape in SHAPES for b in range(BATCH) for it in (1, 2, 3)} | {("U10", "mixed", 0, 2), ("U10", "mixed", 0, 3)}


def pivot_ties(name, nodes, x, u):
    """[(node, lead)] of the intermediate nodes at which two pivot candidates of the complete pivoting of D are equal to rounding (tests/far_iterates.py:
    pivot_margin, PIVOT_MARGIN).  There WHICH of a rigid foot's dependent rows the elimination leaves out is rounding's choice - on the device, in the reference
    bodies and in the oracle alike - and shows in Px wherever the rows are inconsistent (a momentum or joint velocities that are not zero)."""
    from tests import far_iterates as fi
    out = []
    for k in range(int(nodes["N"])):
        if nodes["kind"][k] == 0:
            lead = fi.node_pivot_margin(name, nodes, x, u, k)[0]
            if lead <= fi.PIVOT_MARGIN:
                out.append((k, lead))
    return out


def _signs(shape, sample):
    return np.random.default_rng([20250701, sample]).choice([-1.0, 1.0], shape)


def oracle_qp_floor(name, nodes, x0, x, u):
    """The oracle's QP step at (x, u) against the same step with every entry of the iterate moved by 1e-15 relative (FLOOR_SAMPLES sign patterns), the worst
    per kind (dx, du, K): dict(whole=relative to max(1, |value|_max) as tests/test_hostemu_kernels.py::test_qp_step_pipeline measures, blocks=per
    physical block as tests/tolerances.py measures).  What a perturbation of the size of one rounding error does to the reference itself is what no
    other summation order can be held to (tests/far_iterates.py oracle_solve_floor); without a pivot tie it is ~1e-13."""
    from tests import oracle_bridge as ob
    from tests.tolerances import rel_K, rel_u, rel_x
    om = ob.oracle(name)
    base = om.qp_step(nodes, x0, x, u)
    whole, blocks = np.zeros(3), np.zeros(3)
    for s in range(FLOOR_SAMPLES):
        got = om.qp_step(nodes, x0, x * (1.0 + 1e-15 * _signs(x.shape, s)), u * (1.0 + 1e-15 * _signs(u.shape, 100 + s)))
        whole = np.maximum(whole, [np.abs(g - b).max() / max(1.0, np.abs(b).max()) for g, b in zip(got, base)])
        blocks = np.maximum(blocks, [rel_x(got[0], base[0]), rel_u(got[1], base[1]), rel_K(got[2], base[2])])
    return dict(whole=tuple(float(v) for v in whole), blocks=tuple(float(v) for v in blocks))


def oracle_solve_floor(name, prob, b, iterations, solve=None, start=None):
    """The same for a whole solve from the cold start: ((x, u, K) per physical block as tests/tolerances.py measures, merit, steps_stable) - the oracle's
    solve against its solve from the cold start moved by 1e-15 relative.  steps_stable: every sample accepts the same step lengths.
    solve(x, u) -> (x, u, K, record): another oracle of the same problem (tests/row_kernel_cases.py: under a cone row); start = (x, u): another iterate
    than the cold start."""
    from oracle import reference_py as rp
    from tests import oracle_bridge as ob
    from tests.tolerances import rel_K, rel_u, rel_x
    if solve is None:
        def solve(x, u):
            return ob.oracle_solve_like(prob, b, iterations=iterations, x_init=x, u_init=u, robot=name)
    x, u = start if start is not None else rp.cold_start(ob.model(name), ob.oracle_nodes(prob, b, robot=name), prob["x0"][b])
    xo, uo, Ko, st = solve(x, u)
    floor, merit, stable = np.zeros(3), 0.0, True
    for s in range(FLOOR_SAMPLES):
        x2, u2, K2, st2 = solve(x * (1.0 + 1e-15 * _signs(x.shape, s)), u * (1.0 + 1e-15 * _signs(u.shape, 100 + s)))
        floor = np.maximum(floor, [rel_x(x2, xo), rel_u(u2, uo), rel_K(K2, Ko)])
        merit = max(merit, abs(st2[iterations - 1][4] - st[iterations - 1][4]) / max(1.0, abs(st[iterations - 1][4])))
        stable = stable and np.array_equal(st2[:, 3], st[:, 3])
    return tuple(float(v) for v in floor), float(merit), bool(stable)
