"""Cases for the edge tests of the per-problem kernel family (csrc/k_weights.hip: the kernels a handle launches once a weight row or a cone row has been
set), shared by tests/test_row_kernel_cases.py (CPU) and tests/test_gpu_row_kernel_edges.py.  Host only, no fixtures: numpy and the oracle.  Nothing is
built here that another case module has: the line-search cases are tests/linesearch_cases.py's (lc), the cone rows tests/cone_cases.py's (cc), the weight
variants tests/weight_cases.py's (wc), the robots with a real tree tests/tree_variants.py's (tv).  Oracle solves are cached; callers must not modify them.

  A  lc cases run on the row kernels under the model's rows (LS_CASES, FAMILY_CASE, WIDE_ROUNDS_CASE)
  B  the inputs of TAIL_CASE under a cone row (TAIL_CONE_ROWS) resp. a weight row (TAIL_WEIGHTS) per problem: every search goes through the
     back-tracking tail's own rounds, and the row decides the step or the merit (tail_conditions)
  C  table walks: BPMPC_LIN_TABLES=1 on the H1 / G1 problems of the weight tests under both kinds of rows (ROWS_H1, ROWS_G1); W12 / U10 / L46 under
     cone rows (TREE_CASES)
  D  the same H1 / G1 problems and the two-gait problem (ROWS_TWO_GAITS) under the other switches"""
import functools

import numpy as np

from tests import cone_cases as cc
from tests import linesearch_cases as lc
from tests import oracle_bridge as ob
from tests import tree_variants as tv
from tests import weight_cases as wc

# ---------------------------------------------------------------------------------------------------- A
LS_CASES = ("branches-armijo-d1-it3", "short1-armijo", "short3-defaults", "horizon121-armijo", "stagger", "g1", "openloong", "reject_all")
FAMILY_CASE = "branches-armijo-d1-it1"          # once through the cone table, once through the weight table: one family, the same bits
WIDE_ROUNDS_CASE = "branches-armijo-d1-it3"     # BPMPC_LS_WIDE_ROUNDS 1 and 3 against 2
WIDE_ROUNDS = (1, 3)

# ---------------------------------------------------------------------------------------------------- B
TAIL_CASE = "branches-armijo-d1-it1"
TAIL_CONE_ROWS = ("model", "mu03", "all", "bar1", "mu03", "all")      # of cc.ROWS, in problem order
TAIL_WEIGHTS = ("base", "pose4_force025", "joints01_vel3")            # of wc.VARIANTS, cycled over the six problems
TAIL_CONE_D = 1.0
# the distance of the measured state under the weight rows: the first of lc's steps (1.0, 0.5, 2.0 in that order) at which tail_conditions holds for
# every problem; test_row_kernel_cases.py asserts that it does at this value and not at the two before it (at 1.0 and at 0.5 problem 4 accepts its
# second trial under pose4_force025; at 2.0 the six problems take 4, 7, 3, 9, 3 and 3 trials)
TAIL_WEIGHT_D = 2.0
TAIL_WEIGHT_D_STEPS = (1.0, 0.5, 2.0)
MIN_TRIALS = 3                # rounds 0 and 1 are launches over all nodes at the default BPMPC_LS_WIDE_ROUNDS: from the third trial on the tail evaluates
MERIT_DIFFERENCE = 1e-6       # relative: three orders above the 1e-9 the device's merit is held to


def tail_weight_of(b):
    return TAIL_WEIGHTS[b % len(TAIL_WEIGHTS)]


@functools.lru_cache(maxsize=None)
def tail_inputs(d):
    """(case, problem with the measured state moved by d, warm starts) of TAIL_CASE; at d = 1.0 exactly lc.case_inputs(TAIL_CASE)."""
    c = lc.CASES[TAIL_CASE]
    if d == c["d"]:
        return lc.case_inputs(TAIL_CASE)
    prob = lc.problem(c["robot"], c["batch"], c["n_intervals"], c["gait"])
    warm = lc.warm_start(c["robot"], c["batch"], c["n_intervals"], c["gait"], lc.SEEDS.get(TAIL_CASE))
    return c, dict(prob, x0=lc.measured_state(prob["x0"], d)), warm


def padded_tail_warm(d):
    c, _, warm = tail_inputs(d)
    nx = warm[0][0].shape[1]
    wx, wu = np.zeros((len(warm), c["max_nodes"] + 1, nx)), np.zeros((len(warm), c["max_nodes"], nx))
    for b, (x, u) in enumerate(warm):
        wx[b, :x.shape[0]], wu[b, :u.shape[0]] = x, u
    return wx, wu


def _tail_solve(om, robot, d, b):
    c, prob, warm = tail_inputs(d)
    x, u = warm[b]
    return om.solve(ob.oracle_nodes(prob, b, robot=robot), prob["x0"][b], x, u, iterations=1, **lc.oracle_options(c["robot"], c["settings"]))


@functools.lru_cache(maxsize=None)
def tail_cone_solves(own=True):
    """Per problem the oracle's (x, u, K, record) of one iteration under the problem's cone row (own) or under the model's."""
    return [_tail_solve(cc.oracle_for("h1", cc.row("h1", r if own else "model")), "h1", TAIL_CONE_D, b) for b, r in enumerate(TAIL_CONE_ROWS)]


_WEIGHT_FILES = {}


def weight_files(robot, directory):
    """variant -> wc.write_variant(robot, variant, directory), once per robot (the first registration of a name with the oracle bridge holds)."""
    if robot not in _WEIGHT_FILES:
        _WEIGHT_FILES[robot] = {v: wc.write_variant(robot, v, directory) for v in wc.VARIANTS}
    return _WEIGHT_FILES[robot]


_TAIL_WEIGHT_SOLVES = {}


def tail_weight_solves(directory, own=True, d=None):
    """The same under the problem's weight row: the oracle of the variant's task file (own) or of variant `base`."""
    d = TAIL_WEIGHT_D if d is None else d
    if (own, d) not in _TAIL_WEIGHT_SOLVES:
        files = weight_files("h1", directory)
        names = [files[tail_weight_of(b) if own else "base"]["name"] for b in range(lc.CASES[TAIL_CASE]["batch"])]
        _TAIL_WEIGHT_SOLVES[own, d] = [_tail_solve(ob.oracle(n), n, d, b) for b, n in enumerate(names)]
    return _TAIL_WEIGHT_SOLVES[own, d]


def tail_conditions(own, model, plain):
    """What part B rests on, as a list of the conditions that do NOT hold (empty: all hold).  own / model: per problem the oracle's solve under the
    problem's row / the model's; plain[b]: problem b's row is the model's."""
    missed = []
    for b, ((_, _, _, rec), (_, _, _, rec_m)) in enumerate(zip(own, model)):
        r, m = lc.ran(rec), lc.ran(rec_m)
        if not (len(r) == 1 and r[0][10] >= MIN_TRIALS):
            missed.append(("trials", b, [int(q[10]) for q in r]))
        if not r[0][11] > lc.DECISION_MARGIN:
            missed.append(("margin", b, float(r[0][11])))
        if plain[b]:
            continue
        merit = abs(r[0][4] - m[0][4]) / abs(m[0][4])
        if not (r[0][3] != m[0][3] or merit > MERIT_DIFFERENCE):
            missed.append(("the row decides nothing", b, float(r[0][3]), float(merit)))
    return missed


# ---------------------------------------------------------------------------------------------------- C1, D: both kinds of rows together
ITERATIONS = 2
# (weight variants, cone rows) per problem.  H1: item 4 of the cone tests - problem 0 a weight row alone, problem 1 both, problem 2 a cone row alone
ROWS_H1 = (("joints01_vel3", "pose4_force025", "base"), ("model", "all", "mu03"))
ROWS_G1 = (("base", "pose4_force025"), ("mu03", "all"))
ROWS_TWO_GAITS = (("pose4_force025", "joints01_vel3"), ("all", "mu03"))      # H1, the problem of item 3 of the weight tests
CHUNKS = (2, 3, 7)


def both_rows_problem(which, itf):
    from bipedal_control_amd import scenarios as sc
    if which == "h1":
        return wc.h1_problem(itf)
    if which == "g1":
        return sc.trot_problem(itf, batch=2, n_intervals=wc.N_INTERVALS, gait_start=wc.GAIT_START)
    return sc.gait_sweep_problem(itf, ["trot", "standing_trot"], [(0.3, 0.0)], n_intervals=wc.N_INTERVALS)


def both_rows(which):
    return dict(h1=ROWS_H1, g1=ROWS_G1, two_gaits=ROWS_TWO_GAITS)[which]


_BOTH = {}


def both_rows_solves(which, prob, directory):
    """Per problem the oracle's two-iteration cold-start solve under its weight variant's task file with the cone entries of its cone row."""
    if which not in _BOTH:
        robot = "g1" if which == "g1" else "h1"
        files = weight_files(robot, directory)
        weights, cones = both_rows(which)
        _BOTH[which] = [cc.solve(prob, b, cc.row(files[w]["name"], c), ITERATIONS, robot=files[w]["name"]) for b, (w, c) in enumerate(zip(weights, cones))]
    return _BOTH[which]


# ---------------------------------------------------------------------------------------------------- C2, C3: robots with a real tree, cone rows
TREE_ROWS = ("model", "mu03", "all")
TREE_ITERATIONS = 3
# robot -> shape of tv.SHAPES.  W12 "mixed": nx = 24, three grids (the lineariser's per-grid mapping), all four contact modes; U10 "walk": nx = 22, one
# grid (the compact mapping); L46 "walk": the table-walk tail
TREE_CASES = {"W12": "mixed", "U10": "walk", "L46": "walk"}
# L46 from the cold start: under no row of cc.ROWS does any of the three problems of "walk" take more than two trials in any of three iterations - in no
# assignment of the rows to the problems, nor with problem 0's inputs three times over (search_l46_backtrack, first stage).  The tail's own rounds
# need a third trial, so the three problems are ONE problem's inputs three times over from a far iterate, as cc.backtrack_problem's:
# tests/far_iterates.far_iterate("L46", nodes of the problem, its x0, amp, seed).  From far iterates L46's oracle is decided by rounding even more than
# from the cold start (tv.FLOOR_CASES): over three iterations its own x and u move by 1e-2 .. 1 when the start moves by 1e-15 relative, and for most
# starts the step lengths move with them.  The case is the first hit of search_l46_backtrack (amplitudes, problems, seeds in that order) at which
# the FIRST iteration - linearised at the far iterate itself, which far_iterate keeps free of pivot ties - takes at least MIN_TRIALS trials under every
# row, no decision of any iteration lies within lc.DECISION_MARGIN of its threshold, no search gives up, and all eight samples of the floor accept
# the same step lengths under every row.  trials / steps: what the oracle does under (model, mu03, all) per iteration; floors (x, u) 1.2e-2 .. 1.5e-2.
# The three rows take the same decisions here and differ in x and u by less than that floor: this case holds the table-walk tail to nine searches of
# 6 .. 10 trials with exact step lengths; WHICH row a tail reads is part B's matter.
L46_BACKTRACK = dict(problem=2, amp=0.3, seed=11, trials=((6, 10, 9),) * 3, steps=((2.0 ** -5, 2.0 ** -9, 2.0 ** -8),) * 3)


def tree_problem(name, prob):
    """(problem, per problem (x, u) to start from or None = the cold start).  L46: see L46_BACKTRACK."""
    if name != "L46":
        return prob, None
    from tests import far_iterates as fi
    b = L46_BACKTRACK["problem"]
    nodes = ob.oracle_nodes(prob, b, robot=name)
    x, u, _ = fi.far_iterate(name, nodes, prob["x0"][b], L46_BACKTRACK["amp"], L46_BACKTRACK["seed"])
    same = dict(prob, x0=np.repeat(prob["x0"][b:b + 1], tv.BATCH, axis=0), targets=[prob["targets"][b]] * tv.BATCH)
    return same, [(x, u)] * tv.BATCH


_TREE = {}


def tree_solves(name, prob, start=None, rows=TREE_ROWS):
    """Per problem the oracle's solve of TREE_ITERATIONS iterations under the problem's cone row; (prob, start) = tree_problem(name, ...)."""
    if (name, rows) not in _TREE:
        _TREE[name, rows] = [cc.solve(prob, b, cc.row(name, r), TREE_ITERATIONS, *(start[b] if start else (None, None)), robot=name) for b, r in enumerate(rows)]
    return _TREE[name, rows]


_TREE_FLOOR = {}


def tree_solve_floor(name, prob, start, b):
    """tv.oracle_solve_floor with the oracle under problem b's cone row and from its start: what tv.FLOOR_CASES widens a tolerance to ten times of."""
    if (name, b) not in _TREE_FLOOR:
        _TREE_FLOOR[name, b] = tv.oracle_solve_floor(name, prob, b, TREE_ITERATIONS, start=start[b] if start else None,
                                                     solve=lambda x, u: cc.solve(prob, b, cc.row(name, TREE_ROWS[b]), TREE_ITERATIONS, x, u, robot=name))
    return _TREE_FLOOR[name, b]


def trials_of(solves):
    return tuple(tuple(int(r[10]) for r in lc.ran(rec)) for _, _, _, rec in solves)


def search_l46_backtrack(prob, amps=(0.1, 0.2, 0.3, 0.5, 1.0), seeds=range(12)):
    """The search behind L46_BACKTRACK.  First the cold start: every problem under every row of cc.ROWS (returns ("cold", b, row) on a hit - there is
    none).  Then far iterates, by the rule stated at L46_BACKTRACK.  Two minutes on the CPU; no test runs it."""
    from tests import far_iterates as fi
    name = "L46"
    for b in range(tv.BATCH):
        for r in cc.ROWS:
            if max(trials_of([cc.solve(prob, b, cc.row(name, r), TREE_ITERATIONS, robot=name)])[0]) >= MIN_TRIALS:
                return "cold", b, r
    for amp in amps:
        for b in range(tv.BATCH):
            nodes = ob.oracle_nodes(prob, b, robot=name)
            for seed in seeds:
                x, u, _ = fi.far_iterate(name, nodes, prob["x0"][b], amp, seed)
                try:
                    solves = [cc.solve(prob, b, cc.row(name, r), TREE_ITERATIONS, x, u, robot=name) for r in TREE_ROWS]
                except RuntimeError:      # the oracle refuses an iterate
                    continue
                records = [r for s in solves for r in lc.ran(s[3])]
                if min(t[0] for t in trials_of(solves)) < MIN_TRIALS or min(r[11] for r in records) <= lc.DECISION_MARGIN or min(r[3] for r in records) == 0.0:
                    continue
                if all(tv.oracle_solve_floor(name, prob, b, TREE_ITERATIONS, start=(x, u),
                                             solve=lambda xx, uu, r=r: cc.solve(prob, b, cc.row(name, r), TREE_ITERATIONS, xx, uu, robot=name))[2] for r in TREE_ROWS):
                    return dict(problem=b, amp=amp, seed=seed, trials=trials_of(solves), steps=tuple(tuple(cc.steps(s[3])) for s in solves))
    return None
