"""Cases that make the WBC's active-set QP (csrc/kernels/wbc.h) work hard, labelled with the oracle alone (numpy, no GPU): populations of 32 robots,
modes [3, 1, 2, 0] cycling, one parameter row per robot, deterministic by seed.  Shared by tests/test_wbc_stress_cases.py (CPU: the populations
contain what the GPU assertions rely on) and tests/test_gpu_wbc_stress.py.

  pull     task.info settings, planned contact forces x -0.5, speed 0.4: double stance needs about 20 to 30 KKT solves
  both     torque limits x 0.08, friction x 0.1, speed 1.0
  zeroF    torque limits x 0.08, friction x 0.2, planned forces x 0, speed 1.0
  lowtau   torque limits x 0.05, speed 0.4
  mixed    robot b is robot b of population (pull, both, zeroF, lowtau)[(b // 4) % 4]: successes and fallbacks interleaved, every mode from each

Labels (oracle/wbc_py.py:solve_qp with a trace; the device allows 20 working-set changes = 21 KKT solves):
  A  solved within 21 iterations           B  solved, 22 iterations or more (the device must fall back: change budget)
  C  WorkingSetInconsistent                D  RuntimeError: the add / drop rule cycles (the device must fall back: change budget)
  E  the equalities themselves are inconsistent (does not occur in these populations; asserted)
A robot is decisive if every add / drop of its trace wins by more than 1e-6 relative to max(1, |value|) and no termination test (violation
> tol, multiplier < -tol, tol = 1e-9) lies within a factor 100 of tol: only then are the device's iteration count and working set required to
equal the oracle's."""
import functools

import numpy as np

from oracle import wbc_py as wp
from tests import oracle_bridge as ob
from tests import wbc_params_cases as wc
from tests.test_wbc import _case, _task

B = 32
MODES = [3, 1, 2, 0] * (B // 4)
CAP = 21                                   # KKT solves the device allows: kWbcMaxWorkingSetChanges + 1
TOL, MARGIN, WIN = 1e-9, 100.0, 1e-6
# population -> (factor of the torque limits, of the friction coefficient, of the planned contact forces, speed of tests/test_wbc.py::_case)
POPULATIONS = {"pull": (1.0, 1.0, -0.5, 0.4), "both": (0.08, 0.1, 1.0, 1.0), "zeroF": (0.08, 0.2, 0.0, 1.0), "lowtau": (0.05, 1.0, 1.0, 0.4)}
MIXED_ORDER = ("pull", "both", "zeroF", "lowtau")
ROBOT_POPULATIONS = {"h1": MIXED_ORDER, "g1": MIXED_ORDER, "hunter": ("both", "pull"), "openloong": ("both", "pull")}
# searched on the CPU with the oracle until the conditions of tests/test_wbc_stress_cases.py held (the counts are written there); seeds whose
# population has a cycling robot (D: 400 oracle iterations) were passed over where another served, to keep the oracle's share short
SEEDS = {("h1", "pull"): 2, ("h1", "both"): 1, ("h1", "zeroF"): 1, ("h1", "lowtau"): 1,
         ("g1", "pull"): 0, ("g1", "both"): 1, ("g1", "zeroF"): 1, ("g1", "lowtau"): 6,
         ("hunter", "both"): 3, ("openloong", "both"): 1, ("openloong", "pull"): 0,
         # Hunter's feet are lines (both contact points of a foot at y = 0), and under "pull" the lateral pyramid rows of heel and toe tie to 1e-13:
         # one stream gives 7 to 12 non-decisive robots of 32 with every seed from 0 to 67.  So this population has a seed per robot:
         # robot b takes 100 b + k with the smallest k >= 0 whose robot is decisive.
         ("hunter", "pull"): (0, 100, 201, 300, 400, 500, 600, 700, 800, 900, 1000, 1100, 1202, 1300, 1400, 1500, 1600, 1700, 1803, 1900, 2002,
                              2100, 2200, 2300, 2405, 2500, 2600, 2700, 2802, 2900, 3000, 3100)}
BENIGN_SEEDS = (901, 902)                  # the seeding tick and the recovery tick: _case at speed 0.3 under the task.info settings


def stress_row(robot, name):
    nj = ob.model(robot)["nj"]
    row = wc.default_row(robot)
    tl, fr, _, _ = POPULATIONS[name]
    row[19:19 + nj // 2] *= tl
    row[17] *= fr
    return row


def decisive(trace):
    for e in trace:
        if e["decision"] == "inconsistent":
            continue
        v, mu = e["viol"], e["mu"]
        if TOL / MARGIN < v <= TOL * MARGIN:                                   # the "violated" test
            return False
        if e["decision"] == "add":
            if not v - e["viol_second"] > WIN * max(1.0, abs(v)):
                return False
            continue
        if np.isfinite(mu) and -TOL * MARGIN <= mu < -TOL / MARGIN:           # the "negative multiplier" test
            return False
        if e["decision"] == "drop" and not e["mu_second"] - mu > WIN * max(1.0, abs(mu)):
            return False
    return True


def solve(m, st, case, mode):
    """dict(label, iters, decisive, x, p, work (final working set in the device's row numbering), trace) of one robot."""
    p = wp.formulate(m, st, case[0], case[1], case[2], mode)
    H = p["Aw"].T @ p["Aw"]
    g = -p["Aw"].T @ p["bw"]
    p.update(H=H, g=g)
    trace = []
    out = dict(p=p, trace=trace, x=None, work=None)
    try:
        x, mult, work, iters = wp.solve_qp(H, g, p["Aeq"], p["beq"], p["D"], p["f"], trace=trace)
        # without the opposite pairs the oracle's rows are the device's: 2 nj torque rows, 5 pyramid rows per stance contact
        out.update(label="A" if iters <= CAP else "B", x=x, work=sorted(trace[-1]["work"]))
    except wp.WorkingSetInconsistent:
        out.update(label="C")
    except wp.Infeasible:
        out.update(label="E")
    except RuntimeError:
        out.update(label="D")
    out.update(iters=len(trace), decisive=decisive(trace))
    return out


def _cases(robot, name, seed):
    m = ob.model(robot)
    _, _, force, speed = POPULATIONS[name]
    rng = None if isinstance(seed, tuple) else np.random.default_rng(seed)      # one stream for the population, or a seed per robot
    cases = []
    for b, md in enumerate(MODES):
        x, u, rbd, q, v = _case(m, md, rng or np.random.default_rng(seed[b]), speed=speed)
        u = u.copy()
        u[:12] *= force
        cases.append((x, u, rbd))
    return cases


@functools.lru_cache(maxsize=None)
def population(robot, name, seed=None):
    """dict(robot, name, m, modes, cases [(x, u, rbd)], rows [B, 32], sols [solve(...)]); callers do not modify it."""
    if name == "mixed":
        parts = [population(robot, k) for k in MIXED_ORDER]
        pick = [parts[(b // 4) % 4] for b in range(B)]
        return dict(robot=robot, name=name, m=parts[0]["m"], modes=MODES, cases=[pp["cases"][b] for b, pp in enumerate(pick)],
                    rows=np.array([pp["rows"][b] for b, pp in enumerate(pick)]), sols=[pp["sols"][b] for b, pp in enumerate(pick)])
    m = ob.model(robot)
    seed = SEEDS[(robot, name)] if seed is None else seed
    cases = _cases(robot, name, seed)
    row = stress_row(robot, name)
    st = wc.settings_from_row(row, m["nj"])
    return dict(robot=robot, name=name, m=m, modes=MODES, cases=cases, rows=np.tile(row, (B, 1)), sols=[solve(m, st, c, md) for c, md in zip(cases, MODES)])


def benign_cases(robot, which):
    """the inputs of a tick every robot solves: task.info settings, speed 0.3"""
    rng = np.random.default_rng(BENIGN_SEEDS[which])
    return [_case(ob.model(robot), md, rng, speed=0.3)[:3] for md in MODES]


@functools.lru_cache(maxsize=None)
def benign(robot, which):
    """(benign_cases, their oracle records)"""
    m = ob.model(robot)
    st = wc.settings_from_row(wc.default_row(robot), m["nj"])
    cases = benign_cases(robot, which)
    return cases, [solve(m, st, c, md) for c, md in zip(cases, MODES)]


def counts(pop):
    s = pop["sols"]
    c = {k: sum(x["label"] == k for x in s) for k in "ABCDE"}
    c["nondecisive"] = sum(not x["decisive"] for x in s)
    c["A12"] = sum(x["label"] == "A" and x["decisive"] and x["iters"] >= 12 for x in s)
    c["at21"] = sum(x["label"] == "A" and x["decisive"] and x["iters"] == CAP for x in s)
    c["at22"] = sum(x["label"] == "B" and x["decisive"] and x["iters"] == CAP + 1 for x in s)
    return c


# ------------------------------------------------------------------------------------------------- the KKT statement of the GPU tier
def split_rows(p):
    """(E, e, D, f) of the oracle's QP with the opposite pairs of D as the equalities they amount to and its all-zero rows left out"""
    D, f = p["D"], p["f"]
    pairs, used = [], set()
    for i in range(len(D)):
        for j in range(i + 1, len(D)):
            if i not in used and j not in used and np.array_equal(D[i], -D[j]) and f[i] == -f[j] and np.abs(D[i]).max() > 0.0:
                pairs.append(i); used |= {i, j}
    keep = [i for i in range(len(D)) if i not in used and np.abs(D[i]).max() > 0.0]
    return np.vstack([p["Aeq"], D[pairs]]), np.concatenate([p["beq"], f[pairs]]), D[keep], f[keep]


def tight(D, f, x, tol=1e-7):
    return set(np.nonzero(np.abs(D @ x - f) < tol)[0].tolist())


def nnls(M, r, iters=200):
    """min |M lam - r|, lam >= 0 (Lawson and Hanson's active-set method, dense, for a handful of columns)"""
    n = M.shape[1]
    lam, P = np.zeros(n), np.zeros(n, bool)
    for _ in range(iters):
        w = M.T @ (r - M @ lam)
        if P.all() or w[~P].max() <= 1e-12 * max(1.0, np.abs(M.T @ r).max()):
            break
        P[np.argmax(np.where(P, -np.inf, w))] = True
        while True:
            s = np.zeros(n)
            s[P] = np.linalg.lstsq(M[:, P], r, rcond=None)[0]
            if s[P].min() > 0.0:
                break
            neg = P & (s <= 0.0)
            alpha = (lam[neg] / (lam[neg] - s[neg])).min()
            lam = lam + alpha * (s - lam)
            P &= lam > 1e-14
        lam = s
    return lam


def assert_kkt(p, x, tag):
    """x is a KKT point of the oracle's QP p, by the tolerances of tests/test_wbc.py::test_hip_wbc_matches_oracle: equalities and inequalities to
    1e-7, stationarity on the tight set by least squares to 1e-6 max(1, |g|) - and the least-squares multipliers of the tight inequality rows
    are >= -1e-6 max(1, |g|).  The opposite pairs of the no-contact-motion task count as the equalities they amount to (their two least-squares
    multipliers have opposite signs by construction) and the all-zero rows of swing contacts carry no multiplier.  Where the tight rows are
    linearly dependent - the apex of a friction pyramid, F = 0, has five tight rows in three dimensions; the pull and zeroF populations sit
    there - the multipliers are not unique and the minimum-norm ones of least squares are negative at the oracle's own optimum (to -0.3); the
    statement is then the one they stand for: non-negative multipliers exist that make the point stationary to the same 1e-6 max(1, |g|).
    Returns (stationarity, smallest multiplier), relative to max(1, |g|)."""
    assert np.abs(p["Aeq"] @ x - p["beq"]).max(initial=0.0) < 1e-7 and (p["D"] @ x - p["f"]).max() < 1e-7, tag
    E, e, D, f = split_rows(p)
    rows = sorted(tight(D, f, x))
    Ga = np.vstack([E, D[rows]])
    grad = p["H"] @ x + p["g"]
    lam = np.linalg.lstsq(Ga.T, -grad, rcond=None)[0]
    scale = max(1.0, np.abs(p["g"]).max())
    stat = np.abs(grad + Ga.T @ lam).max() / scale
    assert stat < 1e-6, (tag, stat)
    mu = lam[len(E):].min() / scale if rows else 0.0
    if mu < -1e-6:
        assert np.linalg.matrix_rank(Ga) < len(Ga), (tag, mu, rows)          # unique multipliers, one of them negative: not a minimiser
        # the equalities' multipliers are free: project them out
        Q = np.linalg.svd(E, full_matrices=True)[2][np.linalg.matrix_rank(E):].T if len(E) else np.eye(len(x))
        M, r = Q.T @ D[rows].T, -Q.T @ grad
        mu_pos = nnls(M, r)
        stat = np.abs(M @ mu_pos - r).max() / scale
        assert stat < 1e-6, (tag, "no non-negative multipliers", stat, mu)
        mu = mu_pos.min() / scale
    return stat, mu


# ------------------------------------------------------------------------------------------------- equality-consistency threshold
EQ_SEED = 5
EQ_EPS = tuple(10.0 ** e for e in np.arange(-9.5, 3.0, 0.5))


@functools.lru_cache(maxsize=None)
def equality_blend():
    """H1 double stance with the measured velocity v_c + eps (v - v_c), v_c = consistent_measured_state(v): (cases, eps, residual) with the
    oracle's relative residual of the equality rows at the empty working set (the number solve_qp compares with FEAS_TOL)."""
    m = ob.model("h1")
    st = wp.load_settings(_task("h1"), m["nj"])
    x, u, rbd, q, v = _case(m, 3, np.random.default_rng(EQ_SEED), consistent=False)
    vc = wp.consistent_measured_state(m, q, v, 3)
    cases, res = [], []
    for eps in EQ_EPS:
        c = (x, u, wp.rbd_from(m, q, vc + eps * (v - vc)))
        cases.append(c)
        res.append(solve(m, st, c, 3)["trace"][0]["residual"])
    return cases, np.array(EQ_EPS), np.array(res)
