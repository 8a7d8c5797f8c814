"""Cases of the run-time parameter tests (tests/test_wbc_params_capi.py, tests/test_gpu_wbc_params.py): parameter rows <-> the settings dict of
oracle/wbc_py.py, and a batch with a different row per robot whose rows are fixed on the CPU with the oracle alone, so that the per-robot
inequality data (torque limits, friction) is exercised."""
import numpy as np

from oracle import wbc_py as wp
from tests import oracle_bridge as ob
from tests.test_wbc import _case, _task, _tight

MODES = [3, 1, 2, 0, 3, 1, 2, 3]          # the batch of tests/test_wbc.py::test_hip_wbc_matches_oracle
STATE_SEED, ROW_SEED = 11, 407


def row_from_settings(st, nj):
    row = np.zeros(32)
    row[0:6], row[6:12] = st["base_kp"], st["base_kd"]
    row[12:19] = [st["swing_kp"], st["swing_kd"], st["w_swing"], st["w_base"], st["w_force"], st["friction"], st["contact_tolerance"]]
    row[19:19 + nj // 2] = st["torque_limits"]
    return row


def settings_from_row(row, nj):
    r = np.asarray(row, float)
    return dict(base_kp=r[0:6].copy(), base_kd=r[6:12].copy(), swing_kp=float(r[12]), swing_kd=float(r[13]), w_swing=float(r[14]), w_base=float(r[15]),
                w_force=float(r[16]), friction=float(r[17]), contact_tolerance=float(r[18]), torque_limits=r[19:19 + nj // 2].copy())


def default_row(robot):
    m = ob.model(robot)
    return row_from_settings(wp.load_settings(_task(robot), m["nj"]), m["nj"])


def torque_rows_tight(p, sol, nj):
    """indices j of the torque-limit rows (the first 2 nj rows of the oracle's D) that are tight at sol"""
    return sorted(i for i in _tight(p, sol) if i < 2 * nj)


def friction_rows_tight(p, sol, nj, mode):
    """tight pyramid rows that carry the friction coefficient (rows 1..4 of each stance contact's five; row 0 is the unilateral one)"""
    nst = sum(wp.mode_flags(mode))
    return sorted(i for i in _tight(p, sol) if 2 * nj <= i < 2 * nj + 5 * nst and (i - 2 * nj) % 5 != 0)


def random_rows(robot, B, seed=ROW_SEED):
    """a row per robot: gains and weights inside the ranges of the reference's reconfigure server (kp 0..500, kd 0..100, weights up to 100; the
    weights start at 0.01, the smallest weight of the shipped task.info files - a weight of 0 removes its task and with the contact-force task
    the only term that fixes the internal forces of a stance foot), friction and torque limits varied around the task.info values"""
    nj = ob.model(robot)["nj"]
    base = default_row(robot)
    rng = np.random.default_rng(seed)
    rows = np.tile(base, (B, 1))
    rows[:, 0:6] = rng.uniform(0.0, 500.0, (B, 6))
    rows[:, 6:12] = rng.uniform(0.0, 100.0, (B, 6))
    rows[:, 12] = rng.uniform(0.0, 500.0, B)
    rows[:, 13] = rng.uniform(0.0, 100.0, B)
    rows[:, 14:17] = rng.uniform(0.01, 100.0, (B, 3))
    rows[:, 17] = rng.uniform(0.5, 2.0, B) * base[17]
    rows[:, 19:19 + nj // 2] = rng.uniform(0.5, 1.5, (B, nj // 2)) * base[19:19 + nj // 2]
    return rows


def oracle_batch(robot):
    """(model, cases, rows [8, 32], b_torque, b_friction): the states of test_hip_wbc_matches_oracle with random_rows, then - with the oracle alone -
    robot b_torque gets a torque limit below the largest joint torque of its own solution and robot b_friction a friction coefficient below
    the largest tangential-to-normal force ratio of its own solution.  b_torque is the first robot, b_friction the one with the least vertical forces, for which the row then is active in the
    oracle's solution while no such row is active for the same state under the task.info values (asserted by the callers)."""
    m = ob.model(robot)
    nj, nv = m["nj"], 6 + m["nj"]
    st0 = wp.load_settings(_task(robot), nj)
    rng = np.random.default_rng(STATE_SEED)
    cases = [_case(m, md, rng, speed=0.4) for md in MODES]
    rows = random_rows(robot, len(MODES))
    solve = lambda st, b: wp.update(m, st, cases[b][0], cases[b][1], cases[b][2], MODES[b])      # noqa: E731
    b_torque = b_friction = None
    by_ratio = []
    for b in range(len(MODES)):
        s0, p0 = solve(st0, b)
        so, p = solve(settings_from_row(rows[b], nj), b)
        if p0["status"] != 0 or p["status"] != 0:
            continue
        if b_torque is None and not torque_rows_tight(p0, s0, nj) and not torque_rows_tight(p, so, nj):
            tau = so[nv + 12:]
            k = int(np.argmax(np.abs(tau)))
            trial = rows[b].copy()
            trial[19 + k % (nj // 2)] = 0.8 * abs(tau[k])
            s2, p2 = solve(settings_from_row(trial, nj), b)
            if p2["status"] == 0 and torque_rows_tight(p2, s2, nj):
                rows[b], b_torque = trial, b
                continue
        if MODES[b] != 0 and not friction_rows_tight(p0, s0, nj, MODES[b]) and not friction_rows_tight(p, so, nj, MODES[b]):
            F = so[nv:nv + 12].reshape(4, 3)
            by_ratio.append((max(max(abs(f[0]), abs(f[1])) / f[2] for f, fl in zip(F, wp.mode_flags(MODES[b])) if fl and f[2] > 1.0), b))
    for ratio, b in sorted(by_ratio, reverse=True):      # the least vertical planned forces first: the friction coefficient stays as large as it can
        trial = rows[b].copy()
        trial[17] = 0.7 * ratio
        s2, p2 = solve(settings_from_row(trial, nj), b)
        if p2["status"] == 0 and friction_rows_tight(p2, s2, nj, MODES[b]):
            rows[b], b_friction = trial, b
            break
    return m, cases, rows, b_torque, b_friction
