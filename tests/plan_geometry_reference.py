"""numpy restatement of the plan geometry (include/bpmpc.h "Plan geometry"; csrc/kernels/plan_geometry.h): the node rows, the centre of pressure,
the future footholds and the summary row of ONE robot, in the order the header states for every sum.  The kinematics are oracle/wbc_py.py
fk / contact_points.

  rows(m, t, x, mode, kind, u)     [n + 1, 24]; x may hold the node references instead (the desired block: u = None, the caller drops row n)
  footholds(rows, n)               (entries [count, 6], count): every entry, the caller compares the first 16
  summary(rows, n, count)          [16]
  plan(m, t, x, mode, kind, u)     the three of them
"""
import numpy as np

from oracle import wbc_py as wp

STRIDE, MAX_FOOTHOLDS, FOOTHOLD_STRIDE, SUMMARY_STRIDE = 24, 16, 6, 16
BASE, CONTACT, COP, TIME, MODE, KIND, SUM_Z, MASK, BAD = 0, 3, 15, 18, 19, 20, 21, 22, 23
S_NODES, S_FOOTHOLDS, S_PATH, S_APEX, S_DRIFT, S_MIN_SUM_Z, S_BAD = 0, 1, 2, 3, 7, 11, 12
LANES = 64


def contact_flag(mode, i):
    """contact_flag of reference_gen.h: points 0, 1 the left foot (LF 1, STANCE 3), points 2, 3 the right foot (RF 2, STANCE 3)"""
    return mode in (1, 3) if i < 2 else mode in (2, 3)


def contact_mask(mode):
    return sum(1 << i for i in range(4) if contact_flag(mode, i))


def cop(fz, p):
    """(centre of pressure [3], sum_z): sum_z = ((fz0 + fz1) + fz2) + fz3; ((w0 p0 + w1 p1) + w2 p2) + w3 p3 with w_i = fz_i / sum_z"""
    sum_z = ((fz[0] + fz[1]) + fz[2]) + fz[3]
    if not sum_z > 0.0:
        return np.zeros(3), sum_z
    w = [f / sum_z for f in fz]
    return ((w[0] * p[0] + w[1] * p[1]) + w[2] * p[2]) + w[3] * p[3], sum_z


def rows(m, t, x, mode, kind, u=None):
    nj = m["nj"]
    n = len(t) - 1
    out = np.zeros((n + 1, STRIDE))
    for k in range(n + 1):
        r = out[k]
        q = np.array(x[k][6:12 + nj], float)
        bad = not np.all(np.isfinite(x[k]))
        r[BASE:BASE + 3] = q[0:3]
        if bad:
            r[CONTACT:CONTACT + 12] = np.nan      # unspecified: the caller compares the flag only
        else:
            R, o, _ = wp.fk(m, q)
            r[CONTACT:CONTACT + 12] = np.array(wp.contact_points(m, R, o)).reshape(-1)
        last = k == n
        md, kd = (-1, -1) if last else (int(mode[k]), int(kind[k]))
        if u is not None and not last and not bad:
            r[COP:COP + 3], r[SUM_Z] = cop([u[k][3 * i + 2] for i in range(4)], r[CONTACT:CONTACT + 12].reshape(4, 3))
        elif u is not None and not last:
            r[SUM_Z] = cop([u[k][3 * i + 2] for i in range(4)], np.zeros((4, 3)))[1]
        r[TIME], r[MODE], r[KIND], r[MASK], r[BAD] = t[k], md, kd, contact_mask(md), float(bad)
    return out


def landing_mask(rw, k, n):
    if rw[k, KIND] != 1.0 or not (rw[0, TIME] < rw[k, TIME] < rw[n, TIME]):
        return 0
    before = [j for j in range(k - 1, -1, -1) if rw[j, KIND] == 0.0]
    after = [j for j in range(k + 1, n) if rw[j, KIND] == 0.0]
    if not before or not after:
        return 0
    return ~contact_mask(int(rw[before[0], MODE])) & contact_mask(int(rw[after[0], MODE]))


def footholds(rw, n):
    out = []
    for k in range(n + 1):
        land = landing_mask(rw, k, n)
        for i in range(4):
            if (land >> i) & 1:
                post = rw[k + 1]
                out.append([post[TIME], i, *post[CONTACT + 3 * i:CONTACT + 3 * i + 3], k + 1])
    return np.array(out, float).reshape(-1, FOOTHOLD_STRIDE), len(out)


def summary(rw, n, count):
    """64 accumulators, node k into accumulator k mod 64 with k ascending; the path length summed over the accumulators 0 .. 63"""
    path = np.zeros(LANES)
    apex, drift, min_sum_z, bad = np.full(4, -np.inf), np.zeros(4), np.inf, 0
    for k in range(n + 1):
        r = rw[k]
        if r[BAD] != 0.0:
            bad += 1
            continue
        for i in range(4):
            if r[CONTACT + 3 * i + 2] > apex[i]:
                apex[i] = r[CONTACT + 3 * i + 2]
        if r[KIND] == 0.0 and r[MASK] != 0.0 and r[SUM_Z] < min_sum_z:
            min_sum_z = r[SUM_Z]
        if k >= n or rw[k + 1, BAD] != 0.0:
            continue
        s = rw[k + 1]
        d = s[0:3] - r[0:3]
        path[k % LANES] += np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        both = int(r[MASK]) & int(s[MASK])
        for i in range(4):
            if (both >> i) & 1:
                e = s[CONTACT + 3 * i:CONTACT + 3 * i + 2] - r[CONTACT + 3 * i:CONTACT + 3 * i + 2]
                drift[i] = max(drift[i], np.sqrt(e[0] * e[0] + e[1] * e[1]))
    total = 0.0
    for lane in range(LANES):
        total += path[lane]
    out = np.zeros(SUMMARY_STRIDE)
    out[S_NODES], out[S_FOOTHOLDS], out[S_PATH] = n, count, total
    out[S_APEX:S_APEX + 4] = np.where(np.isinf(apex), 0.0, apex)
    out[S_DRIFT:S_DRIFT + 4] = drift
    out[S_MIN_SUM_Z] = 0.0 if np.isinf(min_sum_z) else min_sum_z
    out[S_BAD] = bad
    return out


def plan(m, t, x, mode, kind, u=None):
    """(rows [n + 1, 24], foothold entries [count, 6], count, summary [16])"""
    rw = rows(m, t, x, mode, kind, u)
    n = len(t) - 1
    entries, count = footholds(rw, n)
    return rw, entries, count, summary(rw, n, count)
