"""Restatement of the value function of the SQP solve (include/bpmpc.h "Value function") in numpy: the closed-loop terms of a node, the backward
recursion with its symmetrisation, the query, and the QP cost it is measured against.  Every function takes the number type to work in, so the
same text runs in double and in np.longdouble (the yardstick of the GPU tier).  Host only; shared by tests/test_value_function_reference.py and
tests/test_gpu_value_function.py.

One problem at a time: A, Q [n, nx, nx], B [n, nx, nu], R [n, nu, nu], P [n, nu, nx], b, q [n, nx], r [n, nu], c [n], K [n, nu, nx], dx [n + 1, nx],
du [n, nu], kind [n] (1: event node - identity jump with the stored b, no cost)."""
import numpy as np

from oracle import reference_py as rp

LQ_NAMES = ("A", "B", "b", "Q", "R", "P", "q", "r", "c")


def closed_loop_terms(lq, K, dx, du, kind, k, dtype=np.float64):
    """(Acl, bcl, Qcl, qcl, ccl) of node k under the sweep's policy du = K dx + kappa, kappa = du_k - K_k dx_k."""
    A, B, b, Q, R, P, q, r = (np.asarray(lq[n][k], dtype) for n in LQ_NAMES[:-1])
    nx = A.shape[0]
    if kind[k] == 1:
        return np.eye(nx, dtype=dtype), b, np.zeros((nx, nx), dtype), np.zeros(nx, dtype), dtype(0)
    c = dtype(lq["c"][k])
    Kk = np.asarray(K[k], dtype)
    kappa = np.asarray(du[k], dtype) - Kk @ np.asarray(dx[k], dtype)
    Acl = A + B @ Kk
    bcl = b + B @ kappa
    Qcl = Q + Kk.T @ (R @ Kk + P) + P.T @ Kk
    qcl = q + Kk.T @ r + (P.T + Kk.T @ R) @ kappa
    ccl = c + r @ kappa + dtype(0.5) * (kappa @ (R @ kappa))
    return Acl, bcl, Qcl, qcl, ccl


def value_recursion(lq, K, dx, du, kind, dtype=np.float64):
    """(S [n + 1, nx, nx], s [n + 1, nx], v [n + 1]) from V_n = 0; S_k symmetrised as computed."""
    n, nx = len(kind), np.shape(lq["A"])[1]
    S, s, v = np.zeros((n + 1, nx, nx), dtype), np.zeros((n + 1, nx), dtype), np.zeros(n + 1, dtype)
    half = dtype(0.5)
    for k in range(n - 1, -1, -1):
        Acl, bcl, Qcl, qcl, ccl = closed_loop_terms(lq, K, dx, du, kind, k, dtype)
        Sp, sp, vp = S[k + 1], s[k + 1], v[k + 1]
        Sk = Qcl + Acl.T @ (Sp @ Acl)
        S[k] = half * (Sk + Sk.T)
        Sb = Sp @ bcl
        s[k] = qcl + Acl.T @ (sp + Sb)
        v[k] = ccl + vp + sp @ bcl + half * (bcl @ Sb)
    return S, s, v


def value_at(S, s, v, k, d):
    return v[k] + s[k] @ d + 0.5 * (d @ (S[k] @ d))


def query(times, S, s, v, x_lin, t, x):
    """(f, dfdx, dfdxx) at (t, x): S, s, v and the expansion point interpolated on the node times (reference_py.time_segment: value = a v[i] +
    (1 - a) v[i + 1], t clamped to the span), re-centred with delta = x - x_lin(t)."""
    i, a = rp.time_segment(np.asarray(times), t)
    mix = lambda z: a * z[i] + (1.0 - a) * z[i + 1]
    St, st, vt, xt = mix(S), mix(s), mix(v), mix(x_lin)
    d = np.asarray(x) - xt
    Sd = St @ d
    return vt + st @ d + 0.5 * (d @ Sd), st + Sd, St


def stage_costs(lq, dx, du, kind):
    """The QP cost of every node at the step (dx, du): c + q'dx + r'du + dx'Q dx / 2 + du'R du / 2 + du'P dx (an event node costs nothing)."""
    n = len(kind)
    out = np.zeros(n)
    for k in range(n):
        if kind[k] == 1:
            continue
        x, u = dx[k], du[k]
        out[k] = lq["c"][k] + lq["q"][k] @ x + lq["r"][k] @ u + 0.5 * (x @ (lq["Q"][k] @ x)) + 0.5 * (u @ (lq["R"][k] @ u)) + u @ (lq["P"][k] @ x)
    return out


def tail_costs(lq, dx, du, kind):
    """[n + 1]: the cost of the nodes k .. n - 1 (summed from the end, as the recursion accumulates it); 0 at n."""
    c = stage_costs(lq, dx, du, kind)
    out = np.zeros(len(kind) + 1)
    for k in range(len(kind) - 1, -1, -1):
        out[k] = out[k + 1] + c[k]
    return out


def oracle_lq(om, nodes, x, u):
    """The LQ model of every node at the iterate (x, u) through oracle_py.OracleModel.node_lq, stacked per quantity."""
    n = int(nodes["N"])
    per = [om.node_lq(nodes["kind"][k], nodes["dt"][k], x[k], u[k], x[k + 1], nodes["xref"][k], nodes["mode"][k], nodes["zref"][k], nodes["zdref"][k])
           for k in range(n)]
    return {name: np.stack([np.asarray(p[name]) for p in per]) for name in LQ_NAMES}


def relative_distance(a, b):
    """Largest per-node distance of a from b relative to the node's largest |b| entry (nodes whose b is all zero: absolute)."""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    scale = np.abs(b).max(axis=1)
    scale[scale == 0] = 1
    return float((np.abs(a - b).max(axis=1) / scale).max())
