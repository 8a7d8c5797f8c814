"""Restatement of the dual solution of the SQP solve (include/bpmpc.h "Dual solution") in numpy: the costates by the adjoint recursion, the input
gradient of the Hamiltonian under the sweep's policy, the minimum-norm multipliers of the state-input equality rows with their gains, the two
certificates and the query.  Every function takes the number type to work in, so the same text runs in double and in np.longdouble (the yardstick
of the GPU tier): the products are done in that type; the pseudo-inverse is numpy's in double, followed by two steps of residual refinement in the
given type.  Host only; shared by tests/test_dual_solution_reference.py and tests/test_gpu_dual_solution.py.

One problem at a time: the LQ model as tests/value_function_reference.py takes it, C [n, 16, nx], D [n, 16, nu], nc [n] (rows in registration
order, 16 slots), K [n, nu, nx], dx [n + 1, nx], du [n, nu], kind [n] (1: event node), S [n + 1, nx, nx], s [n + 1, nx] of the value function."""
import numpy as np

from oracle import reference_py as rp
from tests import value_function_reference as vf

ROWS = 16
RCOND = 1e-6          # singular values of D below RCOND of the largest count as zero


def min_norm(D, G, dtype=np.float64):
    """X = -pinv(D') G: the solution of D'X = -G of least norm in every column (D [nc, nu], G [nu, m] -> [nc, m])."""
    pin = np.linalg.pinv(np.asarray(D, np.float64).T, rcond=RCOND).astype(dtype)
    D, G = np.asarray(D, dtype), np.asarray(G, dtype)
    X = -(pin @ G)
    for _ in range(2):
        X = X - pin @ (G + D.T @ X)
    return X


def costates(lq, K, dx, du, kind, dtype=np.float64):
    """lambda [n + 1, nx] by the adjoint recursion lambda_k = q + Q dx + P'du + A'lambda+ + K'g_u, g_u = r + P dx + R du + B'lambda+, from
    lambda_n = 0 (an event node: lambda_k = lambda+); and g_u [n, nu].  Neither S nor s enters."""
    n, nx = len(kind), np.shape(lq["A"])[1]
    lam, gu = np.zeros((n + 1, nx), dtype), np.zeros((n, np.shape(lq["R"])[1]), dtype)
    for k in range(n - 1, -1, -1):
        if kind[k] == 1:
            lam[k] = lam[k + 1]
            continue
        A, B, b, Q, R, P, q, r = (np.asarray(lq[name][k], dtype) for name in vf.LQ_NAMES[:-1])
        x, u, Kk = np.asarray(dx[k], dtype), np.asarray(du[k], dtype), np.asarray(K[k], dtype)
        gu[k] = r + P @ x + R @ u + B.T @ lam[k + 1]
        lam[k] = q + Q @ x + P.T @ u + A.T @ lam[k + 1] + Kk.T @ gu[k]
    return lam, gu


def node_dual(lq, D, nc, K, dx, du, S, s, k, dtype=np.float64):
    """(Hux [nu, nx], g0 [nu], N [16, nx], nu0 [16]) of the intermediate node k: the input gradient of the Hamiltonian under the sweep's policy,
    g_u(dx) = Hux dx + g0, and [N | nu0] = -pinv(D') [Hux | g0]; rows >= nc are zeros."""
    A, B, b, Q, R, P, q, r = (np.asarray(lq[name][k], dtype) for name in vf.LQ_NAMES[:-1])
    Kk = np.asarray(K[k], dtype)
    kappa = np.asarray(du[k], dtype) - Kk @ np.asarray(dx[k], dtype)
    Sp, sp = np.asarray(S[k + 1], dtype), np.asarray(s[k + 1], dtype)
    Acl, bcl = A + B @ Kk, b + B @ kappa
    Hux = P + R @ Kk + B.T @ (Sp @ Acl)
    g0 = r + R @ kappa + B.T @ (sp + Sp @ bcl)
    nx = A.shape[0]
    X = np.zeros((ROWS, nx + 1), dtype)
    if nc > 0:
        X[:nc] = min_norm(D[k][:nc], np.concatenate([Hux, g0[:, None]], axis=1), dtype)
    return Hux, g0, X[:, :nx], X[:, nx]


def dual_solution(lq, D, nc, K, dx, du, kind, S, s, dtype=np.float64):
    """dict of lambda [n + 1, nx] (adjoint recursion), nu_gain [n, 16, nx], nu0 [n, 16], nu [n, 16], residual [n], gain_residual [n], gnorm [n]
    (the largest |g_u(dx_k)|) and hux [n] (the largest |Hux|); event nodes are zeros."""
    n, nx = len(kind), np.shape(lq["A"])[1]
    lam, _ = costates(lq, K, dx, du, kind, dtype)
    out = dict(nu_gain=np.zeros((n, ROWS, nx), dtype), nu0=np.zeros((n, ROWS), dtype), nu=np.zeros((n, ROWS), dtype), residual=np.zeros(n, dtype),
               gain_residual=np.zeros(n, dtype), gnorm=np.zeros(n, dtype), hux=np.zeros(n, dtype))
    out["lambda"] = lam
    for k in range(n):
        if kind[k] == 1:
            continue
        Hux, g0, N, nu0 = node_dual(lq, D, nc[k], K, dx, du, S, s, k, dtype)
        x = np.asarray(dx[k], dtype)
        Dk = np.asarray(D[k], dtype)
        Dk = np.where(np.arange(ROWS)[:, None] < nc[k], Dk, 0)
        nu = nu0 + N @ x
        gu = Hux @ x + g0
        out["nu_gain"][k], out["nu0"][k], out["nu"][k] = N, nu0, nu
        out["residual"][k] = np.abs(gu + Dk.T @ nu).max()
        out["gain_residual"][k] = np.abs(Hux + Dk.T @ N).max()
        out["gnorm"][k], out["hux"][k] = np.abs(gu).max(), np.abs(Hux).max()
    return out


def x_stationarity(lq, C, K, dx, du, kind, lam, nu, k):
    """lambda_k - (q + Q dx + P'du + A'lambda+ + C'nu) of the intermediate node k: zero where D has full row rank (see the header's caveat)."""
    x, u = dx[k], du[k]
    return lam[k] - (lq["q"][k] + lq["Q"][k] @ x + lq["P"][k].T @ u + lq["A"][k].T @ lam[k + 1] + C[k].T @ nu[k])


def query(times, nu0, nu_gain, nc, x_lin, t, x):
    """(nu [16], rows) at (t, x): the rows of node i of the segment (reference_py.time_segment: an event time belongs to the interval that ends
    there; behind the last node: node n - 1) at delta = x - x_lin(t), x_lin interpolated as the value query interpolates it."""
    i, a = rp.time_segment(np.asarray(times), t)
    d = np.asarray(x) - (a * x_lin[i] + (1.0 - a) * x_lin[i + 1])
    return nu0[i] + nu_gain[i] @ d, int(nc[i])


def rank_classes(D, nc, mode, kind):
    """Per intermediate node (mode, nc, rank of D at RCOND) and the singular values relative to the largest, for the gap assertion."""
    classes, ratios = [], []
    for k in range(len(kind)):
        if kind[k] == 1 or nc[k] == 0:
            continue
        sv = np.linalg.svd(np.asarray(D[k][:nc[k]], np.float64), compute_uv=False)
        ratios.append(sv / sv[0])
        classes.append((int(mode[k]), int(nc[k]), int((sv > RCOND * sv[0]).sum())))
    return classes, np.concatenate(ratios)
