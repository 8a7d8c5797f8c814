"""numpy restatement of the plant's stick-slip contacts (include/bpmpc.h "Plant", step 2 with kt > 0; kernels/plant.h STICK): the substep of
tests/plant_reference.py with a tangential anchor spring per contact point, capped at mu n.  Dense matrices and a LAPACK solve, the rigid-body
quantities from oracle/wbc_py.py as there: no arithmetic is shared with the kernel.  With kt = 0 every operation is the one plant_reference.substep
performs, in its order, so the two return the same bits (tests/test_plant_stiction_reference.py)."""
import numpy as np

from oracle.wbc_py import contact_jacobian, contact_points, fk, mass_matrix, nonlinear_effects
from tests.plant_reference import DEFAULT_ROW, NC


def no_anchors():
    """(anchor [4, 2], anchored [4]) of a robot that has none"""
    return np.zeros((NC, 2)), np.zeros(NC, np.int32)


def substep(m, q, v, cmd, h, kt=0.0, anchor=None, anchored=None, params=None, ground=None, w_ext=None, torque_limits=None, solve=np.linalg.solve):
    """One substep of length h from (q, v) and the anchors (anchor [4, 2] world xy, anchored [4]; None: none).  The other arguments and the
    returned keys are those of plant_reference.substep; beside them anchor, anchored (after the substep), stick [4] (1: sticking, 0: slipping,
    -1: open or kt = 0), phi and cap [4] (the spring force before the clamp and the Coulomb cap mu n the stick / slip decision compared; 0 where
    stick is -1), p [4, 3] (the contact points), J and D (the contact Jacobian and the damping of its rows)."""
    par = DEFAULT_ROW if params is None else np.asarray(params, float)
    kn, cn, d0, mu, veps = par[:5]
    nj = m["nj"]
    q, v = np.asarray(q, float), np.asarray(v, float)
    anchor = np.zeros((NC, 2)) if anchor is None else np.array(anchor, float)
    anchored = np.zeros(NC, np.int32) if anchored is None else np.array(anchored, np.int32)
    M = mass_matrix(m, q)
    nle = nonlinear_effects(m, q, v)
    J = contact_jacobian(m, q)
    R, o, _ = fk(m, q)
    p = np.array(contact_points(m, R, o))
    c = (J @ v).reshape(NC, 3)
    g = np.zeros(NC) if ground is None else np.asarray(ground, float)
    d = g - p[:, 2]
    closed = d > 0.0
    f = np.zeros((NC, 3))
    D = np.zeros(3 * NC)
    n = np.zeros(NC)
    stick = np.full(NC, -1)
    phi, cap = np.zeros(NC), np.zeros(NC)
    for i in range(NC):
        if not closed[i]:
            if kt > 0.0:
                anchored[i] = 0
            continue
        f[i, 2] = kn * d[i]
        cni = cn * min(1.0, d[i] / d0)
        n[i] = max(0.0, kn * d[i] - cni * c[i, 2])
        speed = np.sqrt(c[i, 0] ** 2 + c[i, 1] ** 2 + veps ** 2)
        if kt > 0.0:
            if not anchored[i]:
                anchor[i], anchored[i] = p[i, :2], 1
            s = anchor[i] - p[i, :2]
            phi[i], cap[i] = kt * np.hypot(s[0], s[1]), mu * n[i]
            stick[i] = 0 if phi[i] > cap[i] else 1
            if not stick[i]:      # slip: the anchor is dragged to the cap; nothing is left for the damper and the spring is explicit
                anchor[i] = p[i, :2] + s * (cap[i] / phi[i]) if cap[i] > 0.0 else p[i, :2]
                s = anchor[i] - p[i, :2]
            f[i, :2] = kt * s
            ct = (cap[i] - kt * np.hypot(s[0], s[1])) / speed + h * kt if stick[i] else 0.0
        else:
            ct = mu * n[i] / speed
        D[3 * i:3 * i + 3] = [ct, ct, cni]
    kp, kd = np.asarray(cmd["kp"], float), np.asarray(cmd["kd"], float)
    tau = kp * (np.asarray(cmd["pos_des"], float) - q[6:]) + np.asarray(cmd["tau_ff"], float)
    if torque_limits is not None:
        lim = np.tile(np.asarray(torque_limits, float), 2)
        lim = np.where(lim > 0.0, lim, np.inf)
        tau = np.clip(tau, -lim, lim)
    gen = -nle + J.T @ f.reshape(-1)
    gen[6:] += tau + kd * np.asarray(cmd["vel_des"], float)
    if w_ext is not None:
        gen[0:3] += np.asarray(w_ext, float)
    A = M + h * (J.T * D) @ J + h * np.diag(np.concatenate([np.zeros(6), kd]))
    rhs = M @ v + h * gen
    vp = solve(A, rhs)
    force = f - (D * (J @ vp)).reshape(NC, 3)
    force[~closed] = 0.0
    return dict(q=q + h * vp, v=vp, a=(vp - v)[0:3] / h, d=d, n=n, closed=closed, force=force, spring=float(f[:, 2].sum()), A=A, rhs=rhs,
                anchor=anchor, anchored=anchored, stick=stick, phi=phi, cap=cap, p=p, J=J, D=D)
