"""numpy restatement of the plant's joint model (include/bpmpc.h "Plant", joints; kernels/plant.h JOINT): the substep of
tests/plant_stiction_reference.py with a joint row per robot - armature on the diagonal of M, viscous damping and regularised Coulomb friction as
linearly implicit damping, end stops as an explicit spring with an implicit damper.  Dense matrices and a LAPACK solve, the rigid-body quantities
from oracle/wbc_py.py as there: no arithmetic is shared with the kernel.  With the neutral row every operation is the one
plant_stiction_reference.substep performs, in its order, so the two return the same bits (tests/test_plant_joint_reference.py)."""
import numpy as np

from oracle.wbc_py import contact_jacobian, contact_points, fk, mass_matrix, nonlinear_effects
from tests.plant_reference import DEFAULT_ROW, NC

STRIDE = 64
SLOTS = 12
ARMATURE, DAMPING, FRICTION, LOWER, UPPER, K_LIMIT, C_LIMIT, W_EPS = 0, 12, 24, 36, 48, 60, 61, 62
DEFAULT_W_EPS = 0.01


def neutral_row():
    """Ideal joints: the row every robot has until the joint model is used"""
    row = np.zeros(STRIDE)
    row[LOWER:LOWER + SLOTS], row[UPPER:UPPER + SLOTS] = -np.inf, np.inf
    row[K_LIMIT], row[C_LIMIT], row[W_EPS] = 1e4, 1e2, DEFAULT_W_EPS
    return row


def joint_row(nj, armature=0.0, damping=0.0, friction_loss=0.0, lower=-np.inf, upper=np.inf, k_limit=1e4, c_limit=1e2, w_eps=DEFAULT_W_EPS):
    """A row from per-joint values (a scalar for every joint, or nj values) and the three scalars"""
    row = neutral_row()
    for at, value in ((ARMATURE, armature), (DAMPING, damping), (FRICTION, friction_loss), (LOWER, lower), (UPPER, upper)):
        row[at:at + nj] = value
    row[K_LIMIT], row[C_LIMIT], row[W_EPS] = k_limit, c_limit, w_eps
    return row


def is_neutral(row, nj):
    """What the kernel's ballot decides: no armature, damping or friction, no finite limit on a joint the robot has"""
    row = np.asarray(row, float)
    return bool(np.all(row[ARMATURE:ARMATURE + nj] == 0.0) and np.all(row[DAMPING:DAMPING + nj] == 0.0) and np.all(row[FRICTION:FRICTION + nj] == 0.0)
                and np.all(row[LOWER:LOWER + nj] == -np.inf) and np.all(row[UPPER:UPPER + nj] == np.inf))


def substep(m, q, v, cmd, h, joints=None, kt=0.0, anchor=None, anchored=None, params=None, ground=None, w_ext=None, torque_limits=None,
            solve=np.linalg.solve):
    """One substep of length h from (q, v) with the joint row `joints` [64] (None: the neutral row).  The other arguments and the returned keys are
    those of plant_stiction_reference.substep; beside them tau_lim [nj] (the end-stop torque), c_joint [nj] (the passive damping of each joint) and
    beyond [nj] (whether the joint is past a limit)."""
    par = DEFAULT_ROW if params is None else np.asarray(params, float)
    kn, cn, d0, mu, veps = par[:5]
    nj = m["nj"]
    row = neutral_row() if joints is None else np.asarray(joints, float)
    modelled = not is_neutral(row, nj)
    q, v = np.asarray(q, float), np.asarray(v, float)
    anchor = np.zeros((NC, 2)) if anchor is None else np.array(anchor, float)
    anchored = np.zeros(NC, np.int32) if anchored is None else np.array(anchored, np.int32)
    M = mass_matrix(m, q)
    if modelled:
        M = M + np.diag(np.concatenate([np.zeros(6), row[ARMATURE:ARMATURE + nj]]))      # the M of both sides
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
    tau_lim, c_joint, beyond = np.zeros(nj), np.zeros(nj), np.zeros(nj, bool)
    if modelled:
        w_eps = row[W_EPS] if row[W_EPS] > 0.0 else DEFAULT_W_EPS
        pen_up = np.maximum(q[6:] - row[UPPER:UPPER + nj], 0.0)
        pen_lo = np.maximum(row[LOWER:LOWER + nj] - q[6:], 0.0)
        tau_lim = row[K_LIMIT] * (pen_lo - pen_up)
        beyond = (pen_up > 0.0) | (pen_lo > 0.0)
        c_joint = row[DAMPING:DAMPING + nj] + row[FRICTION:FRICTION + nj] / np.sqrt(v[6:] ** 2 + w_eps ** 2) + np.where(beyond, row[C_LIMIT], 0.0)
        gen[6:] += tau_lim      # outside the clamp: the end stop is not the actuator
        A = M + h * (J.T * D) @ J + h * np.diag(np.concatenate([np.zeros(6), kd + c_joint]))
    else:
        A = M + h * (J.T * D) @ J + h * np.diag(np.concatenate([np.zeros(6), kd]))
    rhs = M @ v + h * gen
    vp = solve(A, rhs)
    force = f - (D * (J @ vp)).reshape(NC, 3)
    force[~closed] = 0.0
    return dict(q=q + h * vp, v=vp, a=(vp - v)[0:3] / h, d=d, n=n, closed=closed, force=force, spring=float(f[:, 2].sum()), A=A, rhs=rhs,
                anchor=anchor, anchored=anchored, stick=stick, phi=phi, cap=cap, p=p, J=J, D=D, tau_lim=tau_lim, c_joint=c_joint, beyond=beyond)
