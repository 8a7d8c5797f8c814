"""numpy restatement of the batched rigid-body plant (include/bpmpc.h "Plant"; kernels/plant.h): one substep with dense matrices and a LAPACK
solve, and the sensor block.  The rigid-body quantities come from oracle/wbc_py.py - the mass matrix from its definition, the nonlinear effects
from the Lagrangian by complex-step derivatives, the contact Jacobian as the derivative of the contact positions - so that the restatement shares
no arithmetic with the kernel's recursive pass.  One substep costs about 70 ms here (the complex-step derivatives): tests run a few dozen at most."""
import numpy as np

from oracle.wbc_py import contact_jacobian, contact_points, euler_rate_map, fk, mass_matrix, nonlinear_effects, rbd_from, rot_zyx

GRAVITY = 9.81
NC = 4
PARAM_NAMES = ("kn", "cn", "d0", "mu", "v_eps", "contact_threshold")
DEFAULT_ROW = np.array([5e4, 5e2, 1e-3, 0.7, 0.01, 1.0, 0.0, 0.0])


def cholesky_solve(A, b):
    """A x = b through A = L L' (the kernel's method, LAPACK's arithmetic): the second solver of the tests that measure the restatement's own floor."""
    L = np.linalg.cholesky(A)
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def substep(m, q, v, cmd, h, params=None, ground=None, w_ext=None, torque_limits=None, solve=np.linalg.solve):
    """One substep of length h from (q, v).  cmd: dict of pos_des, vel_des, tau_ff, kp, kd [nj].  ground [4] (None: 0), w_ext [3] (None: 0),
    torque_limits [nj / 2] (None or <= 0: no limit).  Returns a dict: q, v (the new state), a (base linear acceleration (v+ - v)[0:3] / h), d
    (penetrations), n (start-of-step normal forces), closed, force [4, 3] (spring force minus the implicit damping force), spring (summed spring
    force), A and rhs of the linear system."""
    par = DEFAULT_ROW if params is None else np.asarray(params, float)
    kn, cn, d0, mu, veps = par[:5]
    nj = m["nj"]
    nv = 6 + nj
    q, v = np.asarray(q, float), np.asarray(v, float)
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
    for i in range(NC):
        if not closed[i]:
            continue
        f[i, 2] = kn * d[i]
        cni = cn * min(1.0, d[i] / d0)
        n[i] = max(0.0, kn * d[i] - cni * c[i, 2])
        ct = mu * n[i] / np.sqrt(c[i, 0] ** 2 + c[i, 1] ** 2 + veps ** 2)
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
    return dict(q=q + h * vp, v=vp, a=(vp - v)[0:3] / h, d=d, n=n, closed=closed, force=force, spring=float(f[:, 2].sum()), A=A, rhs=rhs)


def quat_from_zyx(zyx):
    """(x, y, z, w) of Rz(zyx[0]) Ry(zyx[1]) Rx(zyx[2])."""
    cz, sz = np.cos(zyx[0] / 2), np.sin(zyx[0] / 2)
    cy, sy = np.cos(zyx[1] / 2), np.sin(zyx[1] / 2)
    cx, sx = np.cos(zyx[2] / 2), np.sin(zyx[2] / 2)
    return np.array([cz * cy * sx - sz * sy * cx, cz * sy * cx + sz * cy * sx, sz * cy * cx - cz * sy * sx, cz * cy * cx + sz * sy * sx])


def sensors(m, s, params=None, ground=None):
    """The outputs after a substep s (what substep returned): the members of bpmpc_sensor_inputs by name, rbd and contact_force [4, 3]."""
    par = DEFAULT_ROW if params is None else np.asarray(params, float)
    q, v = s["q"], s["v"]
    zyx = q[3:6]
    R = rot_zyx(zyx)
    w_world = euler_rate_map(zyx) @ v[3:6]
    quat = quat_from_zyx(zyx)
    return dict(joint_pos=q[6:].copy(), joint_vel=v[6:].copy(), quat=quat, angular_vel_local=R.T @ w_world,
                linear_accel_local=R.T @ (s["a"] + np.array([0.0, 0.0, GRAVITY])), contact=(s["n"] > par[5]).astype(np.int32),
                feet_heights=np.zeros(NC) if ground is None else np.asarray(ground, float), odom_pos=q[0:3].copy(), odom_quat=quat.copy(),
                odom_lin_vel=v[0:3].copy(), odom_ang_vel=w_world, rbd=rbd_from(m, q, v), contact_force=s["force"])
