"""numpy restatement of the plant's body rows (include/bpmpc.h "Plant", bodies; kernels/plant.h BODY).  A robot with a body row takes the substep
of tests/plant_joint_reference.py on a copy of the oracle's model whose mass / com / inertia are the row's: model_with_row builds that copy, and
no dynamics are written here.  compose restates bpmpc_plant_compose_body_row in numpy with 3 x 3 matrices (the library works on the six entries
of the symmetric matrix); validate restates the rules of a row with numpy's eigenvalues (the library has a Jacobi iteration of its own)."""
import numpy as np

from tests import plant_joint_reference as jr

STRIDE = 160
SLOTS = 16
MASS, COM, INERTIA = 0, 16, 64
SIX = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # xx, xy, xz, yy, yz, zz


def pack(mass, com, inertia):
    """the row of masses [nb], centres of mass [nb, 3] and inertias [nb, 3, 3] (of which the upper triangle is kept)"""
    nb = len(mass)
    row = np.zeros(STRIDE)
    row[MASS:MASS + nb] = mass
    for k in range(3):
        row[COM + k * SLOTS:COM + k * SLOTS + nb] = np.asarray(com)[:, k]
    for k, (i, j) in enumerate(SIX):
        row[INERTIA + k * SLOTS:INERTIA + k * SLOTS + nb] = np.asarray(inertia)[:, i, j]
    return row


def unpack(row, nj):
    """mass [nb], com [nb, 3], inertia [nb, 3, 3] (symmetric) of a robot with nj joints"""
    row = np.asarray(row, float)
    nb = nj + 1
    mass = row[MASS:MASS + nb].copy()
    com = np.array([row[COM + k * SLOTS:COM + k * SLOTS + nb] for k in range(3)]).T.copy()
    inertia = np.zeros((nb, 3, 3))
    for k, (i, j) in enumerate(SIX):
        inertia[:, i, j] = inertia[:, j, i] = row[INERTIA + k * SLOTS:INERTIA + k * SLOTS + nb]
    return mass, com, inertia


def model_row(m):
    """the model row of the oracle's model dict"""
    return pack(m["mass"], m["com"], m["inertia"])


def model_with_row(m, row):
    """a copy of the oracle's model dict with mass / com / inertia replaced by the row's: what a robot with that row is simulated with"""
    out = dict(m)
    out["mass"], out["com"], out["inertia"] = unpack(row, m["nj"])
    return out


def total_mass(row, nj):
    return float(np.asarray(row, float)[MASS:MASS + nj + 1].sum())


def compose(row, nj, body=-1, mass_scale=1.0, com_shift=None, payload_mass=0.0, payload_pos=None):
    """bpmpc_plant_compose_body_row: scale the mass and the inertia of `body`, move its com, merge a point mass; body = -1 scales every body"""
    mass, com, inertia = unpack(row, nj)
    if body < 0:
        return pack(mass * mass_scale, com, inertia * mass_scale)
    mass[body] *= mass_scale
    inertia[body] = inertia[body] * mass_scale
    if com_shift is not None:
        com[body] = com[body] + np.asarray(com_shift, float)
    if payload_mass > 0.0:
        p = np.asarray(payload_pos, float)
        total = mass[body] + payload_mass
        c = (mass[body] * com[body] + payload_mass * p) / total
        steiner = lambda mm, d: mm * (d @ d * np.eye(3) - np.outer(d, d))      # noqa: E731
        inertia[body] = inertia[body] + steiner(mass[body], com[body] - c) + steiner(payload_mass, p - c)
        mass[body], com[body] = total, c
    return pack(mass, com, inertia)


def validate(row, nj):
    """None for a row that obeys the rules of include/bpmpc.h "bodies", else (body, what)"""
    mass, com, inertia = unpack(row, nj)
    used = np.concatenate([np.asarray(row, float)[k * SLOTS:k * SLOTS + nj + 1] for k in range(10)])
    if not np.all(np.isfinite(used)):
        return -1, "not finite"
    for b in range(nj + 1):
        if not mass[b] > 0.0:
            return b, "mass"
        ev = np.linalg.eigvalsh(inertia[b])
        if not ev[0] > 0.0:
            return b, "not positive definite"
        if ev[2] > (ev[0] + ev[1]) * (1.0 + 1e-9):
            return b, "triangle inequality"
    return None


def substep(m, row, q, v, cmd, h, **more):
    """one substep of a robot with the body row `row`: plant_joint_reference.substep, unchanged, on the model with that row"""
    return jr.substep(model_with_row(m, row), q, v, cmd, h, **more)
