"""The URDF's joint position limits (urdf_tree.cpp: <limit lower= upper=> of a revolute joint; both of the reference's joint controllers clamp to
urdf::Joint::limits): a copy of the H1 model with the tags inserted gives those numbers as bpmpc_model_get "joint_lower" / "joint_upper", the
committed models - which carry none - are unbounded, and no other name of bpmpc_model_get changes by one bit."""
import os
import re

import numpy as np
import pytest

from bipedal_control_amd import BipedalRobotInterface, BpmpcError
from bipedal_control_amd import scenarios as sc

NAMES = ("initial_state", "default_joint_state", "Q", "R", "robot_mass", "com_height", "body_mass", "body_com", "body_inertia", "joint_parent",
         "joint_rotation", "joint_offset", "joint_axis", "contact_body", "contact_offset", "cone", "swing", "sqp", "time_horizon", "position_error_gain",
         "phase_transition_stance_time", "hard_cone", "rollout", "ipm", "ddp")


def _with_limits(tmp_path, limits, skip=()):
    """the H1 model with <limit> inserted behind the <axis> of every revolute joint (joint names in `skip` excepted); limits: name -> (lower, upper)"""
    text = open(sc.H1["urdf"]).read()

    def insert(m):
        name = m.group(1)
        if name in skip or name not in limits:
            return m.group(0)
        lo, up = limits[name]
        return m.group(0) + '\n    <limit lower="%r" upper="%r" effort="200" velocity="23"/>' % (lo, up)

    out, n = re.subn(r'<joint name="(\w+)" type="revolute">.*?<axis xyz="[^"]*"/>', insert, text, flags=re.S)
    assert n >= 10
    path = tmp_path / "h1_limits.urdf"
    path.write_text(out)
    return BipedalRobotInterface(sc.H1["task"], str(path), sc.H1["reference"])


def test_inserted_limits_are_read_and_nothing_else_moves(tmp_path):
    plain = sc.interface("h1")
    names = plain.jointNames()
    rng = np.random.default_rng(5)
    limits = {n: (float(-rng.uniform(0.1, 2.0)), float(rng.uniform(0.1, 2.0))) for n in names}
    limits[names[3]] = (-0.26, 2.05)
    itf = _with_limits(tmp_path, limits, skip=(names[7],))
    assert itf.jointNames() == names
    lower, upper = np.array(itf.get("joint_lower")), np.array(itf.get("joint_upper"))
    assert lower.shape == upper.shape == (len(names),)
    for j, n in enumerate(names):
        want = (-np.inf, np.inf) if j == 7 else limits[n]
        assert (lower[j], upper[j]) == want, n
    for name in NAMES:
        assert np.array_equal(np.array(itf.get(name)), np.array(plain.get(name))), name


@pytest.mark.parametrize("robot", sorted(sc.ROBOTS))
def test_committed_models_are_unbounded(robot):
    itf = sc.interface(robot)
    nj = itf.actuatedDofNum
    lower, upper = np.array(itf.get("joint_lower")), np.array(itf.get("joint_upper"))
    assert lower.shape == upper.shape == (nj,) and np.all(np.isneginf(lower)) and np.all(np.isposinf(upper))


def test_a_limit_without_attributes_is_zero_as_in_urdfdom(tmp_path):
    text = open(sc.H1["urdf"]).read()
    out = text.replace('<axis xyz="0 0 1"/>', '<axis xyz="0 0 1"/>\n    <limit effort="200" velocity="23"/>', 1)
    assert out != text
    path = tmp_path / "h1_bare_limit.urdf"
    path.write_text(out)
    itf = BipedalRobotInterface(sc.H1["task"], str(path), sc.H1["reference"])
    lower, upper = np.array(itf.get("joint_lower")), np.array(itf.get("joint_upper"))
    assert np.sum(lower == 0.0) == 1 and np.sum(upper == 0.0) == 1 and np.argmax(lower == 0.0) == np.argmax(upper == 0.0)


def test_unknown_names_are_still_refused():
    with pytest.raises(BpmpcError):
        sc.interface("h1").get("joint_limits")
