"""CPU tier of the plant's joint model (include/bpmpc.h "Plant", joints): the five entry points are declared and exported and refuse null handles
and pointers by name without a GPU; the start row is the neutral row, the scalar keys plantJoints.<name> of a task.info over it, and with
plantJoints.fromUrdf 1 the <limit> and <dynamics> of the URDF under them; every validation rule names its entry; bpmpc_model_get
"joint_damping" / "joint_friction"; the Python mirror; k_plant_joint_step is in the library without scratch memory, beside step kernels that are
still there."""
import ctypes as C
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from bipedal_control_amd import BipedalRobotInterface, load_library
from bipedal_control_amd import scenarios as sc
from tests import plant_joint_reference as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["bpmpc_plant_get_joint_params", "bpmpc_plant_set_joint_params", "bpmpc_plant_reset_joint_params", "bpmpc_plant_load_joint_params",
             "bpmpc_plant_check_joint_params"]
INVALID = -1
_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def test_functions_are_declared_and_exported():
    from bipedal_control_amd import abi
    raw = open(os.path.join(ROOT, "include", "bpmpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = load_library()
    protos = abi.prototypes()
    for name in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared"
        assert hasattr(lib, name), "libbpmpc.so does not export " + name
        assert name in protos and len(getattr(lib, name).argtypes) == len(protos[name][1])
    assert re.search(r"#define\s+BPMPC_PLANT_JOINT_PARAM_STRIDE\s+64\b", text) and re.search(r"#define\s+BPMPC_PLANT_PARAM_STRIDE\s+8\b", text)
    assert " *   joints: " in raw and "plant_joint.hip" in open(os.path.join(ROOT, "bipedal_control_amd", "build.py")).read()
    assert "It has no joint limits" not in raw and "joint limits inside the plant" not in raw
    assert "h^2 k_limit < 4 (I_jj + armature_j + h (kd_j + c_j))" in raw and "nobody has measured them" in raw
    assert lib.bpmpc_plant_set_joint_params.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_int), _dp, C.c_int, C.c_int]
    assert lib.bpmpc_plant_check_joint_params.argtypes == [_dp, C.c_int, C.c_int]


def test_null_handles_and_pointers_are_refused_by_name():
    lib = load_library()
    d = (C.c_double * 256)()
    m = (C.c_int * 4)(1, 0, 1, 0)
    itf = sc.interface("h1")

    def null(rc, name):
        msg = lib.bpmpc_last_error()
        return rc == INVALID and b"null" in msg and name in msg

    for on_device in (0, 1):
        for mask in (m, None):
            assert null(lib.bpmpc_plant_set_joint_params(None, 4, mask, d, 4, on_device), b"bpmpc_plant_set_joint_params")
    assert null(lib.bpmpc_plant_get_joint_params(None, 0, d), b"bpmpc_plant_get_joint_params")
    assert null(lib.bpmpc_plant_reset_joint_params(None), b"bpmpc_plant_reset_joint_params")
    assert null(lib.bpmpc_plant_load_joint_params(None, None, d), b"bpmpc_plant_load_joint_params")
    assert null(lib.bpmpc_plant_load_joint_params(itf.handle, None, None), b"bpmpc_plant_load_joint_params")
    assert null(lib.bpmpc_plant_check_joint_params(None, 1, 10), b"bpmpc_plant_check_joint_params")
    assert lib.bpmpc_plant_check_joint_params(d, 1, 0) == INVALID and lib.bpmpc_plant_check_joint_params(d, 1, 13) == INVALID


def _load(itf, path):
    row = np.full(64, 7.0)
    rc = load_library().bpmpc_plant_load_joint_params(itf.handle, path, _p(row))
    return rc, row


def _task_with(tmp_path, block):
    path = str(tmp_path / ("task_%d.info" % len(os.listdir(tmp_path))))
    shutil.copy(sc.H1["task"], path)
    with open(path, "a") as f:
        f.write("\nplantJoints\n{\n%s}\n" % block)
    return path.encode()


def test_start_row_is_neutral_without_a_block():
    for robot in sorted(sc.ROBOTS):
        itf = sc.interface(robot)
        for path in (None, sc.ROBOTS[robot]["task"].encode()):      # the shipped files have no such keys
            rc, row = _load(itf, path)
            assert rc == 0 and np.array_equal(row, jr.neutral_row()), (robot, path)
    assert jr.neutral_row()[60:].tolist() == [1e4, 1e2, 0.01, 0.0]


def test_scalar_keys_of_task_info_are_ingested(tmp_path):
    lib = load_library()
    itf = sc.interface("h1")
    nj = itf.actuatedDofNum
    rc, row = _load(itf, _task_with(tmp_path, "  armature 0.1\n  damping 1\n  frictionLoss 0.2\n  kLimit 5000\n  cLimit 50\n  wEps 0.02\n"))
    assert rc == 0 and np.array_equal(row, jr.joint_row(nj, armature=0.1, damping=1.0, friction_loss=0.2, k_limit=5000.0, c_limit=50.0, w_eps=0.02))
    assert not row[nj:12].any() and not row[12 + nj:24].any() and not row[24 + nj:36].any()      # the joints the robot does not have stay neutral
    rc, row = _load(itf, _task_with(tmp_path, "  damping 0.5\n"))
    assert rc == 0 and np.array_equal(row, jr.joint_row(nj, damping=0.5))
    rc, row = _load(itf, _task_with(tmp_path, "  fromUrdf 1\n"))
    assert rc == 0 and np.array_equal(row, jr.neutral_row())      # the committed model has neither limits nor dynamics
    for block, name, what in (("  armature -0.1\n", b"armature[0]", b"negative"), ("  damping nan\n", b"damping[0]", b"not a number"),
                              ("  frictionLoss inf\n", b"friction_loss[0]", b"not finite"), ("  wEps 0\n", b"w_eps", b"zero"),
                              ("  kLimit -1\n", b"k_limit", b"negative"), ("  cLimit inf\n", b"c_limit", b"not finite")):
        rc, row = _load(itf, _task_with(tmp_path, block))
        msg = lib.bpmpc_last_error()
        assert rc == INVALID and name in msg and what in msg and np.all(row == 7.0), msg
    assert _load(itf, str(tmp_path / "absent.info").encode())[0] < 0


def _urdf_with(tmp_path, tags):
    """the H1 model with <limit> and <dynamics> inserted behind the <axis> of the revolute joints named in `tags`: name -> the tags' text"""
    text = open(sc.H1["urdf"]).read()
    out, n = re.subn(r'<joint name="(\w+)" type="revolute">.*?<axis xyz="[^"]*"/>', lambda m: m.group(0) + tags.get(m.group(1), ""), text, flags=re.S)
    assert n >= 10
    path = tmp_path / "h1_joints.urdf"
    path.write_text(out)
    return BipedalRobotInterface(sc.H1["task"], str(path), sc.H1["reference"])


def test_from_urdf_takes_limits_and_dynamics(tmp_path):
    plain = sc.interface("h1")
    names = plain.jointNames()
    nj = len(names)
    rng = np.random.default_rng(9)
    lower, upper = -rng.uniform(0.1, 2.0, nj), rng.uniform(0.1, 2.0, nj)
    damping, friction = rng.uniform(0.01, 0.5, nj), rng.uniform(0.05, 0.4, nj)
    tags = {n: '\n    <limit lower="%r" upper="%r" effort="200" velocity="23"/>\n    <dynamics damping="%r" friction="%r"/>'
            % (float(lower[j]), float(upper[j]), float(damping[j]), float(friction[j])) for j, n in enumerate(names)}
    tags[names[2]] = '\n    <dynamics damping="0.3"/>'                      # no limit, no friction attribute
    tags[names[7]] = '\n    <limit lower="-1" upper="1.5" effort="1" velocity="1"/>'      # no dynamics
    lower[2], upper[2], damping[2], friction[2] = -np.inf, np.inf, 0.3, 0.0
    lower[7], upper[7], damping[7], friction[7] = -1.0, 1.5, 0.0, 0.0
    itf = _urdf_with(tmp_path, tags)
    assert itf.jointNames() == names
    assert np.array_equal(np.array(itf.get("joint_damping")), damping) and np.array_equal(np.array(itf.get("joint_friction")), friction)
    assert np.array_equal(np.array(itf.get("joint_lower")), lower) and np.array_equal(np.array(itf.get("joint_upper")), upper)
    assert not np.array(plain.get("joint_damping")).any() and not np.array(plain.get("joint_friction")).any() and len(plain.get("joint_damping")) == nj
    # without fromUrdf the model's tags are not looked at
    assert np.array_equal(_load(itf, None)[1], jr.neutral_row())
    assert np.array_equal(_load(itf, _task_with(tmp_path, "  kLimit 2000\n"))[1], jr.joint_row(nj, k_limit=2000.0))
    rc, row = _load(itf, _task_with(tmp_path, "  fromUrdf 1\n"))
    assert rc == 0 and np.array_equal(row, jr.joint_row(nj, damping=damping, friction_loss=friction, lower=lower, upper=upper))
    # the scalar keys override the URDF's values where both are given; armature has no URDF counterpart
    rc, row = _load(itf, _task_with(tmp_path, "  fromUrdf 1\n  damping 1\n  armature 0.1\n"))
    assert rc == 0 and np.array_equal(row, jr.joint_row(nj, armature=0.1, damping=1.0, friction_loss=friction, lower=lower, upper=upper))
    # the other names of bpmpc_model_get do not move
    for name in ("initial_state", "body_mass", "body_inertia", "joint_axis", "joint_offset", "contact_offset"):
        assert np.array_equal(np.array(itf.get(name)), np.array(plain.get(name))), name


def test_every_validation_rule_names_its_entry():
    lib = load_library()
    nj = 10
    good = np.array([jr.neutral_row(), jr.joint_row(nj, armature=0.1, damping=1.0, friction_loss=0.2, lower=-1.0, upper=2.0, k_limit=0.0, c_limit=0.0, w_eps=1e-6),
                     jr.joint_row(nj, lower=-np.inf, upper=0.5)])
    assert lib.bpmpc_plant_check_joint_params(_p(good), 3, nj) == 0      # +-inf limits are accepted
    cases = []
    for block, name in enumerate(("armature", "damping", "friction_loss")):
        for j in (0, nj - 1):
            cases += [(12 * block + j, "%s[%d]" % (name, j), bad, what) for bad, what in ((np.nan, b"not a number"), (np.inf, b"not finite"), (-1e-300, b"negative"))]
    cases += [(36, "lower[0]", np.nan, b"not a number"), (36 + nj - 1, "lower[%d]" % (nj - 1), np.inf, b"+inf"), (48, "upper[0]", np.nan, b"not a number"),
              (48 + 3, "upper[3]", -np.inf, b"-inf"), (48 + 3, "upper[3]", -1.0, b"not above lower"), (48 + 3, "upper[3]", -1.5, b"not above lower")]
    for e, name in ((60, "k_limit"), (61, "c_limit"), (62, "w_eps")):
        cases += [(e, name, np.nan, b"not finite"), (e, name, np.inf, b"not finite"), (e, name, -1.0, b"negative")]
    cases += [(62, "w_eps", 0.0, b"zero"), (63, "reserved", 1.0, b"not zero"), (63, "reserved", np.nan, b"not zero")]
    for e, name, bad, what in cases:
        rows = good.copy()
        rows[1, e] = bad
        assert lib.bpmpc_plant_check_joint_params(_p(rows), 3, nj) == INVALID, (name, bad)
        msg = lib.bpmpc_last_error()
        assert b"row 1" in msg and ("entry %d (%s)" % (e, name)).encode() in msg and what in msg, msg
        assert lib.bpmpc_plant_check_joint_params(_p(rows), 1, nj) == 0          # the rows before it are good
    # a lower limit that is not below the upper is named at the upper
    rows = good.copy()
    rows[1, 36 + 5] = 2.0
    assert lib.bpmpc_plant_check_joint_params(_p(rows), 3, nj) == INVALID and b"upper[5]" in lib.bpmpc_last_error()
    # entries of joints the robot does not have are ignored
    rows = good.copy()
    rows[1, 10], rows[1, 36 + 11], rows[1, 48 + 11] = -5.0, 3.0, 1.0
    assert lib.bpmpc_plant_check_joint_params(_p(rows), 3, nj) == 0 and lib.bpmpc_plant_check_joint_params(_p(rows), 3, 12) == INVALID


def test_python_mirror():
    import bipedal_control_amd as bp
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]      # noqa: E731
    E = inspect.Parameter.empty
    P = bp.BatchedPlant
    assert sig(P.setJointParams) == [("self", E), ("rows", E), ("mask", None)]
    assert sig(P.getJointParams) == [("self", E), ("robot", -1)]
    assert sig(P.resetJointParams) == [("self", E)]
    J = bp.JointParams
    assert J.STRIDE == 64 and "JointParams" in bp.__all__
    for nj in (10, 12):
        assert np.array_equal(J.neutral(nj).toRow(), jr.neutral_row()) and np.array_equal(J(nj).toRow(), jr.neutral_row())
        assert np.array_equal(J.reference_mjcf(nj).toRow(), jr.joint_row(nj, armature=0.1, damping=1.0))
        upper = np.linspace(0.5, 1.5, nj)
        r = J(nj, friction_loss=0.2, upper=upper, lower=-1.0, k_limit=2e3, w_eps=0.05).toRow()
        assert np.array_equal(r, jr.joint_row(nj, friction_loss=0.2, upper=upper, lower=-1.0, k_limit=2e3, w_eps=0.05))
        back = J.fromRow(r, nj)
        assert np.array_equal(back.upper, upper) and back.k_limit == 2e3 and np.array_equal(back.toRow(), r)
    assert "h1.xml" in J.reference_mjcf.__doc__
    with pytest.raises(ValueError):
        J(10, stiffness=1.0)
    with pytest.raises(ValueError):
        J(10, damping=np.ones(12))
    with pytest.raises(ValueError):
        J.fromRow(np.zeros(8), 10)


def test_joint_kernels_exist_without_scratch():
    """k_plant_joint_step<10> and <12> are in the library, use no scratch memory, and stand beside step kernels that are still there"""
    from tests.test_kernel_resources import _kernels
    kernels = _kernels()
    found = {n.split("(")[0]: scratch for n, scratch, vgpr, lds in kernels if n.startswith("k_plant_joint_step<")}
    assert found == {"k_plant_joint_step<10>": 0, "k_plant_joint_step<12>": 0}, found
    assert {n.split("(")[0] for n, *_ in kernels if n.startswith("k_plant_step<")} == {"k_plant_step<10>", "k_plant_step<12>"}
    assert {n.split("(")[0] for n, *_ in kernels if n.startswith("k_plant_stick_step<")} == {"k_plant_stick_step<10>", "k_plant_stick_step<12>"}
