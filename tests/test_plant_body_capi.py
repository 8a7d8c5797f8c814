"""CPU tier of the plant's body rows (include/bpmpc.h "Plant", bodies): the six entry points are declared and exported and refuse null handles and
pointers by name without a GPU; the start row is the three arrays of bpmpc_model_get bit for bit (H1, G1, Hunter, OpenLoong), the keys
plantBodies.<name> of a task.info over it; bpmpc_plant_compose_body_row against numpy; every validation rule names its entry and garbage in the
slots of bodies the robot does not have is ignored; the Python mirror; k_plant_body_step is in the library without scratch memory, beside step
kernels that are still there."""
import ctypes as C
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from bipedal_control_amd import load_library
from bipedal_control_amd import scenarios as sc
from tests import plant_body_reference as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["bpmpc_plant_get_body_params", "bpmpc_plant_set_body_params", "bpmpc_plant_reset_body_params", "bpmpc_plant_load_body_params",
             "bpmpc_plant_check_body_params", "bpmpc_plant_compose_body_row"]
INVALID = -1
_dp = C.POINTER(C.c_double)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


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
    assert re.search(r"#define\s+BPMPC_PLANT_BODY_PARAM_STRIDE\s+160\b", text) and re.search(r"#define\s+BPMPC_PLANT_JOINT_PARAM_STRIDE\s+64\b", text)
    assert raw.index(" *   joints: ") < raw.index(" *   bodies: ") and "plant_body.hip" in open(os.path.join(ROOT, "bipedal_control_amd", "build.py")).read()
    assert "Device rows are not looked at" in raw and "triangle inequality" in raw
    assert lib.bpmpc_plant_set_body_params.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_int), _dp, C.c_int, C.c_int]
    assert lib.bpmpc_plant_check_body_params.argtypes == [_dp, C.c_int, C.c_int]
    assert lib.bpmpc_plant_compose_body_row.argtypes == [C.c_void_p, _dp, C.c_int, C.c_double, _dp, C.c_double, _dp, _dp]


def test_null_handles_and_pointers_are_refused_by_name():
    lib = load_library()
    d = (C.c_double * 1024)()
    m = (C.c_int * 4)(1, 0, 1, 0)
    itf = sc.interface("h1")

    def null(rc, name):
        msg = lib.bpmpc_last_error()
        return rc == INVALID and b"null" in msg and name in msg

    for on_device in (0, 1):
        for mask in (m, None):
            assert null(lib.bpmpc_plant_set_body_params(None, 4, mask, d, 4, on_device), b"bpmpc_plant_set_body_params")
    assert null(lib.bpmpc_plant_get_body_params(None, 0, d), b"bpmpc_plant_get_body_params")
    assert null(lib.bpmpc_plant_reset_body_params(None), b"bpmpc_plant_reset_body_params")
    assert null(lib.bpmpc_plant_load_body_params(None, None, d), b"bpmpc_plant_load_body_params")
    assert null(lib.bpmpc_plant_load_body_params(itf.handle, None, None), b"bpmpc_plant_load_body_params")
    assert null(lib.bpmpc_plant_check_body_params(None, 1, 10), b"bpmpc_plant_check_body_params")
    assert lib.bpmpc_plant_check_body_params(d, 1, 0) == INVALID and lib.bpmpc_plant_check_body_params(d, 1, 13) == INVALID
    assert null(lib.bpmpc_plant_compose_body_row(None, None, 0, 1.0, None, 0.0, None, d), b"bpmpc_plant_compose_body_row")
    assert null(lib.bpmpc_plant_compose_body_row(itf.handle, None, 0, 1.0, None, 0.0, None, None), b"bpmpc_plant_compose_body_row")


def _load(itf, path):
    row = np.full(br.STRIDE, 7.0)
    rc = load_library().bpmpc_plant_load_body_params(itf.handle, path, _p(row))
    return rc, row


def _model_row(itf):
    """the three arrays of bpmpc_model_get in the layout of a body row"""
    nb = itf.actuatedDofNum + 1
    return br.pack(np.array(itf.get("body_mass")), np.array(itf.get("body_com")).reshape(nb, 3), np.array(itf.get("body_inertia")).reshape(nb, 3, 3))


def _task_with(tmp_path, block, robot="h1"):
    path = str(tmp_path / ("task_%d.info" % len(os.listdir(tmp_path))))
    shutil.copy(sc.ROBOTS[robot]["task"], path)
    with open(path, "a") as f:
        f.write("\nplantBodies\n{\n%s}\n" % block)
    return path.encode()


def test_start_row_is_the_model_row_as_bits():
    for robot in sorted(sc.ROBOTS):
        itf = sc.interface(robot)
        nb = itf.actuatedDofNum + 1
        want = _model_row(itf)
        assert want[br.MASS:br.MASS + nb].min() > 0.0 and not want[br.MASS + nb:br.MASS + br.SLOTS].any()
        for path in (None, sc.ROBOTS[robot]["task"].encode()):      # the shipped files have no such keys
            rc, row = _load(itf, path)
            assert rc == 0 and row.tobytes() == want.tobytes(), (robot, path)
        assert load_library().bpmpc_plant_check_body_params(_p(want), 1, nb - 1) == 0, load_library().bpmpc_last_error()
        assert br.validate(want, nb - 1) is None
    assert sorted(sc.ROBOTS) == ["g1", "h1", "hunter", "openloong"]


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def test_task_keys_are_ingested(tmp_path):
    lib = load_library()
    itf = sc.interface("h1")
    nj = itf.actuatedDofNum
    base = _model_row(itf)
    rc, row = _load(itf, _task_with(tmp_path, "  massScale 0.8\n"))
    assert rc == 0 and _rel(row, br.compose(base, nj, -1, 0.8)) < 1e-12 and abs(br.total_mass(row, nj) - 0.8 * br.total_mass(base, nj)) < 1e-10
    rc, row = _load(itf, _task_with(tmp_path, "  payloadMass 10\n  payloadOffset\n  {\n    (0,0) 0.1\n    (1,0) 0\n    (2,0) 0.3\n  }\n"))
    assert rc == 0 and _rel(row, br.compose(base, nj, 0, 1.0, None, 10.0, [0.1, 0.0, 0.3])) < 1e-12
    rc, row = _load(itf, _task_with(tmp_path, "  payloadMass 2\n  payloadBody 5\n"))      # no offset: at the link's origin
    assert rc == 0 and _rel(row, br.compose(base, nj, 5, 1.0, None, 2.0, [0.0, 0.0, 0.0])) < 1e-12
    rc, row = _load(itf, _task_with(tmp_path, "  massScale 1.2\n  payloadMass 10\n  payloadOffset\n  {\n    (0,0) 0.1\n    (1,0) 0\n    (2,0) 0.3\n  }\n"))
    assert rc == 0 and _rel(row, br.compose(br.compose(base, nj, -1, 1.2), nj, 0, 1.0, None, 10.0, [0.1, 0.0, 0.3])) < 1e-12
    rc, row = _load(itf, _task_with(tmp_path, "  massScale 1\n"))
    assert rc == 0 and row.tobytes() == base.tobytes()
    for block, what in (("  massScale 0\n", b"mass_scale"), ("  massScale nan\n", b"mass_scale"), ("  payloadMass -1\n", b"payload_mass"),
                        ("  payloadMass 1\n  payloadBody 11\n", b"body")):
        rc, row = _load(itf, _task_with(tmp_path, block))
        msg = lib.bpmpc_last_error()
        assert rc == INVALID and what in msg and b"plantBodies" in msg and np.all(row == 7.0), msg
    assert _load(itf, str(tmp_path / "absent.info").encode())[0] < 0


def test_compose_against_numpy():
    lib = load_library()
    rng = np.random.default_rng(12)
    for robot in ("h1", "openloong"):
        itf = sc.interface(robot)
        nj = itf.actuatedDofNum
        base = _model_row(itf)
        worst = 0.0
        cases = [(-1, 0.8, None, 0.0, None), (-1, 0.1, None, 0.0, None), (0, 1.3, [0.03, 0.0, 0.0], 0.0, None), (0, 1.0, None, 10.0, [0.1, 0.0, 0.3]),
                 (nj, 3.0, None, 0.0, None), (3, 0.7, [0.0, -0.02, 0.01], 1.5, [0.05, 0.02, -0.2])]
        cases += [(int(rng.integers(0, nj + 1)), float(rng.uniform(0.2, 3.0)), rng.uniform(-0.05, 0.05, 3), float(rng.uniform(0.0, 20.0)), rng.uniform(-0.3, 0.3, 3))
                  for _ in range(10)]
        for body, scale, shift, mass, pos in cases:
            shift_a = None if shift is None else np.asarray(shift, float)
            pos_a = None if pos is None else np.asarray(pos, float)
            out = np.full(br.STRIDE, 7.0)
            assert lib.bpmpc_plant_compose_body_row(itf.handle, None, body, scale, _p(shift_a), mass, _p(pos_a), _p(out)) == 0, lib.bpmpc_last_error()
            want = br.compose(base, nj, body, scale, shift, mass, pos)
            worst = max(worst, _rel(out, want))
            assert _rel(out, want) < 1e-12, (robot, body, scale)
            assert lib.bpmpc_plant_check_body_params(_p(out), 1, nj) == 0 and br.validate(out, nj) is None      # compose, then validate
            again = out.copy()      # from a given row, in place
            assert lib.bpmpc_plant_compose_body_row(itf.handle, _p(again), 1, 1.1, None, 0.5, _p(np.array([0.0, 0.1, 0.0])), _p(again)) == 0
            assert _rel(again, br.compose(want, nj, 1, 1.1, None, 0.5, [0.0, 0.1, 0.0])) < 1e-12
        print("compose against numpy", robot, "largest relative difference", worst)
        # body = -1 takes no shift or payload
        out = np.zeros(br.STRIDE)
        assert lib.bpmpc_plant_compose_body_row(itf.handle, None, -1, 0.5, _p(np.ones(3)), 3.0, _p(np.ones(3)), _p(out)) == 0
        assert _rel(out, br.compose(base, nj, -1, 0.5)) < 1e-12
        for args, what in (((nj + 1, 1.0, None, 0.0, None), b"body"), ((-2, 1.0, None, 0.0, None), b"body"), ((0, 0.0, None, 0.0, None), b"mass_scale"),
                           ((0, np.inf, None, 0.0, None), b"mass_scale"), ((0, 1.0, None, -1.0, None), b"payload_mass"), ((0, 1.0, None, 1.0, None), b"payload_pos"),
                           ((0, 1.0, np.array([np.nan, 0, 0]), 0.0, None), b"com_shift")):
            out = np.full(br.STRIDE, 7.0)
            body, scale, shift, mass, pos = args
            assert lib.bpmpc_plant_compose_body_row(itf.handle, None, body, scale, _p(shift), mass, _p(pos), _p(out)) == INVALID
            assert what in lib.bpmpc_last_error() and np.all(out == 7.0), lib.bpmpc_last_error()


def test_every_validation_rule_names_its_entry():
    lib = load_library()
    itf = sc.interface("h1")
    nj = itf.actuatedDofNum
    base = _model_row(itf)
    good = np.array([base, br.compose(base, nj, -1, 0.8), br.compose(base, nj, 0, 1.0, None, 10.0, [0.1, 0.0, 0.3])])
    assert lib.bpmpc_plant_check_body_params(_p(good), 3, nj) == 0
    S = br.SLOTS
    cases = [(br.MASS + 2, "mass[2]", 0.0, b"zero"), (br.MASS + 2, "mass[2]", -1.0, b"negative"), (br.MASS, "mass[0]", np.nan, b"not a number"),
             (br.MASS + nj, "mass[%d]" % nj, np.inf, b"not finite"),
             (br.COM + 1, "com_x[1]", np.inf, b"not finite"), (br.COM + S + 3, "com_y[3]", -np.inf, b"not finite"), (br.COM + 2 * S, "com_z[0]", np.nan, b"not a number"),
             (br.INERTIA + S + 4, "ixy[4]", np.nan, b"not a number"), (br.INERTIA + 5 * S, "izz[0]", np.inf, b"not finite")]
    for e, name, bad, what in cases:
        rows = good.copy()
        rows[1, e] = bad
        assert lib.bpmpc_plant_check_body_params(_p(rows), 3, nj) == INVALID, (name, bad)
        msg = lib.bpmpc_last_error()
        assert b"row 1" in msg and ("entry %d (%s)" % (e, name)).encode() in msg and what in msg, msg
        assert lib.bpmpc_plant_check_body_params(_p(rows), 1, nj) == 0          # the rows before it are good
        assert br.validate(rows[1], nj) is not None
    # an inertia that is not positive definite, and one whose principal moments no mass distribution has: named at the body
    for b, change, what in ((1, {3: -1.0}, b"not positive definite"), (4, {1: 1.0}, b"not positive definite"), (0, {0: 0.0}, b"not positive definite"),
                            (2, {5: 10.0}, b"triangle inequality"), (nj, {0: 5.0}, b"triangle inequality")):
        rows = good.copy()
        for k, val in change.items():
            rows[2, br.INERTIA + k * S + b] = val
        assert lib.bpmpc_plant_check_body_params(_p(rows), 3, nj) == INVALID, (b, change)
        msg = lib.bpmpc_last_error()
        assert b"row 2" in msg and ("entry %d (inertia[%d])" % (br.INERTIA + b, b)).encode() in msg and what in msg, msg
        got = br.validate(rows[2], nj)
        assert got is not None and got[0] == b and got[1].encode() == what
    # the library's eigenvalues against numpy's at the border of the triangle inequality: a thin rod (two equal moments, the third almost none)
    rod = good.copy()
    for k, val in enumerate((1e-9, 0.0, 0.0, 0.5, 0.0, 0.5)):
        rod[0, br.INERTIA + k * S + 3] = val
    assert lib.bpmpc_plant_check_body_params(_p(rod), 3, nj) == 0 and br.validate(rod[0], nj) is None
    # garbage in the slots of bodies the robot does not have is ignored
    rows = good.copy()
    for block in range(10):
        rows[1, block * S + nj + 1:(block + 1) * S] = (np.nan, -1.0, np.inf, 0.0, -np.inf)[:S - nj - 1]
    assert lib.bpmpc_plant_check_body_params(_p(rows), 3, nj) == 0
    assert lib.bpmpc_plant_check_body_params(_p(rows), 3, nj + 2) == INVALID


def test_python_mirror():
    import bipedal_control_amd as bp
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]      # noqa: E731
    E = inspect.Parameter.empty
    P = bp.BatchedPlant
    assert sig(P.setBodyParams) == [("self", E), ("rows", E), ("mask", None)]
    assert sig(P.getBodyParams) == [("self", E), ("robot", -1)]
    assert sig(P.resetBodyParams) == [("self", E)]
    Bp = bp.BodyParams
    assert Bp.STRIDE == 160 and "BodyParams" in bp.__all__
    assert sig(Bp.scaled) == [("self", E), ("s", E), ("body", None)] and sig(Bp.shifted) == [("self", E), ("body", E), ("d", E)]
    assert sig(Bp.payload) == [("self", E), ("m", E), ("pos", E), ("body", 0)]
    for robot in ("h1", "g1"):
        itf = sc.interface(robot)
        nj = itf.actuatedDofNum
        base = Bp.model(itf)
        want = _model_row(itf)
        assert base.row.tobytes() == want.tobytes() and base.total_mass == float(np.array(itf.get("body_mass")).sum())
        assert np.array_equal(base.mass, np.array(itf.get("body_mass"))) and np.array_equal(base.com, np.array(itf.get("body_com")).reshape(-1, 3))
        assert np.array_equal(base.inertia[:, 3], np.array(itf.get("body_inertia")).reshape(-1, 3, 3)[:, 1, 1])
        assert _rel(base.scaled(0.8).row, br.compose(want, nj, -1, 0.8)) < 1e-12 and abs(base.scaled(0.8).total_mass - 0.8 * base.total_mass) < 1e-10
        assert _rel(base.scaled(3.0, body=nj).row, br.compose(want, nj, nj, 3.0)) < 1e-12
        assert _rel(base.shifted(0, [0.03, 0, 0]).row, br.compose(want, nj, 0, 1.0, [0.03, 0.0, 0.0])) < 1e-12
        loaded = base.payload(10.0, [0.1, 0.0, 0.3])
        assert _rel(loaded.row, br.compose(want, nj, 0, 1.0, None, 10.0, [0.1, 0.0, 0.3])) < 1e-12 and abs(loaded.total_mass - base.total_mass - 10.0) < 1e-10
        assert base.row.tobytes() == want.tobytes()      # the methods return new rows
        chained = base.scaled(1.3, body=0).shifted(0, [0.03, 0, 0])
        assert _rel(chained.row, br.compose(want, nj, 0, 1.3, [0.03, 0.0, 0.0])) < 1e-12
        with pytest.raises(bp.BpmpcError):
            base.scaled(0.0)
        with pytest.raises(bp.BpmpcError):
            base.payload(1.0, [0, 0, 0], body=nj + 1)
        with pytest.raises(ValueError):
            Bp(itf, np.zeros(8))


def test_body_kernels_exist_without_scratch():
    """k_plant_body_step<10> and <12> are in the library, use no scratch memory and no more than a kilobyte and a bit of LDS beyond the joint
    kernel, and stand beside step kernels that are still there (read from the code object's metadata, as tests/test_kernel_resources.py does)"""
    from tests.test_kernel_resources import _kernels
    kernels = _kernels()
    found = {n.split("(")[0]: (scratch, lds) for n, scratch, vgpr, lds in kernels if n.startswith("k_plant_body_step<")}
    joint = {n.split("(")[0]: lds for n, scratch, vgpr, lds in kernels if n.startswith("k_plant_joint_step<")}
    print("k_plant_body_step (scratch, LDS)", found, "k_plant_joint_step LDS", joint)
    assert {k: v[0] for k, v in found.items()} == {"k_plant_body_step<10>": 0, "k_plant_body_step<12>": 0}, found
    for nj in (10, 12):
        assert found["k_plant_body_step<%d>" % nj][1] - joint["k_plant_joint_step<%d>" % nj] == (nj + 1) * 10 * 8      # the row, and nothing dynamic
    for family in ("k_plant_step<", "k_plant_stick_step<", "k_plant_joint_step<"):
        assert {n.split("(")[0] for n, *_ in kernels if n.startswith(family)} == {family + "10>", family + "12>"}
