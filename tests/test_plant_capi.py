"""CPU tier of the batched rigid-body plant (include/bpmpc.h "Plant"): the entry points are declared and exported and refuse null handles
without a GPU, the keys plant.<name> of a task.info are read over the defaults, bad parameter rows are named, PlantParams packs rows by name, the
Python mirror has its methods, and bpmpc_plant_create without a device ends as the estimator's does."""
import ctypes as C
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from bipedal_control_amd import load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["bpmpc_plant_create", "bpmpc_plant_set_state", "bpmpc_plant_get_state", "bpmpc_plant_step", "bpmpc_plant_device_outputs",
             "bpmpc_plant_step_controlled", "bpmpc_plant_get_params", "bpmpc_plant_set_params", "bpmpc_plant_reset_params", "bpmpc_plant_load_params",
             "bpmpc_plant_check_params", "bpmpc_estimator_update_from_plant"]
INVALID, NO_DEVICE = -1, -4
DEFAULTS = [5e4, 5e2, 1e-3, 0.7, 0.01, 1.0, 0.0, 0.0]


def test_functions_are_declared_and_exported():
    raw = open(os.path.join(ROOT, "include", "bpmpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = load_library()
    for name in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared"
        assert hasattr(lib, name), "libbpmpc.so does not export " + name
    assert re.search(r"\bvoid\s+bpmpc_plant_destroy\s*\(", text) and hasattr(lib, "bpmpc_plant_destroy")
    assert re.search(r"#define\s+BPMPC_PLANT_PARAM_STRIDE\s+8\b", text)
    # the command and output structs in the order the Python mirror marshals them
    from bipedal_control_amd.api import _JointCommand, _PlantOutputs
    body = re.search(r"typedef struct \{([^}]*)\} bpmpc_joint_command;", text).group(1)
    assert tuple(re.findall(r"\*\s*(\w+)", body)) == _JointCommand.NAMES
    body = re.search(r"typedef struct \{([^}]*)\} bpmpc_plant_outputs;", text).group(1)
    assert re.findall(r"(\w+)\s*[;,]", body) == [n for n, _ in _PlantOutputs._fields_]


def test_null_handles_are_refused():
    from bipedal_control_amd.api import _JointCommand, _PlantOutputs
    lib = load_library()
    d = (C.c_double * 1024)()
    m = (C.c_int * 4)(1, 0, 1, 0)
    cmd, outs = _JointCommand(), _PlantOutputs()
    null = lambda rc: rc == INVALID and b"null" in lib.bpmpc_last_error()      # noqa: E731
    h = C.c_void_p()
    assert null(lib.bpmpc_plant_create(None, None, 0, 4, C.byref(h))) and not h
    assert null(lib.bpmpc_plant_step(None, 4, C.byref(cmd), 0, 0.002, 4)) and b"bpmpc_plant_step" in lib.bpmpc_last_error()
    assert null(lib.bpmpc_plant_step_controlled(None, None, 4, 0.002, 4, None, None, 0))
    assert null(lib.bpmpc_estimator_update_from_plant(None, None, 4, 0.002, d))
    assert null(lib.bpmpc_plant_device_outputs(None, C.byref(outs)))
    assert null(lib.bpmpc_plant_get_state(None, 4, d))
    assert null(lib.bpmpc_plant_get_params(None, 0, d))
    assert null(lib.bpmpc_plant_reset_params(None))
    for on_device in (0, 1):
        for mask in (m, None):
            assert null(lib.bpmpc_plant_set_state(None, 4, mask, d, on_device))
            assert null(lib.bpmpc_plant_set_params(None, 4, mask, d, 4, on_device)) and b"bpmpc_plant_set_params" in lib.bpmpc_last_error()
    lib.bpmpc_plant_destroy(None)


def test_python_mirror_exists():
    import bipedal_control_amd as bp
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]      # noqa: E731
    E = inspect.Parameter.empty
    P = bp.BatchedPlant
    assert sig(P.__init__) == [("self", E), ("interface", E), ("max_batch", 1), ("taskFile", None), ("device", 0)]
    assert sig(P.set_state) == [("self", E), ("rbd", E), ("mask", None)]
    assert sig(P.step) == [("self", E), ("pos_des", E), ("vel_des", E), ("tau_ff", E), ("kp", E), ("kd", E), ("base_force", None), ("feet_heights", None),
                           ("period", 0.002), ("substeps", 4)]
    assert sig(P.step_controlled) == [("self", E), ("controller", E), ("base_force", None), ("feet_heights", None), ("period", 0.002), ("substeps", 4)]
    assert sig(P.setParams) == [("self", E), ("rows", E), ("mask", None)] and sig(P.getParams) == [("self", E), ("robot", -1)]
    assert hasattr(P, "get_state") and hasattr(P, "outputs") and hasattr(P, "resetParams")
    assert sig(bp.BatchedStateEstimate.update_from_plant) == [("self", E), ("plant", E), ("period", 0.0025), ("fetch", True)]


def test_plant_params_pack_by_name():
    from bipedal_control_amd import PlantParams
    assert list(PlantParams().toRow()) == DEFAULTS and list(PlantParams.DEFAULTS) == DEFAULTS[:6]
    row = PlantParams(kn=8e4, mu=0.5).toRow()
    assert row[0] == 8e4 and row[3] == 0.5 and list(np.delete(row, [0, 3])) == list(np.delete(DEFAULTS, [0, 3]))
    back = PlantParams.fromRow(np.arange(1.0, 9.0))
    assert [getattr(back, n) for n in PlantParams.FIELDS] == list(np.arange(1.0, 7.0)) and list(back.toRow()[6:]) == [0.0, 0.0]
    assert list(PlantParams.fromRow(row).toRow()) == list(row)
    with pytest.raises(ValueError):
        PlantParams(kt=1.0)
    with pytest.raises(ValueError):
        PlantParams.fromRow(np.zeros(7))


def test_plant_block_of_task_info_is_ingested(tmp_path):
    """The shipped files have no plant block (every key absent: the defaults, as with a NULL path); a copy with the block appended gives its values and
    keeps the defaults of the keys it leaves out; a bad value is refused and named."""
    from bipedal_control_amd import scenarios as sc
    lib = load_library()
    row = (C.c_double * 8)()
    assert lib.bpmpc_plant_load_params(None, row) == 0 and list(row) == DEFAULTS
    row = (C.c_double * 8)(*([7.0] * 8))
    assert lib.bpmpc_plant_load_params(sc.ROBOTS["h1"]["task"].encode(), row) == 0 and list(row) == DEFAULTS
    task = str(tmp_path / "task.info")
    shutil.copy(sc.ROBOTS["h1"]["task"], task)
    with open(task, "a") as f:
        f.write("\nplant\n{\n  kn 8e4\n  contact_threshold 2.5\n}\n")
    assert lib.bpmpc_plant_load_params(task.encode(), row) == 0
    assert list(row) == [8e4, 5e2, 1e-3, 0.7, 0.01, 2.5, 0.0, 0.0]
    bad = str(tmp_path / "bad.info")
    shutil.copy(sc.ROBOTS["h1"]["task"], bad)
    with open(bad, "a") as f:
        f.write("\nplant\n{\n  d0 0.0\n}\n")
    assert lib.bpmpc_plant_load_params(bad.encode(), row) == INVALID and b"d0" in lib.bpmpc_last_error()
    assert lib.bpmpc_plant_load_params(str(tmp_path / "absent.info").encode(), row) < 0
    assert lib.bpmpc_plant_load_params(None, None) == INVALID and b"null" in lib.bpmpc_last_error()


def test_bad_parameter_rows_are_named():
    lib = load_library()
    good = np.tile(np.array(DEFAULTS), (3, 1))
    rows = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    assert lib.bpmpc_plant_check_params(rows(good), 3) == 0
    zero_ok = good.copy()
    zero_ok[1, [1, 3, 5]] = 0.0                                # no damping, no friction, a threshold of zero are settings like any other
    assert lib.bpmpc_plant_check_params(rows(zero_ok), 3) == 0
    for e, value, name, what in ((0, 0.0, b"kn", b"zero"), (1, float("nan"), b"cn", b"not finite"), (3, -0.1, b"mu", b"negative"),
                                 (2, 0.0, b"d0", b"zero"), (4, 0.0, b"v_eps", b"zero"), (5, float("inf"), b"contact_threshold", b"not finite")):
        bad = good.copy()
        bad[2, e] = value
        assert lib.bpmpc_plant_check_params(rows(bad), 3) == INVALID
        msg = lib.bpmpc_last_error()
        assert name in msg and what in msg and b"row 2" in msg and b"entry %d" % e in msg, msg
    assert lib.bpmpc_plant_check_params(None, 1) == INVALID and b"null" in lib.bpmpc_last_error()


def test_create_refuses_bad_arguments():
    """Without a GPU the create call ends with BPMPC_ERR_NO_DEVICE behind its argument checks, as bpmpc_estimator_create."""
    from bipedal_control_amd import scenarios as sc
    lib = load_library()
    r = sc.ROBOTS["h1"]
    model = C.c_void_p()
    assert lib.bpmpc_model_create(r["urdf"].encode(), r["task"].encode(), r["reference"].encode(), C.byref(model)) == 0, lib.bpmpc_last_error()
    h, e = C.c_void_p(), C.c_void_p()
    try:
        assert lib.bpmpc_plant_create(model, None, 0, 0, C.byref(h)) == INVALID
        assert lib.bpmpc_plant_create(model, None, 0, 4, None) == INVALID and b"null" in lib.bpmpc_last_error()
        rc = lib.bpmpc_plant_create(model, r["task"].encode(), 0, 4, C.byref(h))
        rc_est = lib.bpmpc_estimator_create(model, None, 1, 0, 4, C.byref(e))
        assert rc == rc_est and rc in (0, NO_DEVICE)
        if rc == 0:
            lib.bpmpc_plant_destroy(h)
            lib.bpmpc_estimator_destroy(e)
        else:
            assert b"no usable HIP device" in lib.bpmpc_last_error() and not h
    finally:
        lib.bpmpc_model_destroy(model)


def test_kernels_exist_without_scratch():
    """k_plant_step<10> and <12> are in the library and use no scratch memory"""
    from tests.test_kernel_resources import _kernels
    found = {n.split("(")[0]: scratch for n, scratch, vgpr, lds in _kernels() if n.startswith("k_plant_step<")}
    assert found == {"k_plant_step<10>": 0, "k_plant_step<12>": 0}, found
