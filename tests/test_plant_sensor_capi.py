"""CPU tier of the plant's sensor model (include/bpmpc.h "Plant", sensors): the nine entry points are declared and exported and refuse null handles
and null pointers by name without a GPU; the keys plantSensors.<name> and plantSensors.seed of a task.info are read over zeros; every validation
rule names its entry and changes nothing; bpmpc_plant_sensor_draw - the text the kernels compile, on the host - gives the draws of the numpy
restatement; the plant's parameter row and PlantParams are as they were; the Python mirror has its methods; k_plant_sense is in the library
without scratch memory."""
import ctypes as C
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from bipedal_control_amd import load_library
from tests import plant_sensor_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["bpmpc_plant_set_sensor_params", "bpmpc_plant_get_sensor_params", "bpmpc_plant_reset_sensor_params", "bpmpc_plant_load_sensor_params",
             "bpmpc_plant_check_sensor_params", "bpmpc_plant_seed_sensors", "bpmpc_plant_get_sensor_state", "bpmpc_plant_sensed_outputs", "bpmpc_plant_sensor_draw"]
INVALID = -1
_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def test_functions_are_declared_and_exported():
    raw = open(os.path.join(ROOT, "include", "bpmpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = load_library()
    for name in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared"
        assert hasattr(lib, name), "libbpmpc.so does not export " + name
    assert re.search(r"#define\s+BPMPC_PLANT_SENSOR_PARAM_STRIDE\s+16\b", text)
    assert re.search(r"#define\s+BPMPC_PLANT_PARAM_STRIDE\s+8\b", text)


def test_null_handles_and_pointers_are_refused_by_name():
    from bipedal_control_amd.abi import _SensorInputs
    lib = load_library()
    d = (C.c_double * 64)()
    m = (C.c_int * 4)(1, 0, 1, 0)
    o = _SensorInputs()

    def null(rc, name):
        msg = lib.bpmpc_last_error()
        return rc == INVALID and b"null" in msg and name in msg

    for on_device in (0, 1):
        for mask in (m, None):
            assert null(lib.bpmpc_plant_set_sensor_params(None, 4, mask, d, 4, on_device), b"bpmpc_plant_set_sensor_params")
            assert null(lib.bpmpc_plant_seed_sensors(None, 4, mask, 3, on_device), b"bpmpc_plant_seed_sensors")
    assert null(lib.bpmpc_plant_get_sensor_params(None, 0, d), b"bpmpc_plant_get_sensor_params")
    assert null(lib.bpmpc_plant_reset_sensor_params(None), b"bpmpc_plant_reset_sensor_params")
    assert null(lib.bpmpc_plant_get_sensor_state(None, 4, d, d, d), b"bpmpc_plant_get_sensor_state")
    assert null(lib.bpmpc_plant_sensed_outputs(None, C.byref(o)), b"bpmpc_plant_sensed_outputs")
    assert null(lib.bpmpc_plant_load_sensor_params(None, None), b"bpmpc_plant_load_sensor_params")
    assert null(lib.bpmpc_plant_check_sensor_params(None, 1), b"bpmpc_plant_check_sensor_params")
    assert null(lib.bpmpc_plant_sensor_draw(1, 0, 0, None, d), b"bpmpc_plant_sensor_draw")
    assert null(lib.bpmpc_plant_sensor_draw(1, 0, 0, d, None), b"bpmpc_plant_sensor_draw")
    assert lib.bpmpc_plant_sensor_draw(1, -1, 0, d, d) == INVALID and lib.bpmpc_plant_sensor_draw(1, 0, -2, d, d) == INVALID


def test_plant_sensors_of_task_info_are_ingested(tmp_path):
    from bipedal_control_amd import scenarios as sc
    lib = load_library()
    row = (C.c_double * 16)(*([7.0] * 16))
    assert lib.bpmpc_plant_load_sensor_params(None, row) == 0 and list(row) == [0.0] * 16
    row = (C.c_double * 16)(*([7.0] * 16))
    assert lib.bpmpc_plant_load_sensor_params(sc.ROBOTS["h1"]["task"].encode(), row) == 0 and list(row) == [0.0] * 16      # the shipped files have no such keys

    def task_with(block):
        path = str(tmp_path / ("task_%d.info" % len(os.listdir(tmp_path))))
        shutil.copy(sc.ROBOTS["h1"]["task"], path)
        with open(path, "a") as f:
            f.write("\nplantSensors\n{\n%s}\n" % block)
        return path.encode()

    values = [2e-3, 1e-4, 5e-3, 2e-2, 1e-3, 5e-2, 1e-3, 1e-4, 3.8e-4, 1e-2, 0.05, 3.0]
    everything = task_with("".join("  %s %r\n" % (n, v) for n, v in zip(sr.FIELDS, values)) + "  seed 123456789\n")
    assert lib.bpmpc_plant_load_sensor_params(everything, row) == 0 and list(row) == values + [0.0] * 4
    assert lib.bpmpc_plant_load_sensor_params(task_with("  accel_noise 0.5\n  seed -4\n"), row) == 0 and list(row) == sr.row(accel_noise=0.5).tolist()
    # the plant's own row does not take these keys, nor this block the plant's
    prow = (C.c_double * 8)()
    assert lib.bpmpc_plant_load_params(everything, prow) == 0 and list(prow) == [5e4, 5e2, 1e-3, 0.7, 0.01, 1.0, 0.0, 0.0]
    for block, name, what in (("  gyro_noise -1.0\n", b"gyro_noise", b"negative"), ("  accel_bias_walk nan\n", b"accel_bias_walk", b"not finite"),
                              ("  contact_dropout 1.5\n", b"contact_dropout", b"above 1"), ("  delay_steps 2.5\n", b"delay_steps", b"not an integer"),
                              ("  delay_steps 9\n", b"delay_steps", b"above 8"), ("  seed 1.5\n", b"seed", b"integer"), ("  seed inf\n", b"seed", b"integer")):
        row = (C.c_double * 16)(*([7.0] * 16))
        assert lib.bpmpc_plant_load_sensor_params(task_with(block), row) == INVALID
        msg = lib.bpmpc_last_error()
        assert name in msg and what in msg and list(row) == [7.0] * 16, msg
    assert lib.bpmpc_plant_load_sensor_params(str(tmp_path / "absent.info").encode(), row) < 0


def test_every_validation_rule_names_its_entry():
    lib = load_library()
    good = np.array([sr.row(), sr.row(gyro_noise=0.1, contact_dropout=1.0, delay_steps=8.0), sr.row(contact_dropout=0.0, joint_pos_resolution=1e-3)])
    assert lib.bpmpc_plant_check_sensor_params(_p(good), 3) == 0
    for e, name in enumerate(sr.FIELDS + ("reserved",) * 4):
        cases = [(np.nan, b"not finite"), (np.inf, b"not finite")]
        if name == "reserved":
            cases += [(1.0, b"not zero"), (-1.0, b"negative")]
        else:
            cases += [(-1e-300, b"negative")]
        if name == "contact_dropout":
            cases += [(1.0 + 2.0 ** -52, b"above 1")]
        if name == "delay_steps":
            cases += [(0.5, b"not an integer"), (9.0, b"above 8")]
        for bad, what in cases:
            rows = good.copy()
            rows[1, e] = bad
            assert lib.bpmpc_plant_check_sensor_params(_p(rows), 3) == INVALID, (name, bad)
            msg = lib.bpmpc_last_error()
            assert b"row 1" in msg and ("entry %d (%s)" % (e, name)).encode() in msg and what in msg, msg
            assert lib.bpmpc_plant_check_sensor_params(_p(rows), 1) == 0          # the rows before it are good


@pytest.mark.parametrize("seed, robot, tick", [(0, 0, 0), (7, 3, 5), (-3, 4095, -1), (0x123456789ABCDEF, 17, (1 << 32) + 5), (1 << 40, 2, (1 << 62) + 3)])
def test_sensor_draw_matches_restatement(seed, robot, tick):
    """u is exact (integer arithmetic and one exact conversion); z = sqrt(-2 ln u1) cos(2 pi u2) through two libms: 1e-13 absolute on |z| <= 6.76"""
    lib = load_library()
    z, u = np.zeros(64), np.zeros(4)
    assert lib.bpmpc_plant_sensor_draw(seed, robot, tick, _p(z), _p(u)) == 0
    zr, ur = sr.draw(seed, robot, tick)
    print("sensor_draw", (seed, robot, tick), "max |z - z_ref| %.2e" % np.abs(z - zr).max())
    assert np.array_equal(u, ur)
    assert np.abs(z - zr).max() <= 1e-13
    assert np.abs(z).max() <= 6.76 and z.std() > 0.5


def test_parameter_row_and_plant_params_are_unchanged():
    from bipedal_control_amd import PlantParams
    lib = load_library()
    defaults = [5e4, 5e2, 1e-3, 0.7, 0.01, 1.0, 0.0, 0.0]
    row = (C.c_double * 8)()
    assert lib.bpmpc_plant_load_params(None, row) == 0 and list(row) == defaults
    assert PlantParams.STRIDE == 8 and PlantParams.FIELDS == ("kn", "cn", "d0", "mu", "v_eps", "contact_threshold")
    assert list(PlantParams().toRow()) == defaults
    with pytest.raises(ValueError):
        PlantParams(gyro_noise=1.0)


def test_python_mirror():
    import bipedal_control_amd as bp
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]      # noqa: E731
    E = inspect.Parameter.empty
    P = bp.BatchedPlant
    assert sig(P.setSensorParams) == [("self", E), ("rows", E), ("mask", None)]
    assert sig(P.getSensorParams) == [("self", E), ("robot", -1)]
    assert sig(P.resetSensorParams) == [("self", E)]
    assert sig(P.seedSensors) == [("self", E), ("seed", E), ("mask", None)]
    assert sig(P.sensorState) == [("self", E)]
    assert sig(P.sensed) == [("self", E)]
    S = bp.SensorParams
    assert S.STRIDE == 16 and S.FIELDS == sr.FIELDS and "SensorParams" in bp.__all__
    assert list(S().toRow()) == [0.0] * 16
    r = S(gyro_noise=2e-3, delay_steps=3).toRow()
    assert r.tolist() == sr.row(gyro_noise=2e-3, delay_steps=3).tolist() and S.fromRow(r).delay_steps == 3.0
    with pytest.raises(ValueError):
        S(kn=1.0)
    with pytest.raises(ValueError):
        S.fromRow(np.zeros(8))


def test_sense_kernels_exist_without_scratch_or_lds():
    """k_plant_sense<10> and <12> are in the library beside the step kernels and use neither scratch memory nor LDS"""
    from tests.test_kernel_resources import _kernels
    kernels = _kernels()
    found = {n.split("(")[0]: (scratch, lds) for n, scratch, vgpr, lds in kernels if n.startswith("k_plant_sense<")}
    assert found == {"k_plant_sense<10>": (0, 0), "k_plant_sense<12>": (0, 0)}, found
    assert {n.split("(")[0] for n, *_ in kernels if n.startswith("k_plant_step<")} == {"k_plant_step<10>", "k_plant_step<12>"}
