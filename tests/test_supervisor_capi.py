"""CPU tier of the supervisor's C ABI (include/bpmpc.h "Supervisor"): the entry points are declared, exported and typed; null handles are refused
by name; every host validation that needs no handle names its entry; load_params / check_params on the committed task file and on one with
every key set; create without a device is BPMPC_ERR_NO_DEVICE; bpmpc_supervisor_rows_host - the kernel's own text on the host - against the
numpy restatement on random robots; k_supervise is in the library without scratch memory.  (The refusals that need a handle are in
tests/test_gpu_supervisor.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from bipedal_control_amd import abi, load_library
from tests import supervisor_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"bpmpc_supervisor_create": "int", "bpmpc_supervisor_destroy": "void", "bpmpc_supervisor_get_params": "int", "bpmpc_supervisor_set_params": "int",
             "bpmpc_supervisor_reset_params": "int", "bpmpc_supervisor_load_params": "int", "bpmpc_supervisor_check_params": "int",
             "bpmpc_supervisor_set_joint_rows": "int", "bpmpc_supervisor_get_joint_rows": "int", "bpmpc_supervisor_request": "int",
             "bpmpc_supervisor_update": "int", "bpmpc_supervisor_update_controlled": "int", "bpmpc_supervisor_device_outputs": "int",
             "bpmpc_supervisor_get_state": "int", "bpmpc_supervisor_get_commands": "int", "bpmpc_supervisor_rows_host": "int",
             "bpmpc_plant_step_supervised": "int"}
INVALID, IO, NO_DEVICE, CAPACITY = -1, -2, -4, -6
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
EPS = np.finfo(float).eps


def _model(robot):
    from bipedal_control_amd import scenarios as sc
    return sc.interface(robot)


def test_functions_are_declared_exported_and_typed():
    raw = open(os.path.join(ROOT, "include", "bpmpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = load_library()
    protos = abi.prototypes()
    for name, ret in FUNCTIONS.items():
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), text), name + " is not declared"
        assert hasattr(lib, name), "libbpmpc.so does not export " + name
        assert name in protos and protos[name][0] == ret
        assert len(getattr(lib, name).argtypes) == len(protos[name][1]), name
    for define, value in (("BPMPC_SUP_PARAM_STRIDE", 8), ("BPMPC_SUP_INIT", 0), ("BPMPC_SUP_RUN", 1), ("BPMPC_SUP_STOPPED", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (define, value), text), define
    assert re.search(r"typedef\s+struct\s+bpmpc_supervisor\s+bpmpc_supervisor\s*;", text)
    assert lib.bpmpc_supervisor_update.argtypes == [C.c_void_p, C.c_int, _dp, C.POINTER(abi._JointCommand), C.c_int, C.c_double]
    assert lib.bpmpc_supervisor_request.argtypes == [C.c_void_p, C.c_int, _ip, C.c_int, C.c_int, C.c_int]
    assert lib.bpmpc_supervisor_device_outputs.argtypes == [C.c_void_p, C.POINTER(abi._SupervisorOutputs)]
    assert [n for n, _ in abi._SupervisorOutputs._fields_] == ["pos_des", "vel_des", "tau_ff", "kp", "kd", "state", "cause", "unsafe", "ready", "counts", "elapsed", "stream"]
    assert "Not reproduced: per-robot MPC cost weights, UpperJointController" in raw and "the SafetyChecker limits, InitialJointController" not in raw
    with pytest.raises(C.ArgumentError):
        lib.bpmpc_supervisor_request(None, 1, None, 1.5, 0, 0)


def test_null_handles_are_refused_by_name():
    lib = load_library()
    d = (C.c_double * 256)()
    m = (C.c_int * 8)(1, 0, 1, 0)
    h = C.c_void_p()
    itf = _model("h1")
    cmd = abi._JointCommand(*([C.cast(d, _dp)] * 5), None, None)
    out = abi._SupervisorOutputs()

    def null(rc, name):
        msg = lib.bpmpc_last_error()
        return rc == INVALID and b"null" in msg and name in msg

    assert null(lib.bpmpc_supervisor_create(None, None, 0, 4, C.byref(h)), b"bpmpc_supervisor_create")
    assert null(lib.bpmpc_supervisor_create(itf.handle, None, 0, 4, None), b"bpmpc_supervisor_create")
    assert null(lib.bpmpc_supervisor_get_params(None, 0, d), b"bpmpc_supervisor_get_params")
    assert null(lib.bpmpc_supervisor_reset_params(None), b"bpmpc_supervisor_reset_params")
    assert null(lib.bpmpc_supervisor_load_params(None, None), b"bpmpc_supervisor_load_params")
    assert null(lib.bpmpc_supervisor_check_params(None, 1), b"bpmpc_supervisor_check_params")
    assert null(lib.bpmpc_supervisor_get_joint_rows(None, 0, 0, d), b"bpmpc_supervisor_get_joint_rows")
    for on_device in (0, 1):
        assert null(lib.bpmpc_supervisor_set_params(None, 4, m, d, 4, on_device), b"bpmpc_supervisor_set_params")
        assert null(lib.bpmpc_supervisor_set_joint_rows(None, 4, m, 0, d, 1, on_device), b"bpmpc_supervisor_set_joint_rows")
        assert null(lib.bpmpc_supervisor_request(None, 4, m, 1, 0, on_device), b"bpmpc_supervisor_request")
        assert null(lib.bpmpc_supervisor_update(None, 4, d, C.byref(cmd), on_device, 0.002), b"bpmpc_supervisor_update")
        assert null(lib.bpmpc_plant_step_supervised(None, None, 4, 0.002, 4, None, None, on_device), b"bpmpc_plant_step_supervised")
    assert null(lib.bpmpc_supervisor_update_controlled(None, None, None, d, 4, 0.002), b"bpmpc_supervisor_update_controlled")
    assert null(lib.bpmpc_supervisor_device_outputs(None, C.byref(out)), b"bpmpc_supervisor_device_outputs")
    assert null(lib.bpmpc_supervisor_get_state(None, 4, m, m, m, m, d, m), b"bpmpc_supervisor_get_state")
    assert null(lib.bpmpc_supervisor_get_commands(None, 4, d, d, d, d, d), b"bpmpc_supervisor_get_commands")
    f = (C.c_int * 5)()
    assert null(lib.bpmpc_supervisor_rows_host(None, d, d, d, None, 0.002, f, d, d, d), b"bpmpc_supervisor_rows_host")
    assert null(lib.bpmpc_supervisor_rows_host(itf.handle, d, d, d, None, 0.002, None, d, d, d), b"bpmpc_supervisor_rows_host")
    lib.bpmpc_supervisor_destroy(None)                                       # as free(NULL)


def test_check_params_names_the_entry():
    lib = load_library()
    good = sr.DEFAULT_PARAMS.copy()
    good[1:7] = 0.3, 0.5, 0.1, 1.0, 0.2, 4.0
    rows = np.tile(good, (3, 1))
    assert lib.bpmpc_supervisor_check_params(rows.ctypes.data_as(_dp), 3) == 0
    names = ("tilt_limit", "min_base_height", "ramp_time", "settle_pos_tol", "settle_vel_tol", "settle_time", "stop_kd")
    for e, name in enumerate(names):
        for value, why in ((-1.0, b"negative"), (np.nan, b"not finite"), (np.inf, b"not finite")):
            bad = rows.copy()
            bad[2, e] = value
            assert lib.bpmpc_supervisor_check_params(bad.ctypes.data_as(_dp), 3) == INVALID
            msg = lib.bpmpc_last_error()
            assert b"row 2" in msg and ("entry %d (%s)" % (e, name)).encode() in msg and why in msg, msg
    bad = rows.copy()
    bad[1, 0] = 0.0
    assert lib.bpmpc_supervisor_check_params(bad.ctypes.data_as(_dp), 3) == INVALID and b"entry 0 (tilt_limit) is zero" in lib.bpmpc_last_error()
    bad = rows.copy()
    bad[0, 7] = np.nan                                                        # the reserved entry is not used
    assert lib.bpmpc_supervisor_check_params(bad.ctypes.data_as(_dp), 3) == 0


def test_load_params(tmp_path):
    lib = load_library()
    row = np.full(8, -7.0)
    for path in (None, os.path.join(ROOT, "assets", "h1", "task.info").encode(), os.path.join(ROOT, "assets", "g1", "task.info").encode()):
        row[:] = -7.0
        assert lib.bpmpc_supervisor_load_params(path, row.ctypes.data_as(_dp)) == 0, lib.bpmpc_last_error()
        assert np.array_equal(row, sr.DEFAULT_PARAMS)                         # pi / 3 bit for bit; the committed files have no supervisor block
    task = tmp_path / "task.info"
    base = open(os.path.join(ROOT, "assets", "h1", "task.info")).read()
    task.write_text(base + "\nsupervisor\n{\n  tilt_limit 0.75\n  min_base_height 0.4\n  ramp_time 0.5\n  settle_pos_tol 0.05\n  settle_vel_tol 0.25\n"
                    "  settle_time 0.125\n  stop_kd 3.5\n}\n")
    assert lib.bpmpc_supervisor_load_params(str(task).encode(), row.ctypes.data_as(_dp)) == 0, lib.bpmpc_last_error()
    assert row.tolist() == [0.75, 0.4, 0.5, 0.05, 0.25, 0.125, 3.5, 0.0]
    task.write_text(base + "\nsupervisor\n{\n  ramp_time -0.5\n}\n")
    assert lib.bpmpc_supervisor_load_params(str(task).encode(), row.ctypes.data_as(_dp)) == INVALID
    assert b"entry 2 (ramp_time) is negative" in lib.bpmpc_last_error()
    assert lib.bpmpc_supervisor_load_params(str(tmp_path / "absent.info").encode(), row.ctypes.data_as(_dp)) < 0


def test_create_refusals_and_no_device():
    import bipedal_control_amd as bp
    lib = load_library()
    itf = _model("h1")
    h = C.c_void_p(1)
    assert lib.bpmpc_supervisor_create(itf.handle, None, 0, 0, C.byref(h)) == INVALID and b"max_batch" in lib.bpmpc_last_error() and not h.value
    h = C.c_void_p(1)
    rc = lib.bpmpc_supervisor_create(itf.handle, None, 1 << 20, 4, C.byref(h))      # a device nobody has
    assert rc == NO_DEVICE and b"bpmpc_supervisor_create" in lib.bpmpc_last_error() and b"no usable HIP device" in lib.bpmpc_last_error() and not h.value
    h = C.c_void_p()
    rc = lib.bpmpc_supervisor_create(itf.handle, itf.taskFile.encode(), 0, 4, C.byref(h))
    assert rc in (0, NO_DEVICE), lib.bpmpc_last_error()
    if rc == NO_DEVICE:
        assert not h.value
        with pytest.raises(bp.BpmpcError) as err:
            bp.BatchedSupervisor(_model("h1"), 4)
        assert err.value.status == NO_DEVICE
    else:
        lib.bpmpc_supervisor_destroy(h)


def test_python_mirror():
    import bipedal_control_amd as bp
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]      # noqa: E731
    E = inspect.Parameter.empty
    S = bp.BatchedSupervisor
    assert sig(S.__init__) == [("self", E), ("interface", E), ("max_batch", 1), ("taskFile", None), ("device", 0)]
    for name in ("update", "update_controlled", "request", "setParams", "getParams", "resetParams", "setJointRows", "getJointRows", "state", "outputs"):
        assert callable(getattr(S, name)), name
    assert callable(bp.BatchedPlant.step_supervised)
    assert "BatchedSupervisor" in bp.__all__ and "SupervisorParams" in bp.__all__
    P = bp.SupervisorParams
    assert np.array_equal(P().toRow(), sr.DEFAULT_PARAMS) and P.STRIDE == 8
    row = P(ramp_time=0.5, stop_kd=2.0).toRow()
    assert row[2] == 0.5 and row[6] == 2.0 and P.fromRow(row).ramp_time == 0.5
    with pytest.raises(ValueError):
        P(ramp=1.0)
    assert (S.INIT, S.RUN, S.STOPPED) == (sr.INIT, sr.RUN, sr.STOPPED) and S.JOINT_ROWS == sr.JOINT_ROWS


def random_robot(rng, m_q0, nj, state, lower, upper):
    """One robot in `state` before an update: parameters, joint rows, measurement, flags, clocks, latched joints, RUN command (or None)"""
    nv = 6 + nj
    p = sr.DEFAULT_PARAMS.copy()
    p[sr.MIN_BASE_HEIGHT] = rng.choice([0.0, 0.7])
    p[sr.RAMP_TIME] = rng.choice([0.0, 0.05, 0.3])
    p[sr.SETTLE_POS_TOL], p[sr.SETTLE_VEL_TOL] = rng.choice([0.0, 0.6]), rng.choice([0.0, 3.5])
    p[sr.SETTLE_TIME], p[sr.STOP_KD] = rng.choice([0.0, 0.004]), rng.uniform(0.0, 5.0)
    rbd = np.zeros(2 * nv)
    rbd[0] = rng.uniform(-3.0, 3.0)
    rbd[1:3] = rng.uniform(-1.2, 1.2, 2) if rng.random() < 0.5 else rng.uniform(-0.3, 0.3, 2)      # both sides of pi / 3
    rbd[3:5], rbd[5] = rng.uniform(-2.0, 2.0, 2), rng.uniform(0.6, 1.1)
    rbd[6:nv] = m_q0 + rng.uniform(-0.5, 0.5, nj)
    rbd[nv:] = rng.standard_normal(nv)
    if rng.random() < 0.15:
        rbd[rng.integers(0, 2 * nv)] = rng.choice([np.nan, np.inf, -np.inf])
    rows = np.array([m_q0 + rng.uniform(-0.2, 0.2, nj), rng.uniform(0, 100, nj), rng.uniform(0, 10, nj), lower, upper])
    flags = np.array([state, rng.choice([0, 1, 64]) if state == sr.STOPPED else 0, rng.integers(0, 32), rng.integers(0, 2), rng.integers(0, 2)], np.int32)
    clocks = np.array([rng.choice([0.0, 0.002, 0.1, 0.299, 1.0]), rng.choice([0.0, 0.002, 0.5])])
    q_latch = m_q0 + rng.uniform(-0.5, 0.5, nj)
    cmd = None
    if rng.random() < 0.85:
        cmd = [rng.standard_normal(nj) for _ in range(5)]
        if rng.random() < 0.15:
            cmd[rng.integers(0, 5)][rng.integers(0, nj)] = rng.choice([np.nan, np.inf])
    return p, rows, rbd, flags, clocks, q_latch, cmd


def restated(nj, p, rows, rbd, flags, clocks, q_latch, cmd, period):
    s = sr.Supervisor(1, nj, rows[0], params=p, lower=rows[3], upper=rows[4])
    s.rows["kp_init"][0], s.rows["kd_init"][0] = rows[1], rows[2]
    s.state[0], s.cause[0], s.unsafe[0], s.ready[0], s.latch[0] = flags
    s.elapsed[0], s.settled[0] = clocks
    s.q_latch[0] = q_latch
    s.update(rbd[None], None if cmd is None else [a[None] for a in cmd], period)
    return s


@pytest.mark.parametrize("robot", ["h1", "g1"])
def test_rows_host_against_the_restatement(robot):
    import bipedal_control_amd as bp
    itf = _model(robot)
    nj = itf.actuatedDofNum
    q0 = np.array(itf.get("default_joint_state"))
    rng = np.random.default_rng(11 + nj)
    ramped = 0
    for state in (sr.INIT, sr.RUN, sr.STOPPED):
        for k in range(200):
            lower = q0 - (rng.uniform(0.0, 0.4, nj) if k % 2 else np.inf)
            upper = q0 + (rng.uniform(0.0, 0.4, nj) if k % 2 else np.inf)
            p, rows, rbd, flags, clocks, q_latch, cmd = random_robot(rng, q0, nj, state, lower, upper)
            want = restated(nj, p, rows, rbd, flags, clocks, q_latch, cmd, 0.002)
            f, c, ql, out = bp.BatchedSupervisor.rows_host(itf, p, rows, rbd, flags, clocks, q_latch, cmd, 0.002)
            tag = (robot, state, k)
            assert f.tolist() == [want.state[0], want.cause[0], want.unsafe[0], want.ready[0], want.latch[0]], tag
            assert c.tolist() == [want.elapsed[0], want.settled[0]], tag
            got = dict(zip(sr.COMMAND_ROWS, out))
            final = want.state[0]
            if final == sr.INIT:
                assert np.array_equal(ql, want.q_latch[0]), tag
                T = p[sr.RAMP_TIME]
                exact = T == 0 or want.elapsed[0] >= T
                ramped += not exact
                err = np.abs(got["pos_des"] - want.cmd["pos_des"][0])
                bound = 0.0 if exact else 8 * EPS * np.maximum(1.0, np.maximum(np.abs(want.q_latch[0]), np.abs(rows[0])))
                assert np.all(err <= bound), (tag, err.max())
                for name in ("vel_des", "tau_ff", "kp", "kd"):
                    assert np.array_equal(got[name], want.cmd[name][0]), (tag, name)
            else:
                assert np.array_equal(ql, q_latch), tag                      # the latch is INIT's
                for name in sr.COMMAND_ROWS:
                    assert np.array_equal(got[name], want.cmd[name][0], equal_nan=True), (tag, name)
    assert ramped > 20


def test_rows_host_refuses_a_bad_period():
    import bipedal_control_amd as bp
    itf = _model("h1")
    nj = itf.actuatedDofNum
    rows = np.zeros((5, nj))
    for period in (0.0, -0.002, np.nan, np.inf):
        with pytest.raises(bp.BpmpcError) as err:
            bp.BatchedSupervisor.rows_host(itf, sr.DEFAULT_PARAMS, rows, np.zeros(2 * (6 + nj)), [0, 0, 0, 0, 1], [0, 0], np.zeros(nj), None, period)
        assert err.value.status == INVALID and "period" in str(err.value)


def test_supervise_kernel_exists_without_scratch():
    from tests.test_kernel_resources import _kernels
    found = {n.split("(")[0]: (scratch, lds) for n, scratch, vgpr, lds in _kernels() if "k_supervis" in n}
    assert set(found) == {"k_supervise", "k_supervisor_request"}, found
    assert all(scratch == 0 and lds == 0 for scratch, lds in found.values()), found
