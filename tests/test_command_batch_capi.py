"""CPU tier of the device-resident target trajectories (bpmpc_command_batch, include/bpmpc.h): the C ABI is declared and exported, the Python
mirror exists, and every call refuses what it can refuse without a GPU - null handles and outputs - with its status and a message, leaving the
caller's outputs as they were.  The argument checks that need a live handle (bad values in host arrays, sizes, sources of x_obs == NULL) are in
tests/test_gpu_command_batch.py::test_argument_checks_change_nothing."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["bpmpc_command_batch_create", "bpmpc_command_batch_destroy", "bpmpc_command_batch_reset", "bpmpc_command_batch_start",
             "bpmpc_command_batch_cmd_vel", "bpmpc_command_batch_goal", "bpmpc_command_batch_set_targets", "bpmpc_command_batch_get_targets",
             "bpmpc_command_batch_get_status", "bpmpc_solver_attach_commands"]
INVALID = -1   # BPMPC_ERR_INVALID_ARGUMENT


def test_functions_are_declared_and_exported():
    import bipedal_control_amd as bp
    from bipedal_control_amd import abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpmpc.h")).read(), flags=re.S)
    assert "typedef struct bpmpc_command_batch bpmpc_command_batch;" in text
    lib = bp.load_library()
    declared = abi.prototypes()
    for name in FUNCTIONS:
        assert name in declared, name + " is not declared"
        assert hasattr(lib, name), "libbpmpc.so does not export " + name
    assert sorted(n for n in declared if "command_batch" in n or n == "bpmpc_solver_attach_commands") == sorted(FUNCTIONS)
    # plain arrays only: no struct of the header is new, so abi.MIRRORS needs no new mirror
    assert all(("bpmpc_" not in p) or p.startswith(("bpmpc_command_batch*", "bpmpc_solver*")) for n in FUNCTIONS for p in declared[n][1])


def test_null_handles_and_outputs_are_refused():
    import bipedal_control_amd as bp
    lib = bp.load_library()
    out = C.c_void_p(123)
    assert lib.bpmpc_command_batch_create(None, 8, C.byref(out)) == INVALID and not out.value
    assert b"null solver" in lib.bpmpc_last_error()
    assert lib.bpmpc_command_batch_create(None, 8, None) == INVALID
    assert b"null output" in lib.bpmpc_last_error()
    d, i = (C.c_double * 64)(*([7.0] * 64)), (C.c_int * 8)(*([7] * 8))
    n = C.c_int(-5)
    calls = {"reset": lambda: lib.bpmpc_command_batch_reset(None),
             "start": lambda: lib.bpmpc_command_batch_start(None, 1, i, d, d, 0),
             "cmd_vel": lambda: lib.bpmpc_command_batch_cmd_vel(None, 1, i, d, d, d, 0.0, 0),
             "goal": lambda: lib.bpmpc_command_batch_goal(None, 1, i, d, d, d, 1),
             "set_targets": lambda: lib.bpmpc_command_batch_set_targets(None, 1, i, i, d, d, 0),
             "get_targets": lambda: lib.bpmpc_command_batch_get_targets(None, 0, d, d, 2, C.byref(n)),
             "get_status": lambda: lib.bpmpc_command_batch_get_status(None, 1, i)}
    for name, call in calls.items():
        assert call() == INVALID, name
        assert lib.bpmpc_last_error() == ("bpmpc_command_batch_%s: null handle" % name).encode(), name
    assert lib.bpmpc_solver_attach_commands(None, None) == INVALID and b"null solver" in lib.bpmpc_last_error()
    assert list(d) == [7.0] * 64 and list(i) == [7] * 8 and n.value == -5      # nothing was written
    lib.bpmpc_command_batch_destroy(None)                   # a no-op, like the other destroy calls


def test_python_mirror_exists():
    import bipedal_control_amd as bp
    c = bp.BatchedCommands
    expected = {"start": ["self", "t", "x", "mask"], "cmdVel": ["self", "cmd", "t", "x", "mask", "time_to_target"], "goal": ["self", "goal", "t", "x", "mask"],
                "setTargets": ["self", "times", "states", "n_points", "mask"], "targets": ["self", "robot"], "reset": ["self"]}
    for name, params in expected.items():
        assert list(inspect.signature(getattr(c, name)).parameters) == params, name
    assert callable(c.status)
    assert list(inspect.signature(c.__init__).parameters) == ["self", "mpc", "max_points"] and inspect.signature(c.__init__).parameters["max_points"].default == 8
    assert bp.BatchedDdpMpc.attachCommands is bp.BatchedSqpMpc.attachCommands
    assert c.SOURCES == ("none", "start", "velocity", "goal", "trajectory")
