"""The ABI of the value function (include/bpmpc.h "Value function") without a device: the header declares the four entry points with the documented
signatures, the library exports them, the typed binding picks them up by itself, and a null handle is refused through the one error path."""
import ctypes as C

from bipedal_control_amd import abi

SIGNATURES = {
    "bpmpc_solver_enable_value_function": ["bpmpc_solver* solver", "int on"],
    "bpmpc_solver_value_function": ["bpmpc_solver* solver", "double* S", "double* s", "double* v", "double* x_lin", "int* status"],
    "bpmpc_solver_device_value_function": ["bpmpc_solver* solver", "double** S_dev", "double** s_dev", "double** v_dev", "double** x_lin_dev", "int** status_dev"],
    "bpmpc_solver_evaluate_value": ["bpmpc_solver* solver", "int batch", "const double* t", "const double* x", "int inputs_on_device", "double* f", "double* dfdx",
                                    "double* dfdxx"],
}


def test_header_declares_the_entry_points():
    protos = abi.prototypes()
    for name, params in SIGNATURES.items():
        assert protos[name] == ("int", params), name


def test_library_exports_them_and_refuses_a_null_handle():
    import bipedal_control_amd as bp
    lib = bp.api.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert lib.bpmpc_solver_evaluate_value.argtypes == [C.c_void_p, C.c_int, dp, dp, C.c_int, dp, dp, dp]
    assert lib.bpmpc_solver_device_value_function.argtypes == [C.c_void_p] + [C.POINTER(dp)] * 4 + [C.POINTER(ip)]
    assert lib.bpmpc_solver_enable_value_function(None, 1) == -1
    assert b"null solver handle" in lib.bpmpc_last_error()
    assert lib.bpmpc_solver_value_function(None, None, None, None, None, None) == -1
    assert lib.bpmpc_solver_device_value_function(None, None, None, None, None, None) == -1
    assert lib.bpmpc_solver_evaluate_value(None, 1, None, None, 0, None, None, None) == -1
    assert lib.bpmpc_solver_stage(None, b"value") == -1
