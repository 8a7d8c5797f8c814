"""The policy buffer's C ABI (include/bpmpc.h "Policy buffer") without a GPU: every symbol is exported, null handles and null out-pointers are
refused through the one error path, and the Python classes cannot be built without a device."""
import ctypes as C

import pytest

SYMBOLS = ("bpmpc_policy_create", "bpmpc_policy_destroy", "bpmpc_policy_publish", "bpmpc_policy_update", "bpmpc_policy_info",
           "bpmpc_controller_attach_policy")
INVALID = -1


def test_every_symbol_is_declared_and_exported():
    import bipedal_control_amd as bp
    from bipedal_control_amd import abi
    lib = bp.load_library()
    protos = abi.prototypes()
    for name in SYMBOLS:
        assert name in protos, name + " is not declared in include/bpmpc.h"
        assert hasattr(lib, name), "libbpmpc.so does not export " + name
    assert protos["bpmpc_policy_publish"][1] == ["bpmpc_policy* policy", "int batch", "const int* mask", "int inputs_on_device", "int skip_failed"]
    assert protos["bpmpc_policy_update"][1] == ["bpmpc_policy* policy", "int wait", "int* adopted"]


def test_null_arguments_are_refused_with_a_message():
    import bipedal_control_amd as bp
    lib = bp.load_library()
    out, adopted = C.c_void_p(), C.c_int(7)
    fake = C.c_void_p(1)          # never dereferenced: the null argument beside it is refused first
    calls = {
        "create, null solver": lambda: lib.bpmpc_policy_create(None, 4, C.byref(out)),
        "create, null out": lambda: lib.bpmpc_policy_create(fake, 4, None),
        "publish, null policy": lambda: lib.bpmpc_policy_publish(None, 1, None, 0, 0),
        "update, null policy": lambda: lib.bpmpc_policy_update(None, 1, C.byref(adopted)),
        "info, null policy": lambda: lib.bpmpc_policy_info(None, 1, None, None, None),
        "attach, null controller": lambda: lib.bpmpc_controller_attach_policy(None, None),
    }
    for what, call in calls.items():
        lib.bpmpc_solver_run(None)                                   # leaves another message behind
        before = lib.bpmpc_last_error()
        assert call() == INVALID, what
        msg = lib.bpmpc_last_error()
        assert msg and msg != before and (b"policy" in msg or b"attach" in msg), (what, msg)
    assert not out.value and adopted.value == 7
    lib.bpmpc_policy_destroy(None)                                   # like every destroy: a null handle is nothing to do


def test_python_classes_refuse_to_exist_without_a_device():
    import torch
    import bipedal_control_amd as bp
    assert issubclass(bp.PolicyBuffer, bp.api._Handle) and bp.PolicyBuffer._DESTROY == "bpmpc_policy_destroy"
    for name in ("publish", "update", "info"):
        assert callable(getattr(bp.PolicyBuffer, name))
    assert callable(bp.BatchedController.attachPolicy)

    class NoSolver:               # what is left of a solver that could not be built
        _h, batch = None, 0
    with pytest.raises(bp.BpmpcError) as ei:
        bp.PolicyBuffer(NoSolver(), 4)
    assert ei.value.status == INVALID and "null solver" in str(ei.value)
    if not torch.cuda.is_available():
        from bipedal_control_amd import scenarios
        with pytest.raises(bp.BpmpcError) as ei:                    # the way test_capi.py expects it of the solver: the buffer needs one
            bp.PolicyBuffer(bp.BatchedSqpMpc(scenarios.h1_interface(), 2, 16), 2)
        assert ei.value.status == -4 and "no CPU path" in str(ei.value)
