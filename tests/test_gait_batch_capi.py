"""CPU tier of the device-resident gait schedules (bpmpc_gait_batch, include/bpmpc.h): the C ABI is declared and exported, refuses
bad arguments without a GPU, the Python mirror exists, and the recalled tick sequence it implements - getModeSchedule(t0 - H, t0 + 2 H),
then a pending GaitReceiver command inserted at (t0 + H, H) - is restated with the oracle's GaitSchedule and agrees with the product's
host GaitSchedule bit for bit."""
import bisect
import ctypes as C
import os
import re

import pytest

from oracle import ingest, reference_py as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = os.path.join(ROOT, "assets", "h1")
FUNCTIONS = ["bpmpc_gait_batch_create", "bpmpc_gait_batch_destroy", "bpmpc_gait_batch_reset", "bpmpc_gait_batch_insert",
             "bpmpc_gait_batch_command", "bpmpc_gait_batch_mode_schedule", "bpmpc_solver_setup_gaits"]
INVALID = -1   # BPMPC_ERR_INVALID_ARGUMENT


def test_functions_are_declared_and_exported():
    import bipedal_control_amd as bp
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpmpc.h")).read(), flags=re.S)
    assert "typedef struct bpmpc_gait_batch bpmpc_gait_batch;" in text
    lib = bp.load_library()
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, text), name + " is not declared"
        assert hasattr(lib, name), "libbpmpc.so does not export " + name


def test_null_and_out_of_range_arguments_are_refused():
    import bipedal_control_amd as bp
    lib = bp.load_library()
    out = C.c_void_p(123)
    assert lib.bpmpc_gait_batch_create(None, None, 0, C.byref(out)) == INVALID and not out.value
    assert lib.bpmpc_gait_batch_create(None, None, 0, None) == INVALID
    d, i = (C.c_double * 4)(), (C.c_int * 4)()
    assert lib.bpmpc_solver_setup_gaits(None, None, 1, 1.0, d, d, d, 0, 0.0, 0) == INVALID
    assert lib.bpmpc_gait_batch_reset(None) == INVALID
    assert lib.bpmpc_gait_batch_insert(None, 1, i, d, d) == INVALID
    assert lib.bpmpc_gait_batch_command(None, 1, i, 0) == INVALID
    assert lib.bpmpc_gait_batch_command(None, 1, i, 1) == INVALID
    n = C.c_int()
    assert lib.bpmpc_gait_batch_mode_schedule(None, 0, d, i, 4, C.byref(n)) == INVALID
    assert lib.bpmpc_gait_batch_mode_schedule(None, -1, None, None, 0, None) == INVALID
    lib.bpmpc_gait_batch_destroy(None)                      # a no-op, like the other destroy calls
    assert b"null" in lib.bpmpc_last_error()


def test_python_mirror_exists():
    import bipedal_control_amd as bp
    g = bp.BatchedGaitSchedule
    for name in ("insertModeSequenceTemplate", "command", "reset", "modeSchedule"):
        assert callable(getattr(g, name)), name
    assert not hasattr(g, "getModeSchedule")                 # the reference's method of that name mutates; modeSchedule does not
    assert callable(bp.BatchedSqpMpc.setup_gaits)
    import inspect
    params = list(inspect.signature(bp.BatchedSqpMpc.setup_gaits).parameters)
    assert params[:5] == ["self", "gait_schedules", "t0", "x0", "cmd_vel"]
    assert {"horizon", "time_to_target", "from_previous", "goal"} <= set(params)


def test_recalled_tick_sequence_matches_the_host_gait_schedule():
    """SolverBase::preRun [OCS2-upstream, recalled]: every setup first asks the reference manager for getModeSchedule(t0 - H, t0 + 2 H),
    then GaitReceiver::preSolverRun inserts a pending command at (finalTime, timeHorizon) = (t0 + H, H).  The restatement with the oracle's
    GaitSchedule and the product's host GaitSchedule (what bpmpc_gait_batch runs per robot on the device) agree bit for bit."""
    import bipedal_control_amd as bp
    itf = bp.BipedalRobotInterface(os.path.join(A, "task.info"), os.path.join(A, "h1_mpc.urdf"), os.path.join(A, "reference.info"))
    m = ingest.build_model(os.path.join(A, "h1_mpc.urdf"), os.path.join(A, "task.info"), os.path.join(A, "reference.info"))
    names = ["stance", "trot", "standing_trot", "flying_trot"]
    lib_o = [ingest.load_gait_template(os.path.join(A, "gait.info"), n) for n in names]
    lib_p = [bp.loadModeSequenceTemplate(os.path.join(A, "gait.info"), n) for n in names]
    go = rp.GaitSchedule(*m["initial_mode_schedule"], m["default_template"], m["phase_transition_stance_time"])
    gp = bp.GaitSchedule(itf)
    H, tick = 1.0, 0.02
    commands = {0: 1, 5: 3, 6: 2, 14: 0, 15: 0, 21: 1, 30: 2}    # tick -> template; two on consecutive ticks, one to the current gait
    pending, on_stance, applied = None, 0, 0
    for k in range(40):
        t0 = 0.3 + k * tick
        eo = go.get_mode_schedule(t0 - H, t0 + 2 * H)
        ep = gp.getModeSchedule(t0 - H, t0 + 2 * H)
        assert list(ep.eventTimes) == eo[0] and list(ep.modeSequence) == eo[1], k
        if pending is not None:                                # GaitReceiver::preSolverRun of this setup, after the window
            on_stance += go.mode_sequence[bisect.bisect_left(go.event_times, t0 + H)] == rp.STANCE
            go.insert_mode_sequence_template(lib_o[pending], t0 + H, H)
            gp.insertModeSequenceTemplate(lib_p[pending], t0 + H, H)
            pending, applied = None, applied + 1
        if k in commands:                                      # arrives between this setup and the next one
            pending = commands[k]
    assert applied >= 3
    eo = go.get_mode_schedule(1.5 - H, 1.5 + 2 * H)
    ep = gp.getModeSchedule(1.5 - H, 1.5 + 2 * H)
    assert list(ep.eventTimes) == eo[0] and list(ep.modeSequence) == eo[1]
    assert on_stance >= 1                                      # a command that found the last phase already in STANCE (no transition)
