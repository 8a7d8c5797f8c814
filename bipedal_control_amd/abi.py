"""ctypes side of the C ABI: the mirrors of its plain structs, and the signature of every function, read from include/bpmpc.h when the library
is loaded.  The header text is the only source of the signatures - nothing here or elsewhere lists them a second time - so a call with a missing
argument, a wrong pointer type or a float for an int raises in Python instead of handing garbage to C, and a plain Python int or float is
converted to the declared C type.  A declaration this module cannot map is an error when the library is bound, never a fallback.
"""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bpmpc.h")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class _Settings(C.Structure):
    _fields_ = [("device", C.c_int), ("max_batch", C.c_int), ("max_nodes", C.c_int), ("sqp_iterations", C.c_int), ("dt", C.c_double),
                ("return_gains", C.c_int), ("profile", C.c_int), ("stream", C.c_void_p), ("reference_kernels", C.c_int),
                ("pipeline_chunks", C.c_int), ("materialize_lq", C.c_int), ("reg_prim", C.c_double), ("solver", C.c_int), ("feedback_policy", C.c_int)]


class _Schedule(C.Structure):
    _fields_ = [("n_events", C.c_int), ("event_times", _dp), ("modes", _ip)]


class _GaitTemplate(C.Structure):
    _fields_ = [("n_modes", C.c_int), ("switching_times", _dp), ("modes", _ip)]


class _Target(C.Structure):
    _fields_ = [("n_points", C.c_int), ("times", _dp), ("states", _dp)]


class Stats(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("iterations", C.c_int), ("status", C.c_int), ("reserved", C.c_int),
                ("merit_before", C.c_double), ("dynamics_sse_before", C.c_double), ("equality_sse_before", C.c_double),
                ("merit_after", C.c_double), ("dynamics_sse_after", C.c_double), ("equality_sse_after", C.c_double),
                ("step_size", C.c_double), ("armijo_descent", C.c_double), ("dx_norm", C.c_double), ("du_norm", C.c_double)]


class _TickOutputs(C.Structure):
    _fields_ = [("x_obs", _dp), ("x_opt", _dp), ("u_opt", _dp), ("joint_cmd", _dp), ("wbc_solution", _dp), ("planned_mode", _ip), ("wbc_status", _ip),
                ("safe", _ip)]


class _SensorInputs(C.Structure):
    NAMES = ("joint_pos", "joint_vel", "quat", "angular_vel_local", "linear_accel_local", "contact", "mode", "feet_heights", "odom_pos", "odom_quat",
             "odom_lin_vel", "odom_ang_vel")
    _fields_ = [(n, _ip if n in ("contact", "mode") else _dp) for n in NAMES]


class _EstimatorOutputs(C.Structure):
    _fields_ = [("rbd", _dp), ("x_hat", _dp), ("cov", _dp), ("xy_reset", _ip)]


class _JointCommand(C.Structure):
    NAMES = ("pos_des", "vel_des", "tau_ff", "kp", "kd", "base_force", "feet_heights")
    _fields_ = [(n, _dp) for n in NAMES]


class _PlantOutputs(C.Structure):
    _fields_ = [("sensors", _SensorInputs), ("rbd", _dp), ("contact_force", _dp)]


class _PlanOutputs(C.Structure):
    _fields_ = [("optimized", _dp), ("desired", _dp), ("footholds", _dp), ("summary", _dp), ("foothold_count", _ip)]


class _SupervisorOutputs(C.Structure):
    _fields_ = [(n, _dp) for n in ("pos_des", "vel_des", "tau_ff", "kp", "kd")] + [(n, _ip) for n in ("state", "cause", "unsafe", "ready", "counts")] + \
               [("elapsed", _dp), ("stream", C.c_void_p)]


# every `typedef struct { ... } bpmpc_X;` of the header and its mirror: what a `bpmpc_X*` parameter is bound to
MIRRORS = {"bpmpc_settings": _Settings, "bpmpc_mode_schedule": _Schedule, "bpmpc_target": _Target, "bpmpc_stats": Stats,
           "bpmpc_gait_template": _GaitTemplate, "bpmpc_tick_outputs": _TickOutputs, "bpmpc_sensor_inputs": _SensorInputs,
           "bpmpc_estimator_outputs": _EstimatorOutputs, "bpmpc_joint_command": _JointCommand, "bpmpc_plant_outputs": _PlantOutputs,
           "bpmpc_plan_outputs": _PlanOutputs, "bpmpc_supervisor_outputs": _SupervisorOutputs}

# (base type, pointer depth) of a declaration without its const; void is a return type only
_CTYPES = {("int", 0): C.c_int, ("double", 0): C.c_double, ("long", 0): C.c_long, ("char", 1): C.c_char_p, ("double", 1): _dp, ("int", 1): _ip,
           ("double", 2): C.POINTER(_dp), ("int", 2): C.POINTER(_ip)}


def declarations(header_path=HEADER):
    """The header's text without its comments and preprocessor lines."""
    with open(header_path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)


def _prototypes(text):
    out = {}
    for ret, name, params in re.findall(r"([^;{}()]+?)\b(bpmpc_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return out


def prototypes(header_path=HEADER):
    """{name: (return type, [parameter declarations])} of every bpmpc_* function the header declares."""
    return _prototypes(declarations(header_path))


def _ctype(decl, opaque, returned=False):
    """The ctypes type of a parameter declaration (`const double* t0`, `const double cmd_vel[4]`, `bpmpc_solver** out`) or of a return type."""
    m = re.fullmatch(r"(?:const )?(\w+) ?(\**) ?(\w+)?(\[\d*\])?", decl)
    if m and not (returned and (m.group(3) or m.group(4))):
        base, depth = m.group(1), len(m.group(2)) + (1 if m.group(4) else 0)
        if (base, depth) in _CTYPES:
            return _CTYPES[base, depth]
        if returned and (base, depth) == ("void", 0):
            return None
        if base in opaque and depth in (1, 2):
            return C.c_void_p if depth == 1 else C.POINTER(C.c_void_p)
        if base in MIRRORS and depth == 1:
            return C.POINTER(MIRRORS[base])
    raise TypeError("include/bpmpc.h: no ctypes type for the %s '%s'" % ("return type" if returned else "parameter", decl))


def bind(lib, strict=True, header_path=HEADER):
    """Sets argtypes and restype of every function the header declares on `lib` (a ctypes library) and returns it.  A declared function the
    library does not export raises AttributeError; with strict=False it is skipped: the mode for a library built from an earlier commit."""
    text = declarations(header_path)
    opaque = set(re.findall(r"typedef\s+struct\s+(bpmpc_\w+)\s+\1\s*;", text))
    for name, (ret, params) in _prototypes(text).items():
        restype, argtypes = _ctype(ret, opaque, returned=True), [_ctype(p, opaque) for p in params]
        if strict or hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib
