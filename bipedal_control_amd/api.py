"""Host-side mirror of the reference's operator interface for the MPC hot path, over the C ABI (include/bpmpc.h).

Names follow the reference so that code reads like its call sites:
  BipedalRobotInterface(taskFile, urdfFile, referenceFile)   ocs2_bipedal_robot/include/ocs2_bipedal_robot/BipedalRobotInterface.h:56-127
  GaitSchedule.insertModeSequenceTemplate / getModeSchedule  ocs2_bipedal_robot/src/gait/GaitSchedule.cpp:46-102
  BatchedGaitSchedule.command                                one GaitReceiver per robot, ocs2_bipedal_robot/src/gait/GaitReceiver.cpp:49-59
  BatchedCommands.start / cmdVel / goal / setTargets         one stored TargetTrajectories per robot: BipedalController::starting
                                                             (BipedalController.cpp:145,153), TargetTrajectoriesPublisher.h:48-87
  loadModeSequenceTemplate                                   ocs2_bipedal_robot/src/gait/ModeSequenceTemplate.cpp:50-71
  cmdVelToTargetTrajectories / goalToTargetTrajectories      bipedal_controllers/src/TargetTrajectoriesPublisher.cpp:60-99
  BatchedSqpMpc(interface, ...)                              the SqpMpc construction sites bipedal_controllers/src/BipedalController.cpp:303-306
                                                             and ocs2_bipedal_robot_ros/src/BipedalRobotSqpMpcNode.cpp:70, for a batch of problems
Errors: the reference throws std::runtime_error / std::invalid_argument; here every non-zero status of the C ABI
raises BpmpcError carrying bpmpc_last_error().
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from . import abi
from .abi import (Stats, _dp, _EstimatorOutputs, _GaitTemplate, _ip, _JointCommand, _PlantOutputs, _Schedule, _SensorInputs, _Settings,  # noqa: F401
                  _SupervisorOutputs, _Target, _TickOutputs)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

ModeSchedule = namedtuple("ModeSchedule", ["eventTimes", "modeSequence"])
ModeSequenceTemplate = namedtuple("ModeSequenceTemplate", ["switchingTimes", "modeSequence"])
TargetTrajectories = namedtuple("TargetTrajectories", ["timeTrajectory", "stateTrajectory"])
# BatchedSqpMpc.dualSolution (include/bpmpc.h "Dual solution"); the fields are named as the C arrays, `lambda` being a keyword
DualSolution = namedtuple("DualSolution", ["costate", "nu", "nu0", "nu_gain", "residual", "gain_residual", "summary", "status"])
DUAL_ROWS = 16

MODE_NUMBER = {"FLY": 0, "LF": 1, "RF": 2, "STANCE": 3}


class BpmpcError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("bpmpc status %d: %s" % (status, message))
        self.status = status


def library_path():
    return os.path.join(_HERE, "libbpmpc.so")


def load_library():
    """Loads the in-tree HIP library; raises if it has not been built (no fallback of any kind)."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise BpmpcError(-4, "libbpmpc.so is missing - build it with `python -m bipedal_control_amd.build` (hipcc, gfx950)")
        if not os.path.exists(abi.HEADER):
            raise BpmpcError(-4, "include/bpmpc.h is missing - the signatures of libbpmpc.so are bound from it")
        _LIB = abi.bind(C.CDLL(path))
    return _LIB


def _check(rc):
    if rc < 0:
        raise BpmpcError(rc, load_library().bpmpc_last_error().decode())
    return rc


class _Handle:
    """Owner of one opaque handle of the C ABI: `_h`, destroyed by the function a subclass names in _DESTROY."""

    _DESTROY = None

    def __init__(self):
        self._h = C.c_void_p()

    def _call(self, name, *args):
        """lib.<name>(handle, *args), a negative status raised as BpmpcError"""
        return _check(getattr(load_library(), name)(self._h, *args))

    def __del__(self):
        if getattr(self, "_h", None) and _LIB is not None:       # (_LIB is None again while the interpreter shuts down)
            getattr(_LIB, self._DESTROY)(self._h)
            self._h = None


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _restart_arg(a, ctype, count):
    """(pointer, on_device, keep-alive) of a restart argument of `count` int32 (ctype c_int) or float64 entries: a contiguous torch tensor on the
    GPU or any object with __cuda_array_interface__ of that type and size (order its producer against the handle's stream), or a host array."""
    typestr, tname = ("<i4", "torch.int32") if ctype is C.c_int else ("<f8", "torch.float64")
    if hasattr(a, "data_ptr") and getattr(a, "is_cuda", False):
        if str(a.dtype) != tname or not a.is_contiguous() or a.numel() != count:
            raise ValueError("device restart inputs must be contiguous %s tensors of %d elements" % (tname, count))
        return C.cast(C.c_void_p(a.data_ptr()), C.POINTER(ctype)), True, a
    iface = getattr(a, "__cuda_array_interface__", None)
    if iface is not None:
        if iface["typestr"] != typestr or int(np.prod(iface["shape"])) != count or iface.get("strides") not in (None, (int(typestr[-1]),)):
            raise ValueError("device restart inputs must be contiguous %s arrays of %d elements" % (typestr, count))
        return C.cast(C.c_void_p(iface["data"][0]), C.POINTER(ctype)), True, a
    h = np.ascontiguousarray(np.asarray(a).reshape(-1), np.int32 if ctype is C.c_int else np.float64)
    if h.size != count:
        raise ValueError("restart inputs need %d entries, got %d" % (count, h.size))
    return h.ctypes.data_as(C.POINTER(ctype)), False, h


def _count(a):
    return int(np.prod(getattr(a, "shape", np.shape(a))))


def _restart_args(*specs):
    """_restart_arg of every (array, ctype, count) that is not None; all on the device or all on the host."""
    out = [None if a is None else _restart_arg(a, ct, n) for a, ct, n in specs]
    kinds = {o[1] for o in out if o is not None}
    if len(kinds) > 1:
        raise ValueError("restart inputs must all be device tensors or all host arrays")
    return [None if o is None else o[0] for o in out], int(kinds.pop()) if kinds else 0, out


def _shape(a):
    iface = getattr(a, "__cuda_array_interface__", None)
    return tuple(int(n) for n in (a.shape if hasattr(a, "shape") else iface["shape"] if iface is not None else np.shape(a)))


def _rows_args(mask, arrays, width, max_batch):
    """Marshals the rows of a masked per-robot write (bpmpc_wbc_set_params, bpmpc_controller_set_joint_gains): every array of `arrays` has the
    shape [width], [1, width] (one row for every robot written) or [B, width] (a row per robot); mask (None: every robot) has B entries.  B is
    len(mask), else the number of rows, else max_batch.  Returns (batch, n_rows, [mask pointer, row pointers ...], on_device, keep-alive);
    through _restart_args, so device and host inputs are never mixed."""
    shapes = {_shape(a) for a in arrays}
    if len(shapes) != 1:
        raise ValueError("the row arrays must have one shape, got %s" % sorted(shapes))
    shape = shapes.pop()
    if len(shape) not in (1, 2) or shape[-1] != width:
        raise ValueError("rows must have the shape [%d], [1, %d] or [B, %d], got %s" % (width, width, width, list(shape)))
    n_rows = 1 if len(shape) == 1 else shape[0]
    batch = int(np.prod(_shape(mask))) if mask is not None else (n_rows if n_rows > 1 else max_batch)
    if n_rows not in (1, batch) or batch < 1:
        raise ValueError("%d rows for %d robots: one row or a row per robot" % (n_rows, batch))
    ptrs, dev, keep = _restart_args((mask, C.c_int, batch), *[(a, C.c_double, n_rows * width) for a in arrays])
    return batch, n_rows, ptrs, dev, keep


def _param_methods(prefix, stride, get_doc, set_doc, reset_doc=None, stem=""):
    """getParams / setParams / resetParams of a handle class with max_batch, over <prefix>_get_params / _set_params / _reset_params and parameter
    rows of `stride` doubles; the docstrings are the class's own.  With the stem of another table of the handle ("Sensor"): getSensorParams /
    setSensorParams / resetSensorParams over <prefix>_get_sensor_params and the rest."""
    table = stem.lower() + "_" if stem else ""

    def getParams(self, robot=-1):
        row = np.zeros(stride)
        self._call("%s_get_%sparams" % (prefix, table), int(robot), _d(row))
        return row

    def setParams(self, rows, mask=None):
        B, n_rows, (mp, rp), dev, keep = _rows_args(mask, [rows], stride, self.max_batch)
        self._call("%s_set_%sparams" % (prefix, table), B, mp, rp, n_rows, dev)
        del keep

    def resetParams(self):
        self._call("%s_reset_%sparams" % (prefix, table))

    for method, verb, doc in ((getParams, "get", get_doc), (setParams, "set", set_doc), (resetParams, "reset", reset_doc)):
        method.__name__, method.__doc__ = "%s%sParams" % (verb, stem), doc
    return getParams, setParams, resetParams


class _RowParams:
    """What the rows with one named float per entry share: the FIELDS of a subclass name the leading entries of its row of STRIDE doubles, the
    entries behind them are 0, and its DEFAULTS (absent: zeros) are the values without arguments."""

    def __init__(self, **fields):
        unknown = set(fields) - set(self.FIELDS)
        if unknown:
            raise ValueError("unknown parameter(s): %s" % sorted(unknown))
        for name, default in zip(self.FIELDS, getattr(self, "DEFAULTS", (0.0,) * len(self.FIELDS))):
            setattr(self, name, float(fields.get(name, default)))

    @classmethod
    def fromRow(cls, row):
        r = np.asarray(row, float).reshape(-1)
        if r.size != cls.STRIDE:
            raise ValueError("a parameter row has %d entries" % cls.STRIDE)
        return cls(**{name: r[i] for i, name in enumerate(cls.FIELDS)})

    def toRow(self):
        return np.array([float(getattr(self, n)) for n in self.FIELDS] + [0.0] * (self.STRIDE - len(self.FIELDS)))


class WbcParams:
    """A parameter row of the WBC (include/bpmpc.h "Run-time parameters", BPMPC_WBC_PARAM_*) with named fields, so that no caller writes index
    arithmetic: baseKp / baseKd [6] (position x, y, z, orientation x, y, z: WbcBase::setBasePDGains), swingKp / swingKd (setSwingLegPDGains),
    weightSwingLeg / weightBaseAccel / weightContactForce (WeightedWbc::setWeights), and - per robot only in this engine, the reference reads
    them once in loadTasksSetting - frictionCoefficient, contactTolerance (noContactMotionTask.tolerance), torqueLimits [nj / 2]."""

    STRIDE = 32
    FIELDS = ("baseKp", "baseKd", "swingKp", "swingKd", "weightSwingLeg", "weightBaseAccel", "weightContactForce", "frictionCoefficient",
              "contactTolerance", "torqueLimits")
    # what the reference's dynamic_reconfigure server calls the callback with at start-up (BipedalController.cpp:407-478): there these values
    # override task.info from the first tick; here every row starts as task.info and this preset is applied by the caller
    RECONFIGURE_MOTOR_KP, RECONFIGURE_MOTOR_KD = 80.0, 5.0

    def __init__(self, nj, **fields):
        self.nj = int(nj)
        if self.nj not in (10, 12):
            raise ValueError("nj must be 10 or 12")
        unknown = set(fields) - set(self.FIELDS)
        if unknown:
            raise ValueError("unknown parameter(s): %s" % sorted(unknown))
        for name in self.FIELDS:
            setattr(self, name, fields.get(name))

    @classmethod
    def fromRow(cls, row, nj):
        r = np.asarray(row, float).reshape(-1)
        if r.size != cls.STRIDE:
            raise ValueError("a parameter row has %d entries" % cls.STRIDE)
        return cls(nj, baseKp=r[0:6].copy(), baseKd=r[6:12].copy(), swingKp=float(r[12]), swingKd=float(r[13]), weightSwingLeg=float(r[14]),
                   weightBaseAccel=float(r[15]), weightContactForce=float(r[16]), frictionCoefficient=float(r[17]), contactTolerance=float(r[18]),
                   torqueLimits=r[19:19 + int(nj) // 2].copy())

    def toRow(self):
        missing = [n for n in self.FIELDS if getattr(self, n) is None]
        if missing:
            raise ValueError("parameter(s) without a value: %s" % missing)
        r = np.zeros(self.STRIDE)
        for lo, n, name in ((0, 6, "baseKp"), (6, 6, "baseKd"), (19, self.nj // 2, "torqueLimits")):
            v = np.asarray(getattr(self, name), float).reshape(-1)
            if v.size != n:
                raise ValueError("%s needs %d values" % (name, n))
            r[lo:lo + n] = v
        r[12:19] = [self.swingKp, self.swingKd, self.weightSwingLeg, self.weightBaseAccel, self.weightContactForce, self.frictionCoefficient,
                    self.contactTolerance]
        return r

    @classmethod
    def reconfigureDefaults(cls, nj, base=None):
        """The start-up values of the reference's reconfigure server: base kp 0 for x and y and 20 for z and the three orientation axes, base kd 0
        / 0 / 3 / 3 / 3 / 3, swing leg 160 / 18, weights 100 (swing leg) / 1 (base acceleration) / 0.1 (contact force); the leg motors get
        RECONFIGURE_MOTOR_KP / _KD (80 / 5, BatchedController.setLegMotorGains).  The server does not know the friction coefficient, the contact
        tolerance or the torque limits: they are taken from `base` (a row or a WbcParams, e.g. WeightedWbc.getParams()) and stay unset
        without one."""
        rest = {}
        if base is not None:
            b = base if isinstance(base, WbcParams) else cls.fromRow(base, nj)
            rest = dict(frictionCoefficient=b.frictionCoefficient, contactTolerance=b.contactTolerance, torqueLimits=np.array(b.torqueLimits, float))
        return cls(nj, baseKp=np.array([0.0, 0.0, 20.0, 20.0, 20.0, 20.0]), baseKd=np.array([0.0, 0.0, 3.0, 3.0, 3.0, 3.0]), swingKp=160.0, swingKd=18.0,
                   weightSwingLeg=100.0, weightBaseAccel=1.0, weightContactForce=0.1, **rest)


class MpcWeights:
    """A cost-weight row of the MPC (include/bpmpc.h "Per-problem cost weights", BPMPC_SOLVER_WEIGHT_STRIDE): Q [nx, nx] followed by R [nu, nu],
    dense and row major, zeros behind them.  `Q` and `R` are views into `row`, so either may be edited in place."""

    STRIDE = 2 * 24 * 24

    def __init__(self, nx, nu, row=None):
        self.nx, self.nu = int(nx), int(nu)
        self.row = np.zeros(self.STRIDE) if row is None else np.array(row, float).reshape(-1)
        if self.row.size != self.STRIDE:
            raise ValueError("a weight row has %d entries" % self.STRIDE)

    @property
    def Q(self):
        return self.row[:self.nx * self.nx].reshape(self.nx, self.nx)

    @property
    def R(self):
        return self.row[self.nx * self.nx:self.nx * self.nx + self.nu * self.nu].reshape(self.nu, self.nu)

    @classmethod
    def from_model(cls, interface):
        """The model's own weights: what every problem solves under until a row is set."""
        w = cls(interface.stateDim, interface.inputDim)
        Q, R = interface.costMatrices()
        w.Q[:], w.R[:] = Q, R
        return w

    @classmethod
    def from_task(cls, interface, Q_task, R_task):
        """From the two matrices as task.info spells them (bpmpc_model_compose_weights): Q_task [nx, nx] as given, R_task [24, 24] - contact forces,
        then contact-point velocities - mapped as R = blkdiag(R_F, J^T R_v J) with the contact Jacobians at initialState, like the model's own R."""
        q, r = _f64(Q_task).reshape(-1), _f64(R_task).reshape(-1)
        if q.size != interface.stateDim ** 2 or r.size != 24 * 24:
            raise ValueError("Q_task must be [%d, %d] and R_task [24, 24]" % (interface.stateDim, interface.stateDim))
        w = cls(interface.stateDim, interface.inputDim)
        interface._call("bpmpc_model_compose_weights", _d(q), _d(r), _d(w.row))
        return w

    def scaled(self, q=1.0, r=1.0):
        """A copy with Q and R scaled: a factor, a vector of nx (nu) factors d - the congruence diag(sqrt d) W diag(sqrt d), which scales diagonal
        entry i by d_i and keeps the weight symmetric and definite - or a full [n, n] array of per-entry factors."""
        out = MpcWeights(self.nx, self.nu, self.row)
        for block, f in ((out.Q, q), (out.R, r)):
            f = np.asarray(f, float)
            if f.ndim == 1:
                if f.size != block.shape[0] or (f < 0).any():
                    raise ValueError("per-coordinate factors: %d values that are not negative" % block.shape[0])
                f = np.sqrt(np.outer(f, f))
            block *= f
        return out


class ConeParams(_RowParams):
    """A friction-cone row of the MPC (include/bpmpc.h "Per-problem cone parameters", BPMPC_SOLVER_CONE_*): frictionCoefficient, regularization,
    gripperForce and hessianShift of the cone (frictionConeSoftConstraint of task.info and the constants behind it), mu and delta of its relaxed
    barrier (with the hard cone: of the SQP solver's inequality penalty).  `row` is the row of STRIDE doubles, two zeros behind the six values."""

    STRIDE = 8
    FIELDS = ("frictionCoefficient", "regularization", "gripperForce", "hessianShift", "mu", "delta")

    @property
    def row(self):
        return self.toRow()

    @classmethod
    def from_model(cls, interface):
        """The model's own parameters as the solver's kernels read them - what every problem solves under until a row is set: with the hard cone
        sqp.inequalityConstraintMu / Delta as the barrier and no Hessian shift."""
        p = cls.fromRow(np.concatenate([interface.get("cone"), np.zeros(2)]))
        hard = interface.get("hard_cone")
        if hard[0] != 0.0:
            p.hessianShift, p.mu, p.delta = 0.0, float(hard[1]), float(hard[2])
        return p

    def replaced(self, **fields):
        """A copy with the named fields replaced."""
        return ConeParams(**dict({n: getattr(self, n) for n in self.FIELDS}, **fields))


class BipedalRobotInterface(_Handle):
    """Problem definition: model constants + settings (BipedalRobotInterface.cpp:67-204)."""

    _DESTROY = "bpmpc_model_destroy"

    def __init__(self, taskFile, urdfFile, referenceFile, useHardFrictionConeConstraint=False):
        """Fourth argument as in the reference (BipedalRobotInterface.h:66-69): friction cones as inequality constraints, which the SQP
        solver penalises with sqp.inequalityConstraintMu / Delta (include/bpmpc.h bpmpc_model_create_ex)."""
        super().__init__()
        self.useHardFrictionConeConstraint = bool(useHardFrictionConeConstraint)
        _check(load_library().bpmpc_model_create_ex(str(urdfFile).encode(), str(taskFile).encode(), str(referenceFile).encode(),
                                                    1 if useHardFrictionConeConstraint else 0, C.byref(self._h)))
        nx, nu, nc, nj = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._call("bpmpc_model_dims", C.byref(nx), C.byref(nu), C.byref(nc), C.byref(nj))
        self.stateDim, self.inputDim, self.numThreeDofContacts, self.actuatedDofNum = nx.value, nu.value, nc.value, nj.value
        self.taskFile, self.urdfFile, self.referenceFile = str(taskFile), str(urdfFile), str(referenceFile)

    @property
    def handle(self):
        return self._h

    def get(self, name, capacity=4096):
        out = np.zeros(capacity)
        n = self._call("bpmpc_model_get", name.encode(), _d(out), capacity)
        return out[:n].copy()

    def getInitialState(self):
        return self.get("initial_state")

    def jointNames(self):
        buf = C.create_string_buffer(256)
        names = []
        for j in range(self.actuatedDofNum):
            self._call("bpmpc_model_joint_name", j, buf, 256)
            names.append(buf.value.decode())
        return names

    def robotMass(self):
        return float(self.get("robot_mass")[0])

    def sqpSettings(self):
        v = self.get("sqp")
        return dict(dt=v[0], sqpIteration=int(v[1]), deltaTol=v[2], g_max=v[3], g_min=v[4], useFeedbackPolicy=bool(v[5]),
                    projectStateInputEqualityConstraints=bool(v[6]), integratorType="RK2",
                    alpha_decay=v[8], alpha_min=v[9], gamma_c=v[10], armijoFactor=v[11], costTol=v[12])

    _IPM_FIELDS = ("dt", "ipmIteration", "deltaTol", "g_max", "g_min", "computeLagrangeMultipliers", "useFeedbackPolicy", "initialBarrierParameter",
                   "targetBarrierParameter", "barrierLinearDecreaseFactor", "barrierSuperlinearDecreasePower", "barrierReductionCostTol",
                   "barrierReductionConstraintTol", "fractionToBoundaryMargin", "usePrimalStepSizeForDual", "initialSlackLowerBound",
                   "initialDualLowerBound", "initialSlackMarginRate", "initialDualMarginRate", "nThreads", "threadPriority")
    _DDP_FIELDS = ("algorithm", "maxNumIterations", "minRelCost", "constraintTolerance", "AbsTolODE", "RelTolODE", "timeStep", "maxNumStepsPerSecond",
                   "backwardPassIntegratorType", "constraintPenaltyInitialValue", "constraintPenaltyIncreaseRate", "preComputeRiccatiTerms",
                   "useFeedbackPolicy", "strategy", "lineSearch.minStepLength", "lineSearch.maxStepLength", "lineSearch.hessianCorrectionStrategy",
                   "lineSearch.hessianCorrectionMultiple", "nThreads", "threadPriority")
    _DDP_ENUMS = {"algorithm": ("SLQ", "ILQR"), "strategy": ("LINE_SEARCH", "LEVENBERG_MARQUARDT"),
                  "backwardPassIntegratorType": ("ODE45", "EULER", "ODE45_OCS2", "ADAMS_BASHFORTH", "BULIRSCH_STOER", "MODIFIED_MIDPOINT", "RK4", "RK5_VARIABLE",
                                                 "ADAMS_BASHFORTH_MOULTON"),
                  "lineSearch.hessianCorrectionStrategy": ("DIAGONAL_SHIFT", "CHOLESKY_MODIFICATION", "EIGENVALUE_MODIFICATION", "GERSHGORIN_MODIFICATION")}
    _INT_FIELDS = {"ipmIteration", "nThreads", "threadPriority", "maxNumIterations", "maxNumStepsPerSecond"}
    _BOOL_FIELDS = {"computeLagrangeMultipliers", "useFeedbackPolicy", "usePrimalStepSizeForDual", "preComputeRiccatiTerms"}

    def _settings(self, block, fields, enums=()):
        v = self.get(block)
        out = {}
        for name, x in zip(fields, v):
            if name in enums:
                out[name] = enums[name][int(x)]
            elif name in self._BOOL_FIELDS:
                out[name] = bool(x)
            elif name in self._INT_FIELDS:
                out[name] = int(x)
            else:
                out[name] = float(x)
        return out

    def ipmSettings(self):
        """The `ipm` block of task.info as the reference loads it (BipedalRobotInterface.cpp:100, accessor BipedalRobotInterface.h:80).
        The reference constructs no IPM solver; neither does this engine: the settings are loaded and exposed, nothing consumes them."""
        return self._settings("ipm", self._IPM_FIELDS)

    def ddpSettings(self):
        """The `ddp` block of task.info (BipedalRobotInterface.cpp:98); consumed in the reference by the stand-alone DDP node
        (BipedalRobotDdpMpcNode.cpp:70-74), a solver this engine does not have."""
        return self._settings("ddp", self._DDP_FIELDS, self._DDP_ENUMS)

    def rolloutSettings(self):
        v = self.get("rollout")
        return dict(AbsTolODE=v[0], RelTolODE=v[1], timeStep=v[2], maxNumStepsPerSecond=int(v[3]))

    def mpcSettings(self):
        return dict(timeHorizon=float(self.get("time_horizon")[0]))

    def costMatrices(self):
        nx, nu = self.stateDim, self.inputDim
        return self.get("Q").reshape(nx, nx), self.get("R").reshape(nu, nu)

    def checkConeParams(self, row):
        """The host check of BatchedSqpMpc.setConeParams alone (bpmpc_model_check_cone_params; no device): raises BpmpcError(-1) with the entry and
        the reason, else returns None."""
        r = _f64(row.row if isinstance(row, ConeParams) else row).reshape(-1)
        if r.size != ConeParams.STRIDE:
            raise ValueError("a cone row has %d entries" % ConeParams.STRIDE)
        self._call("bpmpc_model_check_cone_params", _d(r))

    # --- target trajectories (TargetTrajectoriesPublisher.cpp:60-99)
    def cmdVelToTargetTrajectories(self, cmdVel, time, state, timeToTarget=None):
        if timeToTarget is None:
            timeToTarget = self.mpcSettings()["timeHorizon"]
        cmd, x = _f64(cmdVel), _f64(state)
        times, states = np.zeros(2), np.zeros((2, self.stateDim))
        self._call("bpmpc_cmd_vel_to_targets", _d(cmd), time, _d(x), timeToTarget, _d(times), _d(states))
        return TargetTrajectories(times, states)

    def goalToTargetTrajectories(self, goal, time, state):
        g, x = _f64(goal), _f64(state)
        times, states = np.zeros(2), np.zeros((2, self.stateDim))
        self._call("bpmpc_goal_to_targets", _d(g), time, _d(x), _d(times), _d(states))
        return TargetTrajectories(times, states)


def loadModeSequenceTemplate(filename, topicName):
    times, modes, n = np.zeros(65), np.zeros(64, np.int32), C.c_int()
    _check(load_library().bpmpc_gait_load_template(str(filename).encode(), topicName.encode(), _d(times), _i(modes), 64, C.byref(n)))
    return ModeSequenceTemplate(times[:n.value + 1].copy(), modes[:n.value].copy())


class GaitSchedule(_Handle):
    """GaitSchedule(initModeSchedule, defaultModeSequenceTemplate, phaseTransitionStanceTime) as loaded by
    BipedalRobotInterface::loadGaitSchedule (BipedalRobotInterface.cpp:209-234)."""

    _DESTROY = "bpmpc_gait_destroy"

    def __init__(self, interface):
        super().__init__()
        _check(load_library().bpmpc_gait_create(interface.handle, C.byref(self._h)))

    def insertModeSequenceTemplate(self, modeSequenceTemplate, startTime, finalTime):
        t, m = _f64(modeSequenceTemplate.switchingTimes), np.ascontiguousarray(modeSequenceTemplate.modeSequence, np.int32)
        self._call("bpmpc_gait_insert_template", _d(t), _i(m), len(m), startTime, finalTime)

    def getModeSchedule(self, lowerBoundTime, upperBoundTime, capacity=4096):
        ev, ms, n = np.zeros(capacity), np.zeros(capacity, np.int32), C.c_int()
        self._call("bpmpc_gait_mode_schedule", lowerBoundTime, upperBoundTime, _d(ev), _i(ms), capacity, C.byref(n))
        return ModeSchedule(ev[:n.value].copy(), ms[:n.value + 1].copy())


class BatchedGaitSchedule(_Handle):
    """One GaitSchedule per robot of a BatchedSqpMpc, kept on the device (bpmpc_gait_batch): gait commands with the semantics of
    GaitReceiver (GaitReceiver.cpp:49-59) take effect in the solver's setup_gaits.  `gaits` is the template library (a list of
    ModeSequenceTemplate); robots refer to a template by its index."""

    _DESTROY = "bpmpc_gait_batch_destroy"

    def __init__(self, mpc, gaits):
        self.mpc, self.gaits, self.max_batch = mpc, list(gaits), mpc.max_batch
        keep, tm = [], (_GaitTemplate * max(1, len(self.gaits)))()
        for i, g in enumerate(self.gaits):
            sw, mo = _f64(g.switchingTimes), np.ascontiguousarray(g.modeSequence, np.int32)
            keep += [sw, mo]
            tm[i] = _GaitTemplate(len(mo), _d(sw), _i(mo))
        super().__init__()
        _check(load_library().bpmpc_gait_batch_create(mpc._h, tm, len(self.gaits), C.byref(self._h)))

    def _robots(self, *arrays):
        shape = np.broadcast(*[np.asarray(a) for a in arrays]).shape
        return (self.max_batch,) if shape == () else shape

    def insertModeSequenceTemplate(self, gait, startTime, finalTime):
        """GaitSchedule::insertModeSequenceTemplate(gaits[gait[b]], startTime[b], finalTime[b]) for robots 0 .. len - 1 (scalars: every
        robot), applied by the next setup before its getModeSchedule; gait[b] < 0 leaves robot b's pending insert as it is."""
        shape = self._robots(gait, startTime, finalTime)
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(gait, np.int32), shape))
        st, fi = _f64(np.broadcast_to(np.asarray(startTime, float), shape)), _f64(np.broadcast_to(np.asarray(finalTime, float), shape))
        self._call("bpmpc_gait_batch_insert", len(g), _i(g), _d(st), _d(fi))

    def command(self, gait):
        """GaitReceiver::mpcModeSequenceCallback for robots 0 .. len(gait) - 1: gait[b] >= 0 becomes robot b's pending template (the latest
        wins), < 0 leaves it as it is.  A numpy array, or a contiguous int32 device array: a torch.int32 tensor on the GPU or any object with
        __cuda_array_interface__ (order its producer against the solver's stream)."""
        iface = getattr(gait, "__cuda_array_interface__", None)
        if iface is not None:
            shape = tuple(iface["shape"])
            if iface["typestr"] != "<i4" or len(shape) != 1 or iface.get("strides") not in (None, (4,)):
                raise ValueError("device gait commands must be a contiguous one-dimensional int32 array")
            self._call("bpmpc_gait_batch_command", int(shape[0]), C.cast(C.c_void_p(iface["data"][0]), _ip), 1)
            return
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(gait, np.int32), self._robots(gait)))
        self._call("bpmpc_gait_batch_command", len(g), _i(g), 0)

    def reset(self):
        """Every robot back to GaitSchedule(initialModeSchedule, defaultModeSequenceTemplate); nothing pending."""
        self._call("bpmpc_gait_batch_reset")

    def restart(self, mask):
        """Robots with mask[b] != 0 (robots 0 .. len(mask) - 1) back to their state after create / reset, their pending insert and command dropped
        (bpmpc_gait_batch_restart); applied by the next setup_gaits before anything recorded after this call.  A numpy array or an int32 device
        tensor (its read-back waits for that setup)."""
        n = _count(mask)
        (mp,), dev, keep = _restart_args((mask, C.c_int, n))
        self._call("bpmpc_gait_batch_restart", n, mp, dev)
        del keep

    def modeSchedule(self, robot, capacity=1024):
        """Robot's schedule after the last setup (does not mutate anything, unlike the reference's getModeSchedule)."""
        ev, ms, n = np.zeros(capacity), np.zeros(capacity, np.int32), C.c_int()
        self._call("bpmpc_gait_batch_mode_schedule", int(robot), _d(ev), _i(ms), capacity, C.byref(n))
        return ModeSchedule(ev[:n.value].copy(), ms[:n.value + 1].copy())


def _on_device(a):
    return a is not None and (bool(getattr(a, "is_cuda", False)) or hasattr(a, "__cuda_array_interface__"))


class BatchedCommands(_Handle):
    """One stored TargetTrajectories per robot of a BatchedSqpMpc, kept on the device (bpmpc_command_batch): `start` is
    BipedalController::starting, `cmdVel` and `goal` are the two messages of TargetTrajectoriesPublisher - computed once, from the observation
    passed with them - and `setTargets` stores any trajectory.  After mpc.attachCommands(commands) the solver's setup_commands and setup_gaits
    take every robot's target from here.  Inputs are numpy arrays (validated; the call returns when they have been read) or device arrays -
    DeviceArray, GPU tensors, anything with __cuda_array_interface__ (not validated, only enqueued on the solver's stream); never mixed.
    Robots are 0 .. B - 1 with B = len(mask), else the rows of the inputs, else the solver's batch; mask[b] == 0 leaves robot b untouched."""

    _DESTROY = "bpmpc_command_batch_destroy"
    SOURCES = ("none", "start", "velocity", "goal", "trajectory")      # status()[:, 2]

    def __init__(self, mpc, max_points=8):
        self.mpc, self.max_batch, self.max_points, self.nx = mpc, mpc.max_batch, int(max_points), mpc.nx
        super().__init__()
        _check(load_library().bpmpc_command_batch_create(mpc._h, self.max_points, C.byref(self._h)))

    def _message(self, name, rows, t, x, mask, *tail):
        given = [a for a in (rows, t, x, mask) if a is not None]
        if mask is not None:
            B = int(np.prod(_shape(mask)))
        else:
            lead = [_shape(a)[0] for a, nd in ((rows, 2), (x, 2), (t, 1)) if a is not None and len(_shape(a)) == nd]
            B = lead[0] if lead else (self.mpc.batch or self.max_batch)
        if not any(_on_device(a) for a in given):
            t = _f64(np.broadcast_to(np.asarray(t, float), (B,)))
            rows = None if rows is None else _f64(np.broadcast_to(np.asarray(rows, float), (B, 4)))
            x = None if x is None else _f64(np.broadcast_to(np.asarray(x, float), (B, self.nx)))
        (mp, rp, tp, xp), dev, keep = _restart_args((mask, C.c_int, B), (rows, C.c_double, B * 4), (t, C.c_double, B), (x, C.c_double, B * self.nx))
        self._call(name, B, mp, *([] if rows is None else [rp]), tp, xp, *tail, dev)
        del keep

    def start(self, t, x=None, mask=None):
        """The target becomes the single point (t[b], x[b]).  x=None: the observations already on the device (the last controller tick,
        otherwise the end states of the last rollout), as setup_commands(x0=None) reads them."""
        self._message("bpmpc_command_batch_start", None, t, x, mask)

    def cmdVel(self, cmd, t, x=None, mask=None, time_to_target=0.0):
        """cmdVelToTargetTrajectories(cmd[b] = (vx, vy, vz, yaw rate), (t[b], x[b])) reaching time_to_target ahead (<= 0: mpc.timeHorizon);
        a message at t == 0.0 is dropped and counted, as the reference's publisher drops it."""
        self._message("bpmpc_command_batch_cmd_vel", cmd, t, x, mask, float(time_to_target))

    def goal(self, goal, t, x=None, mask=None):
        """goalToTargetTrajectories(goal[b] = (x, y, unused, yaw), (t[b], x[b])): the reach time is fixed here, once."""
        self._message("bpmpc_command_batch_goal", goal, t, x, mask)

    def setTargets(self, times, states, n_points=None, mask=None):
        """Stores trajectories as they are: times [B, P] (or [P]: one for every robot written), states [B, P, nx] with P <= max_points, of which
        robot b uses the first n_points[b] (None: all P).  Device arrays have the handle's strides, [B, max_points] and [B, max_points, nx], and
        come with n_points [B] (int32)."""
        if any(_on_device(a) for a in (times, states, n_points, mask)):
            B = _shape(times)[0]
            if n_points is None or _shape(times) != (B, self.max_points):
                raise ValueError("device trajectories need n_points and the strides [B, %d] / [B, %d, %d]" % (self.max_points, self.max_points, self.nx))
        else:
            times, states = np.asarray(times, float), np.asarray(states, float)
            if times.ndim == 1:
                B = int(np.prod(_shape(mask))) if mask is not None else (self.mpc.batch or self.max_batch)
                times, states = np.broadcast_to(times, (B,) + times.shape), np.broadcast_to(states, (B,) + states.shape)
            B, P = times.shape
            if P > self.max_points or states.shape != (B, P, self.nx):
                raise ValueError("times [B, P] and states [B, P, %d] with P <= %d, got %s and %s" % (self.nx, self.max_points, times.shape, states.shape))
            n_points = np.ascontiguousarray(np.broadcast_to(np.asarray(P if n_points is None else n_points, np.int32), (B,)))
            tt, xx = np.zeros((B, self.max_points)), np.zeros((B, self.max_points, self.nx))
            tt[:, :P], xx[:, :P] = times, states
            times, states = tt, xx
        (mp, np_, tp, xp), dev, keep = _restart_args((mask, C.c_int, B), (n_points, C.c_int, B), (times, C.c_double, B * self.max_points),
                                                     (states, C.c_double, B * self.max_points * self.nx))
        self._call("bpmpc_command_batch_set_targets", B, mp, np_, tp, xp, dev)
        del keep

    def targets(self, robot):
        """Robot's stored trajectory, (times [n], states [n, nx]); n = 0 after create / reset.  Synchronises."""
        ts, xs, n = np.zeros(self.max_points), np.zeros((self.max_points, self.nx)), C.c_int()
        self._call("bpmpc_command_batch_get_targets", int(robot), _d(ts), _d(xs), self.max_points, C.byref(n))
        return TargetTrajectories(ts[:n.value].copy(), xs[:n.value].copy())

    def status(self, batch=None):
        """[B, 4] int32 per robot: messages applied, messages dropped, source of the stored target (an index into SOURCES), stored points."""
        B = int(batch or self.max_batch)
        st = np.zeros((B, 4), np.int32)
        self._call("bpmpc_command_batch_get_status", B, _i(st))
        return st

    def reset(self):
        """Every robot back to no target, counters 0."""
        self._call("bpmpc_command_batch_reset")


def swing_reference(interface, modeSchedule, times):
    """SwingTrajectoryPlanner::update + getZpositionConstraint / getZvelocityConstraint (SwingTrajectoryPlanner.cpp:50-118)."""
    ev, ms, t = _f64(modeSchedule.eventTimes), np.ascontiguousarray(modeSchedule.modeSequence, np.int32), _f64(times)
    z, zd = np.zeros((len(t), 4)), np.zeros((len(t), 4))
    _check(load_library().bpmpc_swing_reference(interface.handle, _d(ev), _i(ms), len(ev), _d(t), len(t), _d(z), _d(zd)))
    return z, zd


def time_discretization_with_events(initTime, finalTime, dt, eventTimes, capacity=8192):
    ev = _f64(eventTimes)
    t, e, n = np.zeros(capacity), np.zeros(capacity, np.int32), C.c_int()
    _check(load_library().bpmpc_time_grid(initTime, finalTime, dt, _d(ev), len(ev), _d(t), _i(e), capacity, C.byref(n)))
    return t[:n.value].copy(), e[:n.value].copy()


class BatchedSqpMpc(_Handle):
    # (the DDP variant is the same handle with solver="ddp": BatchedDdpMpc below)
    """A batch of independent SqpMpc instances on one MI355X.  `run` plays the role of MPC_BASE::run(t, x) /
    MPC_MRT_Interface::advanceMpc() (BipedalController.cpp:339) for every problem of the batch at once."""

    _DESTROY = "bpmpc_solver_destroy"

    def __init__(self, interface, max_batch, max_nodes, sqp_iterations=0, dt=0.0, return_gains=False, profile=False, device=0, stream=None,
                 reference_kernels=False, pipeline_chunks=0, materialize_lq=False, reg_prim=0.0, solver="sqp", feedback_policy=None):
        """solver: "sqp" (SqpMpc, default) or "ddp" (GaussNewtonDDP_MPC of BipedalRobotDdpMpcNode.cpp:70-71: one ILQR iteration per run, see
        bpmpc_settings.solver in include/bpmpc.h).  feedback_policy: None = sqp.useFeedbackPolicy of task.info, True / False overrides it for the warm
        start, the policy rollout and the controller built from the solution alike."""
        lib = load_library()
        self.interface = interface
        self.max_batch, self.max_nodes = int(max_batch), int(max_nodes)
        self.nx, self.nu = interface.stateDim, interface.inputDim
        self.return_gains = bool(return_gains)
        if stream is not None and int(stream) == 0:
            # the C ABI reads a NULL stream as "create your own": the legacy default stream cannot be passed.  Work that must be
            # ordered against torch has to run on an explicit stream (torch.cuda.Stream().cuda_stream), see bench.py.
            raise ValueError("stream=0 (the default stream) cannot be handed over; pass an explicit stream handle or None for a solver-owned stream")
        st = _Settings(int(device), self.max_batch, self.max_nodes, int(sqp_iterations), float(dt), int(bool(return_gains)), int(profile),
                       C.c_void_p(int(stream)) if stream is not None else None, int(bool(reference_kernels)), int(pipeline_chunks), int(bool(materialize_lq)), float(reg_prim),
                       {"sqp": 0, "ddp": 1}[solver], 0 if feedback_policy is None else (1 if feedback_policy else 2))
        self.solver = solver
        super().__init__()
        _check(lib.bpmpc_solver_create(interface.handle, C.byref(st), C.byref(self._h)))
        self._keep = None
        self.batch = 0

    # ---- argument marshalling
    def _marshal(self, t0, x0, modeSchedules, targetTrajectories, warm_x, warm_u):
        x0 = _f64(x0).reshape(-1, self.nx)
        B = x0.shape[0]
        t0 = _f64(np.broadcast_to(np.asarray(t0, float), (B,)))
        if isinstance(modeSchedules, ModeSchedule):
            modeSchedules = [modeSchedules]
        if isinstance(targetTrajectories, TargetTrajectories):
            targetTrajectories = [targetTrajectories] * B
        if len(targetTrajectories) != B:
            raise ValueError("%d target trajectories for %d problems (pass one per problem, or a single TargetTrajectories to share)" % (len(targetTrajectories), B))
        if len(modeSchedules) not in (1, B):
            raise ValueError("%d mode schedules for %d problems (pass one to share, or one per problem)" % (len(modeSchedules), B))
        keep = [t0, x0]
        sched = (_Schedule * len(modeSchedules))()
        for i, ms in enumerate(modeSchedules):
            ev, mo = _f64(ms.eventTimes), np.ascontiguousarray(ms.modeSequence, np.int32)
            keep += [ev, mo]
            sched[i] = _Schedule(len(ev), _d(ev), _i(mo))
        tg = (_Target * B)()
        for i, tt in enumerate(targetTrajectories):
            ts, xs = _f64(tt.timeTrajectory), _f64(tt.stateTrajectory)
            keep += [ts, xs]
            tg[i] = _Target(len(ts), _d(ts), _d(xs))
        wx = wu = None
        if warm_x is not None:
            if warm_u is None:
                raise ValueError("warm_x and warm_u must be given together")
            wx, wu = _f64(warm_x), _f64(warm_u)
            if wx.size != B * (self.max_nodes + 1) * self.nx or wu.size != B * self.max_nodes * self.nu:
                raise ValueError("warm start arrays must have the solver's strides: x [%d, %d, %d], u [%d, %d, %d]"
                                 % (B, self.max_nodes + 1, self.nx, B, self.max_nodes, self.nu))
            keep += [wx, wu]
        return B, t0, x0, sched, len(modeSchedules), tg, wx, wu, keep

    def setup(self, t0, x0, modeSchedules, targetTrajectories, horizon=None, warm_x=None, warm_u=None):
        if horizon is None:
            horizon = self.interface.mpcSettings()["timeHorizon"]
        B, t0, x0, sched, ns, tg, wx, wu, keep = self._marshal(t0, x0, modeSchedules, targetTrajectories, warm_x, warm_u)
        self._call("bpmpc_solver_setup", B, horizon, _d(t0), _d(x0), sched, ns, tg, _d(wx), _d(wu))
        self.batch = B
        return self.layout()

    def setup_from_previous(self, t0, x0, modeSchedules, targetTrajectories, horizon=None):
        """Receding-horizon step (MPC_BASE::run with mpc.coldStart false): new measured states / schedules / targets, initial
        iterate shifted on the device from the previous solve of this handle (bpmpc_solver_setup_from_previous)."""
        if horizon is None:
            horizon = self.interface.mpcSettings()["timeHorizon"]
        B, t0, x0, sched, ns, tg, _, _, keep = self._marshal(t0, x0, modeSchedules, targetTrajectories, None, None)
        self._call("bpmpc_solver_setup_from_previous", B, horizon, _d(t0), _d(x0), sched, ns, tg)
        self.batch = B
        return self.layout()

    def setup_commands(self, t0, x0, gaits, gait_of_problem, gait_start, cmd_vel, horizon=None, time_to_target=0.0, from_previous=False, goal=False):
        """The whole pre-pass on the device (bpmpc_solver_setup_commands): `gaits` is a list of ModeSequenceTemplate, problem b
        follows gaits[gait_of_problem[b]] inserted at gait_start[b] (index < 0: initial schedule only) and tracks the velocity
        command cmd_vel[b] = (vx, vy, vz, yaw rate), or with goal=True moves to the pose (x, y, -, yaw) like goalToTargetTrajectories."""
        if horizon is None:
            horizon = self.interface.mpcSettings()["timeHorizon"]
        if x0 is None:                      # continue from the end states of the last rollout (device-resident)
            B = self.batch
        else:
            x0 = _f64(x0).reshape(-1, self.nx)
            B = x0.shape[0]
        t0 = _f64(np.broadcast_to(np.asarray(t0, float), (B,)))
        gop = np.ascontiguousarray(np.broadcast_to(np.asarray(gait_of_problem, np.int32), (B,)))
        gst = _f64(np.broadcast_to(np.asarray(gait_start, float), (B,)))
        cmd = None if cmd_vel is None else _f64(np.broadcast_to(np.asarray(cmd_vel, float), (B, 4)))      # None: an attached BatchedCommands
        keep, tm = [], (_GaitTemplate * max(1, len(gaits)))()
        for i, g in enumerate(gaits):
            sw, mo = _f64(g.switchingTimes), np.ascontiguousarray(g.modeSequence, np.int32)
            keep += [sw, mo]
            tm[i] = _GaitTemplate(len(mo), _d(sw), _i(mo))
        self._call("bpmpc_solver_setup_commands", B, horizon, _d(t0), _d(x0), tm, len(gaits), _i(gop), _d(gst), _d(cmd), int(bool(goal)), time_to_target,
                   int(bool(from_previous)))
        self.batch = B
        return self.layout()

    def setup_gaits(self, gait_schedules, t0, x0, cmd_vel, horizon=None, time_to_target=0.0, from_previous=False, goal=False):
        """setup_commands with every robot's schedule taken from a BatchedGaitSchedule of this solver (bpmpc_solver_setup_gaits): its pending
        inserts, getModeSchedule(t0 - H, t0 + 2 H) as the window of this setup, then its pending commands at (t0 + H, H)."""
        if horizon is None:
            horizon = self.interface.mpcSettings()["timeHorizon"]
        if x0 is None:                      # continue from the end states of the last rollout or tick (device-resident)
            B = self.batch
        else:
            x0 = _f64(x0).reshape(-1, self.nx)
            B = x0.shape[0]
        t0 = _f64(np.broadcast_to(np.asarray(t0, float), (B,)))
        cmd = None if cmd_vel is None else _f64(np.broadcast_to(np.asarray(cmd_vel, float), (B, 4)))      # None: an attached BatchedCommands
        self._call("bpmpc_solver_setup_gaits", gait_schedules._h, B, horizon, _d(t0), _d(x0), _d(cmd), int(bool(goal)), time_to_target, int(bool(from_previous)))
        self.batch = B
        return self.layout()

    def attachCommands(self, commands):
        """setup_commands and setup_gaits take every robot's target from `commands` (a BatchedCommands of this solver) and ignore cmd_vel (None
        is accepted), goal and time_to_target (bpmpc_solver_attach_commands); None detaches: the solver runs what it ran before.  The solver does
        not keep `commands` alive: destroying it detaches it."""
        self._call("bpmpc_solver_attach_commands", None if commands is None else commands._h)

    def rollout(self, duration, t_start=None, x_start=None, fetch=True):
        """MRT_BASE::rolloutPolicy for the batch (bpmpc_solver_rollout): returns (x_end, u_end, steps[batch, 2]); fetch=False only
        enqueues (the end states stay on the device for setup_commands(x0=None))."""
        B = self.batch
        ts = None if t_start is None else _f64(np.broadcast_to(np.asarray(t_start, float), (B,)))
        xs = None if x_start is None else _f64(x_start).reshape(B, self.nx)
        if not fetch:
            self._call("bpmpc_solver_rollout", _d(ts), _d(xs), duration, None, None, None)
            return None
        x_end, u_end, steps = np.zeros((B, self.nx)), np.zeros((B, self.nu)), np.zeros((B, 2), np.int32)
        self._call("bpmpc_solver_rollout", _d(ts), _d(xs), duration, _d(x_end), _d(u_end), _i(steps))
        return x_end, u_end, steps

    def advance(self, t0, x0, modeSchedules, targetTrajectories, horizon=None, gains=False):
        """One MPC tick for the whole batch: warm start from the previous solution, solve, fetch."""
        self.setup_from_previous(t0, x0, modeSchedules, targetTrajectories, horizon)
        self.enqueue()
        return self.fetch(gains=gains)

    def layout(self):
        b, n, g, nx, nu = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._call("bpmpc_solver_layout", C.byref(b), C.byref(n), C.byref(g), C.byref(nx), C.byref(nu))
        return dict(batch=b.value, n_nodes_max=n.value, n_grids=g.value, nx=nx.value, nu=nu.value)

    def reset(self):
        self._call("bpmpc_solver_reset")

    def enqueue(self):
        self._call("bpmpc_solver_run")

    def synchronize(self):
        self._call("bpmpc_solver_sync")

    def stage(self, name):
        self._call("bpmpc_solver_stage", name.encode())

    def fetch(self, gains=False):
        B, N = self.batch, self.max_nodes
        t = np.zeros((B, N + 1))
        x = np.zeros((B, N + 1, self.nx))
        u = np.zeros((B, N, self.nu))
        K = np.zeros((B, N, self.nu, self.nx)) if gains else None
        stats = (Stats * B)()
        self._call("bpmpc_solver_fetch", _d(t), _d(x), _d(u), _d(K), stats)
        return t, x, u, K, list(stats)

    def run(self, t0, x0, modeSchedules, targetTrajectories, horizon=None, warm_x=None, warm_u=None, gains=False):
        """One MPC solve for every problem: returns (t, x, u, K, stats) with strides max_nodes (see stats[b].n_nodes)."""
        self.setup(t0, x0, modeSchedules, targetTrajectories, horizon, warm_x, warm_u)
        self.enqueue()
        self.synchronize()
        return self.fetch(gains)

    def solve_batch(self, t0, x0, modeSchedules, targetTrajectories, horizon=None, warm_x=None, warm_u=None, gains=False):
        """The single-call entry point bpmpc_solve_batch (host buffers in, host buffers out)."""
        if horizon is None:
            horizon = self.interface.mpcSettings()["timeHorizon"]
        B, t0, x0, sched, ns, tg, wx, wu, keep = self._marshal(t0, x0, modeSchedules, targetTrajectories, warm_x, warm_u)
        N = self.max_nodes
        t = np.zeros((B, N + 1))
        x = np.zeros((B, N + 1, self.nx))
        u = np.zeros((B, N, self.nu))
        K = np.zeros((B, N, self.nu, self.nx)) if gains else None
        stats = (Stats * B)()
        self._call("bpmpc_solve_batch", B, horizon, _d(t0), _d(x0), sched, ns, tg, _d(wx), _d(wu), _d(t), _d(x), _d(u), _d(K), stats)
        self.batch = B
        return t, x, u, K, list(stats)

    def read(self, name):
        """Named device buffer as a flat float64 array (tests / debugging)."""
        cap = self._call("bpmpc_solver_read", name.encode(), None, 0)
        out = np.zeros(cap)
        n = self._call("bpmpc_solver_read", name.encode(), _d(out), cap)
        return out[:n]

    def set_materialize(self, materialize_lq):
        """True: the lineariser writes the complete per-node LQ model (parity stages, roofline pass); False: the fused solve mode."""
        self._call("bpmpc_solver_set_materialize", int(bool(materialize_lq)))

    def set_profile(self, level):
        """0 off, 1 every kernel class, 2 the linearisation kernel only."""
        self._call("bpmpc_solver_set_profile", int(level))

    def kernel_time(self, kernel, reset=True):
        ms, n = C.c_double(), C.c_int()
        self._call("bpmpc_solver_kernel_time", kernel.encode(), int(reset), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def device_trajectories(self):
        xp, up = _dp(), _dp()
        self._call("bpmpc_solver_device_trajectories", C.byref(xp), C.byref(up))
        return C.cast(xp, C.c_void_p).value, C.cast(up, C.c_void_p).value

    def constraint_values(self):
        """Values of the active equality rows at the current iterate (after a solve: the solution): (values [B, max_nodes, 16],
        rows [B, max_nodes], modes [B, max_nodes]) - include/bpmpc.h bpmpc_solver_constraint_values."""
        lay = self.layout()
        B = lay["batch"]
        v = np.zeros((B, self.max_nodes, 16))
        rows = np.zeros((B, self.max_nodes), np.int32)
        modes = np.zeros((B, self.max_nodes), np.int32)
        self._call("bpmpc_solver_constraint_values", _d(v), _i(rows), _i(modes))
        return v, rows, modes

    def export_trajectories(self, x_dst_ptr, u_dst_ptr):
        """Async D2D copy of the iterate into device buffers given by raw pointers (e.g. torch tensors' data_ptr())."""
        self._call("bpmpc_solver_export_trajectories", C.cast(x_dst_ptr, _dp), C.cast(u_dst_ptr, _dp))

    def restart(self, mask, x=None):
        """MPC_BASE::reset for the problems with mask[b] != 0 (bpmpc_solver_restart): the next setup gives them the initializer's guess instead of the
        shifted solution; x (nullable, [batch, nx]) replaces their rows of the closed-loop start that x0=None reads.  Until the first run after
        that setup, evaluatePolicy, rollout and a controller tick are refused.  numpy arrays, or int32 / float64 device tensors; len(mask) must be
        the batch of the last setup."""
        B = _count(mask)
        (mp, xp), dev, keep = _restart_args((mask, C.c_int, B), (x, C.c_double, B * self.nx))
        self._call("bpmpc_solver_restart", B, mp, xp, dev)
        del keep

    def setWeights(self, rows, mask=None):
        """Per-problem cost weights (bpmpc_solver_set_weights, include/bpmpc.h "Per-problem cost weights"): the problems with mask[b] != 0 (None:
        every problem of the last setup) solve under rows[b] - [batch, MpcWeights.STRIDE] - or under the one row [STRIDE] / [1, STRIDE], from the
        next run on and without a new setup.  rows: MpcWeights, a list of them, numpy arrays, or float64 device tensors (not checked; with them the
        call only enqueues).  A host row that is not finite, not symmetric, off the model's non-zero pattern or not (semi)definite raises
        BpmpcError(-1) and changes nothing.  The DDP solver and reference_kernels raise BpmpcError(-3)."""
        if isinstance(rows, MpcWeights):
            rows = rows.row
        elif isinstance(rows, (list, tuple)) and rows and isinstance(rows[0], MpcWeights):
            rows = np.stack([w.row for w in rows])
        B, n_rows, (mp, rp), dev, keep = _rows_args(mask, [rows], MpcWeights.STRIDE, self.batch or self.max_batch)
        self._call("bpmpc_solver_set_weights", B, mp, rp, n_rows, dev)
        del keep

    def getWeights(self, robot=-1):
        """The weight row of problem `robot`, or with robot < 0 the start row, the model's Q and R (bpmpc_solver_get_weights; synchronises)."""
        row = np.zeros(MpcWeights.STRIDE)
        self._call("bpmpc_solver_get_weights", int(robot), _d(row))
        return MpcWeights(self.nx, self.nu, row)

    def resetWeights(self):
        """Every row back to the model's weights and the handle back to the kernels it launched before any row was set (bpmpc_solver_reset_weights)."""
        self._call("bpmpc_solver_reset_weights")

    def checkWeights(self, row):
        """The host check of setWeights alone (bpmpc_solver_check_weights): raises BpmpcError(-1) with the entry and the reason, else returns None."""
        r = _f64(row.row if isinstance(row, MpcWeights) else row).reshape(-1)
        if r.size != MpcWeights.STRIDE:
            raise ValueError("a weight row has %d entries" % MpcWeights.STRIDE)
        self._call("bpmpc_solver_check_weights", _d(r))

    def setConeParams(self, rows, mask=None):
        """Per-problem friction-cone parameters (bpmpc_solver_set_cone_params, include/bpmpc.h "Per-problem cone parameters"): the problems with
        mask[b] != 0 (None: every problem of the last setup) solve under rows[b] - [batch, ConeParams.STRIDE] - or under the one row [STRIDE] /
        [1, STRIDE], from the next run on and without a new setup.  rows: ConeParams, a list of them, numpy arrays, or float64 device tensors (not
        checked; with them the call only enqueues).  A host row that BipedalRobotInterface.checkConeParams refuses raises BpmpcError(-1) and
        changes nothing.  The DDP solver and reference_kernels raise BpmpcError(-3)."""
        if isinstance(rows, ConeParams):
            rows = rows.row
        elif isinstance(rows, (list, tuple)) and rows and isinstance(rows[0], ConeParams):
            rows = np.stack([p.row for p in rows])
        B, n_rows, (mp, rp), dev, keep = _rows_args(mask, [rows], ConeParams.STRIDE, self.batch or self.max_batch)
        self._call("bpmpc_solver_set_cone_params", B, mp, rp, n_rows, dev)
        del keep

    def getConeParams(self, robot=-1):
        """The cone row of problem `robot`, or with robot < 0 the start row, the model's parameters (bpmpc_solver_get_cone_params; synchronises)."""
        row = np.zeros(ConeParams.STRIDE)
        self._call("bpmpc_solver_get_cone_params", int(robot), _d(row))
        return ConeParams.fromRow(row)

    def resetConeParams(self):
        """Every row back to the model's parameters; the handle goes back to the kernels it launched before any row was set unless a weight row is
        set (bpmpc_solver_reset_cone_params)."""
        self._call("bpmpc_solver_reset_cone_params")

    def evaluatePolicy(self, t, x):
        """MRT_BASE::evaluatePolicy(t, x) for every problem of the last run (bpmpc_solver_evaluate_policy): t[batch], x[batch, nx] ->
        (x_opt [batch, nx], u_opt [batch, nu], planned mode [batch])."""
        B = self.batch
        t = _f64(np.broadcast_to(np.asarray(t, float), (B,)))
        x = _f64(x).reshape(B, self.nx)
        x_opt, u_opt, mode = np.zeros((B, self.nx)), np.zeros((B, self.nu)), np.zeros(B, np.int32)
        self._call("bpmpc_solver_evaluate_policy", B, _d(t), _d(x), _d(x_opt), _d(u_opt), _i(mode))
        return x_opt, u_opt, mode

    # ---- the value function of the QP a run has solved (include/bpmpc.h "Value function")
    def enableValueFunction(self, on=True):
        """From the next run on, every backward pass is followed by the value function of its QP, V_k(dx) = v_k + s_k'dx + dx'S_k dx / 2 around the
        expansion point x_lin,k of every node (bpmpc_solver_enable_value_function).  The handle then linearises in materialised form (the solution
        keeps its bits).  on=False stops the launches and keeps the buffers.  The DDP solver raises BpmpcError(-3)."""
        self._call("bpmpc_solver_enable_value_function", int(bool(on)))

    def valueFunction(self):
        """(S [B, N + 1, nx, nx], s [B, N + 1, nx], v [B, N + 1], x_lin [B, N + 1, nx], status [B]) of the last run, N = max_nodes
        (bpmpc_solver_value_function; synchronises).  status: 0 none yet, 1 valid, 2 the problem's sweep failed (rows as they were); entries beyond
        n_nodes[b] are never written."""
        B, K, nx = self.layout()["batch"], self.max_nodes + 1, self.nx      # the library copies the batch of ITS last setup
        S, s, v, x_lin, status = np.zeros((B, K, nx, nx)), np.zeros((B, K, nx)), np.zeros((B, K)), np.zeros((B, K, nx)), np.zeros(B, np.int32)
        self._call("bpmpc_solver_value_function", _d(S), _d(s), _d(v), _d(x_lin), _i(status))
        return S, s, v, x_lin, status

    def valueFunctionDevice(self):
        """The same five arrays where they live: a dict of DeviceArray over max_batch problems (bpmpc_solver_device_value_function; no
        synchronisation)."""
        S, s, v, xl, st = _dp(), _dp(), _dp(), _dp(), _ip()
        self._call("bpmpc_solver_device_value_function", C.byref(S), C.byref(s), C.byref(v), C.byref(xl), C.byref(st))
        B, K, nx = self.max_batch, self.max_nodes + 1, self.nx
        ptr = lambda p: C.cast(p, C.c_void_p).value
        return {"S": DeviceArray(ptr(S), (B, K, nx, nx), "<f8"), "s": DeviceArray(ptr(s), (B, K, nx), "<f8"), "v": DeviceArray(ptr(v), (B, K), "<f8"),
                "x_lin": DeviceArray(ptr(xl), (B, K, nx), "<f8"), "status": DeviceArray(ptr(st), (B,), "<i4")}

    def evaluateValue(self, t, x, hessian=True):
        """V(t, x) of every problem of the last run, its gradient and Hessian (bpmpc_solver_evaluate_value): t[batch], x[batch, nx] ->
        (f [batch], dfdx [batch, nx], dfdxx [batch, nx, nx] or None).  t is clamped to the solution's span; S, s, v and the expansion point are
        interpolated as evaluatePolicy interpolates the states.  numpy inputs: numpy results, the call synchronises.  float64 device tensors (e.g.
        the observations of BatchedController.device_outputs()): the call only enqueues on the solver's stream and the results are DeviceArray
        over torch tensors it allocates - synchronise the solver before another stream reads them."""
        B, nx = self.batch, self.nx
        if all(getattr(a, "is_cuda", False) or hasattr(a, "__cuda_array_interface__") for a in (t, x)):
            import torch
            (tp, xp), dev, keep = _restart_args((t, C.c_double, B), (x, C.c_double, B * nx))
            out = [torch.empty(shape, dtype=torch.float64, device="cuda") for shape in ((B,), (B, nx)) + (((B, nx, nx),) if hessian else ())]
            ptrs = [C.cast(C.c_void_p(o.data_ptr()), _dp) for o in out] + ([] if hessian else [None])
            self._call("bpmpc_solver_evaluate_value", B, tp, xp, 1, *ptrs)
            del keep
            views = []
            for o in out:
                views.append(DeviceArray(o.data_ptr(), o.shape, "<f8"))
                views[-1].owner = o                     # the tensor lives as long as its view
            return tuple(views) + (() if hessian else (None,))
        t = _f64(np.broadcast_to(np.asarray(t, float), (B,)))
        x = _f64(x).reshape(B, nx)
        f, g, h = np.zeros(B), np.zeros((B, nx)), np.zeros((B, nx, nx)) if hessian else None
        self._call("bpmpc_solver_evaluate_value", B, _d(t), _d(x), 0, _d(f), _d(g), _d(h))
        return f, g, h

    # ---- the dual solution of the QP a run has solved (include/bpmpc.h "Dual solution")
    def enableDualSolution(self, on=True):
        """From the next run on, the value function's kernels are followed by the dual solution of the same QP: the costates lambda_k = s_k + S_k dx_k,
        the minimum-norm multipliers nu_k = nu0_k + N_k dx_k of the state-input equality rows, and the two residuals that certify the step and the
        gains (bpmpc_solver_enable_dual_solution).  The value function is on while this is on.  on=False stops the launches and keeps the
        buffers.  The DDP solver raises BpmpcError(-3)."""
        self._call("bpmpc_solver_enable_dual_solution", int(bool(on)))

    def dualSolution(self):
        """DualSolution(costate [B, N + 1, nx], nu [B, N, 16], nu0 [B, N, 16], nu_gain [B, N, 16, nx], residual [B, N], gain_residual [B, N],
        summary [B, 6], status [B]) of the last run, N = max_nodes (bpmpc_solver_dual_solution; synchronises).  summary: the maxima over a problem's
        nodes of residual, |g_u|, gain_residual, |Hux|, |nu|, |lambda|; status as valueFunction's.  Nodes beyond n_nodes[b] are never written."""
        B, N, nx, R = self.layout()["batch"], self.max_nodes, self.nx, DUAL_ROWS
        out = DualSolution(np.zeros((B, N + 1, nx)), np.zeros((B, N, R)), np.zeros((B, N, R)), np.zeros((B, N, R, nx)), np.zeros((B, N)), np.zeros((B, N)),
                           np.zeros((B, 6)), np.zeros(B, np.int32))
        self._call("bpmpc_solver_dual_solution", *[_d(a) for a in out[:7]], _i(out.status))
        return out

    def dualSolutionDevice(self):
        """The same eight arrays where they live: a dict of DeviceArray over max_batch problems, keyed as the C arrays ("lambda", "nu", ...)
        (bpmpc_solver_device_dual_solution; no synchronisation)."""
        names = ("lambda", "nu", "nu0", "nu_gain", "residual", "gain_residual", "summary")
        ptrs, st = [_dp() for _ in names], _ip()
        self._call("bpmpc_solver_device_dual_solution", *[C.byref(p) for p in ptrs], C.byref(st))
        B, N, nx, R = self.max_batch, self.max_nodes, self.nx, DUAL_ROWS
        shapes = ((B, N + 1, nx), (B, N, R), (B, N, R), (B, N, R, nx), (B, N), (B, N), (B, 6))
        ptr = lambda p: C.cast(p, C.c_void_p).value
        out = {n: DeviceArray(ptr(p), shp, "<f8") for n, p, shp in zip(names, ptrs, shapes)}
        out["status"] = DeviceArray(ptr(st), (B,), "<i4")
        return out

    def evaluateDual(self, t, x):
        """The multipliers and the costate of every problem of the last run at (t, x) (bpmpc_solver_evaluate_dual): t[batch], x[batch, nx] ->
        (costate [batch, nx], nu [batch, 16], rows [batch]): nu = nu0_i + N_i (x - x_lin(t)) of the interval i that holds t, its first rows[b]
        entries meaningful; the costate is evaluateValue's dfdx.  numpy inputs: numpy results, the call synchronises.  float64 device tensors: the
        call only enqueues on the solver's stream and the results are DeviceArray over torch tensors it allocates."""
        B, nx = self.batch, self.nx
        if all(getattr(a, "is_cuda", False) or hasattr(a, "__cuda_array_interface__") for a in (t, x)):
            import torch
            (tp, xp), dev, keep = _restart_args((t, C.c_double, B), (x, C.c_double, B * nx))
            lam, nu = (torch.empty(shape, dtype=torch.float64, device="cuda") for shape in ((B, nx), (B, DUAL_ROWS)))
            rows = torch.empty((B,), dtype=torch.int32, device="cuda")
            self._call("bpmpc_solver_evaluate_dual", B, tp, xp, 1, C.cast(C.c_void_p(lam.data_ptr()), _dp), C.cast(C.c_void_p(nu.data_ptr()), _dp),
                       C.cast(C.c_void_p(rows.data_ptr()), _ip))
            del keep
            views = []
            for o, ts in ((lam, "<f8"), (nu, "<f8"), (rows, "<i4")):
                views.append(DeviceArray(o.data_ptr(), o.shape, ts))
                views[-1].owner = o                     # the tensor lives as long as its view
            return tuple(views)
        t = _f64(np.broadcast_to(np.asarray(t, float), (B,)))
        x = _f64(x).reshape(B, nx)
        lam, nu, rows = np.zeros((B, nx)), np.zeros((B, DUAL_ROWS)), np.zeros(B, np.int32)
        self._call("bpmpc_solver_evaluate_dual", B, _d(t), _d(x), 0, _d(lam), _d(nu), _i(rows))
        return lam, nu, rows


class WeightedWbc(_Handle):
    """A batch of WeightedWbc instances on one MI355X (bipedal_wbc/include/bipedal_wbc/WeightedWbc.h; construction + loadTasksSetting as
    in bipedal_controllers/src/BipedalController.cpp:97-100).  `update` mirrors WeightedWbc::update(stateDesired, inputDesired,
    rbdStateMeasured, mode, period) (BipedalController.cpp:229) with a leading batch dimension; it returns (x, status) where
    x[b] = [generalised accelerations, contact forces, joint torques] and status[b] = 1 when that robot's QP was not solved and its
    previous solution was returned instead (lastQpSol_)."""

    _DESTROY = "bpmpc_wbc_destroy"

    def __init__(self, interface, taskFile=None, max_batch=1, device=0):
        self.interface = interface
        super().__init__()
        _check(load_library().bpmpc_wbc_create(interface.handle, str(taskFile or interface.taskFile).encode(), int(device), int(max_batch), C.byref(self._h)))
        n, nv = C.c_int(), C.c_int()
        self._call("bpmpc_wbc_dims", C.byref(n), C.byref(nv))
        self.numDecisionVars, self.generalizedCoordinatesNum, self.max_batch = n.value, nv.value, int(max_batch)

    def update(self, stateDesired, inputDesired, rbdStateMeasured, mode, period=0.002, debug=False):
        x = _f64(stateDesired).reshape(-1, self.interface.stateDim)
        B = x.shape[0]
        u = _f64(inputDesired).reshape(B, self.interface.inputDim)
        rbd = _f64(rbdStateMeasured).reshape(B, 2 * self.generalizedCoordinatesNum)
        md = np.ascontiguousarray(np.broadcast_to(np.asarray(mode, np.int32), (B,)))
        sol = np.zeros((B, self.numDecisionVars))
        status = np.zeros(B, np.int32)
        dbg = np.zeros((B, 1024)) if debug else None
        self._call("bpmpc_wbc_update", B, _d(x), _d(u), _d(rbd), _i(md), period, _d(sol), _i(status), _d(dbg))
        return (sol, status, dbg) if debug else (sol, status)

    def reset(self):
        self._call("bpmpc_wbc_reset")

    def restart(self, mask):
        """clearLastQpSol for the robots with mask[b] != 0 (robots 0 .. len(mask) - 1; bpmpc_wbc_restart): their last solution and status become 0."""
        n = _count(mask)
        (mp,), dev, keep = _restart_args((mask, C.c_int, n))
        self._call("bpmpc_wbc_restart", n, mp, dev)
        del keep

    getParams, setParams, resetParams = _param_methods(
        "bpmpc_wbc", WbcParams.STRIDE,
        """The parameter row [32] of `robot` (WbcParams.fromRow names its entries), or with robot < 0 the values loadTasksSetting read from
        task.info, which every row holds until it is set (bpmpc_wbc_get_params; synchronises).""",
        """dynamicReconfigCallback's setBasePDGains / setSwingLegPDGains / setWeights (BipedalController.cpp:407-478) per robot, and this engine's
        per-robot friction, contact tolerance and torque limits (bpmpc_wbc_set_params).  rows: [32] or [1, 32] (one row for every robot written)
        or [B, 32]; mask (None: every robot; else [B], non-zero = write).  numpy arrays are validated and the call synchronises; float64 / int32
        device tensors are only enqueued on the WBC's stream (a later controller tick waits for it).""",
        """Every row back to the task.info values (bpmpc_wbc_reset_params).""")


class KalmanParams(_RowParams):
    """A parameter row of the Kalman state estimator (include/bpmpc.h "State estimation", BPMPC_EST_PARAM_STRIDE) with named fields: the seven
    settings of KalmanFilterEstimate (LinearKalmanFilter.h:45-51), whose defaults are the values without arguments."""

    STRIDE = 8
    FIELDS = ("footRadius", "imuProcessNoisePosition", "imuProcessNoiseVelocity", "footProcessNoisePosition", "footSensorNoisePosition",
              "footSensorNoiseVelocity", "footHeightSensorNoise")
    DEFAULTS = (0.02, 0.02, 0.02, 0.002, 0.005, 0.1, 0.01)


ESTIMATOR_KINDS = {"from_topic": 0, "kalman": 1}


def _sensor_args(kind, nj, max_batch, joint_pos, joint_vel, quat=None, angular_vel_local=None, linear_accel_local=None, contact=None, mode=None,
                 feet_heights=None, odom=None):
    """Marshals the sensors of one update (bpmpc_estimator_update): checks what the kind needs - the Kalman filter its IMU arrays and exactly one
    of contact / mode, the from-topic estimator odom = (position [B, 3], quaternion x y z w [B, 4], linear velocity [B, 3], angular velocity
    [B, 3]) - and the shapes against the batch B = rows of joint_pos.  Returns (B, _SensorInputs, on_device, keep-alive); through _restart_args, so
    device and host inputs are never mixed."""
    if kind not in ESTIMATOR_KINDS:
        raise ValueError("kind must be one of %s" % sorted(ESTIMATOR_KINDS))
    shape = _shape(joint_pos)
    if len(shape) not in (1, 2) or shape[-1] != nj:
        raise ValueError("joint_pos must have the shape [%d] or [B, %d], got %s" % (nj, nj, list(shape)))
    B = 1 if len(shape) == 1 else shape[0]
    if B < 1 or B > max_batch:
        raise ValueError("%d robots for an estimator of max_batch %d" % (B, max_batch))
    if kind == "kalman":
        if quat is None or angular_vel_local is None or linear_accel_local is None:
            raise ValueError("the Kalman filter needs quat, angular_vel_local and linear_accel_local")
        if contact is None and mode is None:
            raise ValueError("no contact source: give contact or mode")
        if contact is not None and mode is not None:
            raise ValueError("two contact sources: give contact or mode, not both")
        if odom is not None:
            raise ValueError("odom belongs to the from-topic estimator")
        odom = (None,) * 4
    else:
        if odom is None or len(odom) != 4 or any(o is None for o in odom):
            raise ValueError("the from-topic estimator needs odom = (position, quaternion, linear velocity, angular velocity)")
        contact = mode = feet_heights = None
    specs = [(joint_pos, C.c_double, B * nj), (joint_vel, C.c_double, B * nj), (quat, C.c_double, B * 4), (angular_vel_local, C.c_double, B * 3),
             (linear_accel_local, C.c_double, B * 3), (contact, C.c_int, B * 4), (mode, C.c_int, B), (feet_heights, C.c_double, B * 4),
             (odom[0], C.c_double, B * 3), (odom[1], C.c_double, B * 4), (odom[2], C.c_double, B * 3), (odom[3], C.c_double, B * 3)]
    ptrs, dev, keep = _restart_args(*specs)
    return B, _SensorInputs(*ptrs), dev, keep


class BatchedStateEstimate(_Handle):
    """BipedalController::updateStateEstimation (bipedal_controllers/src/BipedalController.cpp:360-405) for a batch of robots on one MI355X
    (bpmpc_estimator): IMU, joint encoders and contact flags -> the rbd of BatchedController.tick.  kind "from_topic" is FromTopicStateEstimate, the
    estimator the reference constructs; kind "kalman" is KalmanFilterEstimate, which the reference declares (LinearKalmanFilter.h) and does not
    implement (its source file is empty): the filter is the one specified in include/bpmpc.h, per robot, its state kept on the handle.  taskFile
    (None: the defaults of LinearKalmanFilter.h:45-51) is read for the keys kalmanFilter.<name>."""

    _DESTROY = "bpmpc_estimator_destroy"

    def __init__(self, interface, kind="kalman", taskFile=None, max_batch=1, device=0):
        if kind not in ESTIMATOR_KINDS:
            raise ValueError("kind must be one of %s" % sorted(ESTIMATOR_KINDS))
        self.interface, self.kind, self.max_batch = interface, kind, int(max_batch)
        self.nj = interface.actuatedDofNum
        self.generalizedCoordinatesNum = 6 + self.nj
        super().__init__()
        _check(load_library().bpmpc_estimator_create(interface.handle, None if taskFile is None else str(taskFile).encode(), ESTIMATOR_KINDS[kind],
                                                     int(device), self.max_batch, C.byref(self._h)))
        self.batch = self.max_batch

    def update(self, joint_pos, joint_vel, quat=None, angular_vel_local=None, linear_accel_local=None, contact=None, mode=None, feet_heights=None,
               odom=None, period=0.0025, fetch=True):
        """One update for B = len(joint_pos) robots.  numpy arrays, or float64 / int32 device tensors (then the call only enqueues on the
        estimator's stream).  contact [B, 4] or mode [B] (e.g. planned_mode of the last tick) - exactly one for the Kalman kind.  fetch=True: returns
        rbd [B, 2 (6 + nj)] (synchronises); False: returns None, see device_outputs and BatchedController.tick_estimated."""
        B, inputs, dev, keep = _sensor_args(self.kind, self.nj, self.max_batch, joint_pos, joint_vel, quat, angular_vel_local, linear_accel_local,
                                            contact, mode, feet_heights, odom)
        rbd = np.zeros((B, 2 * self.generalizedCoordinatesNum)) if fetch else None
        self._call("bpmpc_estimator_update", B, C.byref(inputs), dev, period, _d(rbd))
        del keep
        self.batch = B
        return rbd

    def update_from_plant(self, plant, period=0.0025, fetch=True):
        """update on the device outputs of `plant` (BatchedPlant) after its last step (bpmpc_estimator_update_from_plant): the estimator's stream
        waits for a step that was only enqueued and the plant's stream for this update, so plant.step_controlled, this call with fetch=False and
        BatchedController.tick_estimated need no synchronisation between them.  Returns what update returns."""
        B = plant.batch
        rbd = np.zeros((B, 2 * self.generalizedCoordinatesNum)) if fetch else None
        self._call("bpmpc_estimator_update_from_plant", plant._h, B, period, _d(rbd))
        self.batch = B
        return rbd

    def reset(self, mask=None):
        """x_hat = 0, P = 100 I for the robots with mask[b] != 0 (None: every robot); the others do not change by one bit."""
        B = self.max_batch if mask is None else _count(mask)
        (mp,), dev, keep = _restart_args((mask, C.c_int, B))
        self._call("bpmpc_estimator_reset", B, mp, dev)
        del keep

    def getState(self, batch=None):
        """(x_hat [B, 18], P [B, 18, 18]) of the first B robots (None: the batch of the last update); synchronises."""
        B = int(batch or self.batch)
        x, P = np.zeros((B, 18)), np.zeros((B, 18, 18))
        self._call("bpmpc_estimator_get_state", B, _d(x), _d(P))
        return x, P

    def setState(self, x_hat, cov=None, mask=None):
        """x_hat [B, 18] and, unless None, P [B, 18, 18] of the robots with mask[b] != 0 (None: every one of the B)."""
        shape = _shape(x_hat)
        if len(shape) != 2 or shape[1] != 18:
            raise ValueError("x_hat must have the shape [B, 18], got %s" % list(shape))
        B = shape[0]
        (mp, xp, cp), dev, keep = _restart_args((mask, C.c_int, B), (x_hat, C.c_double, B * 18), (cov, C.c_double, B * 18 * 18))
        self._call("bpmpc_estimator_set_state", B, mp, xp, cp, dev)
        del keep

    getParams, setParams, resetParams = _param_methods(
        "bpmpc_estimator", KalmanParams.STRIDE,
        """The parameter row [8] of `robot` (KalmanParams.fromRow names its entries), or with robot < 0 the values every row starts from.""",
        """rows [8], [1, 8] or [B, 8]; mask as WeightedWbc.setParams.  numpy rows are validated (finite, not negative, the three sensor noises
        positive) and the call synchronises; device tensors are only enqueued, ordered before the next update.""")

    def device_outputs(self):
        """rbd, x_hat, cov, xy_reset of the last update where they live: a dict of DeviceArray over the batch of the last update."""
        o = _EstimatorOutputs()
        self._call("bpmpc_estimator_device_outputs", C.byref(o))
        B = self.batch
        shapes = {"rbd": (B, 2 * self.generalizedCoordinatesNum), "x_hat": (B, 18), "cov": (B, 18, 18), "xy_reset": (B,)}
        return {k: DeviceArray(C.cast(getattr(o, k), C.c_void_p).value, shp, "<i4" if k == "xy_reset" else "<f8") for k, shp in shapes.items()}


class DeviceArray:
    """A device buffer of the library seen through __cuda_array_interface__: torch.as_tensor(view, device="cuda") wraps it without a copy
    (`.torch()` does that).  The memory belongs to the handle that returned it."""

    def __init__(self, ptr, shape, typestr):
        self.ptr, self.shape, self.typestr = int(ptr), tuple(int(n) for n in shape), typestr
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": typestr, "data": (self.ptr, False), "version": 3, "strides": None}

    def torch(self):
        import torch
        return torch.as_tensor(self, device="cuda")


class BatchedController(_Handle):
    """BipedalController::update (bipedal_controllers/src/BipedalController.cpp:186-262) for the batch of a BatchedSqpMpc and a WeightedWbc
    (bpmpc_controller_tick): measured rigid-body state -> observation (centroidal state, yaw unwrap), evaluatePolicy of the last run, the WBC,
    SafetyChecker, joint commands - three kernels on the solver's stream.  `tick` takes numpy arrays (host) or device tensors (e.g. torch
    tensors of a GPU simulator; order their producer against the solver's stream, e.g. by creating the solver on a torch stream)."""

    _DESTROY = "bpmpc_controller_destroy"

    NAMES = ("x_obs", "x_opt", "u_opt", "joint_cmd", "wbc_solution", "planned_mode", "wbc_status", "safe")
    JOINT_NAMES = ("joint_torque", "joint_kp", "joint_kd")      # bpmpc_controller_joint_outputs

    def __init__(self, mpc, wbc):
        self.mpc, self.wbc = mpc, wbc
        super().__init__()
        _check(load_library().bpmpc_controller_create(mpc._h, wbc._h, C.byref(self._h)))
        self.nx, self.nu, self.nj = mpc.nx, mpc.nu, mpc.interface.actuatedDofNum
        self.max_batch = wbc.max_batch

    def _shapes(self, B):
        return {"x_obs": (B, self.nx), "x_opt": (B, self.nx), "u_opt": (B, self.nu), "joint_cmd": (B, 3, self.nj),
                "wbc_solution": (B, self.wbc.numDecisionVars), "planned_mode": (B,), "wbc_status": (B,), "safe": (B,)}

    def _device_f64(self, a, count):
        """pointer of a float64 device tensor of `count` entries (a tick input), None for anything that is not a device tensor"""
        if not (hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)):
            return None
        if str(a.dtype) != "torch.float64" or not a.is_contiguous() or a.numel() != count:
            raise ValueError("device inputs must be contiguous float64 tensors of the batch's size")
        return C.cast(C.c_void_p(a.data_ptr()), _dp)

    def _run_tick(self, fetch, name, *args):
        """The part tick and tick_estimated share: host output arrays (fetch), the call - lib.<name>(handle, *args, host_out pointer or None) -,
        the joint outputs."""
        B = self.mpc.batch
        out, ptrs = None, None
        if fetch:
            out = {k: np.zeros(shp, np.int32 if k in ("planned_mode", "wbc_status", "safe") else np.float64) for k, shp in self._shapes(B).items()}
            ptrs = _TickOutputs(*[(_i if out[k].dtype == np.int32 else _d)(out[k]) for k in self.NAMES])
        self._call(name, *args, C.byref(ptrs) if fetch else None)
        if fetch:
            for k in self.JOINT_NAMES:             # every key of device_outputs has its host copy
                out[k] = np.zeros((B, self.nj))
            self._call("bpmpc_controller_joint_outputs", B, *[_d(out[k]) for k in self.JOINT_NAMES], None, None, None)
        return out

    def tick(self, t, rbd, period=0.0025, fetch=True):
        """One tick for the solver's batch.  t: [batch] (or a scalar), rbd: [batch, 2 (6 + nj)].  fetch=True: returns a dict of numpy arrays
        (x_obs, x_opt, u_opt, joint_cmd [batch, 3, nj] = position, velocity, torque, wbc_solution, planned_mode, wbc_status, safe); False: only
        enqueues (see device_outputs).  joint_torque [batch, nj] = kp (posDes - q) + kd (velDes - v) + torque with the robots' joint gains
        (setJointGains; the WBC torque while they are zero) and the gains themselves, joint_kp / joint_kd [batch, nj], come with them."""
        B = self.mpc.batch
        rp = self._device_f64(rbd, B * 2 * self.wbc.generalizedCoordinatesNum)
        on_device = rp is not None
        if on_device:
            tp, keep = self._device_f64(t, B), None
            if tp is None:
                raise ValueError("t and rbd must both be device tensors or both host arrays")
        else:
            tt = _f64(np.broadcast_to(np.asarray(t, float), (B,)))
            rr = _f64(rbd).reshape(B, 2 * self.wbc.generalizedCoordinatesNum)
            tp, rp, keep = _d(tt), _d(rr), (tt, rr)
        out = self._run_tick(fetch, "bpmpc_controller_tick", B, tp, rp, int(on_device), period)
        del keep
        return out

    def tick_estimated(self, t, estimator, period=0.0025, fetch=True):
        """tick on the rbd that `estimator` (BatchedStateEstimate) holds on the device after its last update (bpmpc_controller_tick_estimated):
        the solver's stream waits for an update that was only enqueued, so estimator.update(..., fetch=False) followed by this call needs no
        synchronisation.  t: [batch] numpy (or a scalar) or a float64 device tensor; the batch must be that of the estimator's last update.
        Returns what tick returns."""
        B = self.mpc.batch
        tp = self._device_f64(t, B)
        on_device, keep = tp is not None, t
        if not on_device:
            keep = _f64(np.broadcast_to(np.asarray(t, float), (B,)))
            tp = _d(keep)
        out = self._run_tick(fetch, "bpmpc_controller_tick_estimated", estimator._h, B, tp, int(on_device), period)
        del keep
        return out

    def setJointGains(self, kp, kd, mask=None):
        """The joint-level kp / kd of the reference's joint command (HybridJointHandle::setCommand, BipedalController.cpp:250-254; set by
        dynamicReconfigCallback :423-472) per robot (bpmpc_controller_set_joint_gains): kp, kd [nj], [1, nj] or [B, nj]; mask as
        WeightedWbc.setParams.  On the solver's stream; all gains are 0 after create and survive restarts and reset."""
        B, n_rows, (mp, pp, dp), dev, keep = _rows_args(mask, [kp, kd], self.nj, self.max_batch)
        self._call("bpmpc_controller_set_joint_gains", B, mp, pp, dp, n_rows, dev)
        del keep

    def setLegMotorGains(self, kp_leg, kd_leg, mask=None):
        """setJointGains from nj / 2 values per robot (or one set for all), mirrored onto both legs as dynamicReconfigCallback does (:423-472)."""
        def both(a):
            if hasattr(a, "data_ptr"):
                import torch
                return torch.cat([a, a], dim=-1).contiguous()
            a = np.asarray(a, float)
            return np.concatenate([a, a], axis=-1)
        if _shape(kp_leg)[-1:] != (self.nj // 2,) or _shape(kd_leg)[-1:] != (self.nj // 2,):
            raise ValueError("leg gains need %d values per robot" % (self.nj // 2))
        self.setJointGains(both(kp_leg), both(kd_leg), mask)

    def attachPolicy(self, policy):
        """Ticks, restarts and joint-gain writes move to the stream of `policy` (a PolicyBuffer of the same solver) and the tick evaluates the
        policy it adopted last (bpmpc_controller_attach_policy); None detaches: everything is back on the solver's stream and arrays."""
        self._call("bpmpc_controller_attach_policy", None if policy is None else policy._h)
        self.policy = policy

    def attachTelemetry(self, telemetry):
        """Every tick takes a sample of `telemetry` (a BatchedTelemetry of the same robot and device) behind its commands, on the controller's
        stream and the tick's own device buffers (bpmpc_controller_attach_telemetry); None detaches: a tick is its three launches again."""
        self._call("bpmpc_controller_attach_telemetry", None if telemetry is None else telemetry._h)
        self.telemetry = telemetry
        if telemetry is not None:
            telemetry.batch = self.mpc.batch or telemetry.batch

    def reset(self):
        """yaw_last = 0 for every robot (BipedalController::starting)."""
        self._call("bpmpc_controller_reset")

    def restart(self, mask, rbd):
        """BipedalController::starting for the robots with mask[b] != 0 (bpmpc_controller_restart): their observation from rbd [batch, 2 (6 + nj)]
        with the yaw unwrapped against 0, MPC_BASE::reset from it, clearLastQpSol; the other robots are not touched.  numpy arrays, or an int32 and
        a float64 device tensor (e.g. (safe == 0).int() of device_outputs: then the call only enqueues); len(mask) must be the solver's batch."""
        B = _count(mask)
        (mp, rp), dev, keep = _restart_args((mask, C.c_int, B), (rbd, C.c_double, B * 2 * self.wbc.generalizedCoordinatesNum))
        self._call("bpmpc_controller_restart", B, mp, rp, dev)
        del keep

    def device_outputs(self):
        """The results of the last tick where they live: a dict of DeviceArray (zero-copy; `.torch()` wraps one as a tensor) over the solver's batch."""
        o = _TickOutputs()
        self._call("bpmpc_controller_device_outputs", C.byref(o))
        B = self.mpc.batch
        views = {k: DeviceArray(C.cast(getattr(o, k), C.c_void_p).value, shp, "<i4" if k in ("planned_mode", "wbc_status", "safe") else "<f8")
                 for k, shp in self._shapes(B).items()}
        ptrs = [_dp() for _ in self.JOINT_NAMES]
        self._call("bpmpc_controller_joint_outputs", B, None, None, None, *[C.byref(p) for p in ptrs])
        for k, p in zip(self.JOINT_NAMES, ptrs):
            views[k] = DeviceArray(C.cast(p, C.c_void_p).value, (B, self.nj), "<f8")
        return views


class PolicyBuffer(_Handle):
    """MPC_MRT_Interface between the solve and the control tick (bpmpc_policy_*; BipedalController.cpp:191-200, :332-350): two slots of the
    solution per robot on the device.  `publish` copies the solver's last run into the slot the ticks do not read, on the solver's stream;
    `update` (updatePolicy) makes it the slot they read, on the buffer's own stream.  A BatchedController with the buffer attached
    (attachPolicy) ticks on that stream and on the adopted policy, whatever the solver is doing meanwhile."""

    _DESTROY = "bpmpc_policy_destroy"

    def __init__(self, mpc, max_batch):
        self.mpc, self.max_batch = mpc, int(max_batch)
        super().__init__()
        _check(load_library().bpmpc_policy_create(mpc._h, self.max_batch, C.byref(self._h)))

    def publish(self, mask=None, skip_failed=False):
        """The last run of the solver into the back slot, for the robots with mask[b] != 0 (None: every robot; a numpy array, or an int32 device
        tensor: then nothing synchronises) and, with skip_failed, only those whose solve status on the device is not 2."""
        B = self.mpc.batch
        (mp,), dev, keep = _restart_args((mask, C.c_int, B))
        self._call("bpmpc_policy_publish", B, mp, dev, int(bool(skip_failed)))
        del keep

    def update(self, wait=True):
        """updatePolicy.  wait=True: the buffer's stream waits for the last publish and adopts it, the host does not block; wait=False: adopts it
        only if it has completed.  Returns whether an adoption was enqueued (False with no publish outstanding)."""
        adopted = C.c_int(0)
        self._call("bpmpc_policy_update", int(bool(wait)), C.byref(adopted))
        return bool(adopted.value)

    def info(self, batch=None):
        """{"generation", "t0", "status"}: per robot the number of policies adopted, the time of node 0 of the policy the ticks read and the solve
        status it was published with (synchronises the buffer's stream)."""
        B = int(batch or self.mpc.batch or self.max_batch)
        out = {"generation": np.zeros(B, np.int32), "t0": np.zeros(B), "status": np.zeros(B, np.int32)}
        self._call("bpmpc_policy_info", B, _i(out["generation"]), _d(out["t0"]), _i(out["status"]))
        return out


class TelemetrySample:
    """The fields of a telemetry sample row (include/bpmpc.h "Tracking telemetry"): STRIDE(nj) doubles; fields(nj) maps a name to its
    (offset, shape); split(rows, nj) slices rows [..., STRIDE(nj)] into a dict of named arrays."""

    GROUPS = ("base_pos", "base_zyx", "contact_0", "contact_1", "contact_2", "contact_3", "joint_pos")      # the error groups e0..e6
    STATS_STRIDE = 40

    @staticmethod
    def STRIDE(nj):
        return 40 + 2 * nj

    @staticmethod
    def fields(nj):
        return {"base_pos_desired": (0, (3,)), "base_zyx_desired": (3, (3,)), "base_pos_measured": (6, (3,)), "base_zyx_measured": (9, (3,)),
                "contact_pos_desired": (12, (4, 3)), "contact_pos_measured": (24, (4, 3)), "joint_pos_desired": (36, (nj,)),
                "joint_pos_measured": (36 + nj, (nj,)), "t": (36 + 2 * nj, ()), "safe": (37 + 2 * nj, ()), "planned_mode": (38 + 2 * nj, ()),
                "n": (39 + 2 * nj, ())}

    @classmethod
    def split(cls, rows, nj):
        rows = np.asarray(rows, float)
        if rows.shape[-1] != cls.STRIDE(nj):
            raise ValueError("a sample of a robot with %d joints has %d entries, got %d" % (nj, cls.STRIDE(nj), rows.shape[-1]))
        return {k: rows[..., off:off + int(np.prod(shp, dtype=int))].reshape(rows.shape[:-1] + shp) for k, (off, shp) in cls.fields(nj).items()}


class BatchedTelemetry(_Handle):
    """DebugPublisher::update (bipedal_controllers/src/debug/DebugPublisher.cpp; BipedalController.cpp:270) for a batch of robots, kept on the
    device (bpmpc_telemetry): per update a sample of the desired beside the measured base pose, contact points and joints, tracking-error
    statistics over the episode, and a ring of the last `ring_len` samples per robot that freezes when the robot falls.  Attach it to a
    BatchedController (attachTelemetry) and every tick takes a sample on the controller's stream; nothing reaches the host until stats() or
    ring() ask for it."""

    _DESTROY = "bpmpc_telemetry_destroy"

    def __init__(self, interface, max_batch, ring_len=0, device=0):
        self.interface, self.max_batch, self.ring_len = interface, int(max_batch), int(ring_len)
        self.nj = interface.actuatedDofNum
        super().__init__()
        _check(load_library().bpmpc_telemetry_create(interface.handle, int(device), self.max_batch, self.ring_len, C.byref(self._h)))
        s, r, n = C.c_int(), C.c_int(), C.c_int()
        self._call("bpmpc_telemetry_dims", C.byref(s), C.byref(r), C.byref(n))
        self.sample_stride, self.stats_stride = s.value, r.value
        self.batch = self.max_batch

    def update(self, x_opt, rbd, t=None, safe=None, planned_mode=None):
        """One sample for B = len(x_opt) robots, outside a controller: x_opt [B, 12 + nj], rbd [B, 2 (6 + nj)], t [B], safe [B], planned_mode [B]
        (each of the last three may be None).  numpy arrays (the call synchronises), or float64 / int32 device arrays - torch tensors or
        DeviceArray, e.g. BatchedController.device_outputs() - which are only enqueued on the handle's stream."""
        B = _shape(x_opt)[0]
        nv = 6 + self.nj
        (tp, xp, rp, sp, mp), dev, keep = _restart_args((t, C.c_double, B), (x_opt, C.c_double, B * (12 + self.nj)), (rbd, C.c_double, B * 2 * nv),
                                                        (safe, C.c_int, B), (planned_mode, C.c_int, B))
        self._call("bpmpc_telemetry_update", B, tp, xp, rp, sp, mp, dev)
        del keep
        self.batch = B

    def configure(self, every=1, freeze_on_unsafe=True):
        """Every `every`-th update of a robot goes into its ring; freeze_on_unsafe: a robot's record freezes at its first sample that is unsafe
        or not finite."""
        self._call("bpmpc_telemetry_configure", int(every), int(bool(freeze_on_unsafe)))

    def reset(self, mask=None):
        """The record of the robots with mask[b] != 0 (None: every robot) starts over; the others do not change by one bit.  A numpy mask, or an
        int32 device tensor - e.g. the (safe == 0) mask of BatchedController.restart - which is only enqueued."""
        B = self.max_batch if mask is None else _count(mask)
        (mp,), dev, keep = _restart_args((mask, C.c_int, B))
        self._call("bpmpc_telemetry_reset", B, mp, dev)
        del keep

    def stats(self, batch=None):
        """The statistics of the first B robots (None: the batch of the last update() or the attached controller's; synchronises): rms [B, 7] and
        max [B, 7] of the error groups TelemetrySample.GROUPS, max_at [B, 7] (the update counter n at the maximum), samples [B], first_unsafe [B]
        (-1: none), joint_max [B, nj], frozen [B]."""
        B = int(batch or self.batch)
        rows, frozen = np.zeros((B, self.stats_stride)), np.zeros(B, np.int32)
        self._call("bpmpc_telemetry_get_stats", B, _d(rows), _i(frozen))
        g = rows[:, :21].reshape(B, 7, 3)
        samples = rows[:, 21]
        return {"rms": np.sqrt(g[:, :, 0] / np.maximum(samples, 1.0)[:, None]), "max": g[:, :, 1].copy(), "max_at": g[:, :, 2].astype(np.int64),
                "samples": samples.astype(np.int64), "first_unsafe": rows[:, 22].astype(np.int64), "joint_max": rows[:, 23:23 + self.nj].copy(),
                "frozen": frozen, "rows": rows}

    def ring(self, robots=None, batch=None):
        """The ring of `robots` (a list of indices; None: every robot of the batch), oldest sample first: the fields of TelemetrySample over
        [R, ring_len, ...], `samples` [R, ring_len, stride] and `count` [R] - the slots behind a robot's count are zero.  Synchronises."""
        B = int(batch or self.batch)
        idx = None if robots is None else np.ascontiguousarray(robots, np.int32).reshape(-1)
        R = B if idx is None else idx.size
        rows, count = np.zeros((R, self.ring_len, self.sample_stride)), np.zeros(R, np.int32)
        self._call("bpmpc_telemetry_fetch_ring", B, None if idx is None else _i(idx), R, _d(rows), _i(count))
        out = TelemetrySample.split(rows, self.nj)
        out["samples"], out["count"] = rows, count
        return out

    def outputs(self):
        """The last sample [max_batch, stride], the statistics rows [max_batch, 40] and the frozen flags [max_batch] where they live: a dict of
        DeviceArray."""
        s, r, f = _dp(), _dp(), _ip()
        self._call("bpmpc_telemetry_device_outputs", C.byref(s), C.byref(r), C.byref(f))
        B = self.max_batch
        return {"sample": DeviceArray(C.cast(s, C.c_void_p).value, (B, self.sample_stride), "<f8"),
                "stats": DeviceArray(C.cast(r, C.c_void_p).value, (B, self.stats_stride), "<f8"),
                "frozen": DeviceArray(C.cast(f, C.c_void_p).value, (B,), "<i4")}


class PlanNode:
    """The fields of a node row of the plan geometry (include/bpmpc.h "Plan geometry"): STRIDE doubles; FIELDS maps a name to its
    (offset, shape); split(rows) slices rows [..., STRIDE] into a dict of named arrays.  SUMMARY names the entries of a summary row and FOOTHOLD
    those of a foothold entry the same way."""

    STRIDE, MAX_FOOTHOLDS, FOOTHOLD_STRIDE, SUMMARY_STRIDE = 24, 16, 6, 16
    FIELDS = {"base_pos": (0, (3,)), "contact_pos": (3, (4, 3)), "cop": (15, (3,)), "t": (18, ()), "mode": (19, ()), "kind": (20, ()), "sum_z": (21, ()),
              "contact_mask": (22, ()), "not_finite": (23, ())}
    FOOTHOLD = {"t": (0, ()), "contact": (1, ()), "pos": (2, (3,)), "node": (5, ())}
    SUMMARY = {"n_nodes": (0, ()), "footholds": (1, ()), "base_path_length": (2, ()), "apex": (3, (4,)), "stance_drift": (7, (4,)), "min_sum_z": (11, ()),
               "not_finite": (12, ()), "reserved": (13, (3,))}

    @staticmethod
    def _split(rows, fields, stride):
        rows = np.asarray(rows, float)
        if rows.shape[-1] != stride:
            raise ValueError("a row of %d entries was expected, got %d" % (stride, rows.shape[-1]))
        return {k: rows[..., off:off + int(np.prod(shp, dtype=int))].reshape(rows.shape[:-1] + shp) for k, (off, shp) in fields.items()}

    @classmethod
    def split(cls, rows):
        return cls._split(rows, cls.FIELDS, cls.STRIDE)

    @classmethod
    def split_footholds(cls, entries):
        return cls._split(entries, cls.FOOTHOLD, cls.FOOTHOLD_STRIDE)

    @classmethod
    def split_summary(cls, rows):
        return cls._split(rows, cls.SUMMARY, cls.SUMMARY_STRIDE)


class PlanGeometry(_Handle):
    """BipedalControllerVisualizer::update (bipedal_controllers/src/BipedalControllerVisualizer.cpp:73-87) for a batch of robots, kept on the
    device (bpmpc_plan): for every node of a plan the base position, the four contact points, the centre of pressure and the contact forces'
    sum; the future footholds; a summary row per robot.  A plan comes from a solver (update), from the front slot of a PolicyBuffer
    (update_from_policy) or from arrays (update_arrays); nothing reaches the host until nodes(), footholds() or summary() ask for it."""

    _DESTROY = "bpmpc_plan_destroy"

    def __init__(self, interface, max_batch, max_nodes, device=0):
        self.interface, self.max_batch, self.max_nodes = interface, int(max_batch), int(max_nodes)
        self.nj = interface.actuatedDofNum
        super().__init__()
        _check(load_library().bpmpc_plan_create(interface.handle, int(device), self.max_batch, self.max_nodes, C.byref(self._h)))
        self.batch = self.max_batch

    def configure(self, launches=0):
        """How an update is launched: 1 one kernel, 2 a kernel over the node tiles and one for footholds and summary, 0 the handle chooses."""
        self._call("bpmpc_plan_configure", int(launches))

    def update(self, solver):
        """The current iterate of the solver's last setup (after a run: the solution), enqueued on the solver's stream; nothing synchronises."""
        self._call("bpmpc_plan_update_from_solver", solver._h)
        self.batch = solver.batch

    def update_from_policy(self, buffer):
        """The front slot of a PolicyBuffer, enqueued on the buffer's stream; the desired block is not written."""
        self._call("bpmpc_plan_update_from_policy", buffer._h)
        self.batch = buffer.mpc.batch

    def update_arrays(self, n_nodes, t, x, mode, kind, u=None, xref=None):
        """A plan per robot with the handle's strides, N = max_nodes: n_nodes [B], t [B, N + 1], x [B, N + 1, nx], mode and kind [B, N],
        u [B, N, nu] and xref [B, N, nx] (each of the last two may be None).  numpy arrays (the call synchronises), or float64 / int32 device
        arrays - torch tensors or DeviceArray - which are only enqueued on the handle's stream."""
        B, N, nx = _shape(n_nodes)[0], self.max_nodes, 12 + self.nj
        (np_, tp, xp, up, mp, kp, rp), dev, keep = _restart_args(
            (n_nodes, C.c_int, B), (t, C.c_double, B * (N + 1)), (x, C.c_double, B * (N + 1) * nx), (u, C.c_double, B * N * nx), (mode, C.c_int, B * N),
            (kind, C.c_int, B * N), (xref, C.c_double, B * N * nx))
        self._call("bpmpc_plan_update", B, np_, tp, xp, up, mp, kp, rp, dev)
        del keep
        self.batch = B

    def outputs(self):
        """Where the outputs live: a dict of DeviceArray - optimized and desired [max_batch, N + 1, 24], footholds [max_batch, 16, 6], summary
        [max_batch, 16], foothold_count [max_batch]."""
        o = abi._PlanOutputs()
        self._call("bpmpc_plan_device_outputs", C.byref(o))
        B, K = self.max_batch, self.max_nodes + 1
        ptr = lambda p: C.cast(p, C.c_void_p).value      # noqa: E731
        return {"optimized": DeviceArray(ptr(o.optimized), (B, K, PlanNode.STRIDE), "<f8"), "desired": DeviceArray(ptr(o.desired), (B, K, PlanNode.STRIDE), "<f8"),
                "footholds": DeviceArray(ptr(o.footholds), (B, PlanNode.MAX_FOOTHOLDS, PlanNode.FOOTHOLD_STRIDE), "<f8"),
                "summary": DeviceArray(ptr(o.summary), (B, PlanNode.SUMMARY_STRIDE), "<f8"), "foothold_count": DeviceArray(ptr(o.foothold_count), (B,), "<i4")}

    def nodes(self, which="optimized", batch=None):
        """The node rows [B, N + 1, 24] of the first B robots (None: the batch of the last update; synchronises): which = "optimized" or
        "desired".  PlanNode.split names the entries; rows beyond a robot's n_nodes hold what they held before."""
        B = int(batch or self.batch)
        rows = np.zeros((B, self.max_nodes + 1, PlanNode.STRIDE))
        self._call("bpmpc_plan_get_nodes", B, {"optimized": 0, "desired": 1}[which], _d(rows))
        return rows

    def footholds(self, batch=None):
        """(entries [B, 16, 6], count [B]): the future footholds (t, contact point, x, y, z, node) in the order (node, contact point); count is
        the true number, of which the first 16 are stored.  Synchronises."""
        B = int(batch or self.batch)
        entries, count = np.zeros((B, PlanNode.MAX_FOOTHOLDS, PlanNode.FOOTHOLD_STRIDE)), np.zeros(B, np.int32)
        self._call("bpmpc_plan_get_footholds", B, _d(entries), _i(count))
        return entries, count

    def summary(self, batch=None):
        """The summary rows [B, 16] (PlanNode.split_summary names the entries).  Synchronises."""
        B = int(batch or self.batch)
        rows = np.zeros((B, PlanNode.SUMMARY_STRIDE))
        self._call("bpmpc_plan_get_summary", B, _d(rows))
        return rows

    @staticmethod
    def rows_host(interface, t, x, mode, kind, u=None):
        """bpmpc_plan_rows_host: (rows [n + 1, 24], footholds [16, 6], count, summary [16]) of one robot on the host, no device: t [n + 1],
        x [n + 1, nx], mode and kind [n], u [n, nu] or None."""
        t, x = _f64(t).reshape(-1), _f64(x)
        n = t.size - 1
        mode, kind = np.ascontiguousarray(mode, np.int32).reshape(-1), np.ascontiguousarray(kind, np.int32).reshape(-1)
        nx = 12 + interface.actuatedDofNum
        if x.shape != (n + 1, nx) or mode.size != n or kind.size != n or (u is not None and np.shape(u) != (n, nx)):
            raise ValueError("a plan of %d nodes needs t [%d], x [%d, %d], mode and kind [%d], u [%d, %d] or None" % (n, n + 1, n + 1, nx, n, n, nx))
        u = None if u is None else _f64(u)
        rows, foot, count, summ = np.zeros((n + 1, PlanNode.STRIDE)), np.zeros((PlanNode.MAX_FOOTHOLDS, PlanNode.FOOTHOLD_STRIDE)), C.c_int(0), np.zeros(PlanNode.SUMMARY_STRIDE)
        _check(load_library().bpmpc_plan_rows_host(interface.handle, n, _d(t), _d(x), _d(u), _i(mode), _i(kind), _d(rows), _d(foot), C.byref(count), _d(summ)))
        return rows, foot, count.value, summ


class PlantParams(_RowParams):
    """A parameter row of the plant (include/bpmpc.h "Plant", BPMPC_PLANT_PARAM_STRIDE) with named fields: contact stiffness kn [N/m], normal damping
    cn [N s/m], the penetration d0 [m] at which the normal damping is fully on, friction coefficient mu, the velocity v_eps [m/s] that regularises
    the Coulomb law, and the normal force contact_threshold [N] above which a contact point reports contact.  The defaults are the values without
    arguments."""

    STRIDE = 8
    FIELDS = ("kn", "cn", "d0", "mu", "v_eps", "contact_threshold")
    DEFAULTS = (5e4, 5e2, 1e-3, 0.7, 0.01, 1.0)


class SensorParams(_RowParams):
    """A row of the plant's sensor model (include/bpmpc.h "Plant", sensors; BPMPC_PLANT_SENSOR_PARAM_STRIDE) with named fields: white noise, bias
    random walk and turn-on bias of the gyro [rad/s, rad/s/sqrt(s), rad/s] and of the accelerometer [m/s^2 ...], orientation noise [rad], joint
    position noise and encoder resolution [rad; 0: not quantised], joint velocity noise [rad/s], the probability that a closed contact reports
    open, and the latency in control steps (an integer 0..8).  Every default is 0: the sensors read the truth."""

    STRIDE = 16
    FIELDS = ("gyro_noise", "gyro_bias_walk", "gyro_bias_init", "accel_noise", "accel_bias_walk", "accel_bias_init", "orientation_noise", "joint_pos_noise",
              "joint_pos_resolution", "joint_vel_noise", "contact_dropout", "delay_steps")


class InputParams(_RowParams):
    """A row of the plant's input model (include/bpmpc.h "Plant", inputs; BPMPC_PLANT_INPUT_PARAM_STRIDE) with named fields: the command latency
    delay [s] (the reference's gazebo/delay), the probability dropout that a command does not arrive (the joint holds the previous one), and
    pushes on the base of push_force [N] for push_duration [s], one at a random time and from a random horizontal direction in every
    push_interval [s].  Every default is 0: the step consumes the command it was called with."""

    STRIDE = 8
    FIELDS = ("delay", "dropout", "push_force", "push_interval", "push_duration")


class JointParams:
    """A joint row of the plant (include/bpmpc.h "Plant", joints; BPMPC_PLANT_JOINT_PARAM_STRIDE) with named fields: per joint (arrays of nj)
    armature [kg m^2], damping [N m s/rad], friction_loss [N m], lower and upper [rad, -inf / +inf: no end stop]; per robot the end-stop spring
    k_limit [N m/rad] and damper c_limit [N m s/rad] and the velocity w_eps [rad/s] that regularises the friction law.  A per-joint field takes a
    scalar (every joint) or nj values.  Without arguments the row is the neutral one: ideal joints."""

    STRIDE = 64
    SLOTS = 12
    JOINT_FIELDS = ("armature", "damping", "friction_loss", "lower", "upper")
    JOINT_DEFAULTS = (0.0, 0.0, 0.0, -np.inf, np.inf)
    SCALAR_FIELDS = ("k_limit", "c_limit", "w_eps")
    SCALAR_DEFAULTS = (1e4, 1e2, 0.01)
    FIELDS = JOINT_FIELDS + SCALAR_FIELDS

    def __init__(self, nj, **fields):
        unknown = set(fields) - set(self.FIELDS)
        if unknown:
            raise ValueError("unknown parameter(s): %s" % sorted(unknown))
        self.nj = int(nj)
        if not 1 <= self.nj <= self.SLOTS:
            raise ValueError("a joint row holds 1..%d joints" % self.SLOTS)
        for name, default in zip(self.JOINT_FIELDS, self.JOINT_DEFAULTS):
            value = np.asarray(fields.get(name, default), float)
            if value.ndim and value.shape != (self.nj,):
                raise ValueError("%s takes a scalar or %d values" % (name, self.nj))
            setattr(self, name, np.broadcast_to(value, (self.nj,)).copy())
        for name, default in zip(self.SCALAR_FIELDS, self.SCALAR_DEFAULTS):
            setattr(self, name, float(fields.get(name, default)))

    @classmethod
    def neutral(cls, nj):
        """Ideal joints: no armature, damping or friction, no end stops."""
        return cls(nj)

    @classmethod
    def reference_mjcf(cls, nj):
        """armature 0.1 kg m^2 and damping 1 N m s/rad on every joint: the values the reference's H1 MJCF declares as the default of every joint
        (`<default><joint damping="1" armature="0.1"/></default>`, unitree_h1/h1_description/mjcf/h1.xml:7), taken as data."""
        return cls(nj, armature=0.1, damping=1.0)

    @classmethod
    def fromRow(cls, row, nj):
        r = np.asarray(row, float).reshape(-1)
        if r.size != cls.STRIDE:
            raise ValueError("a joint row has %d entries" % cls.STRIDE)
        nj = int(nj)
        fields = {name: r[i * cls.SLOTS:i * cls.SLOTS + nj] for i, name in enumerate(cls.JOINT_FIELDS)}
        fields.update({name: r[60 + i] for i, name in enumerate(cls.SCALAR_FIELDS)})
        return cls(nj, **fields)

    def toRow(self):
        row = np.zeros(self.STRIDE)
        for i, (name, default) in enumerate(zip(self.JOINT_FIELDS, self.JOINT_DEFAULTS)):
            row[i * self.SLOTS:(i + 1) * self.SLOTS] = default
            row[i * self.SLOTS:i * self.SLOTS + self.nj] = getattr(self, name)
        for i, name in enumerate(self.SCALAR_FIELDS):
            row[60 + i] = float(getattr(self, name))
        return row


class BodyParams:
    """A body row of the plant (include/bpmpc.h "Plant", bodies; BPMPC_PLANT_BODY_PARAM_STRIDE): mass [kg], centre of mass [m, body frame] and
    inertia about it [kg m^2, body frame: xx, xy, xz, yy, yz, zz] of every body of a robot, body 0 the base and body b the link moved by joint b.
    BodyParams.model(interface) is the row the controller plans with; scaled / shifted / payload return a new row built from this one by
    bpmpc_plant_compose_body_row, so the rules of the header hold for every row made here.  `row` [160] is what BatchedPlant.setBodyParams takes."""

    STRIDE = 160
    SLOTS = 16
    MASS, COM, INERTIA = 0, 16, 64

    def __init__(self, model, row=None):
        self._model = model
        self.nj = int(model.actuatedDofNum)
        if row is None:
            row = np.zeros(self.STRIDE)
            model._call("bpmpc_plant_load_body_params", None, _d(row))
        self.row = _f64(row).reshape(-1).copy()
        if self.row.size != self.STRIDE:
            raise ValueError("a body row has %d entries" % self.STRIDE)

    @classmethod
    def model(cls, model):
        """The model row: bpmpc_model_get "body_mass", "body_com" and "body_inertia" in the layout of a body row."""
        return cls(model)

    def _compose(self, body, scale, shift, mass, pos):
        out = np.zeros(self.STRIDE)
        shift = None if shift is None else _f64(shift).reshape(3)
        pos = None if pos is None else _f64(pos).reshape(3)
        self._model._call("bpmpc_plant_compose_body_row", _d(self.row), int(body), float(scale), _d(shift), float(mass), _d(pos), _d(out))
        return type(self)(self._model, out)

    def scaled(self, s, body=None):
        """Mass and inertia of `body` (None: of every body) times s: the same shape at another uniform density."""
        return self._compose(-1 if body is None else body, s, None, 0.0, None)

    def shifted(self, body, d):
        """The centre of mass of `body` moved by d [3] (body frame); its inertia about the new centre of mass is the one it had."""
        return self._compose(body, 1.0, d, 0.0, None)

    def payload(self, m, pos, body=0):
        """A point mass m at pos [3] (body frame) merged into `body`: new mass, new centre of mass, new inertia by the parallel-axis theorem."""
        return self._compose(body, 1.0, None, m, pos)

    @property
    def mass(self):
        return self.row[self.MASS:self.MASS + self.nj + 1].copy()

    @property
    def com(self):
        """[nj + 1, 3]"""
        return self.row[self.COM:self.INERTIA].reshape(3, self.SLOTS)[:, :self.nj + 1].T.copy()

    @property
    def inertia(self):
        """[nj + 1, 6]: xx, xy, xz, yy, yz, zz"""
        return self.row[self.INERTIA:].reshape(6, self.SLOTS)[:, :self.nj + 1].T.copy()

    @property
    def total_mass(self):
        return float(self.mass.sum())


class BatchedPlant(_Handle):
    """A rigid-body simulation of a batch of robots on one MI355X (bpmpc_plant; include/bpmpc.h "Plant" is its specification): joint commands ->
    the sensors BatchedStateEstimate.update takes and the ground-truth rbd.  This engine's own model - penalty contacts with implicit damping, a
    joint PD with an implicit kd term, semi-implicit Euler - and not an imitation of the simulators the reference runs against.  taskFile (None:
    the interface's) is read for the keys plant.<name> and for the WBC's torque limits."""

    _DESTROY = "bpmpc_plant_destroy"

    def __init__(self, interface, max_batch=1, taskFile=None, device=0):
        self.interface, self.max_batch = interface, int(max_batch)
        self.nj = interface.actuatedDofNum
        self.generalizedCoordinatesNum = 6 + self.nj
        super().__init__()
        _check(load_library().bpmpc_plant_create(interface.handle, str(taskFile or interface.taskFile).encode(), int(device), self.max_batch, C.byref(self._h)))
        self.batch = 0

    def set_state(self, rbd, mask=None):
        """q, v of the robots with mask[b] != 0 (None: every one of the B) from rbd [B, 2 (6 + nj)] in the layout of BatchedController.tick; the
        others do not change by one bit.  numpy arrays (validated, synchronises) or float64 / int32 device tensors (only enqueued)."""
        shape = _shape(rbd)
        if len(shape) != 2 or shape[1] != 2 * self.generalizedCoordinatesNum:
            raise ValueError("rbd must have the shape [B, %d], got %s" % (2 * self.generalizedCoordinatesNum, list(shape)))
        B = shape[0]
        (mp, rp), dev, keep = _restart_args((mask, C.c_int, B), (rbd, C.c_double, B * shape[1]))
        self._call("bpmpc_plant_set_state", B, mp, rp, dev)
        del keep
        self.batch = B

    def get_state(self, batch=None):
        """The ground-truth rbd [B, 2 (6 + nj)] of the first B robots (None: the batch of the last set_state); synchronises."""
        B = int(batch or self.batch)
        rbd = np.zeros((B, 2 * self.generalizedCoordinatesNum))
        self._call("bpmpc_plant_get_state", B, _d(rbd))
        return rbd

    def step(self, pos_des, vel_des, tau_ff, kp, kd, base_force=None, feet_heights=None, period=0.002, substeps=4):
        """One control step of `period` in `substeps` substeps for the batch of the last set_state.  pos_des, vel_des, tau_ff, kp, kd: [B, nj];
        base_force [B, 3] (world-frame force on the base origin) and feet_heights [B, 4] (ground height under each contact point) may be None.
        numpy arrays (synchronises) or float64 device tensors (only enqueued; see outputs)."""
        B, nj = self.batch, self.nj
        ptrs, dev, keep = _restart_args(*[(a, C.c_double, B * nj) for a in (pos_des, vel_des, tau_ff, kp, kd)], (base_force, C.c_double, B * 3),
                                        (feet_heights, C.c_double, B * 4))
        cmd = _JointCommand(*ptrs)
        self._call("bpmpc_plant_step", B, C.byref(cmd), dev, period, int(substeps))
        del keep

    def step_controlled(self, controller, base_force=None, feet_heights=None, period=0.002, substeps=4):
        """One control step on the last tick of `controller` (BatchedController): posDes / velDes / torque of its joint_cmd and its joint gains, read
        on the device; the two handles' streams are ordered by events, nothing is synchronised unless base_force / feet_heights are host arrays."""
        B = self.batch
        (fp, gp), dev, keep = _restart_args((base_force, C.c_double, B * 3), (feet_heights, C.c_double, B * 4))
        self._call("bpmpc_plant_step_controlled", controller._h, B, period, int(substeps), fp, gp, dev)
        del keep

    def step_supervised(self, supervisor, base_force=None, feet_heights=None, period=0.002, substeps=4):
        """One control step on the commands of the last update of `supervisor` (BatchedSupervisor), read on the device; ordered by events like
        step_controlled."""
        B = self.batch
        (fp, gp), dev, keep = _restart_args((base_force, C.c_double, B * 3), (feet_heights, C.c_double, B * 4))
        self._call("bpmpc_plant_step_supervised", supervisor._h, B, period, int(substeps), fp, gp, dev)
        del keep

    def outputs(self):
        """The outputs of the last step where they live: a dict of DeviceArray (`.torch()` wraps one without a copy) over the batch of the last
        set_state - the sensors of BatchedStateEstimate.update by name (joint_pos, joint_vel, quat, angular_vel_local, linear_accel_local, contact,
        feet_heights, odom_pos, odom_quat, odom_lin_vel, odom_ang_vel), rbd and contact_force [B, 4, 3]."""
        o = _PlantOutputs()
        self._call("bpmpc_plant_device_outputs", C.byref(o))
        B, nj = self.batch or self.max_batch, self.nj
        shapes = {"joint_pos": (B, nj), "joint_vel": (B, nj), "quat": (B, 4), "angular_vel_local": (B, 3), "linear_accel_local": (B, 3), "contact": (B, 4),
                  "feet_heights": (B, 4), "odom_pos": (B, 3), "odom_quat": (B, 4), "odom_lin_vel": (B, 3), "odom_ang_vel": (B, 3)}
        views = {k: DeviceArray(C.cast(getattr(o.sensors, k), C.c_void_p).value, shp, "<i4" if k == "contact" else "<f8") for k, shp in shapes.items()}
        views["rbd"] = DeviceArray(C.cast(o.rbd, C.c_void_p).value, (B, 2 * self.generalizedCoordinatesNum), "<f8")
        views["contact_force"] = DeviceArray(C.cast(o.contact_force, C.c_void_p).value, (B, 4, 3), "<f8")
        return views

    getParams, setParams, resetParams = _param_methods(
        "bpmpc_plant", PlantParams.STRIDE,
        """The parameter row [8] of `robot` (PlantParams.fromRow names its entries), or with robot < 0 the values every row starts from.""",
        """rows [8], [1, 8] or [B, 8]; mask as WeightedWbc.setParams.  numpy rows are validated (finite; kn, d0, v_eps positive; the others not
        negative) and the call synchronises; device tensors are only enqueued, ordered before the next step.""")

    def setStiction(self, kt, mask=None):
        """The tangential contact stiffness kt [N/m] of the robots with mask[b] != 0 (None: every one): one value for all of them, or [B] values.
        kt = 0 is the plant without stick-slip contacts.  A robot whose kt changes loses its anchors.  numpy values are validated (finite, not
        negative) and the call synchronises; float64 / int32 device tensors are only enqueued, ordered before the next step."""
        if hasattr(kt, "data_ptr"):
            rows = kt.reshape(1) if kt.numel() == 1 else kt.reshape(-1, 1)
        else:
            kt = np.asarray(kt, float).reshape(-1)
            rows = kt if kt.size == 1 else kt.reshape(-1, 1)
        B, n_rows, (mp, kp), dev, keep = _rows_args(mask, [rows], 1, self.max_batch)
        self._call("bpmpc_plant_set_stiction", B, mp, kp, n_rows, dev)
        del keep

    def getStiction(self, robot=-1):
        """kt of `robot`, or with robot < 0 the value every robot starts from (the key plant.kt of the task file; absent: 0)."""
        kt = C.c_double()
        self._call("bpmpc_plant_get_stiction", int(robot), C.byref(kt))
        return kt.value

    def resetStiction(self):
        """Every robot's kt back to the handle's start value; every anchor cleared."""
        self._call("bpmpc_plant_reset_stiction")

    def anchors(self):
        """(anchor [B, 4, 2], anchored [B, 4]) of the batch of the last set_state (before it: max_batch): the world xy each contact point's tangential
        spring is anchored at, and whether it is; synchronises."""
        B = self.batch or self.max_batch
        anchor, anchored = np.zeros((B, 4, 2)), np.zeros((B, 4), np.int32)
        self._call("bpmpc_plant_get_anchors", B, _d(anchor), _i(anchored))
        return anchor, anchored

    getSensorParams, setSensorParams, resetSensorParams = _param_methods(
        "bpmpc_plant", SensorParams.STRIDE,
        """The sensor row [16] of `robot` (SensorParams.fromRow names its entries), or with robot < 0 the row of the task file (the keys
        plantSensors.<name>; absent: 0).""",
        """The sensor rows (SensorParams.toRow) of the robots with mask[b] != 0 (None: every one): rows [16], [1, 16] or [B, 16].  numpy rows are
        validated and the call synchronises; device tensors are only enqueued, ordered before the next step.  From this call on every step measures
        (k_plant_sense) and BatchedStateEstimate.update_from_plant reads sensed(); resetSensorParams ends that.""",
        """Every sensor row, bias and counter zero, every key the start key (plantSensors.seed): the plant is the one without a sensor model again.""",
        stem="Sensor")

    def seedSensors(self, seed, mask=None):
        """Restarts the random streams of the robots with mask[b] != 0 (None: every one of the batch of the last set_state; before it: max_batch)
        under `seed`: tick and sample count 0, the biases drawn anew from gyro_bias_init / accel_bias_init of the robot's current row.  A numpy
        mask synchronises, an int32 device tensor is only enqueued."""
        B = _count(mask) if mask is not None else (self.batch or self.max_batch)
        (mp,), dev, keep = _restart_args((mask, C.c_int, B))
        self._call("bpmpc_plant_seed_sensors", B, mp, int(seed), dev)
        del keep

    def sensorState(self):
        """{"gyro_bias" [B, 3], "accel_bias" [B, 3], "tick" [B], "samples" [B]} of the batch of the last set_state (before it: max_batch): the
        biases, the generator's tick and the samples since the last (re)start; synchronises."""
        B = self.batch or self.max_batch
        bg, ba, ticks = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros((B, 2))
        self._call("bpmpc_plant_get_sensor_state", B, _d(bg), _d(ba), _d(ticks))
        return {"gyro_bias": bg, "accel_bias": ba, "tick": ticks[:, 0].astype(np.uint64), "samples": ticks[:, 1].astype(np.uint64)}

    def sensed(self):
        """What the sensors report after the last step, where it lives: a dict of DeviceArray with the sensor names of outputs().  joint_pos,
        joint_vel, quat, angular_vel_local, linear_accel_local and contact are the sensor model's; feet_heights and the odom_* channels are the
        truth's buffers."""
        o = _SensorInputs()
        self._call("bpmpc_plant_sensed_outputs", C.byref(o))
        B, nj = self.batch or self.max_batch, self.nj
        shapes = {"joint_pos": (B, nj), "joint_vel": (B, nj), "quat": (B, 4), "angular_vel_local": (B, 3), "linear_accel_local": (B, 3), "contact": (B, 4),
                  "feet_heights": (B, 4), "odom_pos": (B, 3), "odom_quat": (B, 4), "odom_lin_vel": (B, 3), "odom_ang_vel": (B, 3)}
        return {k: DeviceArray(C.cast(getattr(o, k), C.c_void_p).value, shp, "<i4" if k == "contact" else "<f8") for k, shp in shapes.items()}

    getInputParams, setInputParams, resetInputParams = _param_methods(
        "bpmpc_plant", InputParams.STRIDE,
        """The input row [8] of `robot` (InputParams.fromRow names its entries), or with robot < 0 the row of the task file (the keys
        plantInputs.<name>; absent: 0).""",
        """The input rows (InputParams.toRow) of the robots with mask[b] != 0 (None: every one): rows [8], [1, 8] or [B, 8].  numpy rows are
        validated and the call synchronises; device tensors are only enqueued, ordered before the next step.  From this call on every step runs
        the input model in front of its step kernel (k_plant_input) and applied() reports what the joints received; resetInputParams ends that.""",
        """Every input row and counter zero, every key the start key (plantInputs.seed): the plant is the one without an input model again.""",
        stem="Input")

    getJointParams, setJointParams, resetJointParams = _param_methods(
        "bpmpc_plant", JointParams.STRIDE,
        """The joint row [64] of `robot` (JointParams.fromRow(row, nj) names its entries), or with robot < 0 the start row (the neutral row under the
        keys plantJoints.<name> of the task file).""",
        """The joint rows (JointParams.toRow) of the robots with mask[b] != 0 (None: every one): rows [64], [1, 64] or [B, 64].  numpy rows are
        validated and the call synchronises; device tensors are only enqueued, ordered before the next step.  From the first call on EVERY robot
        of the plant steps in the kernel that holds the joint model (k_plant_joint_step), also those whose row stays neutral; resetJointParams
        ends that.""",
        """Every joint row back to the start row; with a neutral start row the plant is the one without a joint model again.""",
        stem="Joint")

    getBodyParams, _setBodyRows, resetBodyParams = _param_methods(
        "bpmpc_plant", BodyParams.STRIDE,
        """The body row [160] of `robot` (BodyParams(interface, row) names its entries), or with robot < 0 the start row (the model row under
        the keys plantBodies.<name> of the task file).""",
        None,
        """Every body row back to the start row; with the model row as start row the plant is the one without body rows again.""",
        stem="Body")

    def setBodyParams(self, rows, mask=None):
        """The body rows (BodyParams.row) of the robots with mask[b] != 0 (None: every one): rows [160], [1, 160] or [B, 160].  numpy rows are
        validated and the call synchronises; device tensors are only enqueued, ordered before the next step, and not looked at.  From the first
        call on EVERY robot of the plant steps in the kernel that holds the body rows (k_plant_body_step), also those whose row stays the
        model's; resetBodyParams ends that.  The controller keeps planning with the model's masses: the mismatch is the point."""
        if isinstance(rows, BodyParams):
            rows = rows.row
        elif isinstance(rows, (list, tuple)):
            rows = np.array([r.row if isinstance(r, BodyParams) else r for r in rows])
        self._setBodyRows(rows, mask)

    def seedInputs(self, seed, mask=None):
        """Restarts the random streams of the input model for the robots with mask[b] != 0 (None: every one of the batch of the last set_state;
        before it: max_batch) under `seed`: tick and step count 0, the buffered commands forgotten.  A numpy mask synchronises, an int32 device
        tensor is only enqueued."""
        B = _count(mask) if mask is not None else (self.batch or self.max_batch)
        (mp,), dev, keep = _restart_args((mask, C.c_int, B))
        self._call("bpmpc_plant_seed_inputs", B, mp, int(seed), dev)
        del keep

    def inputState(self):
        """{"tick" [B], "steps" [B], "delay_steps" [B], "lost" [B], "pushing" [B]} of the batch of the last set_state (before it: max_batch): the
        generator's tick, the steps since the last (re)start, and what the input model did in the last step; synchronises."""
        B = self.batch or self.max_batch
        ticks, delay, lost, pushing = np.zeros((B, 2)), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._call("bpmpc_plant_get_input_state", B, _d(ticks), _i(delay), _i(lost), _i(pushing))
        return {"tick": ticks[:, 0].astype(np.uint64), "steps": ticks[:, 1].astype(np.uint64), "delay_steps": delay, "lost": lost, "pushing": pushing}

    def applied(self):
        """The command the last step's kernel consumed, where it lives: a dict of DeviceArray, pos_des, vel_des, tau_ff, kp, kd [B, nj] and
        base_force [B, 3].  Refused on a plant whose input model is untouched and before the first step since it was switched on."""
        o = _JointCommand()
        self._call("bpmpc_plant_applied_command", C.byref(o))
        B, nj = self.batch or self.max_batch, self.nj
        shapes = {"pos_des": (B, nj), "vel_des": (B, nj), "tau_ff": (B, nj), "kp": (B, nj), "kd": (B, nj), "base_force": (B, 3)}
        return {k: DeviceArray(C.cast(getattr(o, k), C.c_void_p).value, shp, "<f8") for k, shp in shapes.items()}


class SupervisorParams(_RowParams):
    """A parameter row of the supervisor (include/bpmpc.h "Supervisor", BPMPC_SUP_PARAM_STRIDE) with named fields: the tilt limit [rad] of
    SafetyChecker, the base height [m] below which a robot is unsafe (0: no limit), the time [s] over which INIT ramps from the latched joints
    to q_init (0: the reference's jump), the settle test's position [rad] and velocity [rad/s] tolerances and the time [s] it must hold, and
    the damping gain of a stopped robot.  The defaults are the values without arguments."""

    STRIDE = 8
    FIELDS = ("tilt_limit", "min_base_height", "ramp_time", "settle_pos_tol", "settle_vel_tol", "settle_time", "stop_kd")
    DEFAULTS = (np.pi / 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


class BatchedSupervisor(_Handle):
    """Which controller drives which robot of a batch, decided on the device (bpmpc_supervisor; include/bpmpc.h "Supervisor" is its
    specification): InitialJointPositionController (state INIT), SafetyChecker with stopRequest (RUN to STOPPED) and the operator's switch
    script (request).  taskFile (None: the interface's) is read for the keys supervisor.<name>."""

    _DESTROY = "bpmpc_supervisor_destroy"
    INIT, RUN, STOPPED = 0, 1, 2
    JOINT_ROWS = ("q_init", "kp_init", "kd_init", "lower", "upper")
    COUNTS = ("init", "run", "stopped", "ready", "unsafe")

    def __init__(self, interface, max_batch=1, taskFile=None, device=0):
        self.interface, self.max_batch = interface, int(max_batch)
        self.nj = interface.actuatedDofNum
        super().__init__()
        _check(load_library().bpmpc_supervisor_create(interface.handle, str(taskFile or interface.taskFile).encode(), int(device), self.max_batch,
                                                      C.byref(self._h)))
        self.batch = self.max_batch

    def update(self, rbd, run_cmd=None, period=0.002):
        """One update of B = len(rbd) robots: rbd [B, 2 (6 + nj)]; run_cmd None or (pos_des, vel_des, tau_ff, kp, kd), [B, nj] each, the command a
        robot in RUN passes on.  numpy arrays (the call synchronises) or float64 device arrays - torch tensors or DeviceArray, e.g.
        BatchedPlant.outputs()["rbd"] - which are only enqueued on the supervisor's stream."""
        B = _shape(rbd)[0]
        specs = [(rbd, C.c_double, B * 2 * (6 + self.nj))] + [(a, C.c_double, B * self.nj) for a in (run_cmd or ())]
        if run_cmd is not None and len(run_cmd) != 5:
            raise ValueError("run_cmd is (pos_des, vel_des, tau_ff, kp, kd)")
        ptrs, dev, keep = _restart_args(*specs)
        cmd = _JointCommand(*ptrs[1:]) if run_cmd is not None else None
        self._call("bpmpc_supervisor_update", B, ptrs[0], None if cmd is None else C.byref(cmd), dev, float(period))
        del keep
        self.batch = B

    def update_controlled(self, controller, estimator=None, rbd=None, period=0.002):
        """One update on the last tick of `controller` (BatchedController), read on the device, and on the rbd of `estimator`
        (BatchedStateEstimate) or, without one, on the float64 device array rbd [B, 2 (6 + nj)]; the streams are ordered by events and nothing
        synchronises.  B is the batch of the controller's last tick."""
        B = controller.mpc.batch
        rp, keep = None, None
        if estimator is None:
            (rp,), dev, keep = _restart_args((rbd, C.c_double, B * 2 * (6 + self.nj)))
            if not dev:
                raise ValueError("update_controlled reads rbd on the device: pass a float64 device array, or an estimator")
        self._call("bpmpc_supervisor_update_controlled", controller._h, None if estimator is None else estimator._h, rp, B, float(period))
        del keep
        self.batch = B

    def request(self, target, mask=None, only_ready=False):
        """Asks for the state `target` (INIT, RUN or STOPPED) for the robots with mask[b] != 0 (None: every robot): INIT and STOPPED apply to all
        of them, RUN only to robots in INIT and with only_ready only to those that are ready; the others do not change by one bit.  A numpy
        mask, or an int32 device tensor, which is only enqueued."""
        B = self.max_batch if mask is None else _count(mask)
        (mp,), dev, keep = _restart_args((mask, C.c_int, B))
        self._call("bpmpc_supervisor_request", B, mp, int(target), int(bool(only_ready)), dev)
        del keep

    getParams, setParams, resetParams = _param_methods(
        "bpmpc_supervisor", SupervisorParams.STRIDE,
        """The parameter row [8] of `robot` (SupervisorParams.fromRow names its entries), or with robot < 0 the values every row starts from.""",
        """rows [8], [1, 8] or [B, 8]; mask as WeightedWbc.setParams.  numpy rows are validated (finite, not negative, tilt_limit positive) and
        the call synchronises; device tensors are only enqueued, ordered before the next update.""",
        """Every row back to the values it started from.""")

    def _which(self, which):
        return self.JOINT_ROWS.index(which) if isinstance(which, str) else int(which)

    def setJointRows(self, which, rows, mask=None):
        """The joint row `which` ("q_init", "kp_init", "kd_init", "lower", "upper" or 0..4) of the robots of `mask`: rows [nj], [1, nj] or [B, nj],
        host (validated; lower <= upper against the robot's other limit, which may be infinite) or device, as setParams."""
        B, n_rows, (mp, rp), dev, keep = _rows_args(mask, [rows], self.nj, self.max_batch)
        self._call("bpmpc_supervisor_set_joint_rows", B, mp, self._which(which), rp, n_rows, dev)
        del keep

    def getJointRows(self, which, robot=-1):
        """The joint row `which` [nj] of `robot`, or with robot < 0 the values every row starts from; synchronises."""
        row = np.zeros(self.nj)
        self._call("bpmpc_supervisor_get_joint_rows", int(robot), self._which(which), _d(row))
        return row

    def state(self, batch=None, commands=False):
        """Host copies for the first B robots (None: the batch of the last update; synchronises): state, cause, unsafe, ready [B] int32, elapsed
        [B], counts = {"init", "run", "stopped", "ready", "unsafe"} of the last update; with commands=True also pos_des, vel_des, tau_ff, kp,
        kd [B, nj]."""
        B = int(batch or self.batch)
        ints = {k: np.zeros(B, np.int32) for k in ("state", "cause", "unsafe", "ready")}
        elapsed, counts = np.zeros(B), np.zeros(8, np.int32)
        self._call("bpmpc_supervisor_get_state", B, *[_i(ints[k]) for k in ("state", "cause", "unsafe", "ready")], _d(elapsed), _i(counts))
        out = dict(ints, elapsed=elapsed, counts=dict(zip(self.COUNTS, counts.tolist())))
        if commands:
            cmd = {k: np.zeros((B, self.nj)) for k in ("pos_des", "vel_des", "tau_ff", "kp", "kd")}
            self._call("bpmpc_supervisor_get_commands", B, *[_d(a) for a in cmd.values()])
            out.update(cmd)
        return out

    def outputs(self):
        """The command rows [max_batch, nj], the per-robot flags [max_batch], the counters [8] and the clock `elapsed` where they live: a dict of
        DeviceArray."""
        o = _SupervisorOutputs()
        self._call("bpmpc_supervisor_device_outputs", C.byref(o))
        B = self.max_batch
        views = {k: DeviceArray(C.cast(getattr(o, k), C.c_void_p).value, (B, self.nj), "<f8") for k in ("pos_des", "vel_des", "tau_ff", "kp", "kd")}
        views.update({k: DeviceArray(C.cast(getattr(o, k), C.c_void_p).value, (B,), "<i4") for k in ("state", "cause", "unsafe", "ready")})
        views["counts"] = DeviceArray(C.cast(o.counts, C.c_void_p).value, (8,), "<i4")
        views["elapsed"] = DeviceArray(C.cast(o.elapsed, C.c_void_p).value, (B,), "<f8")
        return views

    def stream(self):
        """The supervisor's stream as an integer (a hipStream_t; torch.cuda.ExternalStream wraps it): what a caller that reads outputs() orders
        its own work against."""
        o = _SupervisorOutputs()
        self._call("bpmpc_supervisor_device_outputs", C.byref(o))
        return int(o.stream or 0)

    @staticmethod
    def rows_host(interface, params, joint_rows, rbd, flags, clocks, q_latch, run_cmd=None, period=0.002):
        """One update of one robot on the host, from the text the kernel is compiled from (bpmpc_supervisor_rows_host; no device).  params [8],
        joint_rows [5, nj], rbd [2 (6 + nj)], flags = (state, cause, unsafe, ready, latch_pending), clocks = (elapsed, settled), q_latch [nj],
        run_cmd None or five [nj] arrays.  Returns (flags [5] int32, clocks [2], q_latch [nj], command [5, nj])."""
        nj = interface.actuatedDofNum
        p, j, r = _f64(params).reshape(8), _f64(joint_rows).reshape(5, nj), _f64(rbd).reshape(2 * (6 + nj))
        f, c, ql = np.array(flags, np.int32).reshape(5), np.array(clocks, float).reshape(2), np.array(q_latch, float).reshape(nj)
        cmd, keep = None, None
        if run_cmd is not None:
            keep = [_f64(a).reshape(nj) for a in run_cmd]
            cmd = _JointCommand(*[_d(a) for a in keep], None, None)
        out = np.zeros((5, nj))
        _check(load_library().bpmpc_supervisor_rows_host(interface.handle, _d(p), _d(j), _d(r), None if cmd is None else C.byref(cmd), float(period), _i(f),
                                                         _d(c), _d(ql), _d(out)))
        return f, c, ql, out


class BatchedDdpMpc(BatchedSqpMpc):
    """A batch of GaussNewtonDDP_MPC instances (ocs2_bipedal_robot_ros/src/BipedalRobotDdpMpcNode.cpp:70-71; ddp block of task.info): the same
    handle as BatchedSqpMpc with bpmpc_settings.solver = BPMPC_SOLVER_DDP.  `run` returns the accepted roll-out on its own time points:
    t[b, :stats[b].n_nodes + 1], x likewise, u[b, :stats[b].n_nodes]; stats[b].step_size is the accepted step length."""

    def __init__(self, interface, max_batch, max_nodes, **kw):
        kw.pop("solver", None)
        super().__init__(interface, max_batch, max_nodes, solver="ddp", return_gains=True, **kw)
