// Per-problem cone parameters of the MPC (include/bpmpc.h "Per-problem cone parameters"): the row format, the start row of a model and the host
// check of a row.  Host only and free of HIP, so that bpmpc_model_check_cone_params (capi.cpp) needs no device and a plain compiler can build it.
#pragma once
#include <cmath>
#include <string>

#include "../../include/bpmpc.h"
#include "robot_model.h"

namespace bpmpc {

// The start row: what make_device_model puts into the DeviceModel (device_model.cpp) - with the hard cone sqp.inequalityConstraintMu / Delta as the
// barrier and no Hessian shift
inline void cone_start_row(const RobotModel& m, double* row /* BPMPC_SOLVER_CONE_STRIDE */) {
  for (int i = 0; i < BPMPC_SOLVER_CONE_STRIDE; ++i) row[i] = 0.0;
  row[BPMPC_SOLVER_CONE_FRICTION] = m.friction_coefficient;
  row[BPMPC_SOLVER_CONE_REGULARIZATION] = m.cone_regularization;
  row[BPMPC_SOLVER_CONE_GRIPPER_FORCE] = m.cone_gripper_force;
  row[BPMPC_SOLVER_CONE_HESSIAN_SHIFT] = m.hard_friction_cone ? 0.0 : m.cone_hessian_shift;
  row[BPMPC_SOLVER_CONE_BARRIER_MU] = m.hard_friction_cone ? m.sqp_inequality_mu : m.barrier_mu;
  row[BPMPC_SOLVER_CONE_BARRIER_DELTA] = m.hard_friction_cone ? m.sqp_inequality_delta : m.barrier_delta;
}

// Empty: the row is accepted.  Else the entry and the reason, e.g. "entry 0 (friction coefficient) must be positive".
inline std::string check_cone_row(const double* row, bool hard_cone) {
  static const char* const names[BPMPC_SOLVER_CONE_STRIDE] = {"friction coefficient", "regularisation", "gripper force", "Hessian shift",
                                                             "barrier mu", "barrier delta", "reserved", "reserved"};
  auto refuse = [&](int i, const char* why) { return "entry " + std::to_string(i) + " (" + names[i] + ") " + why; };
  for (int i = 0; i < BPMPC_SOLVER_CONE_STRIDE; ++i)
    if (!std::isfinite(row[i])) return refuse(i, "is not finite");
  if (row[BPMPC_SOLVER_CONE_FRICTION] <= 0.0) return refuse(BPMPC_SOLVER_CONE_FRICTION, "must be positive");
  if (row[BPMPC_SOLVER_CONE_REGULARIZATION] <= 0.0)
    return refuse(BPMPC_SOLVER_CONE_REGULARIZATION, "must be positive (sqrt(Fx^2 + Fy^2 + regularisation) is a divisor at zero force)");
  if (row[BPMPC_SOLVER_CONE_GRIPPER_FORCE] < 0.0) return refuse(BPMPC_SOLVER_CONE_GRIPPER_FORCE, "must not be negative");
  if (row[BPMPC_SOLVER_CONE_HESSIAN_SHIFT] < 0.0) return refuse(BPMPC_SOLVER_CONE_HESSIAN_SHIFT, "must not be negative");
  if (hard_cone && row[BPMPC_SOLVER_CONE_HESSIAN_SHIFT] != 0.0)
    return refuse(BPMPC_SOLVER_CONE_HESSIAN_SHIFT, "must be 0 on a model with the hard friction cone (its penalty has no Hessian shift)");
  if (row[BPMPC_SOLVER_CONE_BARRIER_MU] <= 0.0) return refuse(BPMPC_SOLVER_CONE_BARRIER_MU, "must be positive");
  if (row[BPMPC_SOLVER_CONE_BARRIER_DELTA] <= 0.0) return refuse(BPMPC_SOLVER_CONE_BARRIER_DELTA, "must be positive");
  for (int i = BPMPC_SOLVER_CONE_RESERVED; i < BPMPC_SOLVER_CONE_STRIDE; ++i)
    if (row[i] != 0.0) return refuse(i, "must be 0");
  return std::string();
}

}  // namespace bpmpc
