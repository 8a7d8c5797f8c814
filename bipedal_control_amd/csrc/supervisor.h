// The handle of the per-robot supervisor (include/bpmpc.h: bpmpc_supervisor, supervisor.hip).  The per-robot rules are kernels/supervisor.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bpmpc.h"
#include "device_handle.h"
#include "robot_model.h"
#include "kernels/supervisor.h"

struct bpmpc_supervisor {
  bpmpc::RobotModel rm;
  bpmpc::DeviceModel dm;
  bpmpc::DeviceModel* d_model = nullptr;
  int device = 0, max_batch = 0, nj = 0, nv = 0;
  double defaults[bpmpc::kSupParamStride] = {};      // the keys supervisor.<name> of task.info over the defaults: every row after create / reset_params
  bpmpc::DeviceBuffers mem;             // every d_* below
  bpmpc::StreamHandshake hs;            // the handle's stream; nothing is launched on a foreign stream: foreign streams wait for ev_done instead
  hipEvent_t ev_in = nullptr, ev_done = nullptr;      // update_controlled / step_supervised: a foreign stream's work, the supervisor's
  bpmpc::ParamTable params;             // the robots' parameter rows; the start row is `defaults`
  double* d_joint[5] = {};              // q_init, kp_init, kd_init, lower, upper: [max_batch][nj]
  double* d_joint_defaults = nullptr;   // [5][nj]
  double* d_joint_rows = nullptr;       // [max_batch][nj] device copy of host rows
  int* d_mask = nullptr;                // [max_batch] device copy of a host mask
  int *d_state = nullptr, *d_cause = nullptr, *d_unsafe = nullptr, *d_ready = nullptr, *d_latch = nullptr;      // [max_batch]
  int* d_counts = nullptr;              // [kSupCounts]
  double *d_elapsed = nullptr, *d_settled = nullptr, *d_qlatch = nullptr;      // [max_batch], [max_batch], [max_batch][nj]
  double* d_cmd[5] = {};                // pos_des, vel_des, tau_ff, kp, kd: [max_batch][nj]
  // device copies of host inputs
  double *d_rbd = nullptr, *d_run[5] = {};
};

static_assert(bpmpc::kSupParamStride == BPMPC_SUP_PARAM_STRIDE, "the parameter row follows include/bpmpc.h");
static_assert(bpmpc::kSupInit == BPMPC_SUP_INIT && bpmpc::kSupRun == BPMPC_SUP_RUN && bpmpc::kSupStopped == BPMPC_SUP_STOPPED, "the states follow include/bpmpc.h");
