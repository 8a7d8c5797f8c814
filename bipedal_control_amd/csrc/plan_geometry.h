// The handle of the plan geometry (include/bpmpc.h: bpmpc_plan, plan_geometry.hip).  The rows, footholds and summary themselves are
// kernels/plan_geometry.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bpmpc.h"
#include "device_handle.h"
#include "robot_model.h"

struct bpmpc_plan {
  bpmpc::RobotModel rm;
  bpmpc::DeviceModel dm;
  bpmpc::DeviceModel* d_model = nullptr;
  int device = 0, max_batch = 0, nj = 0, nx = 0, N = 0;
  int launches = 0;                     // bpmpc_plan_configure: 0 the handle chooses, 1 k_plan_fused, 2 k_plan_nodes + k_plan_reduce
  bpmpc::DeviceBuffers mem;             // every d_* below
  bpmpc::StreamHandshake hs;            // the handle's stream; foreign launches: an update on a solver's or a policy buffer's stream
  double *d_optimized = nullptr, *d_desired = nullptr;      // [max_batch][N + 1][24]
  double *d_footholds = nullptr, *d_summary = nullptr;      // [max_batch][16][6], [max_batch][16]
  int* d_count = nullptr;                                   // [max_batch]
  // device copies of the host inputs of bpmpc_plan_update, allocated by the first call that brings host arrays
  bool staging = false;
  double *d_t = nullptr, *d_x = nullptr, *d_u = nullptr, *d_xref = nullptr;
  int *d_mode = nullptr, *d_kind = nullptr, *d_nodes = nullptr;
};
