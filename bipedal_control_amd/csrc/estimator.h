// The handle of the batched state estimator (include/bpmpc.h: bpmpc_estimator, estimator.hip) and what the controller tick (controller.cpp)
// needs of it on another handle's stream.  The filter itself is kernels/estimator.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bpmpc.h"
#include "device_handle.h"
#include "robot_model.h"
#include "kernels/estimator.h"

struct bpmpc_estimator {
  bpmpc::RobotModel rm;
  bpmpc::DeviceModel dm;
  bpmpc::DeviceModel* d_model = nullptr;
  bpmpc::EstSettings defaults{};        // LinearKalmanFilter.h:45-51 overridden by the kalmanFilter block of task.info: every row after create / reset_params
  int kind = 0, device = 0, max_batch = 0, nj = 0, nv = 0;
  int last_batch = 0;                   // batch of the last update: the rows of d_rbd that hold an estimate (0 before the first update)
  bpmpc::DeviceBuffers mem;             // every d_* below
  bpmpc::StreamHandshake hs;            // the handle's stream; foreign launches: a controller tick on the solver's stream that reads d_rbd
  double *d_rbd = nullptr, *d_xhat = nullptr, *d_cov = nullptr;      // [max_batch][2 nv], [max_batch][18], [max_batch][18][18]
  int* d_xy_reset = nullptr;                                        // [max_batch]
  bpmpc::ParamTable params;             // the robots' parameter rows (kernels/estimator.h EstSettings); the start row is `defaults`
  int* d_mask = nullptr;                // [max_batch] device copy of a host mask
  double *d_xhat_in = nullptr, *d_cov_in = nullptr;                 // device copies of host states (set_state)
  // device copies of host sensor arrays
  double *d_jp = nullptr, *d_jv = nullptr, *d_quat = nullptr, *d_w = nullptr, *d_a = nullptr, *d_fh = nullptr;
  double *d_opos = nullptr, *d_oquat = nullptr, *d_olin = nullptr, *d_oang = nullptr;
  int *d_contact = nullptr, *d_mode = nullptr;
};

static_assert(bpmpc::kEstParamStride == BPMPC_EST_PARAM_STRIDE, "EstSettings follows the row layout of include/bpmpc.h");

namespace bpmpc {
// The settings of KalmanFilterEstimate (LinearKalmanFilter.h:45-51) overridden by the keys kalmanFilter.<name> of task.info (NULL: the defaults); host
// only (capi.cpp), also behind bpmpc_estimator_load_params
EstSettings estimator_load_settings(const char* task_info_path);
// A host row before it is accepted: every entry finite and not negative, the three sensor noises (R's diagonal) strictly positive; throws
// std::invalid_argument naming the entry
void estimator_check_param_row(const char* who, const double* row, int r);
// A controller tick on `stream` is about to read the estimator's rbd: the stream waits for an update that was only enqueued ...
void estimator_before_foreign_read(bpmpc_estimator* e, int batch, hipStream_t stream);
// ... and the estimator's own stream waits for that tick before the next update overwrites rbd
void estimator_after_foreign_read(bpmpc_estimator* e, hipStream_t stream);
}  // namespace bpmpc
