// The handle of the batched whole-body controller (include/bpmpc.h: bpmpc_wbc, wbc.hip) and the launches on another handle's stream that the
// controller tick (controller.cpp) enqueues.  The QP itself is kernels/wbc.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/bpmpc.h"
#include "device_handle.h"
#include "robot_model.h"
#include "kernels/wbc.h"

struct bpmpc_wbc {
  bpmpc::RobotModel rm;
  bpmpc::DeviceModel dm;
  bpmpc::DeviceModel* d_model = nullptr;
  bpmpc::WbcSettings defaults{};        // what loadTasksSetting reads from task.info: every parameter row after create / bpmpc_wbc_reset_params
  int device = 0, max_batch = 0, nv = 0, n = 0;
  bpmpc::DeviceBuffers mem;             // every d_* below
  bpmpc::StreamHandshake hs;            // the handle's stream; foreign launches: k_wbc and k_wbc_restart of a controller tick / restart on the solver's stream
  double *d_x = nullptr, *d_u = nullptr, *d_rbd = nullptr, *d_sol = nullptr, *d_debug = nullptr;
  int *d_mode = nullptr, *d_status = nullptr;
  int* d_mask = nullptr;                // [max_batch] device copy of a host mask (restart, set_params)
  bpmpc::ParamTable params;             // the robots' parameter rows (kernels/wbc.h WbcSettings), read by k_wbc; the start row is `defaults`
};

static_assert(bpmpc::kWbcParamStride == BPMPC_WBC_PARAM_STRIDE && offsetof(bpmpc::WbcSettings, base_kd) == 8 * BPMPC_WBC_PARAM_BASE_KD &&
                  offsetof(bpmpc::WbcSettings, swing_kp) == 8 * BPMPC_WBC_PARAM_SWING_KP && offsetof(bpmpc::WbcSettings, w_swing) == 8 * BPMPC_WBC_PARAM_WEIGHT_SWING_LEG &&
                  offsetof(bpmpc::WbcSettings, friction) == 8 * BPMPC_WBC_PARAM_FRICTION &&
                  offsetof(bpmpc::WbcSettings, contact_tolerance) == 8 * BPMPC_WBC_PARAM_CONTACT_TOLERANCE &&
                  offsetof(bpmpc::WbcSettings, torque_limits) == 8 * BPMPC_WBC_PARAM_TORQUE_LIMITS &&
                  offsetof(bpmpc::WbcSettings, reserved) == 8 * BPMPC_WBC_PARAM_RESERVED,
              "WbcSettings follows the row layout of include/bpmpc.h");

namespace bpmpc {
// k_wbc on device inputs, enqueued on `stream`; later work on the WBC handle's own stream waits for it.
void wbc_launch_on(bpmpc_wbc* w, int batch, const double* state_des, const double* input_des, const double* rbd_meas, const int* mode, hipStream_t stream);
// bpmpc_wbc_restart on a device mask, enqueued on `stream` with the same cross-stream rule
void wbc_restart_on(bpmpc_wbc* w, int batch, const int* mask, hipStream_t stream);
}  // namespace bpmpc
