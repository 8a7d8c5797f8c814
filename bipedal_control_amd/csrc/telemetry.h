// The handle of the tracking telemetry (include/bpmpc.h: bpmpc_telemetry, telemetry.hip) and what the controller tick (controller.cpp) needs of
// it on its own stream.  The record itself is kernels/telemetry.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bpmpc.h"
#include "device_handle.h"
#include "robot_model.h"

struct bpmpc_telemetry {
  bpmpc::RobotModel rm;
  bpmpc::DeviceModel dm;
  bpmpc::DeviceModel* d_model = nullptr;
  int device = 0, max_batch = 0, nj = 0, nx = 0, nv = 0, stride = 0, ring_len = 0;
  int every = 1, freeze_on_unsafe = 1;  // bpmpc_telemetry_configure
  bpmpc::DeviceBuffers mem;             // every d_* below
  bpmpc::StreamHandshake hs;            // the handle's stream; foreign launches: k_telemetry behind a controller tick on the controller's stream
  double *d_sample = nullptr, *d_stats = nullptr, *d_ring = nullptr;   // [max_batch][stride], [max_batch][40], [max_batch][ring_len][stride]
  int *d_frozen = nullptr, *d_count = nullptr;                         // [max_batch], [max_batch][2]: n, samples recorded into the ring
  // device copies of host inputs
  double *d_t = nullptr, *d_xopt = nullptr, *d_rbd = nullptr;
  int *d_safe = nullptr, *d_mode = nullptr, *d_mask = nullptr;
};

namespace bpmpc {
// k_telemetry for `batch` robots on `stream` (the controller's, behind k_tick_commands) from device inputs; t, safe and mode nullable.  The
// stream waits for work that was only enqueued on the handle's own stream, and the handle's stream for this launch.  The caller has checked
// batch against max_batch (controller.cpp check_tick).
void telemetry_launch_on(bpmpc_telemetry* tm, int batch, const double* t, const double* x_opt, const double* rbd, const int* safe, const int* mode,
                         hipStream_t stream);
}  // namespace bpmpc
