// Controller tick kernels (kernels/tick.h): observation + policy evaluation in one launch, the joint commands behind k_wbc; the observation of
// a controller restart.
#include <hip/hip_runtime.h>

#include "kernel_launchers.h"
#include "kernels/tick.h"

namespace bpmpc {

template <int NJ>
__global__ __launch_bounds__(kWave) void k_tick_observe_policy(const DeviceModel* model, TickArgs a) {
  __shared__ TickLds<NJ> w;
  tick_observe_policy<NJ>(*model, w, a);
}

template <int NJ>
__global__ __launch_bounds__(256) void k_tick_commands(TickCommandArgs a) {
  tick_commands<NJ>(a);
}

template <int NJ>
__global__ __launch_bounds__(kWave) void k_restart_observe(const DeviceModel* model, RestartArgs a) {
  __shared__ TickLds<NJ> w;
  restart_observe<NJ>(*model, w, a);
}

namespace kl {

void tick_observe_policy(int nj, int batch, hipStream_t st, const DeviceModel* model, const TickArgs& a) {
  if (nj == 10) {
    const int grid = (batch + LinFastCfg<10>::NPW - 1) / LinFastCfg<10>::NPW;
    hipLaunchKernelGGL(k_tick_observe_policy<10>, dim3(grid), dim3(kWave), 0, st, model, a);
  } else {
    const int grid = (batch + LinFastCfg<12>::NPW - 1) / LinFastCfg<12>::NPW;
    hipLaunchKernelGGL(k_tick_observe_policy<12>, dim3(grid), dim3(kWave), 0, st, model, a);
  }
}

void tick_commands(int nj, hipStream_t st, const TickCommandArgs& a) {
  const int grid = (a.batch * nj + 255) / 256;
  if (nj == 10) hipLaunchKernelGGL(k_tick_commands<10>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_tick_commands<12>, dim3(grid), dim3(256), 0, st, a);
}

void restart_observe(int nj, int batch, hipStream_t st, const DeviceModel* model, const RestartArgs& a) {
  if (nj == 10) {
    const int grid = (batch + LinFastCfg<10>::NPW - 1) / LinFastCfg<10>::NPW;
    hipLaunchKernelGGL(k_restart_observe<10>, dim3(grid), dim3(kWave), 0, st, model, a);
  } else {
    const int grid = (batch + LinFastCfg<12>::NPW - 1) / LinFastCfg<12>::NPW;
    hipLaunchKernelGGL(k_restart_observe<12>, dim3(grid), dim3(kWave), 0, st, model, a);
  }
}

}  // namespace kl
}  // namespace bpmpc
