// k_plant_stick_step: the plant's control step with stick-slip contacts (kernels/plant.h STICK; include/bpmpc.h "Plant"), what a handle launches once
// stiction has been set on it.  A translation unit of its own, so that k_plant_step in plant.hip is compiled as it was before the plant had
// stiction: with a second caller of the rigid-body pass beside it the compiler inlines and contracts it differently, and its bits change.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "kernel_launchers.h"
#include "plant.h"

namespace bpmpc {

template <int NJ>
__global__ __launch_bounds__(kWave) void k_plant_stick_step(const DeviceModel* model, PlantArgs a, PlantStickArgs sa) {
  __shared__ PlantStickLds<NJ> w;
  const int b = blockIdx.x;
  if (b >= a.batch) return;
  plant_robot<NJ, true>(*model, w, a, sa, b, threadIdx.x);
}

void launch_plant_stick_step(int nj, hipStream_t stream, const DeviceModel* model, const PlantArgs& a, const PlantStickArgs& sa) {
  KL_NJ(nj, hipLaunchKernelGGL(k_plant_stick_step<NJ>, dim3(a.batch), dim3(kWave), 0, stream, model, a, sa));
  HIP_CHECK(hipGetLastError());
}

}  // namespace bpmpc
