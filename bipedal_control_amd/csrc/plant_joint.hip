// k_plant_joint_step: the plant's control step with the joint model and stick-slip contacts (kernels/plant.h JOINT; include/bpmpc.h "Plant",
// joints), what a handle launches once its joint model is in use.  A translation unit of its own for the reason plant_stick.hip is one: k_plant_step
// and k_plant_stick_step are compiled as they were before the plant had a joint model.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "kernel_launchers.h"
#include "plant.h"

namespace bpmpc {

template <int NJ>
__global__ __launch_bounds__(kWave) void k_plant_joint_step(const DeviceModel* model, PlantArgs a, PlantStickArgs sa, PlantJointArgs ja) {
  __shared__ PlantJointLds<NJ> w;
  const int b = blockIdx.x;
  if (b >= a.batch) return;
  plant_robot<NJ, true, true>(*model, w, a, sa, b, threadIdx.x, ja);
}

void launch_plant_joint_step(int nj, hipStream_t stream, const DeviceModel* model, const PlantArgs& a, const PlantStickArgs& sa, const PlantJointArgs& ja) {
  KL_NJ(nj, hipLaunchKernelGGL(k_plant_joint_step<NJ>, dim3(a.batch), dim3(kWave), 0, stream, model, a, sa, ja));
  HIP_CHECK(hipGetLastError());
}

}  // namespace bpmpc
