// k_plant_body_step: the plant's control step with a body row per robot, the joint model and stick-slip contacts (kernels/plant.h BODY;
// include/bpmpc.h "Plant", bodies), what a handle launches once its body rows are in use.  A translation unit of its own for the reason
// plant_stick.hip and plant_joint.hip are: k_plant_step, k_plant_stick_step and k_plant_joint_step are compiled as they were before the plant had
// body rows.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "kernel_launchers.h"
#include "plant.h"

namespace bpmpc {

template <int NJ>
__global__ __launch_bounds__(kWave) void k_plant_body_step(const DeviceModel* model, PlantArgs a, PlantStickArgs sa, PlantJointArgs ja, PlantBodyArgs ba) {
  __shared__ PlantBodyLds<NJ> w;
  const int b = blockIdx.x;
  if (b >= a.batch) return;
  plant_robot<NJ, true, true, true>(*model, w, a, sa, b, threadIdx.x, ja, ba);
}

void launch_plant_body_step(int nj, hipStream_t stream, const DeviceModel* model, const PlantArgs& a, const PlantStickArgs& sa, const PlantJointArgs& ja,
                            const PlantBodyArgs& ba) {
  KL_NJ(nj, hipLaunchKernelGGL(k_plant_body_step<NJ>, dim3(a.batch), dim3(kWave), 0, stream, model, a, sa, ja, ba));
  HIP_CHECK(hipGetLastError());
}

}  // namespace bpmpc
