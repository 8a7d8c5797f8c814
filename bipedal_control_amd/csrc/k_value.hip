// The value function of the SQP solve (bpmpc_solver_enable_value_function): closed-loop terms per node, the backward sweep per problem and the
// query, in a translation unit of their own - the kernels of k_node.hip, k_project.hip and k_riccati*.hip keep their bits.  A handle that never
// enables the feature launches none of them.  Bodies: kernels/value_function.h; arguments: value_kernels.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <stdexcept>

#include "kernel_launchers.h"
#include "value_kernels.h"
#include "kernels/value_function.h"

namespace bpmpc {

// One node per wave, as k_project_fast is launched: batch x klen workgroups of 64 lanes.
// nx = 22: 152 VGPRs, nx = 24: 168; 13184 B of LDS; three waves per SIMD (by registers; LDS would hold twelve per CU).  No scratch.
template <int NJ>
__global__ __launch_bounds__(kWave) void k_value_terms(ValueArgs a) {
  __shared__ ValueTermsLds<NJ> w;
  value_terms_node<NJ>(w, a, blockIdx.x / a.klen, blockIdx.x % a.klen);
}

// One workgroup of four waves per problem, one wave per SIMD.
// nx = 22 and 24: 180 VGPRs (the stage in hand and the next one in flight), 23488 B of LDS; two waves per SIMD, i.e. two problems per CU at a
// time (by registers; LDS would hold six).  No scratch.
template <int NJ>
__global__ __launch_bounds__(4 * kWave) void k_value_sweep(ValueArgs a) {
  __shared__ ValueSweepLds<NJ> w;
  value_sweep_problem<NJ>(w, a, blockIdx.x);
}

// One query per wave.  nx = 22: 70 VGPRs, nx = 24: 62; 512 B of LDS; seven waves per SIMD.  No scratch.
template <int NJ>
__global__ __launch_bounds__(kWave) void k_value_query(ValueQueryArgs a) {
  __shared__ double lds[64];
  value_query_wave<NJ>(lds, a, blockIdx.x);
}

namespace kl {

namespace {
template <typename Kernel, typename Args>
void launch_value_kernel(Kernel kernel, dim3 grid, dim3 block, hipStream_t st, const Args& a, hipEvent_t ev_start, hipEvent_t ev_stop) {
  if (ev_start && ev_stop) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, ev_start, ev_stop, 0, a);
  else hipLaunchKernelGGL(kernel, grid, block, 0, st, a);
}
}  // namespace

void value_terms(int nj, hipStream_t st, const ValueArgs& a, hipEvent_t ev_start, hipEvent_t ev_stop) {
  KL_NJ(nj, launch_value_kernel(k_value_terms<NJ>, dim3(a.batch * a.klen), dim3(kWave), st, a, ev_start, ev_stop));
}
void value_sweep(int nj, hipStream_t st, const ValueArgs& a, hipEvent_t ev_start, hipEvent_t ev_stop) {
  KL_NJ(nj, launch_value_kernel(k_value_sweep<NJ>, dim3(a.batch), dim3(4 * kWave), st, a, ev_start, ev_stop));
}
void value_query(int nj, hipStream_t st, const ValueQueryArgs& a) {
  KL_NJ(nj, hipLaunchKernelGGL(k_value_query<NJ>, dim3(a.batch), dim3(kWave), 0, st, a));
}

}  // namespace kl
}  // namespace bpmpc
