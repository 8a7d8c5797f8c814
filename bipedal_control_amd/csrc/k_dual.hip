// The dual solution of the SQP solve (bpmpc_solver_enable_dual_solution): costates, minimum-norm multipliers and their certificates per node, the
// maxima per problem and the query, in a translation unit of their own - every other kernel keeps its bits.  A handle that never enables the
// feature launches none of them.  Bodies: kernels/dual_solution.h; arguments: dual_kernels.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <stdexcept>

#include "kernel_launchers.h"
#include "dual_kernels.h"
#include "kernels/dual_solution.h"

namespace bpmpc {

// One node per wave, as k_value_terms is launched: batch x klen workgroups of 64 lanes.  Static LDS only, no scratch.
template <int NJ>
__global__ __launch_bounds__(kWave) void k_dual_node(DualArgs a) {
  __shared__ DualNodeLds<NJ> w;
  dual_node<NJ>(w, a, blockIdx.x / a.klen, blockIdx.x % a.klen);
}

// One wave per problem, behind k_dual_node on the same stream (a launch of its own: the maxima need every node of the problem).
template <int NJ>
__global__ __launch_bounds__(kWave) void k_dual_summary(DualArgs a) {
  dual_summary_problem<NJ>(a, blockIdx.x);
}

// One query per wave.
template <int NJ>
__global__ __launch_bounds__(kWave) void k_dual_query(DualQueryArgs a) {
  __shared__ double lds[32];
  dual_query_wave<NJ>(lds, a, blockIdx.x);
}

namespace kl {

void dual_node(int nj, hipStream_t st, const DualArgs& a, hipEvent_t ev_start, hipEvent_t ev_stop) {
  if (ev_start && ev_stop) { KL_NJ(nj, hipExtLaunchKernelGGL(k_dual_node<NJ>, dim3(a.batch * a.klen), dim3(kWave), 0, st, ev_start, ev_stop, 0, a)); }
  else { KL_NJ(nj, hipLaunchKernelGGL(k_dual_node<NJ>, dim3(a.batch * a.klen), dim3(kWave), 0, st, a)); }
}
void dual_summary(int nj, hipStream_t st, const DualArgs& a) {
  KL_NJ(nj, hipLaunchKernelGGL(k_dual_summary<NJ>, dim3(a.batch), dim3(kWave), 0, st, a));
}
void dual_query(int nj, hipStream_t st, const DualQueryArgs& a) {
  KL_NJ(nj, hipLaunchKernelGGL(k_dual_query<NJ>, dim3(a.batch), dim3(kWave), 0, st, a));
}

}  // namespace kl
}  // namespace bpmpc
