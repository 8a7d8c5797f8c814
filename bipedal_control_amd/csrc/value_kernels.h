// The value function of the SQP solve (include/bpmpc.h "Value function"): what its three kernels (k_value.hip; bodies kernels/value_function.h) read
// and write, and their launchers.  The kernels take this argument struct of their own - pointers copied from the handle's Buffers, the value buffers
// and the strides - so that neither Launch nor Buffers, which every other kernel receives by value, changes its layout.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace bpmpc {

struct ValueArgs {
  // the LQ model of the last linearisation in materialised form, slot s = b * N + k: A, Q [s][nx*nx]  B [s][nx*nu]  R [s][nu*nu]  P [s][nu*nx]
  // b, q [s][nx]  r [s][nu]  c [s]; the sweep's policy K [s][nu*nx], dx [b][N + 1][nx], du [s][nu]; the iterate x [b][N + 1][nx]
  const double *A, *B, *b, *Q, *R, *P, *q, *r, *c, *K, *dx, *du, *x;
  const double* summary;      // [b][4]: entry 3 != 0 - the Riccati sweep of problem b failed
  const int *n_info, *active, *p_grid, *g_nodes;
  // the value buffers: S [b][N + 1][nx*nx], s [b][N + 1][nx], v [b][N + 1], x_lin [b][N + 1][nx], status [b]; terms [s][value_terms_stride(nx)]
  double *S, *s, *v, *x_lin, *terms;
  int* status;
  int batch, N, klen;         // N = node stride (max_nodes), klen = the longest grid of the setup
};

// One node of the scratch table: Acl [nx*nx], Qcl [nx*nx], bcl [nx], qcl [nx], ccl and a padding word (16-byte aligned nodes)
__host__ __device__ constexpr int value_terms_stride(int nx) { return 2 * nx * nx + 2 * nx + 2; }

// One evaluate_value call: t [batch], x [batch][nx] -> f [batch], dfdx [batch][nx], dfdxx [batch][nx*nx] (nullable)
struct ValueQueryArgs {
  const double *S, *s, *v, *x_lin, *g_time;      // g_time [grid][N + 1]
  const int *p_grid, *g_nodes;
  const double *t, *x;
  double *f, *dfdx, *dfdxx;
  int batch, N;
};

namespace kl {

// ---- k_value.hip (every function only enqueues)
void value_terms(int nj, hipStream_t st, const ValueArgs& a, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void value_sweep(int nj, hipStream_t st, const ValueArgs& a, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void value_query(int nj, hipStream_t st, const ValueQueryArgs& a);

}  // namespace kl
}  // namespace bpmpc
