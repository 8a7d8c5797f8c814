// The dual solution of the SQP solve (include/bpmpc.h "Dual solution"): what its three kernels (k_dual.hip; bodies kernels/dual_solution.h) read and
// write, and their launchers.  As the value function's kernels they take an argument struct of their own, so neither Launch nor Buffers changes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace bpmpc {

constexpr int kDualRows = 16;      // slots of the state-input equality rows of a node (kMaxEqRows)

struct DualArgs {
  // the LQ model of the last linearisation in materialised form, slot s = b * N + k: B [s][nx*nu]  R [s][nu*nu]  P [s][nu*nx]  r [s][nu]
  // D [s][16][nu]  nc [s]; the sweep's policy K [s][nu*nx], dx [b][N + 1][nx], du [s][nu]
  const double *B, *R, *P, *r, *D, *K, *dx, *du;
  const int* nc;
  const double* summary;      // [b][4]: entry 3 != 0 - the Riccati sweep of problem b failed
  const int *n_info, *active, *p_grid, *g_nodes;
  // of the value function behind the same backward pass: S [b][N + 1][nx*nx], s [b][N + 1][nx], terms [s][value_terms_stride(nx)]
  const double *S, *s, *terms;
  // the dual buffers: lambda [b][N + 1][nx]; nu_gain [s][16][nx], nu0 [s][16], nu [s][16], residual [s], gain_residual [s], aux [s][2] (the
  // largest |g_u|, the largest |Hux|), rows [s]; summary_out [b][6], status [b]
  double *lambda, *nu_gain, *nu0, *nu, *residual, *gain_residual, *aux, *summary_out;
  int *rows, *status;
  int batch, N, klen;         // N = node stride (max_nodes), klen = the longest grid of the setup
};

// One evaluate_dual call: t [batch], x [batch][nx] -> lambda [batch][nx], nu [batch][16], rows [batch]
struct DualQueryArgs {
  const double *S, *s, *x_lin, *g_time;      // g_time [grid][N + 1]
  const double *nu_gain, *nu0;
  const int *node_rows, *p_grid, *g_nodes;
  const double *t, *x;
  double *lambda, *nu;
  int* rows;
  int batch, N;
};

namespace kl {

// ---- k_dual.hip (every function only enqueues)
void dual_node(int nj, hipStream_t st, const DualArgs& a, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void dual_summary(int nj, hipStream_t st, const DualArgs& a);
void dual_query(int nj, hipStream_t st, const DualQueryArgs& a);

}  // namespace kl
}  // namespace bpmpc
