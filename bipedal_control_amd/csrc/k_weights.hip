// Per-problem cost weights and cone parameters (bpmpc_solver_set_weights, bpmpc_solver_set_cone_params): the twins of the three kernel families
// that read Q / R or the friction cone - lineariser, value-only trial (wide rounds and back-tracking tail), change of variables in fused mode - under
// names of their own in a translation unit of their own, so the kernels of k_node.hip and k_project.hip keep their bits.  ONE family with two
// operands: the launch plan (bpmpc_solver::plan_weights) selects it for every problem of the batch once a row of EITHER table has been set, and the
// table that never was holds the model's row in every row.  Bodies: node_kernels.h, project_kernels.h.  W: the weight table
// [batch][kWeightRowStride], row b = Q then R of problem b.  Cone: the cone table [batch][kConeRowStride], row b = the six cone scalars of problem b.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <stdexcept>

#include "kernel_launchers.h"
#include "launch.h"
#include "node_kernels.h"
#include "project_kernels.h"
#include "weight_structure.h"

namespace bpmpc {

// The lineariser with the 16 node slots of a workgroup inside ONE problem, whose row is the Q / R tail of the workgroup's model block:
// ceil(nodes / 16) workgroups per problem in both mappings, the compacted one (Launch::lin_ev_n >= 0: `nodes` = the intermediate nodes; the
// event nodes behind them on workgroups of their own as in k_linearize_fast - they read no weight) and the per-grid one (`nodes` = klen).
// The slots beyond a problem's last node idle: 9 of 112 at 103 intermediate nodes.
template <int NJ>
__host__ __device__ constexpr int lin_slots() { return lin_waves<NJ>() * LinFastCfg<NJ, true>::NPW; }
__host__ __device__ inline int lin_w_workgroups_per_problem(int nodes, int per_wg) { return (nodes + per_wg - 1) / per_wg; }

template <int NJ, bool MAT, bool CHAIN>
__global__ __launch_bounds__(lin_waves<NJ>() * kWave) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_linearize_fast_w(Launch L, const double* W, const double* Cone) {
  using C = LinFastCfg<NJ, true, CHAIN>;
  constexpr int LPN = C::LPN, NPW = C::NPW, kLinWaves = lin_waves<NJ>(), per_wg = kLinWaves * NPW;
  using NL = typename LinKernelLds<NJ, CHAIN>::NL;
  __shared__ NL lds[per_wg];
  __shared__ LinFastShared<NJ> shared;
#ifdef BPMPC_LIN_TIMELINE
  const long long tl0 = wall_clock64();
#else
  const long long tl0 = 0;
#endif
  const int sub = threadIdx.x / LPN, g = threadIdx.x % LPN;
  bool valid, event_wg = false;
  int b, k;
  if (L.lin_ev_n >= 0) {
    const int wpp = lin_w_workgroups_per_problem(L.lin_inter, per_wg), wg_comp = L.batch * wpp;
    if ((int)blockIdx.x < wg_comp) {
      b = blockIdx.x / wpp;
      const int jw = (blockIdx.x % wpp) * per_wg + sub;
      valid = jw < L.lin_inter;
      const int j = valid ? jw : 0;
      int kk = j;                   // the j-th intermediate node: every event i with ev_i - i <= j lies before it
#pragma unroll
      for (int i = 0; i < kLinMaxEvents; ++i) kk += (i < L.lin_ev_n && L.lin_ev[i] - i <= j) ? 1 : 0;
      k = kk;
    } else {
      event_wg = true;              // nothing but event nodes, of any problem: no evaluation, no model block, no weights
      const int e = ((int)blockIdx.x - wg_comp) * per_wg + sub;
      valid = e < L.batch * L.lin_ev_n;
      b = valid ? e / L.lin_ev_n : 0;
      const int i = valid ? e % L.lin_ev_n : 0;
      int kk = L.lin_ev[0];
#pragma unroll
      for (int q = 1; q < kLinMaxEvents; ++q) kk = (i == q) ? L.lin_ev[q] : kk;
      k = kk;
    }
  } else {
    const int wpp = lin_w_workgroups_per_problem(L.klen, per_wg);
    b = blockIdx.x / wpp;           // (the grid is batch * wpp workgroups: b < batch)
    const int j = (blockIdx.x % wpp) * per_wg + sub;
    valid = j < L.klen;
    k = valid ? L.k0 + j : 0;
  }
  const double* row = W + (size_t)b * kWeightRowStride;      // workgroup-uniform (unused by an event workgroup)
  const double* cone = Cone + (size_t)b * kConeRowStride;
  linearize_fast_slot<NJ, MAT, CHAIN, false>(L, shared, lds[sub], valid, b, k, event_wg, g, tl0,
                                             [&] { load_shared_model_rows<kLinWaves * kWave, NJ, true>(*L.model, cone, row, shared, threadIdx.x); });
}

template <int NJ, bool CHAIN>
__global__ __launch_bounds__(kTrialWaves * kWave) __attribute__((amdgpu_waves_per_eu(3, 3)))
void k_trial_fast_w(Launch L, const double* W, const double* Cone) {
  __shared__ TrialConeNodeLds<NJ, CHAIN> lds[kTrialWaves * LinFastCfg<NJ, true, CHAIN>::NPW];
  __shared__ LinFastShared<NJ, false> shared;
  trial_fast_rows_workgroup<NJ, CHAIN>(L, shared, lds, W, Cone);
}

template <int NJ, bool CHAIN>
__global__ __launch_bounds__(kTailThreads) void k_ls_tail_w(Launch L, int first_round, int max_trials, int pending, const double* W, const double* Cone) {
  __shared__ LinFastNodeLds<NJ, false, CHAIN> lds[(kTailThreads / kWave) * LinFastCfg<NJ, true, CHAIN>::NPW];
  __shared__ LinFastShared<NJ, false> shared;
  __shared__ double partial[3 * kTailThreads + 5];
  ls_tail_rows_problem<NJ, CHAIN>(L, first_round, max_trials, pending, shared, lds, partial, W, Cone);
}

// One node per wave: the pointers into the problem's row are wave-uniform (the change of variables reads no cone parameter)
template <int NJ, bool PK, bool WJ>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(PK ? 3 : 2, 4))) void k_project_fast_w(Launch L, const double* W) {
  __shared__ ProjectMfmaWorkspace<NJ, PK> ws;
  constexpr int NX = 12 + NJ;
  project_fast_node<NJ, PK, WJ, false>(ws, L, W, W, W + NX * NX, kWeightRowStride, 0);
}
// ... with a diagonal Q (the pattern rule of bpmpc_solver_set_weights keeps every row's Q diagonal where the model's is): Wqd [batch][kWeightDim],
// the diagonals of the rows (k_weight_diagonals)
template <int NJ, bool PK, bool WJ>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(PK ? 3 : 2, 4))) void k_project_fast_qd_w(Launch L, const double* W, const double* Wqd) {
  __shared__ ProjectMfmaWorkspace<NJ, PK> ws;
  constexpr int NX = 12 + NJ;
  project_fast_node<NJ, PK, WJ, true>(ws, L, W, Wqd, W + NX * NX, kWeightRowStride, kWeightDim);
}

// Wqd[b][c] = Q_b[c][c] for every row of the table (c >= nx: 0); behind every write of rows
__global__ __launch_bounds__(256) void k_weight_diagonals(const double* W, double* Wqd, int rows, int nx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * kWeightDim) return;
  const int b = i / kWeightDim, c = i % kWeightDim;
  Wqd[i] = c < nx ? W[(size_t)b * kWeightRowStride + c * nx + c] : 0.0;
}

namespace kl {

void linearize_fast_w(int nj, bool materialise, hipStream_t st, const Launch& L, const WeightRows& w, hipEvent_t ev_start, hipEvent_t ev_stop) {
  if (L.ilqr) throw std::runtime_error("linearize_fast_w: no ILQR form (the DDP solver keeps the model's weights)");
  KL_NJ(nj, {
    constexpr int per_wg = lin_slots<NJ>();
    const int wgs = L.lin_ev_n >= 0 ? L.batch * lin_w_workgroups_per_problem(L.lin_inter, per_wg) + (L.batch * L.lin_ev_n + per_wg - 1) / per_wg
                                    : L.batch * lin_w_workgroups_per_problem(L.klen, per_wg);
    const dim3 grid(wgs), block(lin_waves<NJ>() * kWave);
    auto launch = [&](auto kernel) {
      if (ev_start && ev_stop) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, ev_start, ev_stop, 0, L, w.rows, w.cone);
      else hipLaunchKernelGGL(kernel, grid, block, 0, st, L, w.rows, w.cone);
    };
    if (L.serial_legs) {
      if (materialise) launch(k_linearize_fast_w<NJ, true, true>);
      else launch(k_linearize_fast_w<NJ, false, true>);
    } else {
      if (materialise) launch(k_linearize_fast_w<NJ, true, false>);
      else launch(k_linearize_fast_w<NJ, false, false>);
    }
  });
}
void trial_fast_w(int nj, int nodes, hipStream_t st, const Launch& L, const WeightRows& w) {
  const int grid = trial_fast_workgroups(nj, nodes);
  KL_NJ(nj, {
    if (L.serial_legs) hipLaunchKernelGGL((k_trial_fast_w<NJ, true>), dim3(grid), dim3(kTrialWaves * kWave), 0, st, L, w.rows, w.cone);
    else hipLaunchKernelGGL((k_trial_fast_w<NJ, false>), dim3(grid), dim3(kTrialWaves * kWave), 0, st, L, w.rows, w.cone);
  });
}
void ls_tail_w(int nj, int batch, hipStream_t st, const Launch& L, int first_round, int max_trials, bool pending, const WeightRows& w) {
  KL_NJ(nj, {
    if (L.serial_legs) hipLaunchKernelGGL((k_ls_tail_w<NJ, true>), dim3(batch), dim3(kTailThreads), 0, st, L, first_round, max_trials, pending ? 1 : 0, w.rows, w.cone);
    else hipLaunchKernelGGL((k_ls_tail_w<NJ, false>), dim3(batch), dim3(kTailThreads), 0, st, L, first_round, max_trials, pending ? 1 : 0, w.rows, w.cone);
  });
}
void project_fast_w(int nj, bool packed, bool joint_rows, int nodes, hipStream_t st, const Launch& L, const WeightRows& w) {
  KL_NJ(nj, {
    if (L.weights_q_diagonal) {
      auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(nodes), dim3(kWave), 0, st, L, w.rows, w.q_diag); };
      if (packed && !joint_rows) launch(k_project_fast_qd_w<NJ, true, false>);
      else if (packed) launch(k_project_fast_qd_w<NJ, true, true>);
      else launch(k_project_fast_qd_w<NJ, false, true>);
    } else {
      auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(nodes), dim3(kWave), 0, st, L, w.rows); };
      if (packed && !joint_rows) launch(k_project_fast_w<NJ, true, false>);
      else if (packed) launch(k_project_fast_w<NJ, true, true>);
      else launch(k_project_fast_w<NJ, false, true>);
    }
  });
}
void weight_diagonals(hipStream_t st, const double* rows, double* q_diag, int n_rows, int nx) {
  hipLaunchKernelGGL(k_weight_diagonals, dim3((n_rows * kWeightDim + 255) / 256), dim3(256), 0, st, rows, q_diag, n_rows, nx);
}

}  // namespace kl
}  // namespace bpmpc
