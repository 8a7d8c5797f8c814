// Host-side entry points of the kernel translation units (k_node.hip, k_project.hip, k_riccati.hip, k_riccati_wave.hip, k_ddp.hip, k_tick.hip): the solver
// (solver.hip, host code) launches every kernel through these, so the kernel families compile in parallel and a change to one of them
// rebuilds one translation unit.  `nj` selects the instantiation (10: nx = nu = 22, 12: nx = nu = 24); every function only enqueues.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <stdexcept>

namespace bpmpc {

// `body` with the instantiation of `nj` as the constant NJ (a launcher's dispatch; nj is 10 or 12, checked when a handle is created)
#define KL_NJ(nj, ...)                                                          \
  do {                                                                          \
    if ((nj) == 10) { constexpr int NJ = 10; __VA_ARGS__; }                     \
    else if ((nj) == 12) { constexpr int NJ = 12; __VA_ARGS__; }                \
    else throw std::runtime_error("unsupported joint count");                   \
  } while (0)

struct Launch;
struct DeviceModel;
struct RolloutArgs;
struct DdpBuffers;
struct TickArgs;
struct TickCommandArgs;
struct RestartArgs;

// The per-problem rows of a solver handle as the kernels read them: rows [batch][BPMPC_SOLVER_WEIGHT_STRIDE], Q then R per problem
// (bpmpc_solver_set_weights); q_diag [batch][kWeightDim], the diagonals of Q derived from the rows; cone [batch][BPMPC_SOLVER_CONE_STRIDE], the cone
// parameters per problem (bpmpc_solver_set_cone_params).  All three or none: rows == nullptr: the model's weights and cone, the kernels of
// k_node.hip / k_project.hip.
struct WeightRows {
  const double* rows = nullptr;
  const double* q_diag = nullptr;
  const double* cone = nullptr;
};

namespace kl {

// ---- k_node.hip: per-node kernels in the lane-per-coordinate mapping, line search, warm start, policy rollout
void prepare(int nj, int slots, hipStream_t st, const Launch& L);
void linearize_reference(int nj, int slots, hipStream_t st, const Launch& L);
void linearize_fast(int nj, bool materialise, int nodes, hipStream_t st, const Launch& L, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void warm_shift(int nj, int slots, hipStream_t st, const Launch& L, const int* restarted = nullptr);   // restarted[b] != 0: problem b keeps k_prepare's guess
void ls_begin(int nj, int batch, hipStream_t st, const Launch& L);
void trial_reference(int nj, int slots, hipStream_t st, const Launch& L);
int trial_fast_workgroups(int nj, int nodes);
void trial_fast(int nj, int nodes, hipStream_t st, const Launch& L);
void ls_decide(int nj, int batch, hipStream_t st, const Launch& L, bool look_first = false);
void ls_tail(int nj, int batch, hipStream_t st, const Launch& L, int first_round, int max_trials, bool pending);
void constraint_values(int nj, int nodes, hipStream_t st, const Launch& L, double* eqv);
void rollout(int nj, bool serial_legs, int batch, hipStream_t st, const DeviceModel* model, const RolloutArgs& a);
void copy_pairs(int grid, hipStream_t st, const double* a_src, double* a_dst, size_t na, const double* b_src, double* b_dst, size_t nb,
                int* iterations, int* active, int batch);

// ---- k_project.hip: constraint elimination and change of variables
void project_reference(int nj, int slots, hipStream_t st, const Launch& L);
void project_lu_s(int nj, int max_vel_rows, bool packed, int nodes, hipStream_t st, const Launch& L);
void project_fast(int nj, bool packed, bool joint_rows, int nodes, hipStream_t st, const Launch& L);

// ---- k_weights.hip: the kernels that read Q / R or the friction cone, on per-problem rows (same arguments as their namesakes; w.rows and w.cone
// != nullptr).  The lineariser maps ceil(nodes / 16) workgroups onto every problem, so it takes no node count
void linearize_fast_w(int nj, bool materialise, hipStream_t st, const Launch& L, const WeightRows& w, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void trial_fast_w(int nj, int nodes, hipStream_t st, const Launch& L, const WeightRows& w);
void ls_tail_w(int nj, int batch, hipStream_t st, const Launch& L, int first_round, int max_trials, bool pending, const WeightRows& w);
void project_fast_w(int nj, bool packed, bool joint_rows, int nodes, hipStream_t st, const Launch& L, const WeightRows& w);
void weight_diagonals(hipStream_t st, const double* rows, double* q_diag, int n_rows, int nx);      // q_diag[b][c] = Q_b[c][c]

// ---- k_riccati.hip: workgroup-per-problem sweeps
void riccati_reference(int nj, int batch, hipStream_t st, const Launch& L);
void riccati_fast(int nj, bool joint_rows, int batch, hipStream_t st, const Launch& L);       // four waves, two problems per CU
void riccati_fast8(int nj, bool joint_rows, int batch, hipStream_t st, const Launch& L);     // joint_rows: Wt holds them (off: completed from Vt by the loaders)

// ---- k_riccati_wave.hip: wave-per-problem sweeps and their roll-out
void riccati_wave(int nj, bool two_per_simd, bool joint_rows, int batch, hipStream_t st, const Launch& L);
void riccati_rollout(int nj, int batch, hipStream_t st, const Launch& L);

// ---- k_ddp.hip: the DDP slice (one ILQR iteration; backward pass on the reference kernel set, line search over policy roll-outs)
void ddp_policy(int nj, int batch, hipStream_t st, const Launch& L, const DdpBuffers& d);
void ddp_cost(int nj, int batch, bool fast, hipStream_t st, const Launch& L, const DdpBuffers& d);
void ddp_select(int nj, int batch, hipStream_t st, const Launch& L, const DdpBuffers& d, double armijo);
void ddp_nominal(int nj, int batch, hipStream_t st, const Launch& L, const DdpBuffers& d);
void ddp_finish(int nj, int batch, hipStream_t st, const Launch& L, const DdpBuffers& d);
void ddp_keep_times(int batch, int N, hipStream_t st, const DdpBuffers& d, const double* g_time, const int* g_kind, const int* g_nodes, const int* p_grid,
                    double* tp_time, int* tp_kind, int* tp_nodes, int* tp_grid);

// ---- k_tick.hip: the controller tick (observation + policy evaluation in one launch; the joint commands behind k_wbc), the restart's observation
void tick_observe_policy(int nj, int batch, hipStream_t st, const DeviceModel* model, const TickArgs& a);
void tick_commands(int nj, hipStream_t st, const TickCommandArgs& a);
void restart_observe(int nj, int batch, hipStream_t st, const DeviceModel* model, const RestartArgs& a);

}  // namespace kl
}  // namespace bpmpc
