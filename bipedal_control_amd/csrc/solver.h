// The solver handle (include/bpmpc.h: bpmpc_solver) and what the units around solver.hip share of it: the batched small transfers
// (transfer.hip), the helpers of the device-side setups (setup_commands in solver.hip, setup_gaits in gait_batch.hip), and the refusals and the
// restart that the controller (controller.cpp) runs on the handle it reads.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bpmpc.h"
#include "device_handle.h"
#include "kernel_launchers.h"
#include "kernel_timers.h"
#include "launch.h"
#include "sweep_plan.h"
#include "value_kernels.h"
#include "dual_kernels.h"
#include "kernels/reference_device.h"

using namespace bpmpc;

struct HostStaging {   // host-side images of the tables bpmpc_solver_setup uploads
  std::vector<int> kind, mode, nodes, pgrid, tgt_n;
  std::vector<double> gdt, gstart, zref, zdref, tgt_t, tgt_x;
};

// Page-locked host memory for the small transfers of the MPC loop (setup_commands, fetch): a copy from / to pageable memory is
// staged by the runtime and blocks the calling thread for ~10 us each; from / to pinned memory it is only enqueued.  Slices stay
// valid until the next reset(), which the callers issue when everything in flight has been waited for.
struct PinnedArena {
  char* base = nullptr;
  size_t cap = 0, used = 0, demand = 0;
  // start of a new cycle: nothing of the previous one is in flight any more.  Grows to what the previous cycle asked for.
  void reset() {
    if (demand > cap) {
      if (base) (void)hipHostFree(base);
      base = nullptr; cap = 0;
      const size_t want = std::max<size_t>(2 * demand, size_t(1) << 20);
      if (hipHostMalloc(reinterpret_cast<void**>(&base), want) == hipSuccess) cap = want; else base = nullptr;
    }
    used = 0; demand = 0;
  }
  void* take(size_t bytes) {                              // nullptr: no room in this cycle, the caller uses the pageable path
    const size_t at = (used + 63) & ~size_t(63);
    demand = ((demand + 63) & ~size_t(63)) + bytes;
    if (!base || at + bytes > cap) return nullptr;
    used = at + bytes;
    return base + at;
  }
  void release() { if (base) (void)hipHostFree(base); base = nullptr; cap = used = demand = 0; }
};

struct bpmpc_command_batch;

struct bpmpc_solver {
  HostStaging staging;
  PinnedArena pin_up, pin_down;
  char* xfer = nullptr;                                     // device staging block of the batched small transfers (upload_batch / Downloads)
  size_t xfer_cap = 0;
  RobotModel rm;
  DeviceModel dm;
  DeviceModel* d_model = nullptr;
  bpmpc_settings settings{};
  int nx = 0, nu = 0;
  int batch = 0, n_grids = 0, n_nodes_max = 0;
  int num_cus = 256;                                        // compute units of the device
  Switches sw;                                              // the environment switches, read when the solver is created (sweep_plan.h)
  // change of variables reading the packed joint rows of the structured elimination: needs an input weight without force / joint-velocity
  // cross terms (checked when the solver is created; BipedalRobotInterface.cpp:239-271 builds it so).  BPMPC_DENSE_PROJECT=1 switches it off.
  bool structured_project = false;
  bool serial_legs() const { return dm.serial_legs && !sw.lin_tables; }      // the per-node kernels run their tree walks by DPP
  // the wave-per-problem sweeps (riccati_wave.h, riccati_wave2.h) and the loaders of the eight-wave sweep (riccati_mfma8.h, PackedStageLoader JR) complete the joint rows of Wt = [At | bt | Bt] from Vt ([I | b | 0] + dt Vt): the change of variables then
  // neither computes nor writes them (3.8 KB per node less each way at the batch sizes where both kernels stream).  The `joint_rows` argument of
  // the launchers: false where every fast sweep does so
  bool joint_rows() const { return sw.wt_joint_rows || !structured_project || settings.reference_kernels; }
  bool has_solution = false;                               // a solve has completed on the current setup
  bool has_rollout = false;                                // roll_x holds the end states of a rollout
  bool rollout_unchecked = false;                          // ... whose status flags have not been read back yet
  // closed loop through the controller tick (k_tick.hip): tick_x holds the observations of the last bpmpc_controller_tick; loop_from_tick says
  // that the tick, not a rollout, ran last on the handle - bpmpc_solver_setup_commands(x0 = NULL) then starts from tick_x instead of roll_x
  double* tick_x = nullptr;
  bool loop_from_tick = false;
  // a controller whose ticks run on a policy buffer's stream (policy.h): that stream's handshake.  What this handle's stream does to tick_x - the
  // read of setup_commands(x0 = NULL), the rows a restart writes - waits for the last such tick, and the next tick waits for it.  NULL: no buffer
  StreamHandshake* tick_hs = nullptr;
  // per-problem restarts (bpmpc_solver_restart, MPC_BASE::reset per problem): restart_flag[b] != 0 from the restart to the next accepted setup,
  // which keeps k_prepare's guess for those problems instead of the shifted solution.  restart_pending: flags recorded and not consumed yet;
  // restart_wait: tick, evaluate_policy and rollout are refused until the first run after that setup (a fresh handle before its first run)
  // the attached command batch (bpmpc_solver_attach_commands, command_batch.hip): the device-side setups window its stored targets into p_tgt_*
  // instead of launching k_command_targets; tgt_flag[b] is the window kernel's verdict (0 taken, < 0 no target, > 0 that many points in the window)
  bpmpc_command_batch* commands = nullptr;
  int* tgt_flag = nullptr;                                 // [max_batch]
  int* restart_flag = nullptr;                             // [max_batch]
  int* restart_mask = nullptr;                             // [max_batch] device copy of a host mask
  double* restart_x = nullptr;                             // [max_batch][nx] device copy of host states
  bool restart_pending = false, restart_wait = false;
  std::vector<int> grid_kind;                               // host copy of the node kinds of the current setup [n_grids][N]
  int max_rows = kMaxEqRows;                                // largest number of equality rows over the nodes of the current setup
  int max_vel_rows = 12;                                    // ... of rows that constrain a contact velocity (12 double stance, 8 single support, 4 flight)
  bool cold = true;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t producer_stream = nullptr;                   // linearisation + projection of the pipelined horizon chunks
  hipEvent_t ev_go = nullptr;
  std::vector<hipEvent_t> ev_chunk;
  Buffers buf{};
  std::vector<void*> allocations;
  struct NamedBuffer { void* ptr; size_t count; bool integer; };      // doubles unless integer
  std::map<std::string, NamedBuffer> named;                // what bpmpc_solver_read hands out
  std::vector<double> node_times;                          // host copy: [n_grids][N+1]
  std::vector<int> grid_nodes, grid_of_problem;
  KernelTimers timers;
  int* h_remaining = nullptr;                              // pinned
  LineSearchSettings ls{};

  template <typename T>
  T* alloc(const char* name, size_t count, bool integer = false) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, count * sizeof(T)));
    HIP_CHECK(hipMemsetAsync(p, 0, count * sizeof(T), stream));
    allocations.push_back(p);
    if (name) named[name] = {p, count, integer};
    return static_cast<T*>(p);
  }

  // Everything a launch reads of the handle, built ONCE per setup (build_plan, the first thing finish_setup does); the stages launch from it.
  // pipelined_backward edits a copy (k0, klen, lin_ev_n).  `buf` stays the owner of the pointers: plan.buf is the copy made at that point.
  // Where the inputs change: buf in preserve_previous only (the swap of the solution buffers); batch, n_grids, n_nodes_max, cold, grid_kind and
  // grid_nodes in the two setup bodies only (setup of solver.hip; accept_reference_grids for setup_commands and setup_gaits) - all of them before
  // finish_setup.  Everything else is fixed when the solver is created: d_model, dm, rm, sw, ls, and of settings max_nodes, reg_prim, solver and
  // feedback_policy (set_materialize and set_profile write fields no launch reads from here).
  Launch plan{};
  // The part of the plan that changes BETWEEN setups: the per-problem cost weights (solver_weights.hip) and cone parameters (solver_cone.hip).
  // rows == nullptr - a handle that never had a row of either table set, or has had both reset - launches the kernels of k_node.hip /
  // k_project.hip; from the first bpmpc_solver_set_weights or bpmpc_solver_set_cone_params on every kernel that reads Q, R or the cone
  // (lineariser, trial, back-tracking tail, change of variables) is its twin of k_weights.hip, for every problem of the batch.  ONE switch
  // (select_row_kernels): the family takes both tables, and both exist from the first set of either - the one that was never set filled with the
  // model's row (an allocated table, not one row at stride 0: the kernels keep compile-time strides, and the change of variables its body).
  // build_plan leaves it alone: the rows enter neither the grids nor the references, so no setup is needed after a set.
  WeightRows plan_weights{};
  bool weights_set = false, cone_set = false;              // a row set since the table's own reset
  void select_row_kernels() { plan_weights = (weights_set || cone_set) ? WeightRows{weights.d_params, weight_q_diag, cone.d_params} : WeightRows{}; }
  DeviceBuffers weight_mem;                                // the memory of both tables (allocated by the first set of either, freed with the handle)
  ParamTable weights;                                      // rows [max_batch][BPMPC_SOLVER_WEIGHT_STRIDE], start row = the model's Q, R
  double* weight_q_diag = nullptr;                         // [max_batch][kWeightDim]: the diagonals of Q, derived behind every write (k_weight_diagonals)
  int* weight_mask = nullptr;                              // [max_batch] device copy of a host mask
  ParamTable cone;                                         // rows [max_batch][BPMPC_SOLVER_CONE_STRIDE], start row = the DeviceModel's cone scalars (in weight_mem)
  int* cone_mask = nullptr;                                // [max_batch] device copy of a host mask
  // The value function (solver_value.hip, include/bpmpc.h "Value function"): its buffers exist from the first bpmpc_solver_enable_value_function
  // on (value.S == nullptr before: nothing allocated, nothing launched); value_on: every backward pass is followed by the two kernels of
  // k_value.hip.  While it is on the handle linearises in materialised form; own_materialize is the setting it goes back to.
  ValueArgs value{};
  DeviceBuffers value_mem;
  bool value_on = false;
  int own_materialize = 0;
  void launch_value();                                     // solver_value.hip: k_value_terms, k_value_sweep on the current buffers, on `stream`
  // The dual solution (solver_dual.hip, include/bpmpc.h "Dual solution"): buffers from the first bpmpc_solver_enable_dual_solution on
  // (dual.lambda == nullptr before: nothing allocated, nothing launched); dual_on: the kernels of k_dual.hip follow every launch_value.  It reads
  // the value function's rows, so the value function runs while either the caller asked for it (value_own) or dual_on: value_on = value_own || dual_on.
  DualArgs dual{};
  DeviceBuffers dual_mem;
  bool dual_on = false, value_own = false;
  void launch_dual();                                      // solver_dual.hip: k_dual_node, k_dual_summary behind launch_value(), on `stream`
  void build_plan() {
    Launch& L = plan;
    L.model = d_model;
    L.buf = buf;
    L.batch = batch;
    L.N = settings.max_nodes;
    L.k0 = 0;
    // node range of a launch: the longest grid of the current setup, not the solver's capacity - the per-node kernels map their
    // workgroups onto batch x klen node slots and every slot beyond a problem's grid is a lane group that idles
    L.klen = n_nodes_max > 0 ? n_nodes_max : settings.max_nodes;
    L.cold = cold ? 1 : 0;
    L.serial_legs = serial_legs() ? 1 : 0;
    L.weights_q_diagonal = (dm.ws.compact && dm.ws.q_diagonal) ? 1 : 0;
    L.feedback = feedback();
    L.ls = ls;
    L.reg_prim = settings.reg_prim;
    L.lin_ev_n = -1; L.lin_inter = 0;
    for (int i = 0; i < kLinMaxEvents; ++i) L.lin_ev[i] = 0;
    if (n_grids == 1 && sw.lin_compact && !grid_kind.empty() && (int)grid_nodes.size() == 1) {
      const int n = grid_nodes[0];
      int ne = 0;
      for (int k = 0; k < n; ++k)
        if (grid_kind[k] == 1) { if (ne < kLinMaxEvents) L.lin_ev[ne] = k; ++ne; }
      if (ne <= kLinMaxEvents && n == L.klen) { L.lin_ev_n = ne; L.lin_inter = n - ne; }
    }
    L.ilqr = is_ddp() ? 1 : 0;                                  // the DDP solver: every kernel of the backward pass works on the Euler-discretised model
    L.ilqr_shift = is_ddp() ? rm.ddp.ls_hessian_correction_multiple : 0.0;
  }
  // The lineariser's events are attached to its dispatch (kl::linearize_fast): their elapsed time is the kernel's duration, without the barrier
  // packets and the dispatch latency a pair of hipEventRecord calls brackets as well
  void launch_linearize_fast(hipStream_t on, const Launch& L, int nodes) {
    if (plan_weights.rows) {                               // per-problem weights: kernel class "linearize_w" (bpmpc_solver_kernel_time)
      if (!KernelTimers::timed(settings.profile, "linearize_w")) { kl::linearize_fast_w(nj(), settings.materialize_lq != 0, on, L, plan_weights); return; }
      timers.attached("linearize_w", [&](hipEvent_t a, hipEvent_t b) { kl::linearize_fast_w(nj(), settings.materialize_lq != 0, on, L, plan_weights, a, b); });
      return;
    }
    if (!KernelTimers::timed(settings.profile, "linearize")) { kl::linearize_fast(nj(), settings.materialize_lq != 0, nodes, on, L); return; }
    timers.attached("linearize", [&](hipEvent_t a, hipEvent_t b) { kl::linearize_fast(nj(), settings.materialize_lq != 0, nodes, on, L, a, b); });
  }

  void stage_prepare();
  void stage_linearize();
  void stage_project();
  void stage_riccati();
  void launch_project(hipStream_t on, const Launch& L, int nodes);
  void launch_riccati(const Launch& L);
  void stage_linesearch();
  void pipelined_backward();
  void run_iterations();
  void run_ddp();
  void ddp_nominal_rollout();
  DdpBuffers ddp{};                                       // the DDP slice (settings.solver = BPMPC_SOLVER_DDP)
  bool is_ddp() const { return settings.solver == BPMPC_SOLVER_DDP; }
  // one value for the warm start, the policy rollout and the controller a caller builds (sqp.useFeedbackPolicy / ddp.useFeedbackPolicy of task.info, or the override)
  int feedback() const { return settings.feedback_policy == 1 ? 1 : (settings.feedback_policy == 2 ? 0 : (is_ddp() ? rm.ddp.use_feedback_policy : rm.sqp.use_feedback_policy)); }
  int nj() const { return rm.nj; }
};

namespace bpmpc {

// ---- batched small transfers (transfer.hip)
// Small transfers in ONE copy.  Every hipMemcpyAsync is a DMA operation of its own on the stream (5 .. 8 us each whatever its size) and a runtime call on the
// host: the nine uploads and five read-backs of a setup_commands and the four results of a fetch were most of what a batch = 1 MPC tick spent outside its
// solve.  Here the pieces travel as one block through `xfer`; a kernel scatters the block to (gathers it from) the arrays the other kernels use.
struct CopyTable {
  static constexpr int kMax = 16;
  void* dst[kMax]; const void* src[kMax]; unsigned words[kMax]; int n;
};
void launch_copy_table(bpmpc_solver* s, const CopyTable& t);
struct TransferPiece { void* device; const void* host_src; void* host_dst; size_t bytes; };
// host -> device, pieces of whole 4-byte words (pin_up.reset() by the caller)
void upload_batch(bpmpc_solver* s, const TransferPiece* pc, int n);
// device -> host: enqueue() behind the work on the stream, the caller waits for the stream, finish() hands the pieces to their owners
struct Downloads {
  static constexpr size_t kPackLimit = size_t(512) << 10;   // larger pieces travel on their own (a packed piece is copied once more on the device)
  struct Item { TransferPiece pc; void* pin; };
  std::vector<Item> items;
  void add(void* host, const void* device, size_t bytes) { if (host && bytes) items.push_back({{const_cast<void*>(device), nullptr, host, bytes}, nullptr}); }
  void enqueue(bpmpc_solver* s);
  void finish() const { for (const Item& it : items) if (it.pin) std::memcpy(it.pc.host_dst, it.pin, it.pc.bytes); }
};

// ---- what the device-side setups share (solver.hip): setup_commands and the gait batch's setup_gaits (gait_batch.hip)
// Host image of the device gait library: the passed templates, then defaultModeSequenceTemplate; initialModeSchedule behind them
struct GaitLibrary {
  std::vector<double> d;
  std::vector<int> i;
  int n_templates = 0, init_n_events = 0;
  size_t first_mode_count = 0, sw_count = 0, mode_count = 0;
  GaitLibraryView view(const double* dev_d, const int* dev_i, double transition_stance_time) const {
    GaitLibraryView v{};
    v.switching = dev_d; v.first_mode = dev_i; v.modes = dev_i + first_mode_count; v.n_templates = n_templates;
    v.init_events = dev_d + sw_count; v.init_modes = dev_i + first_mode_count + mode_count; v.init_n_events = init_n_events;
    v.transition_stance_time = transition_stance_time;
    return v;
  }
};
GaitLibrary gait_library(const RobotModel& rm, const bpmpc_gait_template* gaits, int n_gaits);
void check_device_setup(bpmpc_solver* s, const char* what, int batch, double horizon, const double* t0, const double* x0, const double* cmd_vel,
                        int command_kind, bool invalid_other);
ReferenceGenArgs reference_args(bpmpc_solver* s, const GaitLibraryView& lib, int G, double horizon);
void copy_loop_x0(bpmpc_solver* s, int batch, const double* x0);
CommandTargetArgs command_target_args(const bpmpc_solver* s, int batch, int command_kind, double time_to_target);
void launch_command_targets(bpmpc_solver* s, int batch, double horizon, int command_kind, double time_to_target);
void preserve_previous(bpmpc_solver* s, int batch, bool warm_arrays);
void accept_reference_grids(bpmpc_solver* s, int batch, int G, const std::vector<int>& pgrid);
void finish_setup(bpmpc_solver* s, int batch, const double* warm_x, const double* warm_u, bool from_previous);

// ---- the refusals of the policy (controller tick, evaluate_policy, rollout) and of the restart (solver.hip): std::invalid_argument, Unsupported
void refuse_while_restarting(const bpmpc_solver* s, const char* what);
void check_policy(const bpmpc_solver* s);                 // controller tick / evaluate_policy: SQP, no restart pending, a completed run, the gains
void check_restart(const bpmpc_solver* s, int batch);
void restart(bpmpc_solver* s, int batch, const int* mask, const double* x_new, bool on_device);
void release_weights(bpmpc_solver* s);                    // solver_weights.hip: the memory of the weight and cone tables (bpmpc_solver_destroy)
void ensure_weight_table(bpmpc_solver* s);                // solver_weights.hip / solver_cone.hip: the tables of the per-problem kernel family, allocated and
void ensure_cone_table(bpmpc_solver* s);                  // filled from their start rows by the first set of either
void release_value(bpmpc_solver* s);                      // solver_value.hip: the value buffers (bpmpc_solver_destroy)
void apply_value_state(bpmpc_solver* s, const char* who); // solver_value.hip: value_on = value_own || dual_on, with the buffers and the materialise setting that go with it
void release_dual(bpmpc_solver* s);                       // solver_dual.hip: the dual buffers (bpmpc_solver_destroy)

// The guard of the entry points on a solver handle (guarded): the handle's device is set before the body, BPMPC_ERR_IO for an exception of no
// class of its own.
template <typename F>
int guarded(bpmpc_solver* s, F&& body) {
  if (!s) { set_last_error("null solver handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  const int rc = guarded(BPMPC_ERR_IO, [&] { HIP_CHECK(hipSetDevice(s->settings.device)); body(); });
  if (rc != BPMPC_OK) {
    // a call that threw between enqueueing copies from / to the pinned arenas and its own synchronisation: wait for them before the
    // next call recycles (or frees) that memory
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->producer_stream) (void)hipStreamSynchronize(s->producer_stream);
  }
  return rc;
}

}  // namespace bpmpc
