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
#include "launch.h"
#include "kernels/reference_device.h"

namespace bpmpc {

struct KernelTimer {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double total_ms = 0.0;
  int launches = 0;
};

}  // namespace bpmpc

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
  // change of variables reading the packed joint rows of the structured elimination: needs an input weight without force / joint-velocity
  // cross terms (checked when the solver is created; BipedalRobotInterface.cpp:239-271 builds it so).  BPMPC_DENSE_PROJECT=1 switches it off.
  bool structured_project = false;
  // Riccati sweep by regime: eight waves with fixed roles while every problem has a CU to itself; four-wave workgroups up to two problems per CU;
  // beyond that one wavefront per problem (riccati_wave.h at one wave per SIMD up to four problems per CU, riccati_wave2.h at two beyond).
  // BPMPC_RICCATI_WAVE: 0 never a wave per problem; 1 (default) as described; 2 riccati_wave.h at every batch size, 4 riccati_wave2.h at every
  // batch size (tests); 3 riccati_wave2.h whenever a wave per problem is used
  int riccati_wave = 1;
  bool lin_compact = true;                                  // BPMPC_LIN_COMPACT=0: the lineariser keeps the event nodes in line (A/B, tests)
  bool force_tables = false;                                // BPMPC_LIN_TABLES=1: the table walks also on a robot of two serial legs (tests)
  bool wt_joint_rows = false;                               // BPMPC_WT_JOINT_ROWS=1: the change of variables always writes the joint rows of Wt (A/B of the byte cut below)
  // which sweep runs the current batch (see launch_riccati)
  bool sweep_wave_regime() const { return riccati_wave == 2 || riccati_wave == 4 || ((riccati_wave == 1 || riccati_wave == 3) && batch > 2 * num_cus); }
  bool sweep_two_per_simd() const { return sweep_wave_regime() && (riccati_wave >= 3 || (riccati_wave == 1 && batch > 4 * num_cus)); }
  // the wave-per-problem sweeps (riccati_wave.h, riccati_wave2.h) and the loaders of the eight-wave sweep (riccati_mfma8.h, PackedStageLoader JR) complete the joint rows of Wt = [At | bt | Bt] from Vt ([I | b | 0] + dt Vt): the change of variables then
  // neither computes nor writes them (3.8 KB per node less each way at the batch sizes where both kernels stream)
  bool sweep_completes_joint_rows() const { return !wt_joint_rows && structured_project && !settings.reference_kernels; }     // every fast sweep does
  // The eight-wave sweep holds a CU per problem; a larger batch runs it in ROUNDS (the dispatcher starts a workgroup as a CU becomes free, so the roll-outs
  // behind the sweeps no longer stream at the same time).  Since its roll-out goes through the ring (round 6) two and three rounds of it beat what those batch
  // sizes ran before on the 22-state robots - batch 512: 0.5447 against 0.5837 ms on the four-wave workgroups, 768: 0.807 against 0.878 on a wave per problem;
  // 1024 in four rounds: 1.075 against 0.917, so from there on the wave sweeps - and lose on nx = 24 (G1 / 512: 0.8545 against 0.7682 on the four-wave
  // workgroups), whose eight-wave stage is 55 % longer (`experiments/LOG.md`).  BPMPC_R8_ROUNDS overrides (1: the regimes of rounds 3 to 5; tests).
  int r8_rounds = 0;                                        // 0: by the robot, as measured
  int eight_wave_rounds() const { return r8_rounds > 0 ? r8_rounds : (rm.nj == 10 ? 3 : 1); }
  bool sweep_eight_waves() const { return riccati_wave != 2 && riccati_wave != 4 && batch <= eight_wave_rounds() * num_cus; }
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
  std::map<std::string, std::pair<void*, size_t>> named;   // name -> (device ptr, element count)  (doubles unless in int_named)
  std::map<std::string, bool> is_int;
  std::vector<double> node_times;                          // host copy: [n_grids][N+1]
  std::vector<int> grid_nodes, grid_of_problem;
  std::map<std::string, KernelTimer> timers;
  int* h_remaining = nullptr;                              // pinned
  LineSearchSettings ls{};

  template <typename T>
  T* alloc(const char* name, size_t count, bool integer = false) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, count * sizeof(T)));
    HIP_CHECK(hipMemsetAsync(p, 0, count * sizeof(T), stream));
    allocations.push_back(p);
    if (name) { named[name] = {p, count}; is_int[name] = integer; }
    return static_cast<T*>(p);
  }

  Launch launch_params() const {
    Launch L;
    L.model = d_model;
    L.buf = buf;
    L.batch = batch;
    L.N = settings.max_nodes;
    L.k0 = 0;
    // node range of a launch: the longest grid of the current setup, not the solver's capacity - the per-node kernels map their
    // workgroups onto batch x klen node slots and every slot beyond a problem's grid is a lane group that idles
    L.klen = n_nodes_max > 0 ? n_nodes_max : settings.max_nodes;
    L.cold = cold ? 1 : 0;
    L.serial_legs = (dm.serial_legs && !force_tables) ? 1 : 0;
    L.feedback = feedback();
    L.ls = ls;
    L.reg_prim = settings.reg_prim;
    L.lin_ev_n = -1; L.lin_inter = 0;
    for (int i = 0; i < kLinMaxEvents; ++i) L.lin_ev[i] = 0;
    if (n_grids == 1 && lin_compact && !grid_kind.empty() && (int)grid_nodes.size() == 1) {
      const int n = grid_nodes[0];
      int ne = 0;
      for (int k = 0; k < n; ++k)
        if (grid_kind[k] == 1) { if (ne < kLinMaxEvents) L.lin_ev[ne] = k; ++ne; }
      if (ne <= kLinMaxEvents && n == L.klen) { L.lin_ev_n = ne; L.lin_inter = n - ne; }
    }
    L.ilqr = is_ddp() ? 1 : 0;                                  // the DDP solver: every kernel of the backward pass works on the Euler-discretised model
    L.ilqr_shift = is_ddp() ? rm.ddp.ls_hessian_correction_multiple : 0.0;
    return L;
  }

  // Events that only measure time: no system-scope fence when they complete (hipEventDisableSystemFence: "avoiding the cost of cache writeback and
  // invalidation, and the performance impact of those actions on the execution of following work") - with the default flags the step that carries
  // the roofline kernel's events ran 3 % slower than the steps without them (the kernel behind the lineariser found its inputs flushed from L2)
  static constexpr unsigned kTimingEventFlags = hipEventDisableSystemFence;
  // settings.profile: 0 off, 1 every kernel class, 2 the linearisation kernel only (the roofline measurement of bench.py: every
  // event pair costs one to two microseconds of stream time, ten pairs per solve are 2 % of a step)
  bool timed(const char* cls) const { return settings.profile == 1 || (settings.profile == 2 && std::strcmp(cls, "linearize") == 0); }
  void time_begin(const char* cls, hipEvent_t* a, hipEvent_t* b, hipStream_t on = nullptr) {
    if (!timed(cls)) return;
    HIP_CHECK(hipEventCreateWithFlags(a, kTimingEventFlags));
    if (hipEventCreateWithFlags(b, kTimingEventFlags) != hipSuccess) { (void)hipEventDestroy(*a); throw DeviceError("hipEventCreate failed"); }
    if (hipEventRecord(*a, on ? on : stream) != hipSuccess) { (void)hipEventDestroy(*a); (void)hipEventDestroy(*b); throw DeviceError("hipEventRecord failed"); }
  }
  void time_end(const char* cls, hipEvent_t a, hipEvent_t b, hipStream_t on = nullptr) {
    if (!timed(cls)) return;
    HIP_CHECK(hipEventRecord(b, on ? on : stream));
    KernelTimer& t = timers[cls];
    t.pending.emplace_back(a, b);
    if (t.pending.size() > 4096) collect_timers();   // a profiled loop that never asks for the times must not grow without bound
  }
  // The lineariser's events are attached to its dispatch (kl::linearize_fast): their elapsed time is the kernel's duration, without the barrier
  // packets and the dispatch latency a pair of hipEventRecord calls brackets as well
  void launch_linearize_fast(hipStream_t on, const Launch& L, int nodes) {
    if (!timed("linearize")) { kl::linearize_fast(nj(), settings.materialize_lq != 0, nodes, on, L); return; }
    hipEvent_t a, b;
    HIP_CHECK(hipEventCreateWithFlags(&a, kTimingEventFlags));
    if (hipEventCreateWithFlags(&b, kTimingEventFlags) != hipSuccess) { (void)hipEventDestroy(a); throw DeviceError("hipEventCreate failed"); }
    kl::linearize_fast(nj(), settings.materialize_lq != 0, nodes, on, L, a, b);
    KernelTimer& t = timers["linearize"];
    t.pending.emplace_back(a, b);
    if (t.pending.size() > 4096) collect_timers();
  }
  void collect_timers() {
    for (auto& kv : timers) {
      hipError_t first_error = hipSuccess;                 // the events are destroyed whatever happens; the first failure is reported afterwards
      for (auto& pr : kv.second.pending) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(pr.second);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, pr.first, pr.second);
        if (e == hipSuccess) { kv.second.total_ms += ms; kv.second.launches += 1; }
        else if (first_error == hipSuccess) first_error = e;
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
      }
      kv.second.pending.clear();
      if (first_error != hipSuccess) throw DeviceError(std::string("kernel timers: ") + hipGetErrorString(first_error));
    }
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
void launch_command_targets(bpmpc_solver* s, int batch, double horizon, int command_kind, double time_to_target);
void preserve_previous(bpmpc_solver* s, int batch, bool warm_arrays);
void accept_reference_grids(bpmpc_solver* s, int batch, int G, const std::vector<int>& pgrid);
void finish_setup(bpmpc_solver* s, int batch, const double* warm_x, const double* warm_u, bool from_previous);

// ---- the refusals of the policy (controller tick, evaluate_policy, rollout) and of the restart (solver.hip): std::invalid_argument, Unsupported
void refuse_while_restarting(const bpmpc_solver* s, const char* what);
void check_policy(const bpmpc_solver* s);                 // controller tick / evaluate_policy: SQP, no restart pending, a completed run, the gains
void check_restart(const bpmpc_solver* s, int batch);
void restart(bpmpc_solver* s, int batch, const int* mask, const double* x_new, bool on_device);

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
