// The gait batch (include/bpmpc.h: bpmpc_gait_batch): one GaitSchedule per robot on the device, the runtime gait commands and restarts that
// change them, and bpmpc_solver_setup_gaits, the device-side setup of a solver handle from those schedules (kernels/gait_state.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "solver.h"
#include "kernels/gait_state.h"

// One GaitSchedule per robot on the device (include/bpmpc.h, bpmpc_gait_batch): the schedules live in state slots of a double buffer,
// robots of one slot share their whole history (create / reset, inserts, commands, the t0 of every setup) and so their schedule and their grid.
// bpmpc_solver_setup_gaits advances the front buffer into the back one and swaps them only when every robot was accepted.
struct bpmpc_gait_batch {
  bpmpc_solver* solver = nullptr;
  int max_batch = 0, n_gaits = 0;
  GaitLibraryView lib{};                                    // on the device, uploaded once
  double* ev[2] = {nullptr, nullptr};                      // [slot][kRefMaxEvents]
  int* ms[2] = {nullptr, nullptr};                         // [slot][kRefMaxEvents + 1]
  int* meta[2] = {nullptr, nullptr};                       // [slot][kGaitMeta]
  int front = 0;
  int* grp_i = nullptr;                                    // per group of a setup: source slot, insert gait, command [3][max_batch]
  double* grp_d = nullptr;                                 // ... t0, insert start, insert final [3][max_batch]
  int* cmd_dev = nullptr;                                  // pending commands while device-side commands are outstanding
  bool cmd_on_device = false;                              // cmd_dev, not cmd, holds the pending commands
  std::vector<int> slot;                                   // per robot: state slot in the front buffer, < 0 = the state after create / reset
  std::vector<int> cmd, ins_gait;                          // per robot: pending command / insert (< 0: none)
  std::vector<double> ins_start, ins_final;
  // restarts (bpmpc_gait_batch_restart): restart[b] != 0 - the next accepted setup advances robot b from the state after create / reset.  A device
  // mask writes the number of its call (restart_epoch) to restart_dev[b]; entries above restart_base are read back by the next setup.  Inserts
  // and host-side commands keep the number of device restarts recorded before them (ins_epoch, cmd_epoch): a restart drops only what came first
  std::vector<int> restart, cmd_epoch, ins_epoch;
  int* restart_dev = nullptr;
  int restart_epoch = 0, restart_base = 0;
  bool restart_on_device = false;
  DeviceBuffers mem;
};

namespace {

void check_gait_batch(const bpmpc_gait_batch* g, int batch, const int* gait, bool host_gaits) {
  if (!g) throw std::invalid_argument("null gait batch handle");
  if (batch < 1 || batch > g->max_batch) throw std::invalid_argument("batch exceeds the gait batch's max_batch");
  if (!gait) throw std::invalid_argument("null gait array");
  if (host_gaits)
    for (int b = 0; b < batch; ++b)
      if (gait[b] >= g->n_gaits) throw std::invalid_argument("gait index refers to a template that was not passed");
}

void gait_batch_reset(bpmpc_gait_batch* g) {
  std::fill(g->slot.begin(), g->slot.end(), -1);
  std::fill(g->cmd.begin(), g->cmd.end(), -1);
  std::fill(g->ins_gait.begin(), g->ins_gait.end(), -1);
  std::fill(g->ins_start.begin(), g->ins_start.end(), 0.0);
  std::fill(g->ins_final.begin(), g->ins_final.end(), 0.0);
  g->cmd_on_device = false;
  std::fill(g->restart.begin(), g->restart.end(), 0);
  g->restart_base = g->restart_epoch;
  g->restart_on_device = false;
}

// the pending commands back on the host (synchronises; only after a device-side command)
void gait_commands_to_host(bpmpc_gait_batch* g) {
  if (!g->cmd_on_device) return;
  bpmpc_solver* s = g->solver;
  HIP_CHECK(hipMemcpyAsync(g->cmd.data(), g->cmd_dev, g->max_batch * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
  g->cmd_on_device = false;
  std::fill(g->cmd_epoch.begin(), g->cmd_epoch.end(), g->restart_epoch);   // k_gait_restart already dropped what the device restarts drop
}

// the pending device restarts back on the host (synchronises; only after a device mask): each drops the insert / host command recorded before it
void gait_restarts_to_host(bpmpc_gait_batch* g) {
  if (!g->restart_on_device) return;
  bpmpc_solver* s = g->solver;
  std::vector<int> epoch(g->max_batch);
  HIP_CHECK(hipMemcpyAsync(epoch.data(), g->restart_dev, g->max_batch * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
  for (int b = 0; b < g->max_batch; ++b) {
    if (epoch[b] <= g->restart_base) continue;
    g->restart[b] = 1;
    if (g->cmd_epoch[b] < epoch[b]) g->cmd[b] = -1;
    if (g->ins_epoch[b] < epoch[b]) g->ins_gait[b] = -1;
  }
  g->restart_base = g->restart_epoch;
  g->restart_on_device = false;
}

__global__ __launch_bounds__(256) void k_gait_restart(int batch, const int* mask, int epoch, int* restart, int* cmd) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch || !mask[b]) return;
  restart[b] = epoch;
  if (cmd) cmd[b] = -1;                                   // device-side pending commands are dropped in stream order
}

void gait_batch_restart(bpmpc_gait_batch* g, int batch, const int* mask, bool on_device) {
  if (batch < 1 || batch > g->max_batch) throw std::invalid_argument("bpmpc_gait_batch_restart: batch exceeds the gait batch's max_batch");
  bpmpc_solver* s = g->solver;
  if (!on_device) {
    gait_commands_to_host(g);
    gait_restarts_to_host(g);
    for (int b = 0; b < batch; ++b)
      if (mask[b]) { g->restart[b] = 1; g->cmd[b] = -1; g->ins_gait[b] = -1; }
    return;
  }
  ++g->restart_epoch;
  hipLaunchKernelGGL(k_gait_restart, dim3((batch + 255) / 256), dim3(256), 0, s->stream, batch, mask, g->restart_epoch, g->restart_dev,
                     g->cmd_on_device ? g->cmd_dev : nullptr);
  HIP_CHECK(hipGetLastError());
  g->restart_on_device = true;
}

void gait_batch_command(bpmpc_gait_batch* g, int batch, const int* gait, bool on_device) {
  check_gait_batch(g, batch, gait, !on_device);
  bpmpc_solver* s = g->solver;
  if (!on_device) {
    gait_commands_to_host(g);
    for (int b = 0; b < batch; ++b) if (gait[b] >= 0) { g->cmd[b] = gait[b]; g->cmd_epoch[b] = g->restart_epoch; }
    return;
  }
  if (!g->cmd_on_device) {                                // the device copy takes over: it starts from the host's pending commands
    if (g->restart_on_device && std::any_of(g->cmd.begin(), g->cmd.end(), [](int c) { return c >= 0; })) gait_restarts_to_host(g);   // ... as a restart left them
    if (std::all_of(g->cmd.begin(), g->cmd.end(), [](int c) { return c < 0; })) {
      HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)g->cmd_dev, -1, g->max_batch, s->stream));
    } else {
      HIP_CHECK(hipMemcpyAsync(g->cmd_dev, g->cmd.data(), g->max_batch * sizeof(int), hipMemcpyHostToDevice, s->stream));
      HIP_CHECK(hipStreamSynchronize(s->stream));
    }
  }
  hipLaunchKernelGGL(k_gait_command, dim3((batch + 255) / 256), dim3(256), 0, s->stream, batch, gait, g->cmd_dev);
  HIP_CHECK(hipGetLastError());
  g->cmd_on_device = true;
}

// GaitSchedule state of one robot after the last setup (synchronises)
void gait_batch_mode_schedule(bpmpc_gait_batch* g, int robot, double* event_times, int* modes, int capacity, int* n_events) {
  if (!g || !event_times || !modes || !n_events) throw std::invalid_argument("bpmpc_gait_batch_mode_schedule: null argument");
  if (robot < 0 || robot >= g->max_batch) throw std::invalid_argument("bpmpc_gait_batch_mode_schedule: robot out of range");
  const int slot = g->slot[robot];
  if (slot < 0) {
    const ModeSchedule& init = g->solver->rm.initial_mode_schedule;
    if ((int)init.modes.size() > capacity || (int)init.event_times.size() > capacity) throw std::length_error("mode schedule capacity too small");
    std::copy(init.event_times.begin(), init.event_times.end(), event_times);
    std::copy(init.modes.begin(), init.modes.end(), modes);
    *n_events = (int)init.event_times.size();
    return;
  }
  bpmpc_solver* s = g->solver;
  int meta[kGaitMeta];
  HIP_CHECK(hipMemcpyAsync(meta, g->meta[g->front] + (size_t)slot * kGaitMeta, sizeof(meta), hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
  if (meta[0] > capacity || meta[1] > capacity) throw std::length_error("mode schedule capacity too small");
  HIP_CHECK(hipMemcpyAsync(event_times, g->ev[g->front] + (size_t)slot * kRefMaxEvents, meta[0] * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipMemcpyAsync(modes, g->ms[g->front] + (size_t)slot * (kRefMaxEvents + 1), meta[1] * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
  *n_events = meta[0];
}

// setup_commands with the schedules of the gait batch: the pending inserts, getModeSchedule(t0 - H, t0 + 2 H) as the window of this setup,
// then the pending commands at (t0 + H, H) - per group of robots with one history, in k_gait_advance
void setup_gaits(bpmpc_solver* s, bpmpc_gait_batch* g, int batch, double horizon, const double* t0, const double* x0, const double* cmd_vel,
                 int command_kind, double time_to_target, bool from_previous) {
  if (!g || g->solver != s) throw std::invalid_argument("setup_gaits: the gait batch belongs to another solver");
  if (batch < 1 || batch > g->max_batch) throw std::invalid_argument("setup_gaits: batch exceeds the gait batch's max_batch");
  check_device_setup(s, "setup_gaits", batch, horizon, t0, x0, cmd_vel, command_kind, false);
  gait_commands_to_host(g);
  gait_restarts_to_host(g);
  for (int b = 0; b < batch; ++b)
    if (g->cmd[b] >= g->n_gaits) throw std::invalid_argument("setup_gaits: a gait command refers to a template that was not passed");
  const int NX = s->nx, B = g->max_batch;
  // groups: robots of the batch with one (history, t0, pending insert, pending command) advance together; robots behind the batch
  // keep their state (one group per slot in use)
  std::vector<int> pgrid(batch), new_slot(B, -1), src, ins_g, cmd;
  std::vector<double> gt0, ins_s, ins_f;
  {
    std::map<std::tuple<int, double, int, double, double, int>, int> seen;
    for (int b = 0; b < batch; ++b) {
      const bool ins = g->ins_gait[b] >= 0;
      auto key = std::make_tuple(g->restart[b] ? -1 : g->slot[b], t0[b], ins ? g->ins_gait[b] : -1, ins ? g->ins_start[b] : 0.0, ins ? g->ins_final[b] : 0.0, g->cmd[b] < 0 ? -1 : g->cmd[b]);
      auto it = seen.find(key);
      if (it == seen.end()) {
        it = seen.emplace(key, (int)src.size()).first;
        src.push_back(std::get<0>(key)); gt0.push_back(t0[b]); ins_g.push_back(std::get<2>(key)); ins_s.push_back(std::get<3>(key)); ins_f.push_back(std::get<4>(key));
        cmd.push_back(std::get<5>(key));
      }
      pgrid[b] = new_slot[b] = it->second;
    }
  }
  const int G = (int)src.size();
  {
    std::map<int, int> kept;
    for (int b = batch; b < B; ++b) {
      if (g->slot[b] < 0) continue;
      auto it = kept.find(g->slot[b]);
      if (it == kept.end()) {
        it = kept.emplace(g->slot[b], (int)src.size()).first;
        src.push_back(g->slot[b]); gt0.push_back(0.0); ins_g.push_back(-1); ins_s.push_back(0.0); ins_f.push_back(0.0); cmd.push_back(-1);
      }
      new_slot[b] = it->second;
    }
  }
  const int groups = (int)src.size();
  std::vector<int> gi(3 * (size_t)B, -1);
  std::vector<double> gd(3 * (size_t)B, 0.0);
  std::copy(src.begin(), src.end(), gi.begin()); std::copy(ins_g.begin(), ins_g.end(), gi.begin() + B); std::copy(cmd.begin(), cmd.end(), gi.begin() + 2 * B);
  std::copy(gt0.begin(), gt0.end(), gd.begin()); std::copy(ins_s.begin(), ins_s.end(), gd.begin() + B); std::copy(ins_f.begin(), ins_f.end(), gd.begin() + 2 * B);
  if (from_previous) preserve_previous(s, batch, false);
  Buffers& bf = s->buf;
  s->pin_up.reset();                                      // the previous call waited for its transfers (the synchronisation below)
  {
    const TransferPiece up[6] = {{g->grp_i, gi.data(), nullptr, gi.size() * sizeof(int)}, {g->grp_d, gd.data(), nullptr, gd.size() * sizeof(double)},
                                 {bf.p_grid, pgrid.data(), nullptr, pgrid.size() * sizeof(int)}, {bf.p_t0, t0, nullptr, (size_t)batch * sizeof(double)},
                                 {bf.p_cmd, cmd_vel, nullptr, cmd_vel ? (size_t)batch * 4 * sizeof(double) : 0}, {bf.p_x0, x0, nullptr, x0 ? (size_t)batch * NX * sizeof(double) : 0}};
    upload_batch(s, up, 6);
  }
  GaitAdvanceArgs a{};
  a.ref = reference_args(s, g->lib, G, horizon);
  a.ref.t0 = g->grp_d;
  a.n_advance = G;
  a.src = g->grp_i; a.insert_gait = g->grp_i + B; a.command = g->grp_i + 2 * B;
  a.insert_start = g->grp_d + B; a.insert_final = g->grp_d + 2 * B;
  const int f = g->front, k = 1 - f;
  a.ev_in = g->ev[f]; a.ms_in = g->ms[f]; a.meta_in = g->meta[f];
  a.ev_out = g->ev[k]; a.ms_out = g->ms[k]; a.meta_out = g->meta[k];
  copy_loop_x0(s, batch, x0);
  hipLaunchKernelGGL(k_gait_advance, dim3(groups), dim3(64), 0, s->stream, a);
  HIP_CHECK(hipGetLastError());
  launch_command_targets(s, batch, horizon, command_kind, time_to_target);
  accept_reference_grids(s, batch, G, pgrid);
  // every robot was accepted: the new schedules become the front buffer, the applied inserts and commands are no longer pending
  g->front = k;
  g->slot.swap(new_slot);
  std::fill(g->cmd.begin(), g->cmd.begin() + batch, -1);
  std::fill(g->ins_gait.begin(), g->ins_gait.begin() + batch, -1);
  std::fill(g->restart.begin(), g->restart.begin() + batch, 0);
  finish_setup(s, batch, nullptr, nullptr, from_previous);
}

}  // namespace

extern "C" {

int bpmpc_solver_setup_gaits(bpmpc_solver* s, bpmpc_gait_batch* g, int batch, double horizon, const double* t0, const double* x0, const double* cmd_vel,
                             int command_kind, double time_to_target, int from_previous) {
  return guarded(s, [&] { setup_gaits(s, g, batch, horizon, t0, x0, cmd_vel, command_kind, time_to_target, from_previous != 0); });
}
int bpmpc_gait_batch_create(bpmpc_solver* s, const bpmpc_gait_template* gaits, int n_gaits, bpmpc_gait_batch** out) {
  if (!out) { set_last_error("bpmpc_gait_batch_create: null output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  if (!s) { set_last_error("bpmpc_gait_batch_create: null solver handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  std::unique_ptr<bpmpc_gait_batch> g(new bpmpc_gait_batch);
  const int rc = guarded(BPMPC_ERR_IO, [&] {
    if (n_gaits < 0 || (n_gaits > 0 && !gaits)) throw std::invalid_argument("bpmpc_gait_batch_create: null or invalid gait templates");
    HIP_CHECK(hipSetDevice(s->settings.device));
    const GaitLibrary lib = gait_library(s->rm, gaits, n_gaits);
    const int B = s->settings.max_batch;
    g->solver = s; g->max_batch = B; g->n_gaits = n_gaits;
    DeviceBuffers& m = g->mem;
    double* lib_d = m.alloc<double>(lib.d.size());
    int* lib_i = m.alloc<int>(lib.i.size());
    for (int k = 0; k < 2; ++k) {
      g->ev[k] = m.alloc<double>((size_t)B * kRefMaxEvents);
      g->ms[k] = m.alloc<int>((size_t)B * (kRefMaxEvents + 1));
      g->meta[k] = m.alloc<int>((size_t)B * kGaitMeta);
    }
    g->grp_i = m.alloc<int>(3 * (size_t)B);
    g->grp_d = m.alloc<double>(3 * (size_t)B);
    g->cmd_dev = m.alloc<int>((size_t)B);
    g->restart_dev = m.alloc<int>((size_t)B);
    HIP_CHECK(hipMemsetAsync(g->restart_dev, 0, (size_t)B * sizeof(int), s->stream));
    HIP_CHECK(hipMemcpyAsync(lib_d, lib.d.data(), lib.d.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_CHECK(hipMemcpyAsync(lib_i, lib.i.data(), lib.i.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
    g->lib = lib.view(lib_d, lib_i, s->rm.phase_transition_stance_time);
    g->slot.resize(B); g->cmd.resize(B); g->ins_gait.resize(B); g->ins_start.resize(B); g->ins_final.resize(B);
    g->restart.resize(B); g->cmd_epoch.resize(B); g->ins_epoch.resize(B);
    gait_batch_reset(g.get());
  });
  if (rc != BPMPC_OK) { bpmpc_gait_batch_destroy(g.release()); return rc; }
  *out = g.release();
  return BPMPC_OK;
}
void bpmpc_gait_batch_destroy(bpmpc_gait_batch* g) {
  if (!g) return;
  if (g->solver && g->solver->stream) (void)hipStreamSynchronize(g->solver->stream);
  g->mem.release();
  delete g;
}
int bpmpc_gait_batch_reset(bpmpc_gait_batch* g) {
  if (!g) { set_last_error("bpmpc_gait_batch_reset: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  gait_batch_reset(g);
  return BPMPC_OK;
}
int bpmpc_gait_batch_insert(bpmpc_gait_batch* g, int batch, const int* gait, const double* start_time, const double* final_time) {
  return guarded(BPMPC_ERR_IO, [&] {
    check_gait_batch(g, batch, gait, true);
    if (!start_time || !final_time) throw std::invalid_argument("bpmpc_gait_batch_insert: null start or final times");
    for (int b = 0; b < batch; ++b)
      if (gait[b] >= 0) { g->ins_gait[b] = gait[b]; g->ins_start[b] = start_time[b]; g->ins_final[b] = final_time[b]; g->ins_epoch[b] = g->restart_epoch; }
  });
}
int bpmpc_gait_batch_command(bpmpc_gait_batch* g, int batch, const int* gait, int inputs_on_device) {
  if (!g) { set_last_error("bpmpc_gait_batch_command: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(g->solver, [&] { gait_batch_command(g, batch, gait, inputs_on_device != 0); });
}
int bpmpc_gait_batch_restart(bpmpc_gait_batch* g, int batch, const int* mask, int inputs_on_device) {
  if (!g || !mask) { set_last_error("bpmpc_gait_batch_restart: null handle or mask"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(g->solver, [&] { gait_batch_restart(g, batch, mask, inputs_on_device != 0); });
}
int bpmpc_gait_batch_mode_schedule(bpmpc_gait_batch* g, int robot, double* event_times, int* modes, int capacity, int* n_events) {
  if (!g) { set_last_error("bpmpc_gait_batch_mode_schedule: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(g->solver, [&] { gait_batch_mode_schedule(g, robot, event_times, modes, capacity, n_events); });
}

}  // extern "C"
