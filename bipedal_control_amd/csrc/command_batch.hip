// The command batch (include/bpmpc.h: bpmpc_command_batch): one stored TargetTrajectories per robot on the device, the calls that change them
// with the reference's semantics (starting, the two messages of TargetTrajectoriesPublisher, a given trajectory), their read-backs, and the
// window that the device-side setups of an attached solver take their targets from (kernels/command_batch.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "command_batch.h"
#include "kernels/command_batch.h"

namespace {

std::string robot_entry(const char* who, int b, const std::string& what) { return std::string(who) + ": robot " + std::to_string(b) + ": " + what; }

void check_finite(const char* who, int b, const char* name, const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) throw std::invalid_argument(robot_entry(who, b, std::string(name) + "[" + std::to_string(i) + "] is not finite"));
}

void check_batch(const bpmpc_command_batch* cb, const char* who, int batch) {
  if (batch < 1 || batch > cb->max_batch) throw std::invalid_argument(std::string(who) + ": batch exceeds the command batch's max_batch");
}

CommandStore store_of(const bpmpc_command_batch* cb) { return CommandStore{cb->max_points, cb->nx, cb->status, cb->times, cb->states}; }

// start (source kCommandStart, cmd unused), cmd_vel and goal: validated when they come from the host, staged, one launch on the solver's stream
void message(bpmpc_command_batch* cb, const char* who, int source, int batch, const int* mask, const double* cmd, const double* t_obs, const double* x_obs,
             double time_to_target, bool on_device) {
  bpmpc_solver* s = cb->solver;
  check_batch(cb, who, batch);
  const bool is_message = source != kCommandStart;
  if (!t_obs || (is_message && !cmd)) throw std::invalid_argument(std::string(who) + ": null argument");
  if (!std::isfinite(time_to_target)) throw std::invalid_argument(std::string(who) + ": time_to_target is not finite");
  // x_obs == NULL: the observations that are already on the device, the source of setup(x0 = NULL) (copy_loop_x0)
  if (!x_obs && (!(s->has_rollout || s->loop_from_tick) || batch != s->batch))
    throw std::invalid_argument(std::string(who) + ": x_obs == NULL needs a rollout of the same batch on the solver (or a controller tick)");
  const int NX = cb->nx;
  if (!on_device)
    for (int b = 0; b < batch; ++b) {
      if (mask && !mask[b]) continue;
      if (!std::isfinite(t_obs[b])) throw std::invalid_argument(robot_entry(who, b, "t_obs is not finite"));
      if (source == kCommandVelocity) check_finite(who, b, "cmd", cmd + (size_t)b * 4, 4);
      if (source == kCommandGoal) {                        // x, y, unused, yaw
        check_finite(who, b, "goal", cmd + (size_t)b * 4, 2);
        if (!std::isfinite(cmd[(size_t)b * 4 + 3])) throw std::invalid_argument(robot_entry(who, b, "goal[3] is not finite"));
      }
      if (x_obs) check_finite(who, b, "x_obs", x_obs + (size_t)b * NX, NX);
    }
  CommandMessageArgs a{};
  a.c = command_target_args(s, batch, source == kCommandGoal ? 1 : 0, time_to_target > 0 ? time_to_target : s->rm.time_horizon);
  a.store = store_of(cb);
  a.source = source;
  a.mask = staged(mask, cb->d_mask, (size_t)batch, on_device, s->stream);
  a.c.t0 = staged(t_obs, cb->d_t, (size_t)batch, on_device, s->stream);
  a.c.cmd_vel = is_message ? staged(cmd, cb->d_cmd, (size_t)batch * 4, on_device, s->stream) : nullptr;
  const bool foreign_tick = !x_obs && s->loop_from_tick && s->tick_hs;      // as copy_loop_x0: the ticks that write tick_x run on a policy buffer's stream
  a.c.x0 = x_obs ? staged(x_obs, cb->d_x, (size_t)batch * NX, on_device, s->stream) : (s->loop_from_tick ? s->tick_x : s->buf.roll_x);
  if (foreign_tick) s->tick_hs->before_foreign(s->stream);
  hipLaunchKernelGGL(k_command_message, dim3((batch + 63) / 64), dim3(64), 0, s->stream, a);
  HIP_CHECK(hipGetLastError());
  if (foreign_tick) s->tick_hs->after_foreign(s->stream);
  if (!on_device) HIP_CHECK(hipStreamSynchronize(s->stream));   // the caller's host arrays
}

void set_targets(bpmpc_command_batch* cb, int batch, const int* mask, const int* n_points, const double* times, const double* states, bool on_device) {
  const char* who = "bpmpc_command_batch_set_targets";
  bpmpc_solver* s = cb->solver;
  check_batch(cb, who, batch);
  if (!n_points || !times || !states) throw std::invalid_argument(std::string(who) + ": null argument");
  const int P = cb->max_points, NX = cb->nx;
  if (!on_device)
    for (int b = 0; b < batch; ++b) {
      if (mask && !mask[b]) continue;
      const int n = n_points[b];
      if (n < 1 || n > P) throw std::invalid_argument(robot_entry(who, b, "n_points " + std::to_string(n) + " is outside 1 .. " + std::to_string(P)));
      const double* t = times + (size_t)b * P;
      check_finite(who, b, "times", t, n);
      for (int i = 1; i < n; ++i)
        if (t[i] < t[i - 1]) throw std::invalid_argument(robot_entry(who, b, "times[" + std::to_string(i) + "] is below times[" + std::to_string(i - 1) + "]: the times must not decrease"));
      for (int i = 0; i < n; ++i) check_finite(who, b, ("states[" + std::to_string(i) + "]").c_str(), states + ((size_t)b * P + i) * NX, NX);
    }
  CommandStoreArgs a{};
  a.store = store_of(cb);
  a.batch = batch;
  a.mask = staged(mask, cb->d_mask, (size_t)batch, on_device, s->stream);
  a.n_points = staged(n_points, cb->d_n, (size_t)batch, on_device, s->stream);
  a.times = staged(times, cb->d_times, (size_t)batch * P, on_device, s->stream);
  a.states = staged(states, cb->d_states, (size_t)batch * P * NX, on_device, s->stream);
  hipLaunchKernelGGL(k_command_store, dim3(batch), dim3(64), 0, s->stream, a);
  HIP_CHECK(hipGetLastError());
  if (!on_device) HIP_CHECK(hipStreamSynchronize(s->stream));   // the caller's host arrays
}

// the stored trajectory of one robot (synchronises)
void get_targets(bpmpc_command_batch* cb, int robot, double* times, double* states, int capacity, int* n_points) {
  const char* who = "bpmpc_command_batch_get_targets";
  if (!times || !states || !n_points || capacity < 0) throw std::invalid_argument(std::string(who) + ": null or invalid argument");
  if (robot < 0 || robot >= cb->max_batch) throw std::invalid_argument(std::string(who) + ": robot out of range");
  bpmpc_solver* s = cb->solver;
  int st[kCommandStatus];
  HIP_CHECK(hipMemcpyAsync(st, cb->status + (size_t)robot * kCommandStatus, sizeof(st), hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
  const int n = st[3];
  *n_points = n;
  if (n > capacity) throw std::length_error(std::string(who) + ": the robot's trajectory has " + std::to_string(n) + " points, capacity is " + std::to_string(capacity));
  if (n < 1) return;
  HIP_CHECK(hipMemcpyAsync(times, cb->times + (size_t)robot * cb->max_points, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipMemcpyAsync(states, cb->states + (size_t)robot * cb->max_points * cb->nx, (size_t)n * cb->nx * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
}

}  // namespace

namespace bpmpc {

void launch_command_window(bpmpc_solver* s, int batch, double horizon) {
  const bpmpc_command_batch* cb = s->commands;
  Buffers& bf = s->buf;
  CommandWindowArgs a{};
  a.store = store_of(cb);
  a.batch = batch; a.horizon = horizon; a.t0 = bf.p_t0;
  a.tgt_t = bf.p_tgt_t; a.tgt_x = bf.p_tgt_x; a.tgt_n = bf.p_tgt_n; a.flag = s->tgt_flag;
  hipLaunchKernelGGL(k_command_window, dim3((batch + 63) / 64), dim3(64), 0, s->stream, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace bpmpc

extern "C" {

int bpmpc_command_batch_create(bpmpc_solver* s, int max_points, bpmpc_command_batch** out) {
  if (!out) { set_last_error("bpmpc_command_batch_create: null output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  if (!s) { set_last_error("bpmpc_command_batch_create: null solver handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  std::unique_ptr<bpmpc_command_batch> cb(new bpmpc_command_batch);
  const int rc = guarded(BPMPC_ERR_IO, [&] {
    if (max_points < kCommandMinPoints || max_points > kCommandMaxPoints)
      throw std::invalid_argument("bpmpc_command_batch_create: max_points " + std::to_string(max_points) + " is outside " + std::to_string(kCommandMinPoints) + " .. " +
                                  std::to_string(kCommandMaxPoints));
    HIP_CHECK(hipSetDevice(s->settings.device));
    const size_t B = s->settings.max_batch, P = max_points, NX = s->nx;
    cb->solver = s; cb->max_batch = (int)B; cb->max_points = max_points; cb->nx = (int)NX;
    DeviceBuffers& m = cb->mem;
    cb->status = m.alloc<int>(B * kCommandStatus, true);
    cb->times = m.alloc<double>(B * P, true);
    cb->states = m.alloc<double>(B * P * NX, true);
    cb->d_mask = m.alloc<int>(B); cb->d_n = m.alloc<int>(B); cb->d_t = m.alloc<double>(B); cb->d_cmd = m.alloc<double>(B * 4); cb->d_x = m.alloc<double>(B * NX);
    cb->d_times = m.alloc<double>(B * P); cb->d_states = m.alloc<double>(B * P * NX);
  });
  if (rc != BPMPC_OK) { bpmpc_command_batch_destroy(cb.release()); return rc; }
  *out = cb.release();
  return BPMPC_OK;
}
void bpmpc_command_batch_destroy(bpmpc_command_batch* cb) {
  if (!cb) return;
  if (cb->solver && cb->solver->commands == cb) cb->solver->commands = nullptr;
  if (cb->solver && cb->solver->stream) (void)hipStreamSynchronize(cb->solver->stream);
  cb->mem.release();
  delete cb;
}
int bpmpc_command_batch_reset(bpmpc_command_batch* cb) {
  if (!cb) { set_last_error("bpmpc_command_batch_reset: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(cb->solver, [&] { HIP_CHECK(hipMemsetAsync(cb->status, 0, (size_t)cb->max_batch * kCommandStatus * sizeof(int), cb->solver->stream)); });
}
int bpmpc_command_batch_start(bpmpc_command_batch* cb, int batch, const int* mask, const double* t_obs, const double* x_obs, int inputs_on_device) {
  if (!cb) { set_last_error("bpmpc_command_batch_start: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(cb->solver, [&] { message(cb, "bpmpc_command_batch_start", kCommandStart, batch, mask, nullptr, t_obs, x_obs, 0.0, inputs_on_device != 0); });
}
int bpmpc_command_batch_cmd_vel(bpmpc_command_batch* cb, int batch, const int* mask, const double* cmd, const double* t_obs, const double* x_obs,
                                double time_to_target, int inputs_on_device) {
  if (!cb) { set_last_error("bpmpc_command_batch_cmd_vel: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(cb->solver, [&] { message(cb, "bpmpc_command_batch_cmd_vel", kCommandVelocity, batch, mask, cmd, t_obs, x_obs, time_to_target, inputs_on_device != 0); });
}
int bpmpc_command_batch_goal(bpmpc_command_batch* cb, int batch, const int* mask, const double* goal, const double* t_obs, const double* x_obs, int inputs_on_device) {
  if (!cb) { set_last_error("bpmpc_command_batch_goal: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(cb->solver, [&] { message(cb, "bpmpc_command_batch_goal", kCommandGoal, batch, mask, goal, t_obs, x_obs, 0.0, inputs_on_device != 0); });
}
int bpmpc_command_batch_set_targets(bpmpc_command_batch* cb, int batch, const int* mask, const int* n_points, const double* times, const double* states,
                                    int inputs_on_device) {
  if (!cb) { set_last_error("bpmpc_command_batch_set_targets: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(cb->solver, [&] { set_targets(cb, batch, mask, n_points, times, states, inputs_on_device != 0); });
}
int bpmpc_command_batch_get_targets(bpmpc_command_batch* cb, int robot, double* times, double* states, int capacity, int* n_points) {
  if (!cb) { set_last_error("bpmpc_command_batch_get_targets: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(cb->solver, [&] { get_targets(cb, robot, times, states, capacity, n_points); });
}
int bpmpc_command_batch_get_status(bpmpc_command_batch* cb, int batch, int* status) {
  if (!cb) { set_last_error("bpmpc_command_batch_get_status: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(cb->solver, [&] {
    check_batch(cb, "bpmpc_command_batch_get_status", batch);
    if (!status) throw std::invalid_argument("bpmpc_command_batch_get_status: null argument");
    HIP_CHECK(hipMemcpyAsync(status, cb->status, (size_t)batch * kCommandStatus * sizeof(int), hipMemcpyDeviceToHost, cb->solver->stream));
    HIP_CHECK(hipStreamSynchronize(cb->solver->stream));
  });
}
int bpmpc_solver_attach_commands(bpmpc_solver* s, bpmpc_command_batch* cb) {
  return guarded(s, [&] {
    if (cb && cb->solver != s) throw std::invalid_argument("bpmpc_solver_attach_commands: the command batch belongs to another solver");
    s->commands = cb;
  });
}

}  // extern "C"
