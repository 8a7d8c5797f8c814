// k_supervise (kernels/supervisor.h) and the host side of its handle: the C ABI of include/bpmpc.h "Supervisor".
//   InitialJointPositionController     bipedal_controllers/src/InitialJointController.cpp:110-141
//   SafetyChecker, stopRequest         SafetyChecker.h:39-52, BipedalController.cpp:232-236
//   the switch script                  bipedal_controllers/script/switch_joint_init_pos_controller.py   (bpmpc_supervisor_request)
// A translation unit of its own: every other kernel is compiled as it was before this unit existed, and a loop that never creates a
// bpmpc_supervisor launches nothing of it.  bpmpc_plant_step_supervised lives with the plant's steps (plant.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "estimator.h"
#include "info_tree.h"
#include "plant.h"
#include "supervisor.h"

namespace bpmpc {

__global__ __launch_bounds__(64) void k_supervise(SupervisorArgs a) { supervise_group(a); }

// bpmpc_supervisor_request for the robots of `mask` (NULL: every robot below `batch`), one thread per robot
__global__ __launch_bounds__(256) void k_supervisor_request(int batch, const int* mask, int target, int only_ready, int* state, int* cause, int* ready,
                                                            int* latch, double* elapsed, double* settled) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch || (mask && !mask[b])) return;
  SupRobot r{state[b], cause[b], 0, ready[b], latch[b], elapsed[b], settled[b]};
  sup_request(r, target, only_ready);      // a RUN request that does not apply leaves r as it was read
  state[b] = r.state; cause[b] = r.cause; ready[b] = r.ready; latch[b] = r.latch; elapsed[b] = r.elapsed; settled[b] = r.settled;
}

}  // namespace bpmpc

using namespace bpmpc;

namespace {

const char* const kParamNames[] = {"tilt_limit", "min_base_height", "ramp_time", "settle_pos_tol", "settle_vel_tol", "settle_time", "stop_kd"};
const char* const kJointRowNames[] = {"q_init", "kp_init", "kd_init", "lower", "upper"};
static_assert(sizeof(kParamNames) / sizeof(kParamNames[0]) == kSupParamUsed, "a name per used entry of a parameter row");

// A host row before it is accepted: every used entry finite and not negative, tilt_limit positive
void check_param_row(const char* who, const double* row, int r) {
  for (int e = 0; e < kSupParamUsed; ++e) {
    const char* why = !std::isfinite(row[e]) ? "not finite" : row[e] < 0.0 ? "negative" : (e == kSupTiltLimit && row[e] == 0.0) ? "zero" : nullptr;
    if (why) throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", entry " + std::to_string(e) + " (" + kParamNames[e] + ") is " + why);
  }
}

// The keys supervisor.<name> of task.info over the defaults (NULL: the defaults)
void load_settings(const char* task_info_path, double* row) {
  const double start[kSupParamStride] = {M_PI / 3.0 /* SafetyChecker.h:41 */, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  std::copy(start, start + kSupParamStride, row);
  if (task_info_path) {
    const auto t = read_info_file(task_info_path);
    for (int e = 0; e < kSupParamUsed; ++e) (void)t->get(std::string("supervisor.") + kParamNames[e], row + e);
    check_param_row("supervisor settings", row, 0);
  }
}

// A host joint row before it is accepted: q_init finite; the gains finite and not negative; a limit may be infinite but is a number
void check_joint_row(const char* who, int which, const double* row, int r, int nj) {
  for (int j = 0; j < nj; ++j) {
    const double x = row[j];
    const char* why = which >= 3 ? (std::isnan(x) ? "not a number" : nullptr) : !std::isfinite(x) ? "not finite" : (which != 0 && x < 0.0) ? "negative" : nullptr;
    if (why) throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", entry " + std::to_string(j) + " (" + kJointRowNames[which] + ") is " + why);
  }
}

void check_batch(const bpmpc_supervisor* s, int batch, const char* who) {
  if (batch < 1) throw std::invalid_argument(std::string(who) + ": batch must be positive");
  if (batch > s->max_batch) throw std::length_error(std::string(who) + ": batch exceeds max_batch");
}

void check_period(double period, const char* who) {
  if (!std::isfinite(period) || period <= 0.0) throw std::invalid_argument(std::string(who) + ": period must be finite and positive");
}

void request_on_device(bpmpc_supervisor* s, int batch, const int* mask, int target, int only_ready) {
  hipLaunchKernelGGL(k_supervisor_request, dim3((batch + 255) / 256), dim3(256), 0, s->hs.stream, batch, mask, target, only_ready, s->d_state, s->d_cause,
                     s->d_ready, s->d_latch, s->d_elapsed, s->d_settled);
  HIP_CHECK(hipGetLastError());
}

// the counters zeroed and one launch of k_supervise on the handle's stream; run[0] == nullptr: no RUN command
void launch(bpmpc_supervisor* s, int batch, const double* rbd, const double* const run[5], int cmd_stride, double period) {
  SupervisorArgs a{};
  a.batch = batch; a.nj = s->nj; a.cmd_stride = cmd_stride; a.period = period; a.rbd = rbd;
  a.run_pos = run[0]; a.run_vel = run[1]; a.run_tau = run[2]; a.run_kp = run[3]; a.run_kd = run[4];
  a.params = s->params.d_params;
  a.q_init = s->d_joint[0]; a.kp_init = s->d_joint[1]; a.kd_init = s->d_joint[2]; a.lower = s->d_joint[3]; a.upper = s->d_joint[4];
  a.state = s->d_state; a.cause = s->d_cause; a.unsafe = s->d_unsafe; a.ready = s->d_ready; a.latch = s->d_latch; a.counts = s->d_counts;
  a.elapsed = s->d_elapsed; a.settled = s->d_settled; a.q_latch = s->d_qlatch;
  a.pos_des = s->d_cmd[0]; a.vel_des = s->d_cmd[1]; a.tau_ff = s->d_cmd[2]; a.kp = s->d_cmd[3]; a.kd = s->d_cmd[4];
  HIP_CHECK(hipMemsetAsync(s->d_counts, 0, kSupCounts * sizeof(int), s->hs.stream));
  constexpr int RPW = 64 / kSupGroup;
  hipLaunchKernelGGL(k_supervise, dim3((batch + RPW - 1) / RPW), dim3(64), 0, s->hs.stream, a);
  HIP_CHECK(hipGetLastError());
}

// the default joint rows of a model: defaultJointState; the start-up values of InitialJointControllerParams.cfg (kp 80, kd 5, kd 3 for the
// sixth motor of a six-motor leg); the URDF limits
void default_joint_rows(const RobotModel& rm, double* rows) {
  const int nj = rm.nj;
  for (int j = 0; j < nj; ++j) {
    rows[j] = rm.default_joint_state[j];
    rows[nj + j] = 80.0;
    rows[2 * nj + j] = (nj == 12 && j % 6 == 5) ? 3.0 : 5.0;
    rows[3 * nj + j] = rm.joint_lower[j + 1];
    rows[4 * nj + j] = rm.joint_upper[j + 1];
  }
}

}  // namespace

extern "C" {

int bpmpc_supervisor_create(const bpmpc_model* model, const char* task_info_path, int device, int max_batch, bpmpc_supervisor** out) {
  if (!model || !out) { set_last_error("bpmpc_supervisor_create: null model or output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  if (max_batch < 1) { set_last_error("bpmpc_supervisor_create: max_batch must be positive"); return BPMPC_ERR_INVALID_ARGUMENT; }
  std::unique_ptr<bpmpc_supervisor> s(new bpmpc_supervisor);
  const int rc = guarded(BPMPC_ERR_IO, [&]() -> int {
    if (const int refused = open_side_handle("bpmpc_supervisor_create", s.get(), model, device, max_batch)) return refused;
    load_settings(task_info_path, s->defaults);
    s->nj = s->rm.nj; s->nv = 6 + s->nj;
    const size_t B = max_batch, nj = s->nj;
    DeviceBuffers& m = s->mem;
    s->params.create(m, max_batch, kSupParamStride, kSupParamUsed, s->defaults);
    s->d_joint_defaults = m.alloc<double>(5 * nj); s->d_joint_rows = m.alloc<double>(B * nj); s->d_mask = m.alloc<int>(B);
    s->d_state = m.alloc<int>(B, true); s->d_cause = m.alloc<int>(B, true); s->d_unsafe = m.alloc<int>(B, true); s->d_ready = m.alloc<int>(B, true);
    s->d_latch = m.alloc<int>(B, true); s->d_counts = m.alloc<int>(kSupCounts, true);
    s->d_elapsed = m.alloc<double>(B, true); s->d_settled = m.alloc<double>(B, true); s->d_qlatch = m.alloc<double>(B * nj, true);
    s->d_rbd = m.alloc<double>(B * 2 * s->nv);
    for (int k = 0; k < 5; ++k) { s->d_joint[k] = m.alloc<double>(B * nj); s->d_cmd[k] = m.alloc<double>(B * nj, true); s->d_run[k] = m.alloc<double>(B * nj); }
    std::vector<double> rows(5 * nj);
    default_joint_rows(s->rm, rows.data());
    HIP_CHECK(hipMemcpy(s->d_joint_defaults, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipDeviceSynchronize());      // the zero fills run on the null stream
    s->params.fill_from_start(s->hs.stream, max_batch);
    for (int k = 0; k < 5; ++k) write_rows(s->hs.stream, max_batch, s->nj, s->nj, nullptr, 1, {s->d_joint_defaults + k * nj, nullptr, s->d_joint[k]});
    request_on_device(s.get(), max_batch, nullptr, kSupInit, 0);      // every robot in INIT, its latch pending
    s->hs.synchronise_own();
    return BPMPC_OK;
  });
  if (rc != BPMPC_OK) { bpmpc_supervisor_destroy(s.release()); return rc; }
  *out = s.release();
  return BPMPC_OK;
}

void bpmpc_supervisor_destroy(bpmpc_supervisor* s) {
  if (!s) return;
  if (s->hs.stream) { (void)hipSetDevice(s->device); (void)hipDeviceSynchronize(); }      // a plant step may still read the commands on the plant's stream
  if (s->ev_in) (void)hipEventDestroy(s->ev_in);
  close_side_handle(s);
}

int bpmpc_supervisor_get_params(const bpmpc_supervisor* s, int robot, double* row) {
  return guarded(s, BPMPC_ERR_IO, "bpmpc_supervisor_get_params: null handle or row", row != nullptr, [&] {
    s->params.get("bpmpc_supervisor_get_params", s->hs.stream, s->max_batch, robot, row);
  });
}

int bpmpc_supervisor_set_params(bpmpc_supervisor* s, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  return guarded(s, BPMPC_ERR_IO, "bpmpc_supervisor_set_params: null handle or rows", rows != nullptr, [&] {
    check_batch(s, batch, "bpmpc_supervisor_set_params");
    s->params.set("bpmpc_supervisor_set_params", s->hs.stream, batch, mask, s->d_mask, rows, n_rows, inputs_on_device != 0,
                  [](const double* row, int r) { check_param_row("bpmpc_supervisor_set_params", row, r); });
    s->hs.finish(inputs_on_device != 0);
  });
}

int bpmpc_supervisor_reset_params(bpmpc_supervisor* s) {
  return guarded(s, BPMPC_ERR_IO, "bpmpc_supervisor_reset_params: null handle", [&] {
    s->params.fill_from_start(s->hs.stream, s->max_batch);
    s->hs.synchronise_own();
  });
}

int bpmpc_supervisor_load_params(const char* task_info_path, double* row) {
  if (!row) { set_last_error("bpmpc_supervisor_load_params: null row"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] { load_settings(task_info_path, row); });
}

int bpmpc_supervisor_check_params(const double* rows, int n_rows) {
  if (!rows) { set_last_error("bpmpc_supervisor_check_params: null rows"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    for (int r = 0; r < n_rows; ++r) check_param_row("bpmpc_supervisor_check_params", rows + (size_t)r * kSupParamStride, r);
  });
}

int bpmpc_supervisor_set_joint_rows(bpmpc_supervisor* s, int batch, const int* mask, int which, const double* rows, int n_rows, int inputs_on_device) {
  return guarded(s, BPMPC_ERR_IO, "bpmpc_supervisor_set_joint_rows: null handle or rows", rows != nullptr, [&] {
    const char* who = "bpmpc_supervisor_set_joint_rows";
    check_batch(s, batch, who);
    if (which < 0 || which > 4) throw std::invalid_argument(std::string(who) + ": which must be 0 (q_init), 1 (kp_init), 2 (kd_init), 3 (lower) or 4 (upper)");
    const int nj = s->nj;
    std::vector<double> other;      // host rows of a limit are held against the robots' other limit
    if (!inputs_on_device && which >= 3 && (n_rows == 1 || n_rows == batch)) {
      other.resize((size_t)batch * nj);
      HIP_CHECK(hipMemcpyAsync(other.data(), s->d_joint[7 - which], other.size() * sizeof(double), hipMemcpyDeviceToHost, s->hs.stream));
      s->hs.synchronise_own();
    }
    set_rows(who, s->hs.stream, batch, nj, nj, mask, s->d_mask, n_rows, inputs_on_device != 0,
             [&](int r) {
               const double* row = rows + (size_t)r * nj;
               check_joint_row(who, which, row, r, nj);
               if (which < 3) return;
               for (int b = (n_rows == 1 ? 0 : r); b < (n_rows == 1 ? batch : r + 1); ++b) {
                 if (mask && !mask[b]) continue;
                 for (int j = 0; j < nj; ++j) {
                   const double lo = which == 3 ? row[j] : other[(size_t)b * nj + j], up = which == 4 ? row[j] : other[(size_t)b * nj + j];
                   if (!(lo <= up))
                     throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", entry " + std::to_string(j) + " (" + kJointRowNames[which] +
                                                 "): lower exceeds upper for robot " + std::to_string(b));
                 }
               }
             },
             {rows, s->d_joint_rows, s->d_joint[which]});
    s->hs.finish(inputs_on_device != 0);
  });
}

int bpmpc_supervisor_get_joint_rows(const bpmpc_supervisor* s, int robot, int which, double* row) {
  return guarded(s, BPMPC_ERR_IO, "bpmpc_supervisor_get_joint_rows: null handle or row", row != nullptr, [&] {
    if (which < 0 || which > 4) throw std::invalid_argument("bpmpc_supervisor_get_joint_rows: which must be 0 (q_init), 1 (kp_init), 2 (kd_init), 3 (lower) or 4 (upper)");
    if (robot >= s->max_batch) throw std::length_error("bpmpc_supervisor_get_joint_rows: robot exceeds max_batch");
    const double* src = robot < 0 ? s->d_joint_defaults + (size_t)which * s->nj : s->d_joint[which] + (size_t)robot * s->nj;
    HIP_CHECK(hipMemcpyAsync(row, src, s->nj * sizeof(double), hipMemcpyDeviceToHost, s->hs.stream));
    HIP_CHECK(hipStreamSynchronize(s->hs.stream));
  });
}

int bpmpc_supervisor_request(bpmpc_supervisor* s, int batch, const int* mask, int target, int only_ready, int inputs_on_device) {
  return guarded(s, BPMPC_ERR_DEVICE, "bpmpc_supervisor_request: null supervisor handle", [&] {
    check_batch(s, batch, "bpmpc_supervisor_request");
    if (target < 0 || target > 2) throw std::invalid_argument("bpmpc_supervisor_request: target must be 0 (INIT), 1 (RUN) or 2 (STOPPED)");
    request_on_device(s, batch, staged(mask, s->d_mask, batch, inputs_on_device != 0, s->hs.stream), target, only_ready);
    if (mask && !inputs_on_device) s->hs.synchronise_own();      // the caller's host mask
    else s->hs.enqueued_own();
  });
}

int bpmpc_supervisor_update(bpmpc_supervisor* s, int batch, const double* rbd, const bpmpc_joint_command* c, int inputs_on_device, double period) {
  return guarded(s, BPMPC_ERR_DEVICE, "bpmpc_supervisor_update: null handle or rbd, or a run_cmd with a null member",
                 rbd && (!c || (c->pos_des && c->vel_des && c->tau_ff && c->kp && c->kd)), [&] {
    check_batch(s, batch, "bpmpc_supervisor_update");
    check_period(period, "bpmpc_supervisor_update");
    hipStream_t st = s->hs.stream;
    const bool dev = inputs_on_device != 0;
    const size_t B = batch, nj = s->nj;
    const double* run[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (c) {
      const double* src[5] = {c->pos_des, c->vel_des, c->tau_ff, c->kp, c->kd};
      for (int k = 0; k < 5; ++k) run[k] = staged(src[k], s->d_run[k], B * nj, dev, st);
    }
    launch(s, batch, staged(rbd, s->d_rbd, B * 2 * s->nv, dev, st), run, s->nj, period);
    s->hs.finish(dev);      // host arrays are the caller's; a plant step on the plant's stream waits for an update that was only enqueued
  });
}

// One update on the controller's last tick, read where the tick wrote it, and on the estimator's rbd: the supervisor's stream waits for the
// tick and for an estimator update that was only enqueued; the controller's stream and the estimator's wait for this update before the next
// tick and the next estimate overwrite what it read
int bpmpc_supervisor_update_controlled(bpmpc_supervisor* s, bpmpc_controller* controller, bpmpc_estimator* estimator, const double* rbd_dev, int batch,
                                       double period) {
  return guarded(s, BPMPC_ERR_DEVICE, "bpmpc_supervisor_update_controlled: null supervisor or controller, or neither estimator nor rbd_dev",
                 controller && (estimator || rbd_dev), [&] {
    const char* who = "bpmpc_supervisor_update_controlled";
    const ControllerCommands cc = controller_commands(controller);
    if (cc.nj != s->nj || (estimator && estimator->nj != s->nj)) throw std::invalid_argument(std::string(who) + ": the handles are built for different robots");
    if (cc.device != s->device || (estimator && estimator->device != s->device)) throw std::invalid_argument(std::string(who) + ": the handles live on different devices");
    check_batch(s, batch, who);
    check_period(period, who);
    if (cc.last_tick_batch == 0) throw std::invalid_argument(std::string(who) + ": the controller has not ticked yet: there are no joint commands");
    if (batch != cc.last_tick_batch)
      throw std::invalid_argument(std::string(who) + ": batch " + std::to_string(batch) + " differs from the batch of the controller's last tick (" +
                                  std::to_string(cc.last_tick_batch) + ")");
    hipStream_t st = s->hs.stream;
    StreamHandshake::record(&s->ev_in, cc.stream);
    HIP_CHECK(hipStreamWaitEvent(st, s->ev_in, 0));
    if (estimator) estimator_before_foreign_read(estimator, batch, st);
    const double* run[5] = {cc.joint_cmd, cc.joint_cmd + s->nj, cc.joint_cmd + 2 * s->nj, cc.kp, cc.kd};
    launch(s, batch, estimator ? estimator->d_rbd : rbd_dev, run, 3 * s->nj, period);
    s->hs.enqueued_own();
    HIP_CHECK(hipStreamWaitEvent(cc.stream, s->hs.ev_own, 0));
    if (estimator) estimator_after_foreign_read(estimator, st);
  });
}

int bpmpc_supervisor_device_outputs(bpmpc_supervisor* s, bpmpc_supervisor_outputs* o) {
  if (!s || !o) { set_last_error("bpmpc_supervisor_device_outputs: null supervisor handle or output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  o->pos_des = s->d_cmd[0]; o->vel_des = s->d_cmd[1]; o->tau_ff = s->d_cmd[2]; o->kp = s->d_cmd[3]; o->kd = s->d_cmd[4];
  o->state = s->d_state; o->cause = s->d_cause; o->unsafe = s->d_unsafe; o->ready = s->d_ready; o->counts = s->d_counts;
  o->elapsed = s->d_elapsed; o->stream = s->hs.stream;
  return BPMPC_OK;
}

int bpmpc_supervisor_get_state(bpmpc_supervisor* s, int batch, int* state, int* cause, int* unsafe, int* ready, double* elapsed, int* counts) {
  return guarded(s, BPMPC_ERR_DEVICE, "bpmpc_supervisor_get_state: null supervisor handle", [&] {
    check_batch(s, batch, "bpmpc_supervisor_get_state");
    hipStream_t st = s->hs.stream;
    auto down = [&](void* dst, const void* src, size_t bytes) { if (dst) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); };
    const size_t B = batch;
    down(state, s->d_state, B * sizeof(int)); down(cause, s->d_cause, B * sizeof(int)); down(unsafe, s->d_unsafe, B * sizeof(int));
    down(ready, s->d_ready, B * sizeof(int)); down(elapsed, s->d_elapsed, B * sizeof(double)); down(counts, s->d_counts, kSupCounts * sizeof(int));
    s->hs.synchronise_own();
  });
}

int bpmpc_supervisor_get_commands(bpmpc_supervisor* s, int batch, double* pos_des, double* vel_des, double* tau_ff, double* kp, double* kd) {
  return guarded(s, BPMPC_ERR_DEVICE, "bpmpc_supervisor_get_commands: null supervisor handle", [&] {
    check_batch(s, batch, "bpmpc_supervisor_get_commands");
    double* dst[5] = {pos_des, vel_des, tau_ff, kp, kd};
    for (int k = 0; k < 5; ++k)
      if (dst[k]) HIP_CHECK(hipMemcpyAsync(dst[k], s->d_cmd[k], (size_t)batch * s->nj * sizeof(double), hipMemcpyDeviceToHost, s->hs.stream));
    s->hs.synchronise_own();
  });
}

int bpmpc_supervisor_rows_host(const bpmpc_model* model, const double* params, const double* joint_rows, const double* rbd, const bpmpc_joint_command* c,
                               double period, int* flags, double* clocks, double* q_latch, double* command) {
  if (!model || !params || !joint_rows || !rbd || !flags || !clocks || !q_latch || !command || (c && !(c->pos_des && c->vel_des && c->tau_ff && c->kp && c->kd))) {
    set_last_error("bpmpc_supervisor_rows_host: null model, params, joint_rows, rbd, flags, clocks, q_latch or command, or a run_cmd with a null member");
    return BPMPC_ERR_INVALID_ARGUMENT;
  }
  return guarded(BPMPC_ERR_IO, [&] {
    const int nj = model_of(model).nj;
    if (nj > kSupMaxJoints) throw Unsupported("bpmpc_supervisor_rows_host: more joints than a robot's lanes carry");
    check_period(period, "bpmpc_supervisor_rows_host");
    SupRobot r{flags[0], flags[1], 0, flags[3], flags[4], clocks[0], clocks[1]};
    double q[kSupGroup], v[kSupGroup];
    SupCommand run[kSupGroup] = {};
    int bits = 0;
    for (int g = 0; g < kSupGroup; ++g) {
      bits |= sup_lane_measure(g, nj, rbd, q + g, v + g);
      if (r.state != kSupRun) continue;
      if (!c) bits |= kSupBitCommand;
      else if (g < nj) bits |= sup_lane_run_command(c->pos_des + g, c->vel_des + g, c->tau_ff + g, c->kp + g, c->kd + g, run + g);
    }
    sup_transition(r, bits | sup_limit_bits(params, rbd[2], rbd[1], rbd[5]), period);
    const double s = sup_ramp(params, r.elapsed);
    bool breaks = false;
    for (int g = 0; g < nj; ++g) {
      SupCommand out{};
      const bool lane_breaks = sup_lane_command(r, params, s, q[g], v[g], run[g], joint_rows[g], joint_rows[nj + g], joint_rows[2 * nj + g], joint_rows[3 * nj + g],
                                                joint_rows[4 * nj + g], q_latch + g, &out);
      breaks = breaks || lane_breaks;
      command[g] = out.pos; command[nj + g] = out.vel; command[2 * nj + g] = out.tau; command[3 * nj + g] = out.kp; command[4 * nj + g] = out.kd;
    }
    sup_finish(r, params, s, breaks, period);
    flags[0] = r.state; flags[1] = r.cause; flags[2] = r.unsafe; flags[3] = r.ready; flags[4] = r.latch;
    clocks[0] = r.elapsed; clocks[1] = r.settled;
  });
}

}  // extern "C"
