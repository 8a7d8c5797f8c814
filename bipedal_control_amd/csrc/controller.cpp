// Host side of the controller tick (kernels/tick.h, k_tick.hip) and of MRT_BASE::evaluatePolicy: the C ABI of include/bpmpc.h.
//   BipedalController::update          bipedal_controllers/src/BipedalController.cpp:186-262
//   observation                         :397-403 (computeCentroidalStateFromRbdModel, yaw unwrap)
//   evaluatePolicy / WBC / safety       :199, :229, SafetyChecker.h:39-52;  commands :237-252
// One tick = k_tick_observe_policy, k_wbc (the WBC handle's kernel and its per-robot last solutions), k_tick_commands, all on the solver's
// stream; nothing is synchronised unless outputs are asked for on the host.  k_tick_commands also forms joint_torque from the per-robot joint
// gains of dynamicReconfigCallback (:423-472, bpmpc_controller_set_joint_gains).
// A restart (BipedalController::starting, :123-179) for the robots of a mask = k_restart_observe, bpmpc_solver_restart with the observations,
// k_wbc_restart, on the same stream.
// With a policy buffer attached (bpmpc_controller_attach_policy, policy.h) the stream of all of this is the buffer's, controller_stream, and the
// tick evaluates the buffer's front slot instead of the solver's working arrays; what the solver's stream shares with it is ordered by events.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>

#include "estimator.h"
#include "plant.h"
#include "policy.h"
#include "solver.h"
#include "telemetry.h"
#include "wbc.h"
#include "kernels/tick.h"

using namespace bpmpc;

struct bpmpc_controller {
  bpmpc_solver* s = nullptr;
  bpmpc_wbc* w = nullptr;
  int device = 0, max_batch = 0, nj = 0, nx = 0, nv = 0, n = 0;
  DeviceBuffers mem;      // every d_* below
  double *d_yaw = nullptr, *d_t = nullptr, *d_rbd = nullptr, *d_xobs = nullptr, *d_xopt = nullptr, *d_uopt = nullptr, *d_cmd = nullptr;
  int *d_mode = nullptr, *d_safe = nullptr, *d_mask = nullptr;
  double *d_kp = nullptr, *d_kd = nullptr, *d_torque = nullptr;      // [max_batch][nj]: joint gains (0 after create), the last tick's joint_torque
  double *d_kp_in = nullptr, *d_kd_in = nullptr;                     // device copies of host gain rows
  int last_tick_batch = 0;                                           // rows of d_cmd that hold the commands of a tick (0: no tick yet)
  bpmpc_policy* p = nullptr;                                         // the attached policy buffer (NULL: ticks read the solver's arrays on its stream)
  bpmpc_telemetry* tel = nullptr;                                    // the attached tracking telemetry (NULL: a tick is its three launches and nothing else)
};

namespace {

TickArgs policy_args(const bpmpc_solver* s, int batch) {
  const Buffers& bf = s->buf;
  TickArgs a{};
  a.batch = batch; a.N = s->settings.max_nodes; a.feedback = s->feedback();
  a.p_grid = bf.p_grid; a.g_nodes = bf.g_nodes; a.g_kind = bf.g_kind; a.g_mode = bf.g_mode; a.g_time = bf.g_time; a.x = bf.x; a.u = bf.u; a.K = bf.K;
  return a;
}

// ... of the front slot of a policy buffer: the same strides, a grid row per robot
TickArgs policy_args(const bpmpc_policy* p, int batch) {
  const PolicySlot& sl = p->slot[p->front];
  TickArgs a{};
  a.batch = batch; a.N = p->N; a.feedback = p->feedback;
  a.p_grid = p->d_identity; a.g_nodes = sl.g_nodes; a.g_kind = sl.g_kind; a.g_mode = sl.g_mode; a.g_time = sl.g_time; a.x = sl.x; a.u = sl.u; a.K = sl.K;
  return a;
}

// the stream of everything the controller enqueues: the attached policy buffer's, else the solver's
hipStream_t controller_stream(const bpmpc_controller* c) { return c->p ? c->p->hs.stream : c->s->stream; }

// work was enqueued on controller_stream and the call returns without a synchronise: what the solver's stream shares with a buffered controller waits for it
void enqueued(bpmpc_controller* c) { if (c->p) c->p->hs.enqueued_own(); }

// the controller leaves its policy buffer; the last one to leave takes the buffer's handshake off the solver
void detach(bpmpc_controller* c) {
  if (!c->p) return;
  if (--c->p->attached == 0 && c->s->tick_hs == &c->p->hs) c->s->tick_hs = nullptr;
  c->p = nullptr;
}

// the refusals of a tick: a completed run of an SQP solver since the last setup, the batch of that setup, the WBC's capacity; buffered: an adopted
// policy for every robot, the batch of that policy
void check_tick(const bpmpc_controller* c, int batch, const char* who) {
  if (c->p) check_buffered_tick(c->p, batch, who);
  else {
    check_policy(c->s);
    if (batch != c->s->batch) throw std::invalid_argument(std::string(who) + ": batch differs from the batch of the solver's last setup");
  }
  if (batch > c->max_batch) throw std::length_error(std::string(who) + ": batch exceeds the WBC's max_batch");
  if (c->tel && batch > c->tel->max_batch) throw std::length_error(std::string(who) + ": batch exceeds the attached telemetry's max_batch");
}

// the three launches of a tick on the controller's stream, from device inputs
void enqueue_tick(bpmpc_controller* c, int batch, const double* dt, const double* drbd) {
  bpmpc_solver* s = c->s;
  hipStream_t st = controller_stream(c);
  TickArgs a = c->p ? policy_args(c->p, batch) : policy_args(s, batch);
  a.t = dt; a.rbd = drbd; a.yaw_last = c->d_yaw; a.x_obs = c->d_xobs; a.x_loop = s->tick_x; a.safe = c->d_safe;
  a.x_opt = c->d_xopt; a.u_opt = c->d_uopt; a.mode = c->d_mode;
  kl::tick_observe_policy(c->nj, batch, st, s->d_model, a);
  HIP_CHECK(hipGetLastError());
  s->loop_from_tick = true;          // the next setup_commands(x0 = NULL) starts from tick_x (until the next rollout)
  wbc_launch_on(c->w, batch, c->d_xopt, c->d_uopt, drbd, c->d_mode, st);
  TickCommandArgs ca{};
  ca.batch = batch; ca.x_opt = c->d_xopt; ca.u_opt = c->d_uopt; ca.sol = c->w->d_sol; ca.rbd = drbd; ca.kp = c->d_kp; ca.kd = c->d_kd;
  ca.cmd = c->d_cmd; ca.joint_torque = c->d_torque;
  kl::tick_commands(c->nj, st, ca);
  HIP_CHECK(hipGetLastError());
  // DebugPublisher::update (:270) behind the commands, on the tick's own device buffers
  if (c->tel) telemetry_launch_on(c->tel, batch, dt, c->d_xopt, drbd, c->d_safe, c->d_mode, st);
  c->last_tick_batch = batch;
  enqueued(c);
}

// the host copies of a tick's outputs (host_out NULL: nothing is copied or synchronised)
void fetch_tick(bpmpc_controller* c, int batch, const bpmpc_tick_outputs* host_out) {
  if (!host_out) return;
  hipStream_t st = controller_stream(c);
  const size_t B = batch;
  const bpmpc_tick_outputs& o = *host_out;
  auto down = [&](void* dst, const void* src, size_t bytes) { if (dst) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); };
  down(o.x_obs, c->d_xobs, B * c->nx * sizeof(double));
  down(o.x_opt, c->d_xopt, B * c->nx * sizeof(double));
  down(o.u_opt, c->d_uopt, B * c->nx * sizeof(double));
  down(o.joint_cmd, c->d_cmd, B * 3 * c->nj * sizeof(double));
  down(o.wbc_solution, c->w->d_sol, B * c->n * sizeof(double));
  down(o.planned_mode, c->d_mode, B * sizeof(int));
  down(o.wbc_status, c->w->d_status, B * sizeof(int));
  down(o.safe, c->d_safe, B * sizeof(int));
  HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace

namespace bpmpc {
ControllerCommands controller_commands(const bpmpc_controller* c) {
  return {controller_stream(c), c->d_cmd, c->d_kp, c->d_kd, c->nj, c->device, c->max_batch, c->last_tick_batch};
}
}  // namespace bpmpc

extern "C" {

int bpmpc_solver_evaluate_policy(bpmpc_solver* s, int batch, const double* t, const double* x, double* x_opt, double* u_opt, int* planned_mode) {
  if (!s || !t || !x || !x_opt || !u_opt || !planned_mode) { set_last_error("bpmpc_solver_evaluate_policy: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  void* block = nullptr;
  const int rc = guarded(BPMPC_ERR_DEVICE, [&] {
    check_policy(s);
    if (batch != s->batch) throw std::invalid_argument("bpmpc_solver_evaluate_policy: batch differs from the batch of the last setup");
    HIP_CHECK(hipSetDevice(s->settings.device));
    const size_t B = batch, nx = s->nx, nu = s->nu;
    const size_t bytes = B * (1 + 2 * nx + nu) * sizeof(double) + B * sizeof(int);
    HIP_CHECK(hipMalloc(&block, bytes));
    double* d_t = static_cast<double*>(block);
    double* d_x = d_t + B;
    double* d_xopt = d_x + B * nx;
    double* d_uopt = d_xopt + B * nx;
    int* d_mode = reinterpret_cast<int*>(d_uopt + B * nu);
    HIP_CHECK(hipMemcpyAsync(d_t, t, B * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_CHECK(hipMemcpyAsync(d_x, x, B * nx * sizeof(double), hipMemcpyHostToDevice, s->stream));
    TickArgs a = policy_args(s, batch);
    a.t = d_t; a.x_in = d_x; a.x_opt = d_xopt; a.u_opt = d_uopt; a.mode = d_mode;
    kl::tick_observe_policy(s->rm.nj, batch, s->stream, s->d_model, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(x_opt, d_xopt, B * nx * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipMemcpyAsync(u_opt, d_uopt, B * nu * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipMemcpyAsync(planned_mode, d_mode, B * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
  });
  if (block) (void)hipFree(block);
  return rc;
}

int bpmpc_controller_create(bpmpc_solver* s, bpmpc_wbc* w, bpmpc_controller** out) {
  if (!s || !w || !out) { set_last_error("bpmpc_controller_create: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  std::unique_ptr<bpmpc_controller> c(new bpmpc_controller);
  const int rc = guarded(BPMPC_ERR_DEVICE, [&] {
    if (s->nx != 12 + w->rm.nj) throw std::invalid_argument("bpmpc_controller_create: the solver and the WBC are built for different robots");
    if (s->settings.device != w->device) throw std::invalid_argument("bpmpc_controller_create: the solver and the WBC live on different devices");
    c->s = s; c->w = w; c->device = w->device; c->max_batch = w->max_batch; c->nj = w->rm.nj; c->nx = s->nx; c->nv = w->nv; c->n = w->n;
    HIP_CHECK(hipSetDevice(c->device));
    const size_t B = c->max_batch, nj = c->nj;
    DeviceBuffers& m = c->mem;
    c->d_yaw = m.alloc<double>(B, true);       // yawLast of BipedalController::starting: the first observation's yaw unwraps from 0
    c->d_t = m.alloc<double>(B); c->d_rbd = m.alloc<double>(B * 2 * c->nv);
    c->d_xobs = m.alloc<double>(B * c->nx); c->d_xopt = m.alloc<double>(B * c->nx); c->d_uopt = m.alloc<double>(B * c->nx); c->d_cmd = m.alloc<double>(B * 3 * nj);
    c->d_mode = m.alloc<int>(B); c->d_safe = m.alloc<int>(B); c->d_mask = m.alloc<int>(B);
    c->d_kp = m.alloc<double>(B * nj, true); c->d_kd = m.alloc<double>(B * nj, true); c->d_torque = m.alloc<double>(B * nj, true);
    c->d_kp_in = m.alloc<double>(B * nj); c->d_kd_in = m.alloc<double>(B * nj);
    HIP_CHECK(hipDeviceSynchronize());
  });
  if (rc != BPMPC_OK) { c->mem.release(); return rc; }
  *out = c.release();
  return BPMPC_OK;
}

void bpmpc_controller_destroy(bpmpc_controller* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();           // a tick may still be in flight on the solver's stream or the policy buffer's
  detach(c);
  c->mem.release();
  delete c;
}

int bpmpc_controller_reset(bpmpc_controller* c) {
  return guarded(c, BPMPC_ERR_DEVICE, "null controller handle", [&] {
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemset(c->d_yaw, 0, (size_t)c->max_batch * sizeof(double)));
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int bpmpc_controller_tick(bpmpc_controller* c, int batch, const double* t, const double* rbd, int inputs_on_device, double period,
                          const bpmpc_tick_outputs* host_out) {
  (void)period;      // WeightedWbc::update takes it and does not use it (WbcBase.cpp:242-243), as bpmpc_wbc_update
  return guarded(c, BPMPC_ERR_DEVICE, "bpmpc_controller_tick: null argument", t && rbd, [&] {
    hipStream_t st = controller_stream(c);
    check_tick(c, batch, "bpmpc_controller_tick");
    const double* dt = staged(t, c->d_t, batch, inputs_on_device, st);
    enqueue_tick(c, batch, dt, staged(rbd, c->d_rbd, (size_t)batch * 2 * c->nv, inputs_on_device, st));
    fetch_tick(c, batch, host_out);
  });
}

// bpmpc_controller_tick on the rbd the estimator holds on the device: the controller's stream waits for an update that was only enqueued, and the
// estimator's stream for this tick before its next update overwrites rbd
int bpmpc_controller_tick_estimated(bpmpc_controller* c, bpmpc_estimator* e, int batch, const double* t, int inputs_on_device, double period,
                                    const bpmpc_tick_outputs* host_out) {
  (void)period;      // as bpmpc_controller_tick: the WBC takes it and does not use it; the filter's dt is the period of bpmpc_estimator_update
  return guarded(c, BPMPC_ERR_DEVICE, "bpmpc_controller_tick_estimated: null argument", e && t, [&] {
    hipStream_t st = controller_stream(c);
    if (e->nj != c->nj) throw std::invalid_argument("bpmpc_controller_tick_estimated: the estimator and the controller are built for different robots");
    if (e->device != c->device) throw std::invalid_argument("bpmpc_controller_tick_estimated: the estimator and the controller live on different devices");
    check_tick(c, batch, "bpmpc_controller_tick_estimated");
    estimator_before_foreign_read(e, batch, st);      // refuses a batch without estimates before anything is enqueued
    enqueue_tick(c, batch, staged(t, c->d_t, batch, inputs_on_device, st), e->d_rbd);
    estimator_after_foreign_read(e, st);
    fetch_tick(c, batch, host_out);
  });
}

// BipedalController::starting for the robots of `mask`: the observation unwrapped against yawLast = 0 (:126-127), MPC_BASE::reset from it (:147-148),
// clearLastQpSol (:179).  The refusals of bpmpc_solver_restart (DDP, batch of the last setup) and the tick's (the WBC's max_batch) come first.
int bpmpc_controller_restart(bpmpc_controller* c, int batch, const int* mask, const double* rbd, int inputs_on_device) {
  return guarded(c, BPMPC_ERR_DEVICE, "bpmpc_controller_restart: null argument", mask && rbd, [&] {
    bpmpc_solver* s = c->s;
    hipStream_t st = controller_stream(c);
    check_restart(s, batch);
    if (batch > c->max_batch) throw std::length_error("bpmpc_controller_restart: batch exceeds the WBC's max_batch");
    const int* dmask = staged(mask, c->d_mask, batch, inputs_on_device, st);
    RestartArgs a{};
    a.batch = batch; a.mask = dmask; a.rbd = staged(rbd, c->d_rbd, (size_t)batch * 2 * c->nv, inputs_on_device, st); a.yaw_last = c->d_yaw; a.x_obs = c->d_xobs;
    kl::restart_observe(c->nj, batch, st, s->d_model, a);
    HIP_CHECK(hipGetLastError());
    // buffered: the solver's restart reads the mask and the observations on the solver's stream, behind the observation on the buffer's; the next
    // launch on the buffer's stream waits for it
    enqueued(c);
    if (c->p) c->p->hs.before_foreign(s->stream);
    restart(s, batch, dmask, c->d_xobs, true);
    if (c->p) c->p->hs.after_foreign(s->stream);
    wbc_restart_on(c->w, batch, dmask, st);
    enqueued(c);
    if (c->p) c->p->restart_hold = true;      // the policy of the previous episode is gone for the restarted robots: ticks wait for the next adoption
    if (!inputs_on_device) {                  // the caller's host arrays
      HIP_CHECK(hipStreamSynchronize(st));
      if (c->p) HIP_CHECK(hipStreamSynchronize(s->stream));
    }
  });
}

// The joint-level kp / kd of dynamicReconfigCallback (:423-472) for the robots of `mask`, on the controller's stream: in order with the ticks that read them
int bpmpc_controller_set_joint_gains(bpmpc_controller* c, int batch, const int* mask, const double* kp, const double* kd, int n_rows, int inputs_on_device) {
  return guarded(c, BPMPC_ERR_DEVICE, "bpmpc_controller_set_joint_gains: null handle or gains", kp && kd, [&] {
    if (batch < 1 || batch > c->max_batch) throw std::length_error("bpmpc_controller_set_joint_gains: batch exceeds the WBC's max_batch");
    auto check_row = [&](int r) {
      for (int j = 0; j < c->nj; ++j)
        for (const double* g : {kp, kd})
          if (!std::isfinite(g[r * c->nj + j]) || g[r * c->nj + j] < 0.0)
            throw std::invalid_argument("bpmpc_controller_set_joint_gains: row " + std::to_string(r) + ", joint " + std::to_string(j) + ": " + (g == kp ? "kp" : "kd") +
                                        " must be finite and not negative");
    };
    hipStream_t st = controller_stream(c);
    set_rows("bpmpc_controller_set_joint_gains", st, batch, c->nj, c->nj, mask, c->d_mask, n_rows, inputs_on_device, check_row, {kp, c->d_kp_in, c->d_kp},
             {kd, c->d_kd_in, c->d_kd});
    enqueued(c);
    if (!inputs_on_device) HIP_CHECK(hipStreamSynchronize(st));      // the caller's host arrays
  });
}

int bpmpc_controller_joint_outputs(bpmpc_controller* c, int batch, double* host_torque, double* host_kp, double* host_kd, double** dev_torque,
                                   double** dev_kp, double** dev_kd) {
  return guarded(c, BPMPC_ERR_DEVICE, "null controller handle", [&] {
    if (dev_torque) *dev_torque = c->d_torque;
    if (dev_kp) *dev_kp = c->d_kp;
    if (dev_kd) *dev_kd = c->d_kd;
    if (!host_torque && !host_kp && !host_kd) return;
    if (batch < 1 || batch > c->max_batch) throw std::length_error("bpmpc_controller_joint_outputs: batch exceeds the WBC's max_batch");
    const size_t bytes = (size_t)batch * c->nj * sizeof(double);
    hipStream_t st = controller_stream(c);
    if (host_torque) HIP_CHECK(hipMemcpyAsync(host_torque, c->d_torque, bytes, hipMemcpyDeviceToHost, st));
    if (host_kp) HIP_CHECK(hipMemcpyAsync(host_kp, c->d_kp, bytes, hipMemcpyDeviceToHost, st));
    if (host_kd) HIP_CHECK(hipMemcpyAsync(host_kd, c->d_kd, bytes, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

// The controller's work moves to the buffer's stream (NULL: back to the solver's).  Both streams are drained here, once, so that no launch of the
// one stream is in flight on state the other is about to touch; from then on events order them.
int bpmpc_controller_attach_policy(bpmpc_controller* c, bpmpc_policy* p) {
  return guarded(c, BPMPC_ERR_DEVICE, "bpmpc_controller_attach_policy: null controller handle", [&] {
    if (p && p->s != c->s) throw std::invalid_argument("bpmpc_controller_attach_policy: the policy buffer belongs to another solver");
    if (p && p->device != c->device) throw std::invalid_argument("bpmpc_controller_attach_policy: the policy buffer and the controller live on different devices");
    if (p == c->p) return;
    HIP_CHECK(hipStreamSynchronize(controller_stream(c)));
    HIP_CHECK(hipStreamSynchronize(c->s->stream));
    if (p) HIP_CHECK(hipStreamSynchronize(p->hs.stream));
    detach(c);
    if (p) { c->p = p; ++p->attached; c->s->tick_hs = &p->hs; }
  });
}

// NULL detaches.  Nothing is drained: the telemetry's own stream and the controller's are ordered by events around every launch (telemetry.h).
int bpmpc_controller_attach_telemetry(bpmpc_controller* c, bpmpc_telemetry* tm) {
  return guarded(c, BPMPC_ERR_DEVICE, "bpmpc_controller_attach_telemetry: null controller handle", [&] {
    if (tm && tm->nj != c->nj) throw std::invalid_argument("bpmpc_controller_attach_telemetry: the telemetry's model and the controller are built for different robots");
    if (tm && tm->device != c->device) throw std::invalid_argument("bpmpc_controller_attach_telemetry: the telemetry and the controller live on different devices");
    c->tel = tm;
  });
}

int bpmpc_controller_device_outputs(bpmpc_controller* c, bpmpc_tick_outputs* o) {
  if (!c || !o) { set_last_error("bpmpc_controller_device_outputs: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  o->x_obs = c->d_xobs; o->x_opt = c->d_xopt; o->u_opt = c->d_uopt; o->joint_cmd = c->d_cmd; o->wbc_solution = c->w->d_sol;
  o->planned_mode = c->d_mode; o->wbc_status = c->w->d_status; o->safe = c->d_safe;
  return BPMPC_OK;
}

}  // extern "C"
