// Host side of the controller tick (kernels/tick.h, k_tick.hip) and of MRT_BASE::evaluatePolicy: the C ABI of include/bpmpc.h.
//   BipedalController::update          bipedal_controllers/src/BipedalController.cpp:186-262
//   observation                         :397-403 (computeCentroidalStateFromRbdModel, yaw unwrap)
//   evaluatePolicy / WBC / safety       :199, :229, SafetyChecker.h:39-52;  commands :237-252
// One tick = k_tick_observe_policy, k_wbc (the WBC handle's kernel and its per-robot last solutions), k_tick_commands, all on the solver's
// stream; nothing is synchronised unless outputs are asked for on the host.  k_tick_commands also forms joint_torque from the per-robot joint
// gains of dynamicReconfigCallback (:423-472, bpmpc_controller_set_joint_gains).
// A restart (BipedalController::starting, :123-179) for the robots of a mask = k_restart_observe, bpmpc_solver_restart with the observations,
// k_wbc_restart, on the same stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>

#include "estimator.h"
#include "solver.h"
#include "wbc.h"
#include "kernels/tick.h"

using namespace bpmpc;

struct bpmpc_controller {
  bpmpc_solver* s = nullptr;
  bpmpc_wbc* w = nullptr;
  int device = 0, max_batch = 0, nj = 0, nx = 0, nv = 0, n = 0;
  double *d_yaw = nullptr, *d_t = nullptr, *d_rbd = nullptr, *d_xobs = nullptr, *d_xopt = nullptr, *d_uopt = nullptr, *d_cmd = nullptr;
  int *d_mode = nullptr, *d_safe = nullptr, *d_mask = nullptr;
  double *d_kp = nullptr, *d_kd = nullptr, *d_torque = nullptr;      // [max_batch][nj]: joint gains (0 after create), the last tick's joint_torque
  double *d_kp_in = nullptr, *d_kd_in = nullptr;                     // device copies of host gain rows
};

namespace {

TickArgs policy_args(const bpmpc_solver* s, int batch) {
  const Buffers& bf = s->buf;
  TickArgs a{};
  a.batch = batch; a.N = s->settings.max_nodes; a.feedback = s->feedback();
  a.p_grid = bf.p_grid; a.g_nodes = bf.g_nodes; a.g_kind = bf.g_kind; a.g_mode = bf.g_mode; a.g_time = bf.g_time; a.x = bf.x; a.u = bf.u; a.K = bf.K;
  return a;
}

void free_all(bpmpc_controller* c) {
  for (void* p : {(void*)c->d_yaw, (void*)c->d_t, (void*)c->d_rbd, (void*)c->d_xobs, (void*)c->d_xopt, (void*)c->d_uopt, (void*)c->d_cmd, (void*)c->d_mode,
                  (void*)c->d_safe, (void*)c->d_mask, (void*)c->d_kp, (void*)c->d_kd, (void*)c->d_torque, (void*)c->d_kp_in, (void*)c->d_kd_in})
    if (p) (void)hipFree(p);
}

// the refusals of a tick: a completed run of an SQP solver since the last setup, the batch of that setup, the WBC's capacity
void check_tick(const bpmpc_controller* c, int batch, const char* who) {
  check_policy(c->s);
  if (batch != c->s->batch) throw std::invalid_argument(std::string(who) + ": batch differs from the batch of the solver's last setup");
  if (batch > c->max_batch) throw std::length_error(std::string(who) + ": batch exceeds the WBC's max_batch");
}

// the three launches of a tick on the solver's stream, from device inputs
void enqueue_tick(bpmpc_controller* c, int batch, const double* dt, const double* drbd) {
  bpmpc_solver* s = c->s;
  TickArgs a = policy_args(s, batch);
  a.t = dt; a.rbd = drbd; a.yaw_last = c->d_yaw; a.x_obs = c->d_xobs; a.x_loop = s->tick_x; a.safe = c->d_safe;
  a.x_opt = c->d_xopt; a.u_opt = c->d_uopt; a.mode = c->d_mode;
  kl::tick_observe_policy(c->nj, batch, s->stream, s->d_model, a);
  HIP_CHECK(hipGetLastError());
  s->loop_from_tick = true;          // the next setup_commands(x0 = NULL) starts from tick_x (until the next rollout)
  wbc_launch_on(c->w, batch, c->d_xopt, c->d_uopt, drbd, c->d_mode, s->stream);
  TickCommandArgs ca{};
  ca.batch = batch; ca.x_opt = c->d_xopt; ca.u_opt = c->d_uopt; ca.sol = c->w->d_sol; ca.rbd = drbd; ca.kp = c->d_kp; ca.kd = c->d_kd;
  ca.cmd = c->d_cmd; ca.joint_torque = c->d_torque;
  kl::tick_commands(c->nj, s->stream, ca);
  HIP_CHECK(hipGetLastError());
}

// the host copies of a tick's outputs (host_out NULL: nothing is copied or synchronised)
void fetch_tick(bpmpc_controller* c, int batch, const bpmpc_tick_outputs* host_out) {
  if (!host_out) return;
  bpmpc_solver* s = c->s;
  const size_t B = batch;
  const bpmpc_tick_outputs& o = *host_out;
  auto down = [&](void* dst, const void* src, size_t bytes) { if (dst) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s->stream)); };
  down(o.x_obs, c->d_xobs, B * c->nx * sizeof(double));
  down(o.x_opt, c->d_xopt, B * c->nx * sizeof(double));
  down(o.u_opt, c->d_uopt, B * c->nx * sizeof(double));
  down(o.joint_cmd, c->d_cmd, B * 3 * c->nj * sizeof(double));
  down(o.wbc_solution, c->w->d_sol, B * c->n * sizeof(double));
  down(o.planned_mode, c->d_mode, B * sizeof(int));
  down(o.wbc_status, c->w->d_status, B * sizeof(int));
  down(o.safe, c->d_safe, B * sizeof(int));
  HIP_CHECK(hipStreamSynchronize(s->stream));
}

}  // namespace

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
    const size_t B = c->max_batch;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&c->d_yaw), B * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&c->d_t), B * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&c->d_rbd), B * 2 * c->nv * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&c->d_xobs), B * c->nx * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&c->d_xopt), B * c->nx * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&c->d_uopt), B * c->nx * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&c->d_cmd), B * 3 * c->nj * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&c->d_mode), B * sizeof(int)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&c->d_safe), B * sizeof(int)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&c->d_mask), B * sizeof(int)));
    for (double** p : {&c->d_kp, &c->d_kd, &c->d_torque, &c->d_kp_in, &c->d_kd_in}) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), B * c->nj * sizeof(double)));
    HIP_CHECK(hipMemset(c->d_kp, 0, B * c->nj * sizeof(double)));
    HIP_CHECK(hipMemset(c->d_kd, 0, B * c->nj * sizeof(double)));
    HIP_CHECK(hipMemset(c->d_torque, 0, B * c->nj * sizeof(double)));
    HIP_CHECK(hipMemset(c->d_yaw, 0, B * sizeof(double)));       // yawLast of BipedalController::starting: the first observation's yaw unwraps from 0
    HIP_CHECK(hipDeviceSynchronize());
  });
  if (rc != BPMPC_OK) { free_all(c.get()); return rc; }
  *out = c.release();
  return BPMPC_OK;
}

void bpmpc_controller_destroy(bpmpc_controller* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();           // a tick may still be in flight on the solver's stream
  free_all(c);
  delete c;
}

int bpmpc_controller_reset(bpmpc_controller* c) {
  if (!c) { set_last_error("null controller handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_DEVICE, [&] {
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemset(c->d_yaw, 0, (size_t)c->max_batch * sizeof(double)));
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int bpmpc_controller_tick(bpmpc_controller* c, int batch, const double* t, const double* rbd, int inputs_on_device, double period,
                          const bpmpc_tick_outputs* host_out) {
  (void)period;      // WeightedWbc::update takes it and does not use it (WbcBase.cpp:242-243), as bpmpc_wbc_update
  if (!c || !t || !rbd) { set_last_error("bpmpc_controller_tick: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_DEVICE, [&] {
    bpmpc_solver* s = c->s;
    check_tick(c, batch, "bpmpc_controller_tick");
    HIP_CHECK(hipSetDevice(c->device));
    const size_t B = batch;
    const double *dt = t, *drbd = rbd;
    if (!inputs_on_device) {
      HIP_CHECK(hipMemcpyAsync(c->d_t, t, B * sizeof(double), hipMemcpyHostToDevice, s->stream));
      HIP_CHECK(hipMemcpyAsync(c->d_rbd, rbd, B * 2 * c->nv * sizeof(double), hipMemcpyHostToDevice, s->stream));
      dt = c->d_t; drbd = c->d_rbd;
    }
    enqueue_tick(c, batch, dt, drbd);
    fetch_tick(c, batch, host_out);
  });
}

// bpmpc_controller_tick on the rbd the estimator holds on the device: the solver's stream waits for an update that was only enqueued, and the
// estimator's stream for this tick before its next update overwrites rbd
int bpmpc_controller_tick_estimated(bpmpc_controller* c, bpmpc_estimator* e, int batch, const double* t, int inputs_on_device, double period,
                                    const bpmpc_tick_outputs* host_out) {
  (void)period;      // as bpmpc_controller_tick: the WBC takes it and does not use it; the filter's dt is the period of bpmpc_estimator_update
  if (!c || !e || !t) { set_last_error("bpmpc_controller_tick_estimated: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_DEVICE, [&] {
    bpmpc_solver* s = c->s;
    if (e->nj != c->nj) throw std::invalid_argument("bpmpc_controller_tick_estimated: the estimator and the controller are built for different robots");
    if (e->device != c->device) throw std::invalid_argument("bpmpc_controller_tick_estimated: the estimator and the controller live on different devices");
    check_tick(c, batch, "bpmpc_controller_tick_estimated");
    HIP_CHECK(hipSetDevice(c->device));
    estimator_before_foreign_read(e, batch, s->stream);      // refuses a batch without estimates before anything is enqueued
    const double* dt = t;
    if (!inputs_on_device) {
      HIP_CHECK(hipMemcpyAsync(c->d_t, t, (size_t)batch * sizeof(double), hipMemcpyHostToDevice, s->stream));
      dt = c->d_t;
    }
    enqueue_tick(c, batch, dt, e->d_rbd);
    estimator_after_foreign_read(e, s->stream);
    fetch_tick(c, batch, host_out);
  });
}

// BipedalController::starting for the robots of `mask`: the observation unwrapped against yawLast = 0 (:126-127), MPC_BASE::reset from it (:147-148),
// clearLastQpSol (:179).  The refusals of bpmpc_solver_restart (DDP, batch of the last setup) and the tick's (the WBC's max_batch) come first.
int bpmpc_controller_restart(bpmpc_controller* c, int batch, const int* mask, const double* rbd, int inputs_on_device) {
  if (!c || !mask || !rbd) { set_last_error("bpmpc_controller_restart: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_DEVICE, [&] {
    bpmpc_solver* s = c->s;
    check_restart(s, batch);
    if (batch > c->max_batch) throw std::length_error("bpmpc_controller_restart: batch exceeds the WBC's max_batch");
    HIP_CHECK(hipSetDevice(c->device));
    const int* dmask = mask;
    const double* drbd = rbd;
    if (!inputs_on_device) {
      HIP_CHECK(hipMemcpyAsync(c->d_mask, mask, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, s->stream));
      HIP_CHECK(hipMemcpyAsync(c->d_rbd, rbd, (size_t)batch * 2 * c->nv * sizeof(double), hipMemcpyHostToDevice, s->stream));
      dmask = c->d_mask; drbd = c->d_rbd;
    }
    RestartArgs a{};
    a.batch = batch; a.mask = dmask; a.rbd = drbd; a.yaw_last = c->d_yaw; a.x_obs = c->d_xobs;
    kl::restart_observe(c->nj, batch, s->stream, s->d_model, a);
    HIP_CHECK(hipGetLastError());
    restart(s, batch, dmask, c->d_xobs, true);
    wbc_restart_on(c->w, batch, dmask, s->stream);
    if (!inputs_on_device) HIP_CHECK(hipStreamSynchronize(s->stream));     // the caller's host arrays
  });
}

// The joint-level kp / kd of dynamicReconfigCallback (:423-472) for the robots of `mask`, on the solver's stream
int bpmpc_controller_set_joint_gains(bpmpc_controller* c, int batch, const int* mask, const double* kp, const double* kd, int n_rows, int inputs_on_device) {
  if (!c || !kp || !kd) { set_last_error("bpmpc_controller_set_joint_gains: null handle or gains"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_DEVICE, [&] {
    if (batch < 1 || batch > c->max_batch) throw std::length_error("bpmpc_controller_set_joint_gains: batch exceeds the WBC's max_batch");
    if (n_rows != 1 && n_rows != batch) throw std::invalid_argument("bpmpc_controller_set_joint_gains: n_rows must be 1 or batch");
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t stream = c->s->stream;
    const int* dmask = mask;
    const double *dkp = kp, *dkd = kd;
    if (!inputs_on_device) {
      for (int r = 0; r < n_rows; ++r) {
        if (n_rows != 1 && mask && !mask[r]) continue;
        for (int j = 0; j < c->nj; ++j)
          for (const double* g : {kp, kd})
            if (!std::isfinite(g[r * c->nj + j]) || g[r * c->nj + j] < 0.0)
              throw std::invalid_argument("bpmpc_controller_set_joint_gains: row " + std::to_string(r) + ", joint " + std::to_string(j) + ": " + (g == kp ? "kp" : "kd") +
                                          " must be finite and not negative");
      }
      const size_t bytes = (size_t)n_rows * c->nj * sizeof(double);
      HIP_CHECK(hipMemcpyAsync(c->d_kp_in, kp, bytes, hipMemcpyHostToDevice, stream));
      HIP_CHECK(hipMemcpyAsync(c->d_kd_in, kd, bytes, hipMemcpyHostToDevice, stream));
      if (mask) HIP_CHECK(hipMemcpyAsync(c->d_mask, mask, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, stream));
      dmask = mask ? c->d_mask : nullptr; dkp = c->d_kp_in; dkd = c->d_kd_in;
    }
    kl::set_joint_gains(c->nj, batch, stream, dmask, dkp, dkd, n_rows, c->d_kp, c->d_kd);
    HIP_CHECK(hipGetLastError());
    if (!inputs_on_device) HIP_CHECK(hipStreamSynchronize(stream));      // the caller's host arrays
  });
}

int bpmpc_controller_joint_outputs(bpmpc_controller* c, int batch, double* host_torque, double* host_kp, double* host_kd, double** dev_torque,
                                   double** dev_kp, double** dev_kd) {
  if (!c) { set_last_error("null controller handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_DEVICE, [&] {
    if (dev_torque) *dev_torque = c->d_torque;
    if (dev_kp) *dev_kp = c->d_kp;
    if (dev_kd) *dev_kd = c->d_kd;
    if (!host_torque && !host_kp && !host_kd) return;
    if (batch < 1 || batch > c->max_batch) throw std::length_error("bpmpc_controller_joint_outputs: batch exceeds the WBC's max_batch");
    HIP_CHECK(hipSetDevice(c->device));
    const size_t bytes = (size_t)batch * c->nj * sizeof(double);
    if (host_torque) HIP_CHECK(hipMemcpyAsync(host_torque, c->d_torque, bytes, hipMemcpyDeviceToHost, c->s->stream));
    if (host_kp) HIP_CHECK(hipMemcpyAsync(host_kp, c->d_kp, bytes, hipMemcpyDeviceToHost, c->s->stream));
    if (host_kd) HIP_CHECK(hipMemcpyAsync(host_kd, c->d_kd, bytes, hipMemcpyDeviceToHost, c->s->stream));
    HIP_CHECK(hipStreamSynchronize(c->s->stream));
  });
}

int bpmpc_controller_device_outputs(bpmpc_controller* c, bpmpc_tick_outputs* o) {
  if (!c || !o) { set_last_error("bpmpc_controller_device_outputs: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  o->x_obs = c->d_xobs; o->x_opt = c->d_xopt; o->u_opt = c->d_uopt; o->joint_cmd = c->d_cmd; o->wbc_solution = c->w->d_sol;
  o->planned_mode = c->d_mode; o->wbc_status = c->w->d_status; o->safe = c->d_safe;
  return BPMPC_OK;
}

}  // extern "C"
