// Host side of the batched whole-body controller (kernels/wbc.h): settings ingest, device buffers, the C ABI (include/bpmpc.h).
//   WeightedWbc construction + loadTasksSetting     bipedal_controllers/src/BipedalController.cpp:97-100, bipedal_wbc/src/WbcBase.cpp:405-447,
//                                                   bipedal_wbc/src/WeightedWbc.cpp:100-116
//   WeightedWbc::update                             bipedal_controllers/src/BipedalController.cpp:229
//   setBasePDGains / setSwingLegPDGains / setWeights bipedal_controllers/src/BipedalController.cpp:407-419 (dynamicReconfigCallback), per robot: the
//                                                   parameter rows of the handle (bpmpc_wbc_get_params / set_params / reset_params)
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "info_tree.h"
#include "kernel_launchers.h"
#include "wbc.h"

namespace bpmpc {

template <int NJ>
__global__ __launch_bounds__(kWave) void k_wbc(const DeviceModel* model, WbcArgs a) {
  __shared__ WbcLds<NJ> w;
  const int b = blockIdx.x;
  if (b >= a.batch) return;
  wbc_robot<NJ>(*model, w, a, b, threadIdx.x);
}

// WeightedWbc::clearLastQpSol for the robots of `mask` (bpmpc_wbc_restart): their last solution and status become 0
__global__ __launch_bounds__(256) void k_wbc_restart(int batch, int n, const int* mask, double* sol, int* status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= batch * n) return;
  const int b = i / n;
  if (!mask[b]) return;
  sol[i] = 0.0;
  if (i % n == 0) status[b] = 0;
}

}  // namespace bpmpc

using namespace bpmpc;

namespace {

WbcSettings load_wbc_settings(const std::string& task_info, int nj) {
  const auto t = read_info_file(task_info);
  WbcSettings s{};
  const std::vector<double> lim = load_matrix(*t, "torqueLimitsTask", nj / 2, 1);
  for (int i = 0; i < nj / 2; ++i) s.torque_limits[i] = lim[i];
  auto need = [&](const char* key, double* out) { if (!t->get(key, out)) throw std::runtime_error(std::string("task.info: missing ") + key); };
  need("frictionConeTask.frictionCoefficient", &s.friction);
  need("swingLegTask.kp", &s.swing_kp);
  need("swingLegTask.kd", &s.swing_kd);
  const std::vector<double> kp = load_matrix(*t, "baseAccelPDTask.baseKp", 6, 1), kd = load_matrix(*t, "baseAccelPDTask.baseKd", 6, 1);
  for (int i = 0; i < 6; ++i) { s.base_kp[i] = kp[i]; s.base_kd[i] = kd[i]; }
  // [OCS2-upstream] loadData::loadPtreeValue keeps the member's initial value when the key is absent (it only warns): the Hunter
  // configuration has no noContactMotionTask section, and WbcBase.h:131 initialises noContactMotionTolerance_{} = 0
  s.contact_tolerance = 0.0;
  (void)t->get("noContactMotionTask.tolerance", &s.contact_tolerance);
  need("weight.swingLeg", &s.w_swing);
  need("weight.baseAccel", &s.w_base);
  need("weight.contactForce", &s.w_force);
  return s;
}

// k_wbc of the handle's robot on `stream`
void launch_wbc(const bpmpc_wbc* w, const WbcArgs& a, hipStream_t stream) {
  KL_NJ(w->rm.nj, hipLaunchKernelGGL(k_wbc<NJ>, dim3(a.batch), dim3(kWave), 0, stream, w->d_model, a));
  HIP_CHECK(hipGetLastError());
}

// A host row before it is accepted: every used entry finite; gains, weights, friction and torque limits not negative
void check_param_row(const double* row, int r, int nj) {
  static const char* const kNames[] = {"base kp", "base kd", "swing kp", "swing kd", "weight swing leg", "weight base acceleration", "weight contact force",
                                       "friction coefficient", "no-contact-motion tolerance", "torque limit"};
  for (int e = 0; e < BPMPC_WBC_PARAM_TORQUE_LIMITS + nj / 2; ++e) {
    const int kind = e < 6 ? 0 : e < 12 ? 1 : e < BPMPC_WBC_PARAM_TORQUE_LIMITS ? e - 10 : 9;
    const bool negative_ok = e == BPMPC_WBC_PARAM_CONTACT_TOLERANCE;
    if (!std::isfinite(row[e]) || (!negative_ok && row[e] < 0.0))
      throw std::invalid_argument("bpmpc_wbc_set_params: row " + std::to_string(r) + ", entry " + std::to_string(e) + " (" + kNames[kind] + ") is " +
                                  (std::isfinite(row[e]) ? "negative" : "not finite"));
  }
}
}  // namespace

namespace bpmpc {

// The launch of bpmpc_wbc_update without its transfers: device inputs, the handle's last solutions and statuses, on the caller's stream.
void wbc_launch_on(bpmpc_wbc* w, int batch, const double* state_des, const double* input_des, const double* rbd_meas, const int* mode, hipStream_t stream) {
  if (batch < 1 || batch > w->max_batch) throw std::length_error("controller tick: batch exceeds the WBC's max_batch");
  w->hs.before_foreign(stream);
  WbcArgs a{};
  a.batch = batch; a.nx = w->rm.nx; a.state_des = state_des; a.input_des = input_des; a.rbd_meas = rbd_meas; a.mode = mode;
  a.sol = w->d_sol; a.status = w->d_status; a.debug = nullptr; a.params = w->params.d_params; a.max_working_set_changes = kWbcMaxWorkingSetChanges;
  launch_wbc(w, a, stream);
  w->hs.after_foreign(stream);
}

// k_wbc_restart on a device mask, enqueued on `stream` under the rule of wbc_launch_on (the handle's own stream: no events)
void wbc_restart_on(bpmpc_wbc* w, int batch, const int* mask, hipStream_t stream) {
  if (batch < 1 || batch > w->max_batch) throw std::length_error("restart: batch exceeds the WBC's max_batch");
  w->hs.before_foreign(stream);
  hipLaunchKernelGGL(k_wbc_restart, dim3((batch * w->n + 255) / 256), dim3(256), 0, stream, batch, w->n, mask, w->d_sol, w->d_status);
  HIP_CHECK(hipGetLastError());
  w->hs.after_foreign(stream);
}

}  // namespace bpmpc

extern "C" {

int bpmpc_wbc_create(const bpmpc_model* model, const char* task_info_path, int device, int max_batch, bpmpc_wbc** out) {
  if (!model || !task_info_path || !out || max_batch < 1) { set_last_error("bpmpc_wbc_create: bad argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  std::unique_ptr<bpmpc_wbc> w(new bpmpc_wbc);
  const int rc = guarded(BPMPC_ERR_IO, [&]() -> int {
    if (const int refused = open_side_handle("bpmpc_wbc_create", w.get(), model, device, max_batch)) return refused;
    w->defaults = load_wbc_settings(task_info_path, w->rm.nj);
    w->nv = 6 + w->rm.nj; w->n = w->nv + 12 + w->rm.nj;
    const size_t B = max_batch;
    DeviceBuffers& m = w->mem;
    w->d_x = m.alloc<double>(B * w->rm.nx); w->d_u = m.alloc<double>(B * w->rm.nu); w->d_rbd = m.alloc<double>(B * 2 * w->nv);
    w->d_sol = m.alloc<double>(B * w->n, true);      // lastQpSol_ starts at zero (WeightedWbc.h)
    w->d_debug = m.alloc<double>(B * kWbcDebugStride);
    w->d_mode = m.alloc<int>(B); w->d_status = m.alloc<int>(B); w->d_mask = m.alloc<int>(B);
    w->params.create(m, max_batch, kWbcParamStride, BPMPC_WBC_PARAM_RESERVED, w->defaults.base_kp);
    w->params.fill_from_start(w->hs.stream, max_batch);
    w->hs.synchronise_own();
    return BPMPC_OK;
  });
  if (rc != BPMPC_OK) { bpmpc_wbc_destroy(w.release()); return rc; }
  *out = w.release();
  return BPMPC_OK;
}

void bpmpc_wbc_destroy(bpmpc_wbc* w) { close_side_handle(w); }

int bpmpc_wbc_dims(const bpmpc_wbc* w, int* n_decision, int* nv) {
  if (!w) { set_last_error("null wbc handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  if (n_decision) *n_decision = w->n;
  if (nv) *nv = w->nv;
  return BPMPC_OK;
}

int bpmpc_wbc_update(bpmpc_wbc* w, int batch, const double* state_desired, const double* input_desired, const double* rbd_state_measured,
                     const int* mode, double period, double* solution, int* status, double* debug) {
  (void)period;      // the joint-acceleration feed-forward that used it is commented out in the reference (WbcBase.cpp:242-243)
  return guarded(w, BPMPC_ERR_IO, "bpmpc_wbc_update: null argument", state_desired && input_desired && rbd_state_measured && mode && solution, [&] {
    if (batch < 1 || batch > w->max_batch) throw std::length_error("bpmpc_wbc_update: batch exceeds max_batch");
    for (int b = 0; b < batch; ++b) if (mode[b] < 0 || mode[b] > 3) throw std::invalid_argument("bpmpc_wbc_update: mode must be 0..3");
    const size_t B = batch;
    HIP_CHECK(hipMemcpyAsync(w->d_x, state_desired, B * w->rm.nx * sizeof(double), hipMemcpyHostToDevice, w->hs.stream));
    HIP_CHECK(hipMemcpyAsync(w->d_u, input_desired, B * w->rm.nu * sizeof(double), hipMemcpyHostToDevice, w->hs.stream));
    HIP_CHECK(hipMemcpyAsync(w->d_rbd, rbd_state_measured, B * 2 * w->nv * sizeof(double), hipMemcpyHostToDevice, w->hs.stream));
    HIP_CHECK(hipMemcpyAsync(w->d_mode, mode, B * sizeof(int), hipMemcpyHostToDevice, w->hs.stream));
    WbcArgs a{};
    a.batch = batch; a.nx = w->rm.nx; a.state_des = w->d_x; a.input_des = w->d_u; a.rbd_meas = w->d_rbd; a.mode = w->d_mode;
    a.sol = w->d_sol; a.status = w->d_status; a.debug = debug ? w->d_debug : nullptr;
    a.params = w->params.d_params; a.max_working_set_changes = kWbcMaxWorkingSetChanges;
    launch_wbc(w, a, w->hs.stream);
    HIP_CHECK(hipMemcpyAsync(solution, w->d_sol, B * w->n * sizeof(double), hipMemcpyDeviceToHost, w->hs.stream));
    if (status) HIP_CHECK(hipMemcpyAsync(status, w->d_status, B * sizeof(int), hipMemcpyDeviceToHost, w->hs.stream));
    if (debug) HIP_CHECK(hipMemcpyAsync(debug, w->d_debug, B * kWbcDebugStride * sizeof(double), hipMemcpyDeviceToHost, w->hs.stream));
    w->hs.synchronise_own();
  });
}

int bpmpc_wbc_reset(bpmpc_wbc* w) {
  return guarded(w, BPMPC_ERR_IO, "null wbc handle", [&] {
    HIP_CHECK(hipMemsetAsync(w->d_sol, 0, (size_t)w->max_batch * w->n * sizeof(double), w->hs.stream));
    w->hs.synchronise_own();
  });
}

int bpmpc_wbc_restart(bpmpc_wbc* w, int batch, const int* mask, int inputs_on_device) {
  return guarded(w, BPMPC_ERR_IO, "bpmpc_wbc_restart: null handle or mask", mask != nullptr, [&] {
    if (batch < 1 || batch > w->max_batch) throw std::length_error("bpmpc_wbc_restart: batch exceeds max_batch");
    wbc_restart_on(w, batch, staged(mask, w->d_mask, batch, inputs_on_device, w->hs.stream), w->hs.stream);
    w->hs.finish(inputs_on_device);      // device inputs are only enqueued: the next launch on another stream (a controller tick) waits for it
  });
}

int bpmpc_wbc_get_params(const bpmpc_wbc* w, int robot, double* row) {
  return guarded(w, BPMPC_ERR_IO, "bpmpc_wbc_get_params: null handle or row", row != nullptr, [&] {
    w->params.get("bpmpc_wbc_get_params", w->hs.stream, w->max_batch, robot, row);
  });
}

int bpmpc_wbc_set_params(bpmpc_wbc* w, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  return guarded(w, BPMPC_ERR_IO, "bpmpc_wbc_set_params: null handle or rows", rows != nullptr, [&] {
    if (batch < 1 || batch > w->max_batch) throw std::length_error("bpmpc_wbc_set_params: batch exceeds max_batch");
    w->params.set("bpmpc_wbc_set_params", w->hs.stream, batch, mask, w->d_mask, rows, n_rows, inputs_on_device,
                  [&](const double* row, int r) { check_param_row(row, r, w->rm.nj); });
    w->hs.finish(inputs_on_device);      // as bpmpc_wbc_restart
  });
}

int bpmpc_wbc_reset_params(bpmpc_wbc* w) {
  return guarded(w, BPMPC_ERR_IO, "null wbc handle", [&] {
    w->params.fill_from_start(w->hs.stream, w->max_batch);
    w->hs.synchronise_own();
  });
}

}  // extern "C"
