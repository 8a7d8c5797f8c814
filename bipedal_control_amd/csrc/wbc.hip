// Host side of the batched whole-body controller (kernels/wbc.h): settings ingest, device buffers, the C ABI (include/bpmpc.h).
//   WeightedWbc construction + loadTasksSetting     bipedal_controllers/src/BipedalController.cpp:97-100, bipedal_wbc/src/WbcBase.cpp:405-447,
//                                                   bipedal_wbc/src/WeightedWbc.cpp:100-116
//   WeightedWbc::update                             bipedal_controllers/src/BipedalController.cpp:229
#include <hip/hip_runtime.h>

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
__global__ __launch_bounds__(kWave) void k_wbc(const DeviceModel* model, WbcSettings st, WbcArgs a) {
  __shared__ WbcLds<NJ> w;
  const int b = blockIdx.x;
  if (b >= a.batch) return;
  wbc_robot<NJ>(*model, st, w, a, b, threadIdx.x);
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
  s.max_working_set_changes = 20;      // int nWsr = 20, WeightedWbc.cpp:57
  return s;
}

// k_wbc of the handle's robot on `stream`
void launch_wbc(const bpmpc_wbc* w, const WbcArgs& a, hipStream_t stream) {
  KL_NJ(w->rm.nj, hipLaunchKernelGGL(k_wbc<NJ>, dim3(a.batch), dim3(kWave), 0, stream, w->d_model, w->st, a));
  HIP_CHECK(hipGetLastError());
}
}  // namespace

namespace bpmpc {

// The launch of bpmpc_wbc_update without its transfers: device inputs, the handle's last solutions and statuses, on the caller's stream.
void wbc_launch_on(bpmpc_wbc* w, int batch, const double* state_des, const double* input_des, const double* rbd_meas, const int* mode, hipStream_t stream) {
  if (batch < 1 || batch > w->max_batch) throw std::length_error("controller tick: batch exceeds the WBC's max_batch");
  if (w->own_pending) HIP_CHECK(hipStreamWaitEvent(stream, w->ev_own, 0));
  WbcArgs a{};
  a.batch = batch; a.nx = w->rm.nx; a.state_des = state_des; a.input_des = input_des; a.rbd_meas = rbd_meas; a.mode = mode;
  a.sol = w->d_sol; a.status = w->d_status; a.debug = nullptr;
  launch_wbc(w, a, stream);
  if (!w->ev_foreign) HIP_CHECK(hipEventCreateWithFlags(&w->ev_foreign, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(w->ev_foreign, stream));
  HIP_CHECK(hipStreamWaitEvent(w->stream, w->ev_foreign, 0));
}

// k_wbc_restart on a device mask, enqueued on `stream` under the rule of wbc_launch_on (the handle's own stream: no events)
void wbc_restart_on(bpmpc_wbc* w, int batch, const int* mask, hipStream_t stream) {
  if (batch < 1 || batch > w->max_batch) throw std::length_error("restart: batch exceeds the WBC's max_batch");
  const bool foreign = stream != w->stream;
  if (foreign && w->own_pending) HIP_CHECK(hipStreamWaitEvent(stream, w->ev_own, 0));
  hipLaunchKernelGGL(k_wbc_restart, dim3((batch * w->n + 255) / 256), dim3(256), 0, stream, batch, w->n, mask, w->d_sol, w->d_status);
  HIP_CHECK(hipGetLastError());
  if (foreign) {
    if (!w->ev_foreign) HIP_CHECK(hipEventCreateWithFlags(&w->ev_foreign, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(w->ev_foreign, stream));
    HIP_CHECK(hipStreamWaitEvent(w->stream, w->ev_foreign, 0));
  }
}

}  // namespace bpmpc

extern "C" {

int bpmpc_wbc_create(const bpmpc_model* model, const char* task_info_path, int device, int max_batch, bpmpc_wbc** out) {
  if (!model || !task_info_path || !out || max_batch < 1) { set_last_error("bpmpc_wbc_create: bad argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1 || device < 0 || device >= count) {
    set_last_error("bpmpc_wbc_create: no usable HIP device (this engine has no CPU path)");
    return BPMPC_ERR_NO_DEVICE;
  }
  std::unique_ptr<bpmpc_wbc> w(new bpmpc_wbc);
  const int rc = guarded(BPMPC_ERR_IO, [&]() -> int {
    w->rm = model_of(model);
    if (w->rm.nj != 10 && w->rm.nj != 12) { set_last_error("only 10- and 12-joint bipeds are instantiated"); return BPMPC_ERR_UNSUPPORTED; }
    w->dm = make_device_model(w->rm);
    w->st = load_wbc_settings(task_info_path, w->rm.nj);
    w->device = device; w->max_batch = max_batch; w->nv = 6 + w->rm.nj; w->n = w->nv + 12 + w->rm.nj;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&w->d_model), sizeof(DeviceModel)));
    HIP_CHECK(hipMemcpy(w->d_model, &w->dm, sizeof(DeviceModel), hipMemcpyHostToDevice));
    const size_t B = max_batch;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&w->d_x), B * w->rm.nx * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&w->d_u), B * w->rm.nu * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&w->d_rbd), B * 2 * w->nv * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&w->d_sol), B * w->n * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&w->d_debug), B * kWbcDebugStride * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&w->d_mode), B * sizeof(int)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&w->d_status), B * sizeof(int)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&w->d_mask), B * sizeof(int)));
    HIP_CHECK(hipMemset(w->d_sol, 0, B * w->n * sizeof(double)));      // lastQpSol_ starts at zero (WeightedWbc.h)
    return BPMPC_OK;
  });
  if (rc != BPMPC_OK) { bpmpc_wbc_destroy(w.release()); return rc; }
  *out = w.release();
  return BPMPC_OK;
}

void bpmpc_wbc_destroy(bpmpc_wbc* w) {
  if (!w) return;
  if (w->stream) { (void)hipStreamSynchronize(w->stream); (void)hipStreamDestroy(w->stream); }
  if (w->ev_foreign) (void)hipEventDestroy(w->ev_foreign);
  if (w->ev_own) (void)hipEventDestroy(w->ev_own);
  for (void* p : {(void*)w->d_model, (void*)w->d_x, (void*)w->d_u, (void*)w->d_rbd, (void*)w->d_sol, (void*)w->d_debug, (void*)w->d_mode, (void*)w->d_status,
                  (void*)w->d_mask})
    if (p) (void)hipFree(p);
  delete w;
}

int bpmpc_wbc_dims(const bpmpc_wbc* w, int* n_decision, int* nv) {
  if (!w) { set_last_error("null wbc handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  if (n_decision) *n_decision = w->n;
  if (nv) *nv = w->nv;
  return BPMPC_OK;
}

int bpmpc_wbc_update(bpmpc_wbc* w, int batch, const double* state_desired, const double* input_desired, const double* rbd_state_measured,
                     const int* mode, double period, double* solution, int* status, double* debug) {
  (void)period;      // the joint-acceleration feed-forward that used it is commented out in the reference (WbcBase.cpp:242-243)
  if (!w || !state_desired || !input_desired || !rbd_state_measured || !mode || !solution) { set_last_error("bpmpc_wbc_update: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    if (batch < 1 || batch > w->max_batch) throw std::length_error("bpmpc_wbc_update: batch exceeds max_batch");
    for (int b = 0; b < batch; ++b) if (mode[b] < 0 || mode[b] > 3) throw std::invalid_argument("bpmpc_wbc_update: mode must be 0..3");
    HIP_CHECK(hipSetDevice(w->device));
    const size_t B = batch;
    HIP_CHECK(hipMemcpyAsync(w->d_x, state_desired, B * w->rm.nx * sizeof(double), hipMemcpyHostToDevice, w->stream));
    HIP_CHECK(hipMemcpyAsync(w->d_u, input_desired, B * w->rm.nu * sizeof(double), hipMemcpyHostToDevice, w->stream));
    HIP_CHECK(hipMemcpyAsync(w->d_rbd, rbd_state_measured, B * 2 * w->nv * sizeof(double), hipMemcpyHostToDevice, w->stream));
    HIP_CHECK(hipMemcpyAsync(w->d_mode, mode, B * sizeof(int), hipMemcpyHostToDevice, w->stream));
    WbcArgs a{};
    a.batch = batch; a.nx = w->rm.nx; a.state_des = w->d_x; a.input_des = w->d_u; a.rbd_meas = w->d_rbd; a.mode = w->d_mode;
    a.sol = w->d_sol; a.status = w->d_status; a.debug = debug ? w->d_debug : nullptr;
    launch_wbc(w, a, w->stream);
    HIP_CHECK(hipMemcpyAsync(solution, w->d_sol, B * w->n * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    if (status) HIP_CHECK(hipMemcpyAsync(status, w->d_status, B * sizeof(int), hipMemcpyDeviceToHost, w->stream));
    if (debug) HIP_CHECK(hipMemcpyAsync(debug, w->d_debug, B * kWbcDebugStride * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    HIP_CHECK(hipStreamSynchronize(w->stream));
    w->own_pending = false;
  });
}

int bpmpc_wbc_reset(bpmpc_wbc* w) {
  if (!w) { set_last_error("null wbc handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    HIP_CHECK(hipSetDevice(w->device));
    HIP_CHECK(hipMemsetAsync(w->d_sol, 0, (size_t)w->max_batch * w->n * sizeof(double), w->stream));
    HIP_CHECK(hipStreamSynchronize(w->stream));
    w->own_pending = false;
  });
}

int bpmpc_wbc_restart(bpmpc_wbc* w, int batch, const int* mask, int inputs_on_device) {
  if (!w || !mask) { set_last_error("bpmpc_wbc_restart: null handle or mask"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    if (batch < 1 || batch > w->max_batch) throw std::length_error("bpmpc_wbc_restart: batch exceeds max_batch");
    HIP_CHECK(hipSetDevice(w->device));
    if (!inputs_on_device) {
      HIP_CHECK(hipMemcpyAsync(w->d_mask, mask, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, w->stream));
      wbc_restart_on(w, batch, w->d_mask, w->stream);
      HIP_CHECK(hipStreamSynchronize(w->stream));
      w->own_pending = false;
    } else {                            // only enqueued: the next launch on another stream (a controller tick) waits for it
      wbc_restart_on(w, batch, mask, w->stream);
      if (!w->ev_own) HIP_CHECK(hipEventCreateWithFlags(&w->ev_own, hipEventDisableTiming));
      HIP_CHECK(hipEventRecord(w->ev_own, w->stream));
      w->own_pending = true;
    }
  });
}

}  // extern "C"
