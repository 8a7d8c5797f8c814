// Host side of the batched state estimator (kernels/estimator.h): settings ingest, device buffers, the C ABI (include/bpmpc.h "State estimation").
//   updateStateEstimation                       bipedal_controllers/src/BipedalController.cpp:360-405 (sensor handles -> updateJointStates, updateContact,
//                                               updateImu, stateEstimate_->update)
//   construction                                :354-358 (FromTopicStateEstimate; KalmanFilterEstimate is declared, its source file is empty)
//   KalmanFilterEstimate::loadSettings          declared in LinearKalmanFilter.h:33; the prefix kalmanFilter. and loadPtreeValue semantics (an absent key
//                                               keeps the member's initial value, :45-51) are those of the project the header cites
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>

#include "capi_internal.h"
#include "estimator.h"
#include "kernel_launchers.h"

namespace bpmpc {

template <int NJ>
__global__ __launch_bounds__(kWave) void k_estimate(const DeviceModel* model, EstArgs a) {
  __shared__ EstLds<NJ> w;
  const int b = blockIdx.x;
  if (b >= a.batch) return;
  estimate_robot<NJ>(*model, w, a, b, threadIdx.x);
}

// bpmpc_estimator_reset / set_state for the robots of `mask` (NULL: every robot below `batch`): x_hat = x_in[b] (NULL: 0), P = cov_in[b]
// (NULL: 100 I with reset != 0, kept otherwise).  One thread per entry of [x_hat | P].
__global__ __launch_bounds__(256) void k_est_set_state(int batch, const int* mask, const double* x_in, const double* cov_in, int reset, double* x_hat, double* cov) {
  constexpr int N = kEstStates, E = N + N * N;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= batch * E) return;
  const int b = i / E, e = i % E;
  if (mask && !mask[b]) return;
  if (e < N) x_hat[b * N + e] = x_in ? x_in[b * N + e] : 0.0;
  else {
    const int k = e - N;
    if (cov_in) cov[(size_t)b * N * N + k] = cov_in[(size_t)b * N * N + k];
    else if (reset) cov[(size_t)b * N * N + k] = (k / N == k % N) ? 100.0 : 0.0;
  }
}

// bpmpc_estimator_set_params: as k_wbc_set_params on rows of kEstParamStride entries, the reserved entry written as 0
__global__ __launch_bounds__(256) void k_est_set_params(int batch, const int* mask, const double* rows, int n_rows, double* params) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= batch * kEstParamStride) return;
  const int b = i / kEstParamStride, e = i % kEstParamStride;
  if (mask && !mask[b]) return;
  params[i] = e < kEstParamStride - 1 ? rows[(size_t)(n_rows == 1 ? 0 : b) * kEstParamStride + e] : 0.0;
}

}  // namespace bpmpc

using namespace bpmpc;

namespace {

void set_params_on_device(bpmpc_estimator* e, int batch, const int* mask, const double* rows, int n_rows) {
  hipLaunchKernelGGL(k_est_set_params, dim3((batch * kEstParamStride + 255) / 256), dim3(256), 0, e->stream, batch, mask, rows, n_rows, e->d_params);
  HIP_CHECK(hipGetLastError());
}

void set_state_on_device(bpmpc_estimator* e, int batch, const int* mask, const double* x_in, const double* cov_in, int reset) {
  constexpr int E = kEstStates + kEstStates * kEstStates;
  hipLaunchKernelGGL(k_est_set_state, dim3((batch * E + 255) / 256), dim3(256), 0, e->stream, batch, mask, x_in, cov_in, reset, e->d_xhat, e->d_cov);
  HIP_CHECK(hipGetLastError());
}

void check_batch(const bpmpc_estimator* e, int batch, const char* who) {
  if (batch < 1) throw std::invalid_argument(std::string(who) + ": batch must be positive");
  if (batch > e->max_batch) throw std::length_error(std::string(who) + ": batch exceeds max_batch");
}

template <typename T>
void alloc(T** p, size_t count) { HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T))); }

}  // namespace

namespace bpmpc {

void estimator_before_foreign_read(bpmpc_estimator* e, int batch, hipStream_t stream) {
  if (batch > e->max_batch) throw std::length_error("bpmpc_controller_tick_estimated: batch exceeds the estimator's max_batch");
  if (batch != e->last_batch)
    throw std::invalid_argument("bpmpc_controller_tick_estimated: batch " + std::to_string(batch) + " differs from the batch of the estimator's last update (" +
                                std::to_string(e->last_batch) + "): the other rows of rbd hold no estimate of this tick");
  if (e->own_pending) HIP_CHECK(hipStreamWaitEvent(stream, e->ev_own, 0));
}

void estimator_after_foreign_read(bpmpc_estimator* e, hipStream_t stream) {
  if (!e->ev_foreign) HIP_CHECK(hipEventCreateWithFlags(&e->ev_foreign, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(e->ev_foreign, stream));
  HIP_CHECK(hipStreamWaitEvent(e->stream, e->ev_foreign, 0));
}

}  // namespace bpmpc

extern "C" {

int bpmpc_estimator_create(const bpmpc_model* model, const char* task_info_path, int kind, int device, int max_batch, bpmpc_estimator** out) {
  if (!model || !out) { set_last_error("bpmpc_estimator_create: null model or output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  if (max_batch < 1 || (kind != BPMPC_ESTIMATOR_FROM_TOPIC && kind != BPMPC_ESTIMATOR_KALMAN)) {
    set_last_error("bpmpc_estimator_create: kind must be BPMPC_ESTIMATOR_FROM_TOPIC or BPMPC_ESTIMATOR_KALMAN and max_batch positive");
    return BPMPC_ERR_INVALID_ARGUMENT;
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1 || device < 0 || device >= count) {
    set_last_error("bpmpc_estimator_create: no usable HIP device (this engine has no CPU path)");
    return BPMPC_ERR_NO_DEVICE;
  }
  std::unique_ptr<bpmpc_estimator> e(new bpmpc_estimator);
  const int rc = guarded(BPMPC_ERR_IO, [&]() -> int {
    e->rm = model_of(model);
    if (e->rm.nj != 10 && e->rm.nj != 12) { set_last_error("only 10- and 12-joint bipeds are instantiated"); return BPMPC_ERR_UNSUPPORTED; }
    e->dm = make_device_model(e->rm);
    e->defaults = estimator_load_settings(task_info_path);
    e->kind = kind; e->device = device; e->max_batch = max_batch; e->nj = e->rm.nj; e->nv = 6 + e->rm.nj;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    alloc(&e->d_model, 1);
    HIP_CHECK(hipMemcpy(e->d_model, &e->dm, sizeof(DeviceModel), hipMemcpyHostToDevice));
    const size_t B = max_batch, N = kEstStates;
    alloc(&e->d_rbd, B * 2 * e->nv); alloc(&e->d_xhat, B * N); alloc(&e->d_cov, B * N * N); alloc(&e->d_xy_reset, B);
    alloc(&e->d_params, B * kEstParamStride); alloc(&e->d_rows, (B + 1) * kEstParamStride); alloc(&e->d_mask, B);
    alloc(&e->d_xhat_in, B * N); alloc(&e->d_cov_in, B * N * N);
    alloc(&e->d_jp, B * e->nj); alloc(&e->d_jv, B * e->nj); alloc(&e->d_quat, B * 4); alloc(&e->d_w, B * 3); alloc(&e->d_a, B * 3); alloc(&e->d_fh, B * 4);
    alloc(&e->d_opos, B * 3); alloc(&e->d_oquat, B * 4); alloc(&e->d_olin, B * 3); alloc(&e->d_oang, B * 3);
    alloc(&e->d_contact, B * 4); alloc(&e->d_mode, B);
    HIP_CHECK(hipMemset(e->d_rbd, 0, B * 2 * e->nv * sizeof(double)));
    HIP_CHECK(hipMemset(e->d_xy_reset, 0, B * sizeof(int)));
    HIP_CHECK(hipMemcpy(e->d_rows + B * kEstParamStride, &e->defaults, sizeof(EstSettings), hipMemcpyHostToDevice));
    set_params_on_device(e.get(), max_batch, nullptr, e->d_rows + B * kEstParamStride, 1);
    set_state_on_device(e.get(), max_batch, nullptr, nullptr, nullptr, 1);
    HIP_CHECK(hipStreamSynchronize(e->stream));
    return BPMPC_OK;
  });
  if (rc != BPMPC_OK) { bpmpc_estimator_destroy(e.release()); return rc; }
  *out = e.release();
  return BPMPC_OK;
}

void bpmpc_estimator_destroy(bpmpc_estimator* e) {
  if (!e) return;
  if (e->stream) { (void)hipStreamSynchronize(e->stream); (void)hipStreamDestroy(e->stream); }
  if (e->ev_foreign) (void)hipEventDestroy(e->ev_foreign);
  if (e->ev_own) (void)hipEventDestroy(e->ev_own);
  for (void* p : {(void*)e->d_model, (void*)e->d_rbd, (void*)e->d_xhat, (void*)e->d_cov, (void*)e->d_xy_reset, (void*)e->d_params, (void*)e->d_rows, (void*)e->d_mask,
                  (void*)e->d_xhat_in, (void*)e->d_cov_in, (void*)e->d_jp, (void*)e->d_jv, (void*)e->d_quat, (void*)e->d_w, (void*)e->d_a, (void*)e->d_fh,
                  (void*)e->d_opos, (void*)e->d_oquat, (void*)e->d_olin, (void*)e->d_oang, (void*)e->d_contact, (void*)e->d_mode})
    if (p) (void)hipFree(p);
  delete e;
}

int bpmpc_estimator_update(bpmpc_estimator* e, int batch, const bpmpc_sensor_inputs* in, int inputs_on_device, double period, double* host_rbd) {
  if (!e || !in) { set_last_error("bpmpc_estimator_update: null handle or inputs"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    const bool kalman = e->kind == BPMPC_ESTIMATOR_KALMAN;
    if (!in->joint_pos || !in->joint_vel) throw std::invalid_argument("bpmpc_estimator_update: null joint_pos or joint_vel");
    if (kalman) {
      if (!in->quat || !in->angular_vel_local || !in->linear_accel_local)
        throw std::invalid_argument("bpmpc_estimator_update: the Kalman filter needs quat, angular_vel_local and linear_accel_local (null given)");
      if (!in->contact && !in->mode) throw std::invalid_argument("bpmpc_estimator_update: no contact source: give contact or mode");
      if (in->contact && in->mode) throw std::invalid_argument("bpmpc_estimator_update: two contact sources: give contact or mode, not both");
      if (!std::isfinite(period) || period < 0.0) throw std::invalid_argument("bpmpc_estimator_update: period must be finite and not negative");
    } else if (!in->odom_pos || !in->odom_quat || !in->odom_lin_vel || !in->odom_ang_vel) {
      throw std::invalid_argument("bpmpc_estimator_update: the from-topic estimator needs odom_pos, odom_quat, odom_lin_vel and odom_ang_vel (null given)");
    }
    check_batch(e, batch, "bpmpc_estimator_update");
    if (!inputs_on_device && kalman && in->mode)
      for (int b = 0; b < batch; ++b) if (in->mode[b] < 0 || in->mode[b] > 3) throw std::invalid_argument("bpmpc_estimator_update: mode must be 0..3");
    HIP_CHECK(hipSetDevice(e->device));
    const size_t B = batch;
    EstArgs a{};
    a.batch = batch; a.kind = e->kind; a.dt = period;
    auto in_d = [&](const double* src, double* staging, size_t per_robot) -> const double* {
      if (!src || inputs_on_device) return src;
      HIP_CHECK(hipMemcpyAsync(staging, src, B * per_robot * sizeof(double), hipMemcpyHostToDevice, e->stream));
      return staging;
    };
    auto in_i = [&](const int* src, int* staging, size_t per_robot) -> const int* {
      if (!src || inputs_on_device) return src;
      HIP_CHECK(hipMemcpyAsync(staging, src, B * per_robot * sizeof(int), hipMemcpyHostToDevice, e->stream));
      return staging;
    };
    a.joint_pos = in_d(in->joint_pos, e->d_jp, e->nj);
    a.joint_vel = in_d(in->joint_vel, e->d_jv, e->nj);
    if (kalman) {
      a.quat = in_d(in->quat, e->d_quat, 4);
      a.ang_local = in_d(in->angular_vel_local, e->d_w, 3);
      a.acc_local = in_d(in->linear_accel_local, e->d_a, 3);
      a.contact = in_i(in->contact, e->d_contact, 4);
      a.mode = in_i(in->mode, e->d_mode, 1);
      a.feet_heights = in_d(in->feet_heights, e->d_fh, 4);
    } else {
      a.odom_pos = in_d(in->odom_pos, e->d_opos, 3);
      a.odom_quat = in_d(in->odom_quat, e->d_oquat, 4);
      a.odom_lin = in_d(in->odom_lin_vel, e->d_olin, 3);
      a.odom_ang = in_d(in->odom_ang_vel, e->d_oang, 3);
    }
    a.params = e->d_params; a.x_hat = e->d_xhat; a.cov = e->d_cov; a.rbd = e->d_rbd; a.xy_reset = e->d_xy_reset;
    KL_NJ(e->nj, hipLaunchKernelGGL(k_estimate<NJ>, dim3(batch), dim3(kWave), 0, e->stream, e->d_model, a));
    HIP_CHECK(hipGetLastError());
    e->last_batch = batch;
    if (host_rbd) {
      HIP_CHECK(hipMemcpyAsync(host_rbd, e->d_rbd, B * 2 * e->nv * sizeof(double), hipMemcpyDeviceToHost, e->stream));
      HIP_CHECK(hipStreamSynchronize(e->stream));
      e->own_pending = false;
    } else {
      if (!inputs_on_device) HIP_CHECK(hipStreamSynchronize(e->stream));      // the caller's host arrays
      if (!e->ev_own) HIP_CHECK(hipEventCreateWithFlags(&e->ev_own, hipEventDisableTiming));
      HIP_CHECK(hipEventRecord(e->ev_own, e->stream));
      e->own_pending = true;
    }
  });
}

int bpmpc_estimator_device_outputs(bpmpc_estimator* e, bpmpc_estimator_outputs* o) {
  if (!e || !o) { set_last_error("bpmpc_estimator_device_outputs: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  o->rbd = e->d_rbd; o->x_hat = e->d_xhat; o->cov = e->d_cov; o->xy_reset = e->d_xy_reset;
  return BPMPC_OK;
}

int bpmpc_estimator_reset(bpmpc_estimator* e, int batch, const int* mask, int inputs_on_device) {
  if (!e) { set_last_error("bpmpc_estimator_reset: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    check_batch(e, batch, "bpmpc_estimator_reset");
    HIP_CHECK(hipSetDevice(e->device));
    const int* dmask = mask;
    if (mask && !inputs_on_device) {
      HIP_CHECK(hipMemcpyAsync(e->d_mask, mask, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, e->stream));
      dmask = e->d_mask;
    }
    set_state_on_device(e, batch, dmask, nullptr, nullptr, 1);
    if (!inputs_on_device) HIP_CHECK(hipStreamSynchronize(e->stream));
  });
}

int bpmpc_estimator_get_state(bpmpc_estimator* e, int batch, double* x_hat, double* cov) {
  if (!e) { set_last_error("bpmpc_estimator_get_state: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    check_batch(e, batch, "bpmpc_estimator_get_state");
    HIP_CHECK(hipSetDevice(e->device));
    const size_t B = batch, N = kEstStates;
    if (x_hat) HIP_CHECK(hipMemcpyAsync(x_hat, e->d_xhat, B * N * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (cov) HIP_CHECK(hipMemcpyAsync(cov, e->d_cov, B * N * N * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_CHECK(hipStreamSynchronize(e->stream));
  });
}

int bpmpc_estimator_set_state(bpmpc_estimator* e, int batch, const int* mask, const double* x_hat, const double* cov, int inputs_on_device) {
  if (!e || !x_hat) { set_last_error("bpmpc_estimator_set_state: null handle or x_hat"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    check_batch(e, batch, "bpmpc_estimator_set_state");
    HIP_CHECK(hipSetDevice(e->device));
    const size_t B = batch, N = kEstStates;
    const int* dmask = mask;
    const double *dx = x_hat, *dc = cov;
    if (!inputs_on_device) {
      for (size_t i = 0; i < B * N; ++i)
        if (!mask || mask[i / N]) if (!std::isfinite(x_hat[i])) throw std::invalid_argument("bpmpc_estimator_set_state: x_hat of robot " + std::to_string(i / N) + " is not finite");
      if (cov)
        for (size_t i = 0; i < B * N * N; ++i)
          if (!mask || mask[i / (N * N)]) if (!std::isfinite(cov[i])) throw std::invalid_argument("bpmpc_estimator_set_state: cov of robot " + std::to_string(i / (N * N)) + " is not finite");
      if (mask) { HIP_CHECK(hipMemcpyAsync(e->d_mask, mask, B * sizeof(int), hipMemcpyHostToDevice, e->stream)); dmask = e->d_mask; }
      HIP_CHECK(hipMemcpyAsync(e->d_xhat_in, x_hat, B * N * sizeof(double), hipMemcpyHostToDevice, e->stream));
      dx = e->d_xhat_in;
      if (cov) { HIP_CHECK(hipMemcpyAsync(e->d_cov_in, cov, B * N * N * sizeof(double), hipMemcpyHostToDevice, e->stream)); dc = e->d_cov_in; }
    }
    set_state_on_device(e, batch, dmask, dx, dc, 0);
    if (!inputs_on_device) HIP_CHECK(hipStreamSynchronize(e->stream));
  });
}

int bpmpc_estimator_get_params(const bpmpc_estimator* e, int robot, double* row) {
  if (!e || !row) { set_last_error("bpmpc_estimator_get_params: null handle or row"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    if (robot >= e->max_batch) throw std::length_error("bpmpc_estimator_get_params: robot exceeds max_batch");
    HIP_CHECK(hipSetDevice(e->device));
    const double* src = robot < 0 ? e->d_rows + (size_t)e->max_batch * kEstParamStride : e->d_params + (size_t)robot * kEstParamStride;
    HIP_CHECK(hipMemcpyAsync(row, src, sizeof(EstSettings), hipMemcpyDeviceToHost, e->stream));
    HIP_CHECK(hipStreamSynchronize(e->stream));
  });
}

int bpmpc_estimator_set_params(bpmpc_estimator* e, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  if (!e || !rows) { set_last_error("bpmpc_estimator_set_params: null handle or rows"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    check_batch(e, batch, "bpmpc_estimator_set_params");
    if (n_rows != 1 && n_rows != batch) throw std::invalid_argument("bpmpc_estimator_set_params: n_rows must be 1 or batch");
    HIP_CHECK(hipSetDevice(e->device));
    if (!inputs_on_device) {
      for (int r = 0; r < n_rows; ++r)
        if (n_rows == 1 || !mask || mask[r]) estimator_check_param_row("bpmpc_estimator_set_params", rows + (size_t)r * kEstParamStride, r);
      HIP_CHECK(hipMemcpyAsync(e->d_rows, rows, (size_t)n_rows * sizeof(EstSettings), hipMemcpyHostToDevice, e->stream));
      if (mask) HIP_CHECK(hipMemcpyAsync(e->d_mask, mask, (size_t)batch * sizeof(int), hipMemcpyHostToDevice, e->stream));
      set_params_on_device(e, batch, mask ? e->d_mask : nullptr, e->d_rows, n_rows);
      HIP_CHECK(hipStreamSynchronize(e->stream));
    } else {                            // only enqueued on the handle's stream: the next update runs behind it
      set_params_on_device(e, batch, mask, rows, n_rows);
    }
  });
}

int bpmpc_estimator_reset_params(bpmpc_estimator* e) {
  if (!e) { set_last_error("bpmpc_estimator_reset_params: null handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    HIP_CHECK(hipSetDevice(e->device));
    set_params_on_device(e, e->max_batch, nullptr, e->d_rows + (size_t)e->max_batch * kEstParamStride, 1);
    HIP_CHECK(hipStreamSynchronize(e->stream));
  });
}

}  // extern "C"
