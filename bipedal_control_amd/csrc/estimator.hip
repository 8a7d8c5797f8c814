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

}  // namespace bpmpc

using namespace bpmpc;

namespace {

void set_state_on_device(bpmpc_estimator* e, int batch, const int* mask, const double* x_in, const double* cov_in, int reset) {
  constexpr int E = kEstStates + kEstStates * kEstStates;
  hipLaunchKernelGGL(k_est_set_state, dim3((batch * E + 255) / 256), dim3(256), 0, e->hs.stream, batch, mask, x_in, cov_in, reset, e->d_xhat, e->d_cov);
  HIP_CHECK(hipGetLastError());
}

void check_batch(const bpmpc_estimator* e, int batch, const char* who) {
  if (batch < 1) throw std::invalid_argument(std::string(who) + ": batch must be positive");
  if (batch > e->max_batch) throw std::length_error(std::string(who) + ": batch exceeds max_batch");
}

}  // namespace

namespace bpmpc {

void estimator_before_foreign_read(bpmpc_estimator* e, int batch, hipStream_t stream) {
  if (batch > e->max_batch) throw std::length_error("bpmpc_controller_tick_estimated: batch exceeds the estimator's max_batch");
  if (batch != e->last_batch)
    throw std::invalid_argument("bpmpc_controller_tick_estimated: batch " + std::to_string(batch) + " differs from the batch of the estimator's last update (" +
                                std::to_string(e->last_batch) + "): the other rows of rbd hold no estimate of this tick");
  e->hs.before_foreign(stream);
}

void estimator_after_foreign_read(bpmpc_estimator* e, hipStream_t stream) { e->hs.after_foreign(stream); }

}  // namespace bpmpc

extern "C" {

int bpmpc_estimator_create(const bpmpc_model* model, const char* task_info_path, int kind, int device, int max_batch, bpmpc_estimator** out) {
  if (!model || !out) { set_last_error("bpmpc_estimator_create: null model or output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  if (max_batch < 1 || (kind != BPMPC_ESTIMATOR_FROM_TOPIC && kind != BPMPC_ESTIMATOR_KALMAN)) {
    set_last_error("bpmpc_estimator_create: kind must be BPMPC_ESTIMATOR_FROM_TOPIC or BPMPC_ESTIMATOR_KALMAN and max_batch positive");
    return BPMPC_ERR_INVALID_ARGUMENT;
  }
  std::unique_ptr<bpmpc_estimator> e(new bpmpc_estimator);
  const int rc = guarded(BPMPC_ERR_IO, [&]() -> int {
    if (const int refused = open_side_handle("bpmpc_estimator_create", e.get(), model, device, max_batch)) return refused;
    e->defaults = estimator_load_settings(task_info_path);
    e->kind = kind; e->nj = e->rm.nj; e->nv = 6 + e->rm.nj;
    const size_t B = max_batch, N = kEstStates, nj = e->nj;
    DeviceBuffers& m = e->mem;
    e->d_rbd = m.alloc<double>(B * 2 * e->nv, true); e->d_xhat = m.alloc<double>(B * N); e->d_cov = m.alloc<double>(B * N * N); e->d_xy_reset = m.alloc<int>(B, true);
    e->d_mask = m.alloc<int>(B);
    e->d_xhat_in = m.alloc<double>(B * N); e->d_cov_in = m.alloc<double>(B * N * N);
    e->d_jp = m.alloc<double>(B * nj); e->d_jv = m.alloc<double>(B * nj); e->d_quat = m.alloc<double>(B * 4); e->d_w = m.alloc<double>(B * 3); e->d_a = m.alloc<double>(B * 3);
    e->d_fh = m.alloc<double>(B * 4); e->d_opos = m.alloc<double>(B * 3); e->d_oquat = m.alloc<double>(B * 4); e->d_olin = m.alloc<double>(B * 3); e->d_oang = m.alloc<double>(B * 3);
    e->d_contact = m.alloc<int>(B * 4); e->d_mode = m.alloc<int>(B);
    e->params.create(m, max_batch, kEstParamStride, kEstParamStride - 1, &e->defaults.foot_radius);
    e->params.fill_from_start(e->hs.stream, max_batch);
    set_state_on_device(e.get(), max_batch, nullptr, nullptr, nullptr, 1);
    HIP_CHECK(hipStreamSynchronize(e->hs.stream));
    return BPMPC_OK;
  });
  if (rc != BPMPC_OK) { bpmpc_estimator_destroy(e.release()); return rc; }
  *out = e.release();
  return BPMPC_OK;
}

void bpmpc_estimator_destroy(bpmpc_estimator* e) { close_side_handle(e); }

int bpmpc_estimator_update(bpmpc_estimator* e, int batch, const bpmpc_sensor_inputs* in, int inputs_on_device, double period, double* host_rbd) {
  return guarded(e, BPMPC_ERR_IO, "bpmpc_estimator_update: null handle or inputs", in != nullptr, [&] {
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
    const size_t B = batch;
    EstArgs a{};
    a.batch = batch; a.kind = e->kind; a.dt = period;
    auto input = [&](auto* src, auto* staging, size_t per_robot) { return staged(src, staging, B * per_robot, inputs_on_device, e->hs.stream); };
    a.joint_pos = input(in->joint_pos, e->d_jp, e->nj);
    a.joint_vel = input(in->joint_vel, e->d_jv, e->nj);
    if (kalman) {
      a.quat = input(in->quat, e->d_quat, 4);
      a.ang_local = input(in->angular_vel_local, e->d_w, 3);
      a.acc_local = input(in->linear_accel_local, e->d_a, 3);
      a.contact = input(in->contact, e->d_contact, 4);
      a.mode = input(in->mode, e->d_mode, 1);
      a.feet_heights = input(in->feet_heights, e->d_fh, 4);
    } else {
      a.odom_pos = input(in->odom_pos, e->d_opos, 3);
      a.odom_quat = input(in->odom_quat, e->d_oquat, 4);
      a.odom_lin = input(in->odom_lin_vel, e->d_olin, 3);
      a.odom_ang = input(in->odom_ang_vel, e->d_oang, 3);
    }
    a.params = e->params.d_params; a.x_hat = e->d_xhat; a.cov = e->d_cov; a.rbd = e->d_rbd; a.xy_reset = e->d_xy_reset;
    KL_NJ(e->nj, hipLaunchKernelGGL(k_estimate<NJ>, dim3(batch), dim3(kWave), 0, e->hs.stream, e->d_model, a));
    HIP_CHECK(hipGetLastError());
    e->last_batch = batch;
    if (host_rbd) {
      HIP_CHECK(hipMemcpyAsync(host_rbd, e->d_rbd, B * 2 * e->nv * sizeof(double), hipMemcpyDeviceToHost, e->hs.stream));
      e->hs.synchronise_own();
    } else {
      if (!inputs_on_device) HIP_CHECK(hipStreamSynchronize(e->hs.stream));      // the caller's host arrays
      e->hs.enqueued_own();      // rbd stays on the device: the next controller tick on another stream waits for it
    }
  });
}

int bpmpc_estimator_device_outputs(bpmpc_estimator* e, bpmpc_estimator_outputs* o) {
  if (!e || !o) { set_last_error("bpmpc_estimator_device_outputs: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  o->rbd = e->d_rbd; o->x_hat = e->d_xhat; o->cov = e->d_cov; o->xy_reset = e->d_xy_reset;
  return BPMPC_OK;
}

int bpmpc_estimator_reset(bpmpc_estimator* e, int batch, const int* mask, int inputs_on_device) {
  return guarded(e, BPMPC_ERR_IO, "bpmpc_estimator_reset: null handle", [&] {
    check_batch(e, batch, "bpmpc_estimator_reset");
    set_state_on_device(e, batch, staged(mask, e->d_mask, batch, inputs_on_device, e->hs.stream), nullptr, nullptr, 1);
    if (!inputs_on_device) HIP_CHECK(hipStreamSynchronize(e->hs.stream));
  });
}

int bpmpc_estimator_get_state(bpmpc_estimator* e, int batch, double* x_hat, double* cov) {
  return guarded(e, BPMPC_ERR_IO, "bpmpc_estimator_get_state: null handle", [&] {
    check_batch(e, batch, "bpmpc_estimator_get_state");
    const size_t B = batch, N = kEstStates;
    if (x_hat) HIP_CHECK(hipMemcpyAsync(x_hat, e->d_xhat, B * N * sizeof(double), hipMemcpyDeviceToHost, e->hs.stream));
    if (cov) HIP_CHECK(hipMemcpyAsync(cov, e->d_cov, B * N * N * sizeof(double), hipMemcpyDeviceToHost, e->hs.stream));
    HIP_CHECK(hipStreamSynchronize(e->hs.stream));
  });
}

int bpmpc_estimator_set_state(bpmpc_estimator* e, int batch, const int* mask, const double* x_hat, const double* cov, int inputs_on_device) {
  return guarded(e, BPMPC_ERR_IO, "bpmpc_estimator_set_state: null handle or x_hat", x_hat != nullptr, [&] {
    check_batch(e, batch, "bpmpc_estimator_set_state");
    const size_t B = batch, N = kEstStates;
    if (!inputs_on_device) {
      for (size_t i = 0; i < B * N; ++i)
        if (!mask || mask[i / N]) if (!std::isfinite(x_hat[i])) throw std::invalid_argument("bpmpc_estimator_set_state: x_hat of robot " + std::to_string(i / N) + " is not finite");
      if (cov)
        for (size_t i = 0; i < B * N * N; ++i)
          if (!mask || mask[i / (N * N)]) if (!std::isfinite(cov[i])) throw std::invalid_argument("bpmpc_estimator_set_state: cov of robot " + std::to_string(i / (N * N)) + " is not finite");
    }
    hipStream_t st = e->hs.stream;
    set_state_on_device(e, batch, staged(mask, e->d_mask, B, inputs_on_device, st), staged(x_hat, e->d_xhat_in, B * N, inputs_on_device, st),
                        staged(cov, e->d_cov_in, B * N * N, inputs_on_device, st), 0);
    if (!inputs_on_device) HIP_CHECK(hipStreamSynchronize(e->hs.stream));
  });
}

int bpmpc_estimator_get_params(const bpmpc_estimator* e, int robot, double* row) {
  return guarded(e, BPMPC_ERR_IO, "bpmpc_estimator_get_params: null handle or row", row != nullptr, [&] {
    e->params.get("bpmpc_estimator_get_params", e->hs.stream, e->max_batch, robot, row);
  });
}

int bpmpc_estimator_set_params(bpmpc_estimator* e, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  return guarded(e, BPMPC_ERR_IO, "bpmpc_estimator_set_params: null handle or rows", rows != nullptr, [&] {
    check_batch(e, batch, "bpmpc_estimator_set_params");
    e->params.set("bpmpc_estimator_set_params", e->hs.stream, batch, mask, e->d_mask, rows, n_rows, inputs_on_device,
                  [](const double* row, int r) { estimator_check_param_row("bpmpc_estimator_set_params", row, r); });
    e->hs.finish(inputs_on_device);      // device rows are only enqueued on the handle's stream: the next update runs behind them
  });
}

int bpmpc_estimator_reset_params(bpmpc_estimator* e) {
  return guarded(e, BPMPC_ERR_IO, "bpmpc_estimator_reset_params: null handle", [&] {
    e->params.fill_from_start(e->hs.stream, e->max_batch);
    e->hs.synchronise_own();
  });
}

}  // extern "C"
