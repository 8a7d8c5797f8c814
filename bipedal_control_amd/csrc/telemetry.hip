// k_telemetry (kernels/telemetry.h) and the host side of its handle: the C ABI of include/bpmpc.h "Tracking telemetry".
//   DebugPublisher::update               bipedal_controllers/src/debug/DebugPublisher.cpp, called at BipedalController.cpp:270
// A translation unit of its own: the tick, WBC and plant kernels are compiled as they were before the telemetry existed, and a controller
// without an attached handle launches nothing of this unit.
#include <hip/hip_runtime.h>

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "kernel_launchers.h"
#include "telemetry.h"
#include "kernels/telemetry.h"

static_assert(bpmpc::kTelStatsStride == BPMPC_TELEMETRY_STATS_STRIDE, "the statistics row follows include/bpmpc.h");
static_assert(bpmpc::telemetry_sample_stride(10) == BPMPC_TELEMETRY_SAMPLE_STRIDE(10), "the sample follows include/bpmpc.h");

namespace bpmpc {

template <int NJ>
__global__ __launch_bounds__(kWave) void k_telemetry(const DeviceModel* model, TelemetryArgs a) {
  __shared__ TelemetryLds<NJ> w;
  telemetry_robot<NJ>(*model, w, a);
}

// bpmpc_telemetry_reset for the robots of `mask` (NULL: every robot below `batch`): counters and flag 0, the statistics row 0 with
// first_unsafe_n = -1, the last sample 0.  One thread per entry of [row | sample]; the ring is left as it is (its count is 0).
__global__ __launch_bounds__(256) void k_telemetry_reset(int batch, const int* mask, int stride, double* stats, double* sample, int* frozen, int* count) {
  const int E = kTelStatsStride + stride;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= batch * E) return;
  const int b = i / E, e = i % E;
  if (mask && !mask[b]) return;
  if (e < kTelStatsStride) stats[(size_t)b * kTelStatsStride + e] = e == kTelFirstUnsafe ? -1.0 : 0.0;
  else sample[(size_t)b * stride + e - kTelStatsStride] = 0.0;
  if (e == 0) { frozen[b] = 0; count[2 * b] = 0; count[2 * b + 1] = 0; }
}

}  // namespace bpmpc

using namespace bpmpc;

namespace {

void check_batch(const bpmpc_telemetry* tm, int batch, const char* who) {
  if (batch < 1) throw std::invalid_argument(std::string(who) + ": batch must be positive");
  if (batch > tm->max_batch) throw std::length_error(std::string(who) + ": batch exceeds max_batch");
}

void launch(bpmpc_telemetry* tm, int batch, const double* t, const double* x_opt, const double* rbd, const int* safe, const int* mode, hipStream_t st) {
  TelemetryArgs a{};
  a.batch = batch; a.ring_len = tm->ring_len; a.every = tm->every; a.freeze = tm->freeze_on_unsafe;
  a.t = t; a.x_opt = x_opt; a.rbd = rbd; a.safe = safe; a.mode = mode;
  a.sample = tm->d_sample; a.stats = tm->d_stats; a.ring = tm->d_ring; a.frozen = tm->d_frozen; a.count = tm->d_count;
  KL_NJ(tm->nj, hipLaunchKernelGGL(k_telemetry<NJ>, dim3((batch + LinFastCfg<NJ>::NPW - 1) / LinFastCfg<NJ>::NPW), dim3(kWave), 0, st, tm->d_model, a));
  HIP_CHECK(hipGetLastError());
}

void reset_on_device(bpmpc_telemetry* tm, int batch, const int* mask) {
  const int E = kTelStatsStride + tm->stride;
  hipLaunchKernelGGL(k_telemetry_reset, dim3((batch * E + 255) / 256), dim3(256), 0, tm->hs.stream, batch, mask, tm->stride, tm->d_stats, tm->d_sample,
                     tm->d_frozen, tm->d_count);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

namespace bpmpc {

void telemetry_launch_on(bpmpc_telemetry* tm, int batch, const double* t, const double* x_opt, const double* rbd, const int* safe, const int* mode,
                         hipStream_t stream) {
  tm->hs.before_foreign(stream);
  launch(tm, batch, t, x_opt, rbd, safe, mode, stream);
  tm->hs.after_foreign(stream);
}

}  // namespace bpmpc

extern "C" {

int bpmpc_telemetry_create(const bpmpc_model* model, int device, int max_batch, int ring_len, bpmpc_telemetry** out) {
  if (!model || !out) { set_last_error("bpmpc_telemetry_create: null model or output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  if (max_batch < 1) { set_last_error("bpmpc_telemetry_create: max_batch must be positive"); return BPMPC_ERR_INVALID_ARGUMENT; }
  if (ring_len < 0) { set_last_error("bpmpc_telemetry_create: ring_len must not be negative"); return BPMPC_ERR_INVALID_ARGUMENT; }
  std::unique_ptr<bpmpc_telemetry> tm(new bpmpc_telemetry);
  const int rc = guarded(BPMPC_ERR_DEVICE, [&]() -> int {
    if (const int refused = open_side_handle("bpmpc_telemetry_create", tm.get(), model, device, max_batch)) return refused;
    tm->nj = tm->rm.nj; tm->nx = 12 + tm->nj; tm->nv = 6 + tm->nj; tm->stride = telemetry_sample_stride(tm->nj); tm->ring_len = ring_len;
    const size_t B = max_batch, S = tm->stride;
    DeviceBuffers& m = tm->mem;
    tm->d_sample = m.alloc<double>(B * S); tm->d_stats = m.alloc<double>(B * kTelStatsStride); tm->d_ring = m.alloc<double>(B * ring_len * S, true);
    tm->d_frozen = m.alloc<int>(B); tm->d_count = m.alloc<int>(2 * B);
    tm->d_t = m.alloc<double>(B); tm->d_xopt = m.alloc<double>(B * tm->nx); tm->d_rbd = m.alloc<double>(B * 2 * tm->nv);
    tm->d_safe = m.alloc<int>(B); tm->d_mode = m.alloc<int>(B); tm->d_mask = m.alloc<int>(B);
    reset_on_device(tm.get(), max_batch, nullptr);
    HIP_CHECK(hipDeviceSynchronize());      // the zero fill of the ring runs on the null stream
    return BPMPC_OK;
  });
  if (rc != BPMPC_OK) { bpmpc_telemetry_destroy(tm.release()); return rc; }
  *out = tm.release();
  return BPMPC_OK;
}

void bpmpc_telemetry_destroy(bpmpc_telemetry* tm) {
  if (tm && tm->hs.stream) { (void)hipSetDevice(tm->device); (void)hipDeviceSynchronize(); }      // a tick's launch may still be in flight on a controller's stream
  close_side_handle(tm);
}

int bpmpc_telemetry_dims(const bpmpc_telemetry* tm, int* sample_stride, int* stats_stride, int* ring_len) {
  if (!tm) { set_last_error("bpmpc_telemetry_dims: null telemetry handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  if (sample_stride) *sample_stride = tm->stride;
  if (stats_stride) *stats_stride = kTelStatsStride;
  if (ring_len) *ring_len = tm->ring_len;
  return BPMPC_OK;
}

int bpmpc_telemetry_update(bpmpc_telemetry* tm, int batch, const double* t, const double* x_opt, const double* rbd, const int* safe,
                           const int* planned_mode, int inputs_on_device) {
  return guarded(tm, BPMPC_ERR_DEVICE, "bpmpc_telemetry_update: null handle, x_opt or rbd", x_opt && rbd, [&] {
    check_batch(tm, batch, "bpmpc_telemetry_update");
    hipStream_t st = tm->hs.stream;
    const size_t B = batch;
    const bool dev = inputs_on_device != 0;
    launch(tm, batch, staged(t, tm->d_t, B, dev, st), staged(x_opt, tm->d_xopt, B * tm->nx, dev, st), staged(rbd, tm->d_rbd, B * 2 * tm->nv, dev, st),
           staged(safe, tm->d_safe, B, dev, st), staged(planned_mode, tm->d_mode, B, dev, st), st);
    tm->hs.finish(dev);      // host arrays are the caller's; the next tick of a controller this handle is attached to waits for what was only enqueued
  });
}

int bpmpc_telemetry_configure(bpmpc_telemetry* tm, int every, int freeze_on_unsafe) {
  return guarded(tm, BPMPC_ERR_DEVICE, "bpmpc_telemetry_configure: null telemetry handle", [&] {
    if (every < 1) throw std::invalid_argument("bpmpc_telemetry_configure: every must be at least 1");
    tm->every = every; tm->freeze_on_unsafe = freeze_on_unsafe != 0;
  });
}

int bpmpc_telemetry_reset(bpmpc_telemetry* tm, int batch, const int* mask, int inputs_on_device) {
  return guarded(tm, BPMPC_ERR_DEVICE, "bpmpc_telemetry_reset: null telemetry handle", [&] {
    check_batch(tm, batch, "bpmpc_telemetry_reset");
    reset_on_device(tm, batch, staged(mask, tm->d_mask, batch, inputs_on_device != 0, tm->hs.stream));
    if (mask && !inputs_on_device) tm->hs.synchronise_own();      // the caller's host mask
    else tm->hs.enqueued_own();
  });
}

int bpmpc_telemetry_device_outputs(bpmpc_telemetry* tm, double** sample, double** stats, int** frozen) {
  if (!tm) { set_last_error("bpmpc_telemetry_device_outputs: null telemetry handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  if (sample) *sample = tm->d_sample;
  if (stats) *stats = tm->d_stats;
  if (frozen) *frozen = tm->d_frozen;
  return BPMPC_OK;
}

int bpmpc_telemetry_get_stats(bpmpc_telemetry* tm, int batch, double* host_stats, int* host_frozen) {
  return guarded(tm, BPMPC_ERR_DEVICE, "bpmpc_telemetry_get_stats: null telemetry handle", [&] {
    check_batch(tm, batch, "bpmpc_telemetry_get_stats");
    hipStream_t st = tm->hs.stream;
    if (host_stats) HIP_CHECK(hipMemcpyAsync(host_stats, tm->d_stats, (size_t)batch * kTelStatsStride * sizeof(double), hipMemcpyDeviceToHost, st));
    if (host_frozen) HIP_CHECK(hipMemcpyAsync(host_frozen, tm->d_frozen, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
    tm->hs.synchronise_own();
  });
}

int bpmpc_telemetry_fetch_ring(bpmpc_telemetry* tm, int batch, const int* robots, int n_robots, double* host_samples, int* host_counts) {
  return guarded(tm, BPMPC_ERR_DEVICE, "bpmpc_telemetry_fetch_ring: null handle or host_counts", host_counts != nullptr, [&] {
    check_batch(tm, batch, "bpmpc_telemetry_fetch_ring");
    if (!robots) n_robots = batch;
    if (n_robots < 0) throw std::invalid_argument("bpmpc_telemetry_fetch_ring: n_robots must not be negative");
    for (int r = 0; robots && r < n_robots; ++r)
      if (robots[r] < 0 || robots[r] >= batch)
        throw std::invalid_argument("bpmpc_telemetry_fetch_ring: robots[" + std::to_string(r) + "] = " + std::to_string(robots[r]) + " lies outside the batch");
    hipStream_t st = tm->hs.stream;
    std::vector<int> count(2 * (size_t)batch);
    HIP_CHECK(hipMemcpyAsync(count.data(), tm->d_count, count.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    tm->hs.synchronise_own();
    const size_t L = tm->ring_len, S = tm->stride;
    for (int r = 0; r < n_robots; ++r) {
      const size_t b = robots ? robots[r] : r, rec = count[2 * b + 1];
      const size_t have = rec < L ? rec : L, first = rec <= L ? 0 : rec % L;     // the oldest sample's slot (ring_len 0: nothing was recorded)
      host_counts[r] = (int)have;
      if (!host_samples || have == 0) continue;
      const double* ring = tm->d_ring + b * L * S;
      double* dst = host_samples + (size_t)r * L * S;
      const size_t head = have - first;                                            // slots first .. have - 1, then 0 .. first - 1
      HIP_CHECK(hipMemcpyAsync(dst, ring + first * S, head * S * sizeof(double), hipMemcpyDeviceToHost, st));
      if (first) HIP_CHECK(hipMemcpyAsync(dst + head * S, ring, first * S * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    tm->hs.synchronise_own();
  });
}

}  // extern "C"
