// What the device handles beside the solver (bpmpc_wbc, bpmpc_estimator, bpmpc_controller; the gait batch for its memory) share on the host:
// owned device buffers, the handshake between a handle's own stream and another handle's, the staging of host inputs, the masked per-robot
// row write (device_handle.hip) and the per-robot row table it fills, opening and entering a handle.  Plain structs and free functions; the kernels stay with their handles.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "device_model.h"

namespace bpmpc {

// The device memory of a handle: every buffer comes from alloc, release frees them all.
struct DeviceBuffers {
  std::vector<void*> owned;
  template <typename T>
  T* alloc(size_t count, bool zero = false) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16)));
    owned.push_back(p);
    if (zero) HIP_CHECK(hipMemset(p, 0, count * sizeof(T)));
    return static_cast<T*>(p);
  }
  void release() {
    for (void* p : owned) (void)hipFree(p);
    owned.clear();
  }
};

// A handle's own stream and its ordering against launches that another handle enqueues on a foreign stream (the controller tick on the
// solver's): work only enqueued on the own stream is waited for by the next foreign launch, and the own stream waits for a foreign launch.
struct StreamHandshake {
  hipStream_t stream = nullptr;
  hipEvent_t ev_own = nullptr, ev_foreign = nullptr;      // created on first use
  bool own_pending = false;                               // ev_own marks work that no synchronise has waited for

  // around a launch that touches the handle's buffers on `foreign` (the own stream itself: in order already, no events)
  void before_foreign(hipStream_t foreign) {
    if (foreign != stream && own_pending) HIP_CHECK(hipStreamWaitEvent(foreign, ev_own, 0));
  }
  void after_foreign(hipStream_t foreign) {
    if (foreign == stream) return;
    record(&ev_foreign, foreign);
    HIP_CHECK(hipStreamWaitEvent(stream, ev_foreign, 0));
  }
  // work was enqueued on the own stream and the call returns without a synchronise
  void enqueued_own() {
    record(&ev_own, stream);
    own_pending = true;
  }
  // the own stream is drained: nothing is left for a foreign launch to wait for
  void synchronise_own() {
    HIP_CHECK(hipStreamSynchronize(stream));
    own_pending = false;
  }
  // the end of a call that enqueued on the own stream: host inputs are waited for (the caller's arrays), device inputs are only enqueued
  void finish(bool on_device) {
    if (!on_device) synchronise_own();
    else enqueued_own();
  }
  void destroy() {
    if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    if (ev_foreign) (void)hipEventDestroy(ev_foreign);
    if (ev_own) (void)hipEventDestroy(ev_own);
  }
  // `*ev` (created on first use) marks what has been enqueued on `on` so far; also for the events a handle keeps beside these two
  static void record(hipEvent_t* ev, hipStream_t on) {
    if (!*ev) HIP_CHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(*ev, on));
  }
};

// An input as the kernels read it: a host array (inputs_on_device == 0) is copied into `staging` on `stream`, a device array or NULL is returned as it is.
template <typename T>
const T* staged(const T* src, T* staging, size_t count, bool on_device, hipStream_t stream) {
  if (!src || on_device) return src;
  HIP_CHECK(hipMemcpyAsync(staging, src, count * sizeof(T), hipMemcpyHostToDevice, stream));
  return staging;
}

// One source of a masked row write, its device copy when it comes from the host, and the rows it is written to ([batch][width])
struct RowPair {
  const double* src = nullptr;
  double* staging = nullptr;
  double* dst = nullptr;
};

// device_handle.hip: dst[b] of the robots of `mask` (device; NULL: every robot below `batch`) becomes src[b] (n_rows == batch) or src[0]
// (n_rows == 1) in its first `used` entries and 0 behind them; one launch for one or two pairs of device rows
void write_rows(hipStream_t stream, int batch, int width, int used, const int* mask, int n_rows, const RowPair& a, const RowPair& b = {});

// A set_params / set_joint_gains call of entry point `who` behind its batch check: n_rows is 1 or batch, check_row(r) throws for a host row
// that a selected robot would take, host rows and mask are staged, write_rows is enqueued on `stream`.  Nothing is enqueued after a refusal.
template <typename CheckRow>
void set_rows(const char* who, hipStream_t stream, int batch, int width, int used, const int* mask, int* mask_staging, int n_rows, bool on_device,
              CheckRow&& check_row, RowPair a, RowPair b = {}) {
  if (n_rows != 1 && n_rows != batch) throw std::invalid_argument(std::string(who) + ": n_rows must be 1 or batch");
  if (!on_device)
    for (int r = 0; r < n_rows; ++r)
      if (n_rows == 1 || !mask || mask[r]) check_row(r);
  mask = staged(mask, mask_staging, batch, on_device, stream);
  a.src = staged(a.src, a.staging, (size_t)n_rows * width, on_device, stream);
  b.src = staged(b.src, b.staging, (size_t)n_rows * width, on_device, stream);
  write_rows(stream, batch, width, used, mask, n_rows, a, b);
}

// A per-robot row table of a handle: d_params [max_batch][stride], which the kernels read, and d_rows [max_batch + 1][stride], the device copy
// of host rows, whose last row holds the start row.  A written row keeps its first `used` entries; the others read 0.
struct ParamTable {
  int stride = 0, used = 0;
  double* d_params = nullptr;
  double* d_rows = nullptr;

  void create(DeviceBuffers& mem, int max_batch, int stride_, int used_, const double* start_row) {
    stride = stride_; used = used_;
    d_params = mem.alloc<double>((size_t)max_batch * stride);
    d_rows = mem.alloc<double>((size_t)(max_batch + 1) * stride);
    HIP_CHECK(hipMemcpy(start(max_batch), start_row, stride * sizeof(double), hipMemcpyHostToDevice));
  }
  double* start(int max_batch) const { return d_rows + (size_t)max_batch * stride; }
  double* row(int b) const { return d_params + (size_t)b * stride; }
  // every robot's row becomes the start row; enqueued on `stream`
  void fill_from_start(hipStream_t stream, int max_batch) { write_rows(stream, max_batch, stride, used, nullptr, 1, {start(max_batch), nullptr, d_params}); }
  // out[stride] = the row of `robot`, or with robot < 0 the start row; synchronises `stream`
  void get(const char* who, hipStream_t stream, int max_batch, int robot, double* out) const {
    if (robot >= max_batch) throw std::length_error(std::string(who) + ": robot exceeds max_batch");
    HIP_CHECK(hipMemcpyAsync(out, robot < 0 ? start(max_batch) : row(robot), stride * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  // set_rows on the table's own pair; check_row(row, r) throws for host row r
  template <typename CheckRow>
  void set(const char* who, hipStream_t stream, int batch, const int* mask, int* mask_staging, const double* rows, int n_rows, bool on_device, CheckRow&& check_row) {
    set_rows(who, stream, batch, stride, used, mask, mask_staging, n_rows, on_device, [&](int r) { check_row(rows + (size_t)r * stride, r); }, {rows, d_rows, d_params});
  }
};

// What bpmpc_wbc_create and bpmpc_estimator_create (`who`) begin with, inside their guard: the device and the joint count are refused (status
// returned, bpmpc_last_error() set), then the device model, the handle's non-blocking stream and the model on the device.
template <typename H>
int open_side_handle(const char* who, H* h, const bpmpc_model* model, int device, int max_batch) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1 || device < 0 || device >= count) {
    set_last_error(std::string(who) + ": no usable HIP device (this engine has no CPU path)");
    return BPMPC_ERR_NO_DEVICE;
  }
  h->rm = model_of(model);
  if (h->rm.nj != 10 && h->rm.nj != 12) { set_last_error("only 10- and 12-joint bipeds are instantiated"); return BPMPC_ERR_UNSUPPORTED; }
  h->dm = make_device_model(h->rm);
  h->device = device; h->max_batch = max_batch;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipStreamCreateWithFlags(&h->hs.stream, hipStreamNonBlocking));
  h->d_model = h->mem.template alloc<DeviceModel>(1);
  HIP_CHECK(hipMemcpy(h->d_model, &h->dm, sizeof(DeviceModel), hipMemcpyHostToDevice));
  return BPMPC_OK;
}

template <typename H>
void close_side_handle(H* h) {
  if (!h) return;
  if (h->hs.stream || !h->mem.owned.empty()) (void)hipSetDevice(h->device);      // a create refused before it set the device leaves the caller's
  h->hs.destroy();
  h->mem.release();
  delete h;
}

// The guard of the entry points on these handles, as guarded(bpmpc_solver*, ...): a null handle (or another required pointer that is missing:
// `arguments_given` false) is refused with `null_message`, the handle's device is set, then the body runs under guarded(fallback, ...).
template <typename H, typename F>
int guarded(H* h, int fallback, const char* null_message, bool arguments_given, F&& body) {
  if (!h || !arguments_given) { set_last_error(null_message); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(fallback, [&] { HIP_CHECK(hipSetDevice(h->device)); return body(); });
}
template <typename H, typename F>
int guarded(H* h, int fallback, const char* null_message, F&& body) { return guarded(h, fallback, null_message, true, body); }

}  // namespace bpmpc
