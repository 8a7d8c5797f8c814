// Event timers per kernel class (bpmpc_solver_kernel_time): the solver handle owns one KernelTimers and passes its profile level and the stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "capi_internal.h"

namespace bpmpc {

struct KernelTimer {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double total_ms = 0.0;
  int launches = 0;
};

struct KernelTimers {
  std::map<std::string, KernelTimer> by_class;

  // Events that only measure time: no system-scope fence when they complete (hipEventDisableSystemFence: "avoiding the cost of cache writeback and
  // invalidation, and the performance impact of those actions on the execution of following work") - with the default flags the step that carries
  // the roofline kernel's events ran 3 % slower than the steps without them (the kernel behind the lineariser found its inputs flushed from L2)
  static constexpr unsigned kTimingEventFlags = hipEventDisableSystemFence;
  // profile (settings.profile): 0 off, 1 every kernel class, 2 the linearisation kernel only (the roofline measurement of bench.py: every
  // event pair costs one to two microseconds of stream time, ten pairs per solve are 2 % of a step)
  static bool timed(int profile, const char* cls) { return profile == 1 || (profile == 2 && std::strcmp(cls, "linearize") == 0); }

  // a pair of hipEventRecord calls around one launch or a short sequence of launches on `on` (TIMED / TIMED_ON of solver.hip)
  void begin(int profile, hipStream_t on, const char* cls, hipEvent_t* a, hipEvent_t* b) {
    if (!timed(profile, cls)) return;
    create_pair(a, b);
    if (hipEventRecord(*a, on) != hipSuccess) { destroy_pair(*a, *b); throw DeviceError("hipEventRecord failed"); }
  }
  void end(int profile, hipStream_t on, const char* cls, hipEvent_t a, hipEvent_t b) {
    if (!timed(profile, cls)) return;
    HIP_CHECK(hipEventRecord(b, on));
    keep(cls, a, b);
  }
  // launch(a, b) attaches the pair to its dispatch: the elapsed time is the kernel's duration, without the barrier packets and the dispatch latency
  // a pair of hipEventRecord calls brackets as well
  template <typename F>
  void attached(const char* cls, F&& launch) {
    hipEvent_t a, b;
    create_pair(&a, &b);
    try { launch(a, b); } catch (...) { destroy_pair(a, b); throw; }
    keep(cls, a, b);
  }
  void collect() {
    for (auto& kv : by_class) {
      hipError_t first_error = hipSuccess;                 // the events are destroyed whatever happens; the first failure is reported afterwards
      for (auto& pr : kv.second.pending) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(pr.second);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, pr.first, pr.second);
        if (e == hipSuccess) { kv.second.total_ms += ms; kv.second.launches += 1; }
        else if (first_error == hipSuccess) first_error = e;
        destroy_pair(pr.first, pr.second);
      }
      kv.second.pending.clear();
      if (first_error != hipSuccess) throw DeviceError(std::string("kernel timers: ") + hipGetErrorString(first_error));
    }
  }

 private:
  // an event pair: both are created or none, both are destroyed
  static void destroy_pair(hipEvent_t a, hipEvent_t b) { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
  static void create_pair(hipEvent_t* a, hipEvent_t* b) {
    HIP_CHECK(hipEventCreateWithFlags(a, kTimingEventFlags));
    if (hipEventCreateWithFlags(b, kTimingEventFlags) != hipSuccess) { (void)hipEventDestroy(*a); throw DeviceError("hipEventCreate failed"); }
  }
  void keep(const char* cls, hipEvent_t a, hipEvent_t b) {
    KernelTimer& t = by_class[cls];
    t.pending.emplace_back(a, b);
    if (t.pending.size() > 4096) collect();   // a profiled loop that never asks for the times must not grow without bound
  }
};

}  // namespace bpmpc
