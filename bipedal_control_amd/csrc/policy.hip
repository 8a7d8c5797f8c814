// Host side and kernels of the policy buffer (policy.h; include/bpmpc.h "Policy buffer"): MPC_MRT_Interface::updatePolicy for a batch.
//   publish   k_policy_publish on the SOLVER's stream, behind the run whose solution it copies and behind the last adoption
//   update    k_policy_adopt on the BUFFER's stream, behind the last publish; the host flips the slot the next ticks are handed
// Nothing here synchronises the host except bpmpc_policy_info, a host mask of publish, create and destroy.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "policy.h"
#include "solver.h"

namespace bpmpc {

namespace {

constexpr int kPublishThreads = 256;

// `count` 16-byte words from src to dst, word i of this workgroup's share: i = first, first + stride, ..  Four loads in flight per lane.
__device__ __forceinline__ void copy_words(double2* __restrict__ dst, const double2* __restrict__ src, int count, int first, int stride) {
  int i = first;
  for (; i + 3 * stride < count; i += 4 * stride) {
    const double2 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
  }
  for (; i < count; i += stride) dst[i] = src[i];
}

}  // namespace

// A masked gather-copy: gridDim.x / wg_per_robot robots at a time, wg_per_robot workgroups on each.  Every decision depends on the robot alone,
// so a workgroup takes or leaves a robot as a whole.  x, u and K go as 16-byte words (every per-robot block is a multiple of 16 bytes: NX is even);
// the node times, whose rows have an odd length, and the int tables go word by word.
__global__ __launch_bounds__(kPublishThreads) void k_policy_publish(PolicyPublishArgs a) {
  const int W = a.wg_per_robot, w = blockIdx.x % W, per_pass = gridDim.x / W;
  const int N = a.N, NX = a.nx, NU = a.nx;
  const int first = w * kPublishThreads + threadIdx.x, stride = W * kPublishThreads;
  for (int b = blockIdx.x / W; b < a.batch; b += per_pass) {
    const bool take = (!a.mask || a.mask[b] != 0) && !(a.skip_failed && (int)a.stats[(size_t)b * kStatsStride + 2] == 2);
    if (!take && !a.first) continue;
    const int row = take ? a.p_grid[b] : b;
    const double* sx = take ? a.x : a.front.x;
    const double* su = take ? a.u : a.front.u;
    const double* sK = take ? a.K : a.front.K;
    const double* st = (take ? a.g_time : a.front.g_time) + (size_t)row * (N + 1);
    const int* sk = (take ? a.g_kind : a.front.g_kind) + (size_t)row * N;
    const int* sm = (take ? a.g_mode : a.front.g_mode) + (size_t)row * N;
    int n = (take ? a.g_nodes : a.front.g_nodes)[row];
    n = n < 0 ? 0 : (n > N ? N : n);                 // a slot that never held a policy: nothing outside the robot's rows is touched
    const size_t ox = (size_t)b * (N + 1) * NX, ou = (size_t)b * N * NU;
    copy_words(reinterpret_cast<double2*>(a.back.x + ox), reinterpret_cast<const double2*>(sx + ox), (n + 1) * NX / 2, first, stride);
    copy_words(reinterpret_cast<double2*>(a.back.u + ou), reinterpret_cast<const double2*>(su + ou), n * NU / 2, first, stride);
    if (a.feedback)
      copy_words(reinterpret_cast<double2*>(a.back.K + ou * NX), reinterpret_cast<const double2*>(sK + ou * NX), n * NU * (NX / 2), first, stride);
    if (w == W - 1) {                                // the tables of the robot's grid row: its last workgroup
      double* dt = a.back.g_time + (size_t)b * (N + 1);
      int* dk = a.back.g_kind + (size_t)b * N;
      int* dm = a.back.g_mode + (size_t)b * N;
      for (int i = threadIdx.x; i <= n; i += kPublishThreads) dt[i] = st[i];
      for (int i = threadIdx.x; i < n; i += kPublishThreads) { dk[i] = sk[i]; dm[i] = sm[i]; }
      if (threadIdx.x == 0) {
        a.back.g_nodes[b] = n;
        if (take) { a.pending[b] = 1; a.t0_pend[b] = st[0]; a.status_pend[b] = (int)a.stats[(size_t)b * kStatsStride + 2]; }
      }
    }
  }
}

// bpmpc_policy_update: the robots of the publishes since the last adoption take their new policy's generation, t0 and status.  One thread per robot.
__global__ __launch_bounds__(256) void k_policy_adopt(int max_batch, int* pending, int* generation, const double* t0_pend, double* t0, const int* status_pend,
                                                      int* status) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= max_batch || !pending[b]) return;
  generation[b] += 1;
  t0[b] = t0_pend[b];
  status[b] = status_pend[b];
  pending[b] = 0;
}

// ev_start / ev_stop (both or neither): events attached to the kernel's own dispatch, as kl::linearize_fast
void launch_policy_publish(hipStream_t stream, int num_cus, const PolicyPublishArgs& a, hipEvent_t ev_start, hipEvent_t ev_stop) {
  // eight workgroups of four waves fill a CU; a robot's share of them, at most one per pass of 16-byte words over its largest block
  const int target = 8 * (num_cus > 0 ? num_cus : 256);
  const int words = (a.feedback ? a.N * a.nx * a.nx : (a.N + 1) * a.nx) / 2;
  PolicyPublishArgs k = a;
  k.wg_per_robot = std::max(1, std::min(target / a.batch, (words + kPublishThreads - 1) / kPublishThreads));
  const int robots = std::max(1, std::min(a.batch, target / k.wg_per_robot));
  const dim3 grid(robots * k.wg_per_robot), block(kPublishThreads);
  if (ev_start && ev_stop) hipExtLaunchKernelGGL(k_policy_publish, grid, block, 0, stream, ev_start, ev_stop, 0, k);
  else hipLaunchKernelGGL(k_policy_publish, grid, block, 0, stream, k);
  HIP_CHECK(hipGetLastError());
}

void check_buffered_tick(const bpmpc_policy* p, int batch, const char* who) {
  if (!p->ready)
    throw std::invalid_argument(std::string(who) + ": waiting for the initial policy: no bpmpc_policy_publish(mask = NULL, skip_failed = 0) has been adopted yet");
  if (p->restart_hold) throw std::invalid_argument(std::string(who) + ": a restart (bpmpc_controller_restart) waits for the next bpmpc_policy_update that adopts a policy");
  if (batch != p->batch) throw std::invalid_argument(std::string(who) + ": batch differs from the batch of the published policy");
}

}  // namespace bpmpc

using namespace bpmpc;

namespace {

void record(hipEvent_t* ev, hipStream_t on) {
  if (!*ev) HIP_CHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(*ev, on));
}

}  // namespace

extern "C" {

int bpmpc_policy_create(bpmpc_solver* s, int max_batch, bpmpc_policy** out) {
  if (!s || !out) { set_last_error("bpmpc_policy_create: null solver or output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  if (max_batch < 1) { set_last_error("bpmpc_policy_create: max_batch must be positive"); return BPMPC_ERR_INVALID_ARGUMENT; }
  std::unique_ptr<bpmpc_policy> p(new bpmpc_policy);
  const int rc = guarded(BPMPC_ERR_DEVICE, [&] {
    if (s->is_ddp())
      throw Unsupported("bpmpc_policy_create: the DDP solution is a FeedforwardController on the time points of its own roll-out, not on the shooting grid "
                        "the policy is interpolated on");
    if (max_batch > s->settings.max_batch) throw std::length_error("bpmpc_policy_create: max_batch exceeds the solver's max_batch");
    if (s->nx % 2 != 0 || s->nu != s->nx) throw Unsupported("bpmpc_policy_create: the 16-byte copy needs an even state dimension and as many inputs");
    if (s->feedback() && !s->buf.K) throw std::invalid_argument("bpmpc_policy_create: the feedback policy needs the gains (return_gains with reference kernels)");
    p->s = s; p->device = s->settings.device; p->max_batch = max_batch; p->N = s->settings.max_nodes; p->nx = s->nx; p->nu = s->nu; p->feedback = s->feedback();
    HIP_CHECK(hipSetDevice(p->device));
    HIP_CHECK(hipStreamCreateWithFlags(&p->hs.stream, hipStreamNonBlocking));
    const size_t B = max_batch, N = p->N, NX = p->nx, NU = p->nu;
    DeviceBuffers& m = p->mem;
    for (PolicySlot& sl : p->slot) {
      sl.x = m.alloc<double>(B * (N + 1) * NX, true); sl.u = m.alloc<double>(B * N * NU, true);
      if (p->feedback) sl.K = m.alloc<double>(B * N * NU * NX, true);
      sl.g_time = m.alloc<double>(B * (N + 1), true);
      sl.g_kind = m.alloc<int>(B * N, true); sl.g_mode = m.alloc<int>(B * N, true); sl.g_nodes = m.alloc<int>(B, true);
    }
    p->d_identity = m.alloc<int>(B);
    std::vector<int> id(B);
    for (size_t b = 0; b < B; ++b) id[b] = (int)b;
    HIP_CHECK(hipMemcpy(p->d_identity, id.data(), B * sizeof(int), hipMemcpyHostToDevice));
    p->d_pending = m.alloc<int>(B, true); p->d_generation = m.alloc<int>(B, true); p->d_status = m.alloc<int>(B, true); p->d_status_pend = m.alloc<int>(B, true);
    p->d_mask = m.alloc<int>(B);
    p->d_t0 = m.alloc<double>(B, true); p->d_t0_pend = m.alloc<double>(B, true);
    HIP_CHECK(hipDeviceSynchronize());
  });
  if (rc != BPMPC_OK) { bpmpc_policy_destroy(p.release()); return rc; }
  *out = p.release();
  return BPMPC_OK;
}

void bpmpc_policy_destroy(bpmpc_policy* p) {
  if (!p) return;
  if (p->hs.stream || !p->mem.owned.empty()) {
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();           // a publish may still be in flight on the solver's stream, a tick on the buffer's
  }
  if (p->s && p->s->tick_hs == &p->hs) p->s->tick_hs = nullptr;
  if (p->ev_publish) (void)hipEventDestroy(p->ev_publish);
  if (p->ev_adopt) (void)hipEventDestroy(p->ev_adopt);
  p->hs.destroy();
  p->mem.release();
  delete p;
}

int bpmpc_policy_publish(bpmpc_policy* p, int batch, const int* mask, int inputs_on_device, int skip_failed) {
  return guarded(p, BPMPC_ERR_DEVICE, "bpmpc_policy_publish: null policy handle", [&] {
    bpmpc_solver* s = p->s;
    check_policy(s);
    if (batch != s->batch) throw std::invalid_argument("bpmpc_policy_publish: batch differs from the batch of the solver's last setup");
    if (batch > p->max_batch) throw std::length_error("bpmpc_policy_publish: batch exceeds the buffer's max_batch");
    const bool full = !mask && !skip_failed;
    if (!full && batch != p->batch) throw std::invalid_argument("bpmpc_policy_publish: a publish that changes the batch must cover every robot (mask = NULL, skip_failed = 0)");
    hipStream_t st = s->stream;
    const Buffers& bf = s->buf;
    PolicyPublishArgs a{};
    a.batch = batch; a.N = p->N; a.nx = p->nx; a.feedback = p->feedback; a.skip_failed = skip_failed ? 1 : 0; a.first = p->outstanding ? 0 : 1;
    a.mask = staged(mask, p->d_mask, batch, inputs_on_device, st);
    a.stats = bf.stats; a.p_grid = bf.p_grid; a.g_nodes = bf.g_nodes; a.g_kind = bf.g_kind; a.g_mode = bf.g_mode; a.g_time = bf.g_time;
    a.x = bf.x; a.u = bf.u; a.K = bf.K;
    a.front = p->slot[p->front]; a.back = p->slot[1 - p->front];
    a.pending = p->d_pending; a.status_pend = p->d_status_pend; a.t0_pend = p->d_t0_pend;
    if (p->ev_adopt) HIP_CHECK(hipStreamWaitEvent(st, p->ev_adopt, 0));      // ticks enqueued before the last adoption may still read the back slot
    if (KernelTimers::timed(s->settings.profile, "policy_publish"))      // bpmpc_solver_kernel_time("policy_publish"): the kernel's own duration (tools/policy_buffer_probe.py)
      s->timers.attached("policy_publish", [&](hipEvent_t e0, hipEvent_t e1) { launch_policy_publish(st, s->num_cus, a, e0, e1); });
    else launch_policy_publish(st, s->num_cus, a);
    record(&p->ev_publish, st);
    p->batch = batch; p->outstanding = true; p->full_outstanding = p->full_outstanding || full;
    if (mask && !inputs_on_device) HIP_CHECK(hipStreamSynchronize(st));      // the caller's host mask
  });
}

int bpmpc_policy_update(bpmpc_policy* p, int wait, int* adopted) {
  return guarded(p, BPMPC_ERR_DEVICE, "bpmpc_policy_update: null handle or adopted", adopted != nullptr, [&] {
    *adopted = 0;
    if (!p->outstanding) return;
    if (wait) HIP_CHECK(hipStreamWaitEvent(p->hs.stream, p->ev_publish, 0));
    else {
      const hipError_t q = hipEventQuery(p->ev_publish);
      if (q == hipErrorNotReady) return;             // the solve or its publish is still running: the ticks keep the last policy
      HIP_CHECK(q);
    }
    hipLaunchKernelGGL(k_policy_adopt, dim3((p->max_batch + 255) / 256), dim3(256), 0, p->hs.stream, p->max_batch, p->d_pending, p->d_generation, p->d_t0_pend,
                       p->d_t0, p->d_status_pend, p->d_status);
    HIP_CHECK(hipGetLastError());
    record(&p->ev_adopt, p->hs.stream);
    p->front = 1 - p->front;
    if (p->full_outstanding) p->ready = true;
    p->outstanding = p->full_outstanding = false;
    p->restart_hold = false;
    *adopted = 1;
  });
}

int bpmpc_policy_info(bpmpc_policy* p, int batch, int* generation, double* t0, int* status) {
  return guarded(p, BPMPC_ERR_DEVICE, "bpmpc_policy_info: null policy handle", [&] {
    if (batch < 1 || batch > p->max_batch) throw std::length_error("bpmpc_policy_info: batch exceeds the buffer's max_batch");
    hipStream_t st = p->hs.stream;
    if (generation) HIP_CHECK(hipMemcpyAsync(generation, p->d_generation, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
    if (t0) HIP_CHECK(hipMemcpyAsync(t0, p->d_t0, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost, st));
    if (status) HIP_CHECK(hipMemcpyAsync(status, p->d_status, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
    p->hs.synchronise_own();
  });
}

}  // extern "C"
