// The kernels of the plan geometry (kernels/plan_geometry.h) and the host side of its handle: the C ABI of include/bpmpc.h "Plan geometry".
//   BipedalControllerVisualizer::update    bipedal_controllers/src/BipedalControllerVisualizer.cpp:73-87
// A translation unit of its own: every other kernel is compiled as it was before this unit existed, and a process that never creates a
// bpmpc_plan launches nothing of it.
#include <hip/hip_runtime.h>

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "kernel_launchers.h"
#include "plan_geometry.h"
#include "policy.h"
#include "solver.h"
#include "kernels/plan_geometry.h"

static_assert(bpmpc::kPlanNodeStride == BPMPC_PLAN_NODE_STRIDE, "the node row follows include/bpmpc.h");
static_assert(bpmpc::kPlanMaxFootholds == BPMPC_PLAN_MAX_FOOTHOLDS, "the foothold list follows include/bpmpc.h");
static_assert(bpmpc::kPlanSummaryStride == BPMPC_PLAN_SUMMARY_STRIDE, "the summary row follows include/bpmpc.h");

namespace bpmpc {

// one launch: a workgroup owns a robot.  Its wavefronts share the tiles of both blocks; behind the barrier, which makes the rows visible to the
// workgroup, wavefront 0 reads them back for footholds and summary
template <int NJ>
__global__ __launch_bounds__(kPlanFusedWaves* kWave) void k_plan_fused(const DeviceModel* model, PlanArgs a) {
  __shared__ PlanTileLds<NJ> w[kPlanFusedWaves];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, b = blockIdx.x;
  for (int j = wave; j < a.tiles * a.blocks; j += kPlanFusedWaves) plan_tile<NJ>(*model, w[wave], a, b, j / a.tiles, j % a.tiles, lane);
  __syncthreads();
  if (wave == 0) plan_reduce(a, b, lane);
}

// two launches: one wavefront per (robot, block, tile), then one wavefront per robot
template <int NJ>
__global__ __launch_bounds__(kWave) void k_plan_nodes(const DeviceModel* model, PlanArgs a) {
  __shared__ PlanTileLds<NJ> w;
  const int per_robot = a.tiles * a.blocks, b = blockIdx.x / per_robot, j = blockIdx.x % per_robot;
  plan_tile<NJ>(*model, w, a, b, j / a.tiles, j % a.tiles, threadIdx.x);
}
__global__ __launch_bounds__(kWave) void k_plan_reduce(PlanArgs a) { plan_reduce(a, blockIdx.x, threadIdx.x); }

}  // namespace bpmpc

using namespace bpmpc;

namespace {

// Where the handle chooses: two launches, the faster at batch 1, 256 and 4096 (tools/plan_geometry_probe.py, profiles/plan_geometry_probe.jsonl)
constexpr int kDefaultLaunches = 2;

void check_batch(const bpmpc_plan* pl, int batch, const char* who) {
  if (batch < 1) throw std::invalid_argument(std::string(who) + ": batch must be positive");
  if (batch > pl->max_batch) throw std::length_error(std::string(who) + ": batch exceeds max_batch");
}

// the outputs of the handle into a; the launch for a.batch robots whose longest plan has at most `longest` nodes
void launch(bpmpc_plan* pl, PlanArgs a, int longest, hipStream_t st) {
  a.N = pl->N;
  a.tiles = (longest + 1 + kPlanTile - 1) / kPlanTile;
  a.blocks = a.xref ? 2 : 1;
  a.optimized = pl->d_optimized; a.desired = pl->d_desired; a.footholds = pl->d_footholds; a.summary = pl->d_summary; a.count = pl->d_count;
  const int launches = pl->launches ? pl->launches : kDefaultLaunches;
  if (launches == 1) {
    KL_NJ(pl->nj, hipLaunchKernelGGL(k_plan_fused<NJ>, dim3(a.batch), dim3(kPlanFusedWaves * kWave), 0, st, pl->d_model, a));
  } else {
    KL_NJ(pl->nj, hipLaunchKernelGGL(k_plan_nodes<NJ>, dim3(a.batch * a.tiles * a.blocks), dim3(kWave), 0, st, pl->d_model, a));
    hipLaunchKernelGGL(k_plan_reduce, dim3(a.batch), dim3(kWave), 0, st, a);
  }
  HIP_CHECK(hipGetLastError());
}

void launch_on(bpmpc_plan* pl, const PlanArgs& a, int longest, hipStream_t stream) {
  pl->hs.before_foreign(stream);
  launch(pl, a, longest, stream);
  pl->hs.after_foreign(stream);
}

// bpmpc_plan_rows_host: the rows, footholds and summary of one robot from the text the kernels are compiled from
void rows_host(const DeviceModel& md, int n, const double* t, const double* x, const double* u, const int* mode, const int* kind, double* rows,
               double* footholds, int* count, double* summary) {
  const int nj = md.nj, nx = 12 + nj;
  PlanChains chains{};
  for (int e = 0; e < kPlanChainEntries; ++e) plan_chains_fill(md, chains, e);
  std::vector<double> own;
  if (!rows) { own.resize((size_t)(n + 1) * kPlanNodeStride); rows = own.data(); }
  for (int k = 0; k <= n; ++k) {
    const double* xk = x + (size_t)k * nx;
    double* row = rows + (size_t)k * kPlanNodeStride;
    bool bad = false;
    for (int c = 0; c < nx; ++c) bad = bad || !std::isfinite(xk[c]);
    double T[kMaxJoints * 9];
    for (int j = 0; j < nj; ++j) plan_joint_rotation(md, j + 1, xk[12 + j], T + 9 * j);
    double sc[6];
    for (int a = 0; a < 3; ++a) plan_base_sincos(xk[9 + a], sc + 2 * a);
    for (int i = 0; i < kNumContacts; ++i) plan_chain_point(chains, i, xk + 6, sc, T, row + kPgContact + 3 * i);
    const bool is_last = k == n;
    plan_row_tail(row, xk, (u && !is_last) ? u + (size_t)k * nx : nullptr, t[k], is_last ? -1 : mode[k], is_last ? -1 : kind[k], bad);
  }
  PlanAcc acc[kWave];
  for (PlanAcc& a : acc) plan_acc_init(a);
  int total = 0;
  for (int k = 0; k <= n; ++k) {
    plan_acc_node(acc[k % kWave], rows, k, n);
    const int landing = plan_landing_mask(rows, k, n);
    for (int i = 0; i < kNumContacts; ++i) {
      if (!((landing >> i) & 1)) continue;
      if (total < kPlanMaxFootholds && footholds) plan_foothold_entry(rows, k, i, footholds + (size_t)total * kPlanFootholdStride);
      ++total;
    }
  }
  double path = 0.0;
  for (int l = 0; l < kWave; ++l) path += acc[l].path;
  for (int l = 1; l < kWave; ++l) plan_acc_merge(acc[0], acc[l]);
  acc[0].path = path;
  if (summary) plan_summary_row(acc[0], n, total, summary);
  if (count) *count = total;
}

}  // namespace

extern "C" {

int bpmpc_plan_create(const bpmpc_model* model, int device, int max_batch, int max_nodes, bpmpc_plan** out) {
  if (!model || !out) { set_last_error("bpmpc_plan_create: null model or output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  if (max_batch < 1) { set_last_error("bpmpc_plan_create: max_batch must be positive"); return BPMPC_ERR_INVALID_ARGUMENT; }
  if (max_nodes < 1) { set_last_error("bpmpc_plan_create: max_nodes must be positive"); return BPMPC_ERR_INVALID_ARGUMENT; }
  std::unique_ptr<bpmpc_plan> pl(new bpmpc_plan);
  const int rc = guarded(BPMPC_ERR_DEVICE, [&]() -> int {
    if (const int refused = open_side_handle("bpmpc_plan_create", pl.get(), model, device, max_batch)) return refused;
    pl->nj = pl->rm.nj; pl->nx = 12 + pl->nj; pl->N = max_nodes;
    const size_t B = max_batch, K = (size_t)max_nodes + 1;
    DeviceBuffers& m = pl->mem;
    pl->d_optimized = m.alloc<double>(B * K * kPlanNodeStride, true); pl->d_desired = m.alloc<double>(B * K * kPlanNodeStride, true);
    pl->d_footholds = m.alloc<double>(B * kPlanMaxFootholds * kPlanFootholdStride, true); pl->d_summary = m.alloc<double>(B * kPlanSummaryStride, true);
    pl->d_count = m.alloc<int>(B, true);
    HIP_CHECK(hipDeviceSynchronize());      // the zero fills run on the null stream
    return BPMPC_OK;
  });
  if (rc != BPMPC_OK) { bpmpc_plan_destroy(pl.release()); return rc; }
  *out = pl.release();
  return BPMPC_OK;
}

void bpmpc_plan_destroy(bpmpc_plan* pl) {
  if (pl && pl->hs.stream) { (void)hipSetDevice(pl->device); (void)hipDeviceSynchronize(); }      // an update may still be in flight on a solver's or a buffer's stream
  close_side_handle(pl);
}

int bpmpc_plan_dims(const bpmpc_plan* pl, int* max_batch, int* max_nodes, int* node_stride, int* max_footholds, int* summary_stride) {
  if (!pl) { set_last_error("bpmpc_plan_dims: null plan handle"); return BPMPC_ERR_INVALID_ARGUMENT; }
  if (max_batch) *max_batch = pl->max_batch;
  if (max_nodes) *max_nodes = pl->N;
  if (node_stride) *node_stride = kPlanNodeStride;
  if (max_footholds) *max_footholds = kPlanMaxFootholds;
  if (summary_stride) *summary_stride = kPlanSummaryStride;
  return BPMPC_OK;
}

int bpmpc_plan_configure(bpmpc_plan* pl, int launches) {
  return guarded(pl, BPMPC_ERR_DEVICE, "bpmpc_plan_configure: null plan handle", [&] {
    if (launches < 0 || launches > 2) throw std::invalid_argument("bpmpc_plan_configure: launches must be 0 (the handle chooses), 1 or 2");
    pl->launches = launches;
  });
}

int bpmpc_plan_update_from_solver(bpmpc_plan* pl, bpmpc_solver* s) {
  return guarded(pl, BPMPC_ERR_DEVICE, "bpmpc_plan_update_from_solver: null plan or solver handle", s != nullptr, [&] {
    const char* who = "bpmpc_plan_update_from_solver";
    if (s->nj() != pl->nj) throw std::invalid_argument(std::string(who) + ": the plan's model and the solver are built for different robots");
    if (s->settings.device != pl->device) throw std::invalid_argument(std::string(who) + ": the plan and the solver live on different devices");
    if (s->is_ddp()) throw Unsupported(std::string(who) + ": the DDP solution lives on the time points of its own roll-out, not on the shooting grid");
    if (s->batch < 1) throw std::invalid_argument(std::string(who) + ": no setup yet: the solver holds no plan");
    if (s->batch > pl->max_batch) throw std::length_error(std::string(who) + ": the solver's batch exceeds the plan's max_batch");
    if (s->settings.max_nodes > pl->N) throw std::length_error(std::string(who) + ": the solver's max_nodes exceeds the plan's max_nodes");
    const Buffers& bf = s->buf;
    PlanArgs a{};
    a.batch = s->batch; a.in_N = s->settings.max_nodes;
    a.x = bf.x; a.u = bf.u; a.xref = bf.xref;
    a.g_time = bf.g_time; a.g_kind = bf.g_kind; a.g_mode = bf.g_mode; a.g_nodes = bf.g_nodes; a.p_grid = bf.p_grid;
    launch_on(pl, a, s->n_nodes_max > 0 ? s->n_nodes_max : s->settings.max_nodes, s->stream);
  });
}

int bpmpc_plan_update_from_policy(bpmpc_plan* pl, bpmpc_policy* p) {
  return guarded(pl, BPMPC_ERR_DEVICE, "bpmpc_plan_update_from_policy: null plan or policy handle", p != nullptr, [&] {
    const char* who = "bpmpc_plan_update_from_policy";
    if (p->nx != pl->nx) throw std::invalid_argument(std::string(who) + ": the plan's model and the policy buffer are built for different robots");
    if (p->device != pl->device) throw std::invalid_argument(std::string(who) + ": the plan and the policy buffer live on different devices");
    if (!p->ready)
      throw std::invalid_argument(std::string(who) + ": waiting for the initial policy: no bpmpc_policy_publish(mask = NULL, skip_failed = 0) has been adopted yet");
    if (p->batch > pl->max_batch) throw std::length_error(std::string(who) + ": the policy's batch exceeds the plan's max_batch");
    if (p->N > pl->N) throw std::length_error(std::string(who) + ": the policy's max_nodes exceeds the plan's max_nodes");
    const PolicySlot& sl = p->slot[p->front];
    PlanArgs a{};
    a.batch = p->batch; a.in_N = p->N;
    a.x = sl.x; a.u = sl.u; a.xref = nullptr;
    a.g_time = sl.g_time; a.g_kind = sl.g_kind; a.g_mode = sl.g_mode; a.g_nodes = sl.g_nodes; a.p_grid = nullptr;
    launch_on(pl, a, p->N, p->hs.stream);
  });
}

int bpmpc_plan_update(bpmpc_plan* pl, int batch, const int* n_nodes, const double* t, const double* x, const double* u, const int* mode, const int* kind,
                      const double* xref, int inputs_on_device) {
  return guarded(pl, BPMPC_ERR_DEVICE, "bpmpc_plan_update: null handle, n_nodes, t, x, mode or kind", n_nodes && t && x && mode && kind, [&] {
    check_batch(pl, batch, "bpmpc_plan_update");
    const bool dev = inputs_on_device != 0;
    const size_t B = batch, N = pl->N, NX = pl->nx;
    int longest = pl->N;
    if (!dev) {
      longest = 1;
      for (int b = 0; b < batch; ++b) {
        if (n_nodes[b] < 1 || n_nodes[b] > pl->N)
          throw std::invalid_argument("bpmpc_plan_update: n_nodes[" + std::to_string(b) + "] = " + std::to_string(n_nodes[b]) + " lies outside 1 .. max_nodes");
        longest = std::max(longest, n_nodes[b]);
      }
      if (!pl->staging) {
        const size_t M = pl->max_batch;
        DeviceBuffers& m = pl->mem;
        pl->d_t = m.alloc<double>(M * (N + 1)); pl->d_x = m.alloc<double>(M * (N + 1) * NX); pl->d_u = m.alloc<double>(M * N * NX);
        pl->d_xref = m.alloc<double>(M * N * NX);
        pl->d_mode = m.alloc<int>(M * N); pl->d_kind = m.alloc<int>(M * N); pl->d_nodes = m.alloc<int>(M);
        pl->staging = true;
      }
    }
    hipStream_t st = pl->hs.stream;
    PlanArgs a{};
    a.batch = batch; a.in_N = pl->N;
    a.g_nodes = staged(n_nodes, pl->d_nodes, B, dev, st); a.g_time = staged(t, pl->d_t, B * (N + 1), dev, st);
    a.x = staged(x, pl->d_x, B * (N + 1) * NX, dev, st); a.u = staged(u, pl->d_u, B * N * NX, dev, st);
    a.g_mode = staged(mode, pl->d_mode, B * N, dev, st); a.g_kind = staged(kind, pl->d_kind, B * N, dev, st);
    a.xref = staged(xref, pl->d_xref, B * N * NX, dev, st);
    a.p_grid = nullptr;
    launch(pl, a, longest, st);
    pl->hs.finish(dev);      // host arrays are the caller's; the next update from a solver or a policy buffer waits for what was only enqueued
  });
}

int bpmpc_plan_device_outputs(bpmpc_plan* pl, bpmpc_plan_outputs* out) {
  if (!pl || !out) { set_last_error("bpmpc_plan_device_outputs: null plan handle or output"); return BPMPC_ERR_INVALID_ARGUMENT; }
  out->optimized = pl->d_optimized; out->desired = pl->d_desired; out->footholds = pl->d_footholds; out->summary = pl->d_summary;
  out->foothold_count = pl->d_count;
  return BPMPC_OK;
}

int bpmpc_plan_get_nodes(bpmpc_plan* pl, int batch, int which, double* host_rows) {
  return guarded(pl, BPMPC_ERR_DEVICE, "bpmpc_plan_get_nodes: null plan handle", [&] {
    check_batch(pl, batch, "bpmpc_plan_get_nodes");
    if (which != 0 && which != 1) throw std::invalid_argument("bpmpc_plan_get_nodes: which must be 0 (optimized) or 1 (desired)");
    const size_t bytes = (size_t)batch * (pl->N + 1) * kPlanNodeStride * sizeof(double);
    if (host_rows) HIP_CHECK(hipMemcpyAsync(host_rows, which == 0 ? pl->d_optimized : pl->d_desired, bytes, hipMemcpyDeviceToHost, pl->hs.stream));
    pl->hs.synchronise_own();
  });
}

int bpmpc_plan_get_footholds(bpmpc_plan* pl, int batch, double* host_entries, int* host_counts) {
  return guarded(pl, BPMPC_ERR_DEVICE, "bpmpc_plan_get_footholds: null plan handle", [&] {
    check_batch(pl, batch, "bpmpc_plan_get_footholds");
    hipStream_t st = pl->hs.stream;
    if (host_entries)
      HIP_CHECK(hipMemcpyAsync(host_entries, pl->d_footholds, (size_t)batch * kPlanMaxFootholds * kPlanFootholdStride * sizeof(double), hipMemcpyDeviceToHost, st));
    if (host_counts) HIP_CHECK(hipMemcpyAsync(host_counts, pl->d_count, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
    pl->hs.synchronise_own();
  });
}

int bpmpc_plan_get_summary(bpmpc_plan* pl, int batch, double* host_rows) {
  return guarded(pl, BPMPC_ERR_DEVICE, "bpmpc_plan_get_summary: null plan handle", [&] {
    check_batch(pl, batch, "bpmpc_plan_get_summary");
    if (host_rows) HIP_CHECK(hipMemcpyAsync(host_rows, pl->d_summary, (size_t)batch * kPlanSummaryStride * sizeof(double), hipMemcpyDeviceToHost, pl->hs.stream));
    pl->hs.synchronise_own();
  });
}

int bpmpc_plan_rows_host(const bpmpc_model* model, int n_nodes, const double* t, const double* x, const double* u, const int* mode, const int* kind,
                         double* rows, double* footholds, int* count, double* summary) {
  if (!model || !t || !x || !mode || !kind) { set_last_error("bpmpc_plan_rows_host: null model, t, x, mode or kind"); return BPMPC_ERR_INVALID_ARGUMENT; }
  if (n_nodes < 1) { set_last_error("bpmpc_plan_rows_host: n_nodes must be positive"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] {
    const RobotModel& rm = model_of(model);
    if (rm.nj > kMaxJoints) throw Unsupported("bpmpc_plan_rows_host: more joints than the device model holds");
    const DeviceModel md = make_device_model(rm);
    rows_host(md, n_nodes, t, x, u, mode, kind, rows, footholds, count, summary);
  });
}

}  // extern "C"
