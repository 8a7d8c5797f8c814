// The dual solution of the solver handle (include/bpmpc.h "Dual solution"): its buffers, the launch behind the value function's, and the entry points
// bpmpc_solver_enable_dual_solution / dual_solution / device_dual_solution / evaluate_dual.  The kernels are in k_dual.hip; where a run launches
// them is decided in solver.hip (run_iterations, pipelined_backward, the "dual" stage) from bpmpc_solver::dual_on, directly behind launch_value().
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "solver.h"

namespace bpmpc {
namespace {

// [max_batch] problems of max_nodes intervals (max_nodes + 1 costates).  Zero-filled: status 0.  nu_gain is the large one: 16 nx doubles per node
void ensure_buffers(bpmpc_solver* s) {
  if (s->dual.lambda) return;
  const size_t B = s->settings.max_batch, N = s->settings.max_nodes, NX = s->nx, R = kDualRows;
  DualArgs& d = s->dual;
  d.lambda = s->dual_mem.alloc<double>(B * (N + 1) * NX, true);
  d.nu_gain = s->dual_mem.alloc<double>(B * N * R * NX, true);
  d.nu0 = s->dual_mem.alloc<double>(B * N * R, true);
  d.nu = s->dual_mem.alloc<double>(B * N * R, true);
  d.residual = s->dual_mem.alloc<double>(B * N, true);
  d.gain_residual = s->dual_mem.alloc<double>(B * N, true);
  d.aux = s->dual_mem.alloc<double>(B * N * 2, true);
  d.summary_out = s->dual_mem.alloc<double>(B * 6, true);
  d.rows = s->dual_mem.alloc<int>(B * N, true);
  d.status = s->dual_mem.alloc<int>(B, true);
}

void check_supported(const bpmpc_solver* s, const char* who) {
  if (s->is_ddp()) throw Unsupported(std::string(who) + ": the DDP solver has no dual solution here (it has no value function: its backward pass works on the Euler-discretised model)");
}
void check_enabled(const bpmpc_solver* s, const char* who) {
  check_supported(s, who);
  if (!s->dual.lambda) throw std::invalid_argument(std::string(who) + ": the dual solution is not enabled (bpmpc_solver_enable_dual_solution)");
}

}  // namespace

void release_dual(bpmpc_solver* s) { s->dual_mem.release(); }

}  // namespace bpmpc

// behind launch_value() of the same backward pass: the model, gains and step as the handle's buffers stand now, S, s and the terms table as the value
// kernels have just been enqueued to write them
void bpmpc_solver::launch_dual() {
  DualArgs a = dual;
  const Buffers& bf = buf;
  a.B = bf.B; a.R = bf.R; a.P = bf.P; a.r = bf.r; a.D = bf.D; a.nc = bf.nc;
  a.K = bf.K; a.dx = bf.dx; a.du = bf.du; a.summary = bf.summary;
  a.n_info = bf.n_info; a.active = bf.active; a.p_grid = bf.p_grid; a.g_nodes = bf.g_nodes;
  a.S = value.S; a.s = value.s; a.terms = value.terms;
  a.batch = batch; a.N = settings.max_nodes; a.klen = plan.klen;
  if (KernelTimers::timed(settings.profile, "dual")) timers.attached("dual", [&](hipEvent_t e0, hipEvent_t e1) { kl::dual_node(nj(), stream, a, e0, e1); });
  else kl::dual_node(nj(), stream, a);
  kl::dual_summary(nj(), stream, a);
  HIP_CHECK(hipGetLastError());
}

extern "C" {

int bpmpc_solver_enable_dual_solution(bpmpc_solver* s, int on) {
  return guarded(s, [&] {
    const char* who = "bpmpc_solver_enable_dual_solution";
    check_supported(s, who);
    const bool before = s->dual_on;
    s->dual_on = on != 0;
    try {
      apply_value_state(s, who);                           // the value function on while this is on; back to the caller's own choice behind it
      if (on) ensure_buffers(s);
    } catch (...) {
      s->dual_on = before;
      throw;
    }
  });
}

int bpmpc_solver_dual_solution(bpmpc_solver* s, double* lambda, double* nu, double* nu0, double* nu_gain, double* residual, double* gain_residual,
                               double* summary, int* status) {
  return guarded(s, [&] {
    check_enabled(s, "bpmpc_solver_dual_solution");
    const size_t B = s->batch, N = s->settings.max_nodes, NX = s->nx, R = kDualRows;
    const DualArgs& a = s->dual;
    auto down = [&](void* dst, const void* src, size_t bytes) { if (dst && bytes) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s->stream)); };
    down(lambda, a.lambda, B * (N + 1) * NX * sizeof(double));
    down(nu, a.nu, B * N * R * sizeof(double));
    down(nu0, a.nu0, B * N * R * sizeof(double));
    down(nu_gain, a.nu_gain, B * N * R * NX * sizeof(double));
    down(residual, a.residual, B * N * sizeof(double));
    down(gain_residual, a.gain_residual, B * N * sizeof(double));
    down(summary, a.summary_out, B * 6 * sizeof(double));
    down(status, a.status, B * sizeof(int));
    HIP_CHECK(hipStreamSynchronize(s->stream));
  });
}

int bpmpc_solver_device_dual_solution(bpmpc_solver* s, double** lambda_dev, double** nu_dev, double** nu0_dev, double** nu_gain_dev, double** residual_dev,
                                      double** gain_residual_dev, double** summary_dev, int** status_dev) {
  return guarded(s, [&] {
    check_enabled(s, "bpmpc_solver_device_dual_solution");
    const DualArgs& a = s->dual;
    if (lambda_dev) *lambda_dev = a.lambda;
    if (nu_dev) *nu_dev = a.nu;
    if (nu0_dev) *nu0_dev = a.nu0;
    if (nu_gain_dev) *nu_gain_dev = a.nu_gain;
    if (residual_dev) *residual_dev = a.residual;
    if (gain_residual_dev) *gain_residual_dev = a.gain_residual;
    if (summary_dev) *summary_dev = a.summary_out;
    if (status_dev) *status_dev = a.status;
  });
}

int bpmpc_solver_evaluate_dual(bpmpc_solver* s, int batch, const double* t, const double* x, int inputs_on_device, double* lambda, double* nu, int* rows) {
  if (s && (!t || !x || !lambda || !nu || !rows)) { set_last_error("bpmpc_solver_evaluate_dual: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  void* block = nullptr;
  const int rc = guarded(s, [&] {
    const char* who = "bpmpc_solver_evaluate_dual";
    check_enabled(s, who);
    if (s->batch < 1 || !s->has_solution) throw std::invalid_argument(std::string(who) + " needs a completed bpmpc_solver_run since the last setup");
    if (batch != s->batch) throw std::invalid_argument(std::string(who) + ": batch differs from the batch of the last setup");
    const size_t B = batch, NX = s->nx, R = kDualRows;
    DualQueryArgs q{};
    q.S = s->value.S; q.s = s->value.s; q.x_lin = s->value.x_lin;
    q.nu_gain = s->dual.nu_gain; q.nu0 = s->dual.nu0; q.node_rows = s->dual.rows;
    q.g_time = s->buf.g_time; q.p_grid = s->buf.p_grid; q.g_nodes = s->buf.g_nodes;
    q.batch = batch; q.N = s->settings.max_nodes;
    if (inputs_on_device) {
      q.t = t; q.x = x; q.lambda = lambda; q.nu = nu; q.rows = rows;
      kl::dual_query(s->nj(), s->stream, q);
      HIP_CHECK(hipGetLastError());
      return;
    }
    const size_t doubles = B * (1 + NX + NX + R);
    HIP_CHECK(hipMalloc(&block, doubles * sizeof(double) + B * sizeof(int)));
    double* d_t = static_cast<double*>(block);
    double* d_x = d_t + B;
    double* d_l = d_x + B * NX;
    double* d_n = d_l + B * NX;
    int* d_r = reinterpret_cast<int*>(d_n + B * R);
    HIP_CHECK(hipMemcpyAsync(d_t, t, B * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_CHECK(hipMemcpyAsync(d_x, x, B * NX * sizeof(double), hipMemcpyHostToDevice, s->stream));
    q.t = d_t; q.x = d_x; q.lambda = d_l; q.nu = d_n; q.rows = d_r;
    kl::dual_query(s->nj(), s->stream, q);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(lambda, d_l, B * NX * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipMemcpyAsync(nu, d_n, B * R * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipMemcpyAsync(rows, d_r, B * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
  });
  if (block) (void)hipFree(block);
  return rc;
}

}  // extern "C"
