// The value function of the solver handle (include/bpmpc.h "Value function"): its buffers, the launch behind a backward pass, and the entry points
// bpmpc_solver_enable_value_function / value_function / device_value_function / evaluate_value.  The kernels are in k_value.hip; where a run
// launches them is decided in solver.hip (run_iterations, pipelined_backward, the "value" stage) from bpmpc_solver::value_on.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "solver.h"

namespace bpmpc {
namespace {

// [max_batch] problems of max_nodes + 1 nodes each; the scratch table of the closed-loop terms has one row per interval.  Zero-filled: status 0
void ensure_buffers(bpmpc_solver* s) {
  if (s->value.S) return;
  const size_t B = s->settings.max_batch, N = s->settings.max_nodes, NX = s->nx;
  ValueArgs& v = s->value;
  v.S = s->value_mem.alloc<double>(B * (N + 1) * NX * NX, true);
  v.s = s->value_mem.alloc<double>(B * (N + 1) * NX, true);
  v.v = s->value_mem.alloc<double>(B * (N + 1), true);
  v.x_lin = s->value_mem.alloc<double>(B * (N + 1) * NX, true);
  v.terms = s->value_mem.alloc<double>(B * N * value_terms_stride((int)NX), true);
  v.status = s->value_mem.alloc<int>(B, true);
}

void check_supported(const bpmpc_solver* s, const char* who) {
  if (s->is_ddp()) throw Unsupported(std::string(who) + ": the DDP solver has no value function here (its backward pass works on the Euler-discretised model and its solution lives on the roll-out's time points)");
}
void check_enabled(const bpmpc_solver* s, const char* who) {
  check_supported(s, who);
  if (!s->value.S) throw std::invalid_argument(std::string(who) + ": the value function is not enabled (bpmpc_solver_enable_value_function)");
}

}  // namespace

void release_value(bpmpc_solver* s) { s->value_mem.release(); }

// The value function runs while the caller asked for it (value_own) or the dual solution, which reads its rows, is on (dual_on)
void apply_value_state(bpmpc_solver* s, const char* who) {
  check_supported(s, who);
  if (s->settings.reference_kernels && !s->settings.return_gains)
    throw std::invalid_argument(std::string(who) + ": the value function needs the feedback gains (return_gains with reference kernels)");
  const bool on = s->value_own || s->dual_on;
  if (on) {
    ensure_buffers(s);
    s->settings.materialize_lq = 1;                        // the kernels read A .. c as the lineariser writes them in this mode
  } else {
    s->settings.materialize_lq = s->own_materialize;
  }
  s->value_on = on;
}

}  // namespace bpmpc

// the model, gains and step of the backward pass that has just been enqueued, as the handle's buffers stand now (x, K trade places with their
// kept copies in setup_from_previous: the pointers are taken per launch)
void bpmpc_solver::launch_value() {
  ValueArgs a = value;
  const Buffers& bf = buf;
  a.A = bf.A; a.B = bf.B; a.b = bf.b; a.Q = bf.Q; a.R = bf.R; a.P = bf.P; a.q = bf.q; a.r = bf.r; a.c = bf.c;
  a.K = bf.K; a.dx = bf.dx; a.du = bf.du; a.x = bf.x; a.summary = bf.summary;
  a.n_info = bf.n_info; a.active = bf.active; a.p_grid = bf.p_grid; a.g_nodes = bf.g_nodes;
  a.batch = batch; a.N = settings.max_nodes; a.klen = plan.klen;
  if (KernelTimers::timed(settings.profile, "value_terms")) {
    timers.attached("value_terms", [&](hipEvent_t e0, hipEvent_t e1) { kl::value_terms(nj(), stream, a, e0, e1); });
    timers.attached("value_sweep", [&](hipEvent_t e0, hipEvent_t e1) { kl::value_sweep(nj(), stream, a, e0, e1); });
  } else {
    kl::value_terms(nj(), stream, a);
    kl::value_sweep(nj(), stream, a);
  }
  HIP_CHECK(hipGetLastError());
}

extern "C" {

int bpmpc_solver_enable_value_function(bpmpc_solver* s, int on) {
  return guarded(s, [&] {
    const bool before = s->value_own;
    s->value_own = on != 0;
    try { apply_value_state(s, "bpmpc_solver_enable_value_function"); } catch (...) { s->value_own = before; throw; }
  });
}

int bpmpc_solver_value_function(bpmpc_solver* s, double* S, double* sv, double* v, double* x_lin, int* status) {
  return guarded(s, [&] {
    check_enabled(s, "bpmpc_solver_value_function");
    const size_t B = s->batch, N = s->settings.max_nodes, NX = s->nx;
    const ValueArgs& a = s->value;
    auto down = [&](void* dst, const void* src, size_t bytes) { if (dst && bytes) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s->stream)); };
    down(S, a.S, B * (N + 1) * NX * NX * sizeof(double));
    down(sv, a.s, B * (N + 1) * NX * sizeof(double));
    down(v, a.v, B * (N + 1) * sizeof(double));
    down(x_lin, a.x_lin, B * (N + 1) * NX * sizeof(double));
    down(status, a.status, B * sizeof(int));
    HIP_CHECK(hipStreamSynchronize(s->stream));
  });
}

int bpmpc_solver_device_value_function(bpmpc_solver* s, double** S_dev, double** s_dev, double** v_dev, double** x_lin_dev, int** status_dev) {
  return guarded(s, [&] {
    check_enabled(s, "bpmpc_solver_device_value_function");
    if (S_dev) *S_dev = s->value.S;
    if (s_dev) *s_dev = s->value.s;
    if (v_dev) *v_dev = s->value.v;
    if (x_lin_dev) *x_lin_dev = s->value.x_lin;
    if (status_dev) *status_dev = s->value.status;
  });
}

int bpmpc_solver_evaluate_value(bpmpc_solver* s, int batch, const double* t, const double* x, int inputs_on_device, double* f, double* dfdx, double* dfdxx) {
  if (s && (!t || !x || !f || !dfdx)) { set_last_error("bpmpc_solver_evaluate_value: null argument"); return BPMPC_ERR_INVALID_ARGUMENT; }
  void* block = nullptr;
  const int rc = guarded(s, [&] {
    const char* who = "bpmpc_solver_evaluate_value";
    check_enabled(s, who);
    if (s->batch < 1 || !s->has_solution) throw std::invalid_argument(std::string(who) + " needs a completed bpmpc_solver_run since the last setup");
    if (batch != s->batch) throw std::invalid_argument(std::string(who) + ": batch differs from the batch of the last setup");
    const size_t B = batch, NX = s->nx;
    ValueQueryArgs q{};
    q.S = s->value.S; q.s = s->value.s; q.v = s->value.v; q.x_lin = s->value.x_lin;
    q.g_time = s->buf.g_time; q.p_grid = s->buf.p_grid; q.g_nodes = s->buf.g_nodes;
    q.batch = batch; q.N = s->settings.max_nodes;
    if (inputs_on_device) {
      q.t = t; q.x = x; q.f = f; q.dfdx = dfdx; q.dfdxx = dfdxx;
      kl::value_query(s->nj(), s->stream, q);
      HIP_CHECK(hipGetLastError());
      return;
    }
    const size_t doubles = B * (1 + NX + 1 + NX + (dfdxx ? NX * NX : 0));
    HIP_CHECK(hipMalloc(&block, doubles * sizeof(double)));
    double* d_t = static_cast<double*>(block);
    double* d_x = d_t + B;
    double* d_f = d_x + B * NX;
    double* d_g = d_f + B;
    double* d_h = dfdxx ? d_g + B * NX : nullptr;
    HIP_CHECK(hipMemcpyAsync(d_t, t, B * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_CHECK(hipMemcpyAsync(d_x, x, B * NX * sizeof(double), hipMemcpyHostToDevice, s->stream));
    q.t = d_t; q.x = d_x; q.f = d_f; q.dfdx = d_g; q.dfdxx = d_h;
    kl::value_query(s->nj(), s->stream, q);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(f, d_f, B * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipMemcpyAsync(dfdx, d_g, B * NX * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (dfdxx) HIP_CHECK(hipMemcpyAsync(dfdxx, d_h, B * NX * NX * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
  });
  if (block) (void)hipFree(block);
  return rc;
}

}  // extern "C"
