// Per-problem cone parameters of the solver handle (include/bpmpc.h "Per-problem cone parameters"): the row table and the entry points
// bpmpc_solver_set_cone_params / get_cone_params / reset_cone_params.  The host check of a row is cone_params.h (bpmpc_model_check_cone_params,
// capi.cpp, runs it without a device).  The kernels that read the rows are the per-problem family of k_weights.hip, which the cost weights
// (solver_weights.hip) launch as well: bpmpc_solver::select_row_kernels (solver.h) is the one switch.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "cone_params.h"
#include "solver.h"
#include "kernels/linearize_fast.h"

namespace bpmpc {
namespace {

constexpr int kStride = BPMPC_SOLVER_CONE_STRIDE;
static_assert(kStride == kConeRowStride && BPMPC_SOLVER_CONE_RESERVED == kConeRowUsed, "one row format for the ABI, the table and the kernels");
static_assert(BPMPC_SOLVER_CONE_FRICTION * 8 == offsetof(ConeScalars, friction) && BPMPC_SOLVER_CONE_REGULARIZATION * 8 == offsetof(ConeScalars, cone_reg) &&
              BPMPC_SOLVER_CONE_GRIPPER_FORCE * 8 == offsetof(ConeScalars, cone_grip) && BPMPC_SOLVER_CONE_HESSIAN_SHIFT * 8 == offsetof(ConeScalars, cone_shift) &&
              BPMPC_SOLVER_CONE_BARRIER_MU * 8 == offsetof(ConeScalars, barrier_mu) && BPMPC_SOLVER_CONE_BARRIER_DELTA * 8 == offsetof(ConeScalars, barrier_delta),
              "the index macros name the fields the kernels read");

void check_supported(const bpmpc_solver* s, const char* who) {
  if (s->is_ddp())
    throw Unsupported(std::string(who) + ": the DDP solver keeps the model's cone parameters (its cost of recorded points and its ILQR lineariser read them)");
  if (s->settings.reference_kernels)
    throw Unsupported(std::string(who) + ": per-problem cone parameters are implemented by the fast kernels only (settings.reference_kernels reads the model's)");
}

void check_host_row(const bpmpc_solver* s, const char* who, const double* row, int r) {
  const std::string why = check_cone_row(row, s->rm.hard_friction_cone);
  if (!why.empty()) throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", " + why);
}

}  // namespace

// the table exists from the first set of EITHER table on (2 x max_batch rows of 64 bytes); every row starts as the model's
void ensure_cone_table(bpmpc_solver* s) {
  if (s->cone.d_params) return;
  const int B = s->settings.max_batch;
  double start[kStride];
  cone_start_row(s->rm, start);
  s->cone.create(s->weight_mem, B, kStride, kStride, start);
  s->cone_mask = s->weight_mem.alloc<int>(B);
  s->cone.fill_from_start(s->stream, B);
}

}  // namespace bpmpc

extern "C" {

int bpmpc_solver_set_cone_params(bpmpc_solver* s, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  if (s && !rows) { set_last_error("bpmpc_solver_set_cone_params: null rows"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(s, [&] {
    const char* who = "bpmpc_solver_set_cone_params";
    check_supported(s, who);
    if (s->batch < 1 || batch != s->batch) throw std::invalid_argument(std::string(who) + ": batch must equal the batch of the last setup");
    const bool on_device = inputs_on_device != 0;
    if (n_rows != 1 && n_rows != batch) throw std::invalid_argument(std::string(who) + ": n_rows must be 1 or batch");
    if (!on_device)      // before anything is allocated or enqueued
      for (int r = 0; r < n_rows; ++r)
        if (n_rows == 1 || !mask || mask[r]) check_host_row(s, who, rows + (size_t)r * kStride, r);
    ensure_cone_table(s);
    ensure_weight_table(s);                        // the family's other operand: the model's weights in every row unless set
    s->cone.set(who, s->stream, batch, mask, s->cone_mask, rows, n_rows, on_device, [](const double*, int) {});
    s->cone_set = true;
    s->select_row_kernels();                       // every run enqueued from here on: the per-problem kernels
    if (!on_device) HIP_CHECK(hipStreamSynchronize(s->stream));               // the caller's host arrays
  });
}

int bpmpc_solver_get_cone_params(bpmpc_solver* s, int robot, double* row) {
  if (s && !row) { set_last_error("bpmpc_solver_get_cone_params: null row"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(s, [&] {
    if (robot >= s->settings.max_batch) throw std::length_error("bpmpc_solver_get_cone_params: robot exceeds max_batch");
    if (robot < 0 || !s->cone.d_params) {          // the start row, which is also every row of a handle that never had one set
      cone_start_row(s->rm, row);
      return;
    }
    s->cone.get("bpmpc_solver_get_cone_params", s->stream, s->settings.max_batch, robot, row);
  });
}

int bpmpc_solver_reset_cone_params(bpmpc_solver* s) {
  return guarded(s, [&] {
    s->cone_set = false;
    s->select_row_kernels();                       // back to the default kernels unless a weight row is set
    if (s->cone.d_params) s->cone.fill_from_start(s->stream, s->settings.max_batch);
  });
}

}  // extern "C"
