// Per-problem cost weights of the solver handle (include/bpmpc.h "Per-problem cost weights"): the row table, the host check of a row, and the entry
// points bpmpc_solver_set_weights / get_weights / reset_weights / check_weights.  The kernels that read the rows are in k_weights.hip; which kernels
// a stage launches is decided where every kernel is chosen, from bpmpc_solver::plan_weights (solver.h, solver.hip).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "solver.h"
#include "weight_structure.h"

namespace bpmpc {
namespace {

constexpr int kStride = BPMPC_SOLVER_WEIGHT_STRIDE;
static_assert(kStride == kWeightRowStride && kStride >= 2 * kWeightDim * kWeightDim, "one row format for the ABI, the table and the kernels");

// the model's Q then R, zeros behind them: the start row
std::vector<double> model_row(const bpmpc_solver* s) {
  std::vector<double> row(kStride, 0.0);
  std::copy(s->rm.Q.begin(), s->rm.Q.end(), row.begin());
  std::copy(s->rm.R.begin(), s->rm.R.end(), row.begin() + s->nx * s->nx);
  return row;
}

void check_supported(const bpmpc_solver* s, const char* who) {
  if (s->is_ddp())
    throw Unsupported(std::string(who) + ": the DDP solver keeps the model's weights (its cost of recorded points and its ILQR lineariser read them)");
  if (s->settings.reference_kernels)
    throw Unsupported(std::string(who) + ": per-problem weights are implemented by the fast kernels only (settings.reference_kernels reads the model's Q and R)");
}

void check_host_row(const bpmpc_solver* s, const char* who, const double* row, int r) {
  const WeightVerdict v = check_weight_row(row, s->rm.Q.data(), s->nx, s->rm.R.data(), s->nu);
  if (v.fault == WeightFault::None) return;
  throw std::invalid_argument(std::string(who) + ": row " + std::to_string(r) + ", " + v.matrix + "[" + std::to_string(v.row) + "][" + std::to_string(v.col) + "] " +
                              weight_fault_text(v.fault));
}

void derive_diagonals(bpmpc_solver* s) {
  kl::weight_diagonals(s->stream, s->weights.d_params, s->weight_q_diag, s->settings.max_batch, s->nx);
  HIP_CHECK(hipGetLastError());
}

}  // namespace

// the table exists from the first set of EITHER table on (bpmpc_solver_set_weights, bpmpc_solver_set_cone_params: one kernel family reads both;
// 2 x max_batch rows of 9 KB); every row starts as the model's
void ensure_weight_table(bpmpc_solver* s) {
  if (s->weights.d_params) return;
  const int B = s->settings.max_batch;
  s->weights.create(s->weight_mem, B, kStride, s->nx * s->nx + s->nu * s->nu, model_row(s).data());
  s->weight_q_diag = s->weight_mem.alloc<double>((size_t)B * kWeightDim);
  s->weight_mask = s->weight_mem.alloc<int>(B);
  s->weights.fill_from_start(s->stream, B);
  derive_diagonals(s);
}

void release_weights(bpmpc_solver* s) { s->weight_mem.release(); }

}  // namespace bpmpc

extern "C" {

int bpmpc_solver_set_weights(bpmpc_solver* s, int batch, const int* mask, const double* rows, int n_rows, int inputs_on_device) {
  if (s && !rows) { set_last_error("bpmpc_solver_set_weights: null rows"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(s, [&] {
    const char* who = "bpmpc_solver_set_weights";
    check_supported(s, who);
    if (s->batch < 1 || batch != s->batch) throw std::invalid_argument(std::string(who) + ": batch must equal the batch of the last setup");
    const bool on_device = inputs_on_device != 0;
    if (n_rows != 1 && n_rows != batch) throw std::invalid_argument(std::string(who) + ": n_rows must be 1 or batch");
    if (!on_device)      // before anything is allocated or enqueued
      for (int r = 0; r < n_rows; ++r)
        if (n_rows == 1 || !mask || mask[r]) check_host_row(s, who, rows + (size_t)r * kStride, r);
    ensure_weight_table(s);
    ensure_cone_table(s);                          // the family's other operand: the model's cone parameters in every row unless set
    s->weights.set(who, s->stream, batch, mask, s->weight_mask, rows, n_rows, on_device, [](const double*, int) {});
    derive_diagonals(s);
    s->weights_set = true;
    s->select_row_kernels();                       // every run enqueued from here on: the per-problem kernels
    if (!on_device) HIP_CHECK(hipStreamSynchronize(s->stream));               // the caller's host arrays
  });
}

int bpmpc_solver_get_weights(bpmpc_solver* s, int robot, double* row) {
  if (s && !row) { set_last_error("bpmpc_solver_get_weights: null row"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(s, [&] {
    if (robot >= s->settings.max_batch) throw std::length_error("bpmpc_solver_get_weights: robot exceeds max_batch");
    if (robot < 0 || !s->weights.d_params) {      // the start row, which is also every row of a handle that never had one set
      const std::vector<double> start = model_row(s);
      std::copy(start.begin(), start.end(), row);
      return;
    }
    s->weights.get("bpmpc_solver_get_weights", s->stream, s->settings.max_batch, robot, row);
  });
}

int bpmpc_solver_reset_weights(bpmpc_solver* s) {
  return guarded(s, [&] {
    s->weights_set = false;
    s->select_row_kernels();                       // the kernels of a handle that never had a row set, unless a cone row is set
    if (!s->weights.d_params) return;
    s->weights.fill_from_start(s->stream, s->settings.max_batch);
    derive_diagonals(s);
  });
}

int bpmpc_solver_check_weights(const bpmpc_solver* s, const double* row) {
  if (!s || !row) { set_last_error("bpmpc_solver_check_weights: null solver handle or row"); return BPMPC_ERR_INVALID_ARGUMENT; }
  return guarded(BPMPC_ERR_IO, [&] { check_host_row(s, "bpmpc_solver_check_weights", row, 0); });
}

}  // extern "C"
