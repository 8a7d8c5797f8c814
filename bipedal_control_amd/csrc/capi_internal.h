// Shared between the host-only part (capi.cpp) and the device part (solver.hip) of libbpmpc.so.
#pragma once
#include <hip/hip_runtime.h>

#include <exception>
#include <string>

#include "../../include/bpmpc.h"
#include "robot_model.h"

namespace bpmpc {
void set_last_error(const std::string& message);
const RobotModel& model_of(const bpmpc_model* handle);

struct DeviceModel;

// ---- controller tick (controller.cpp): what it reads of the solver and the WBC handles
struct SolverTickView {
  int device, batch, N, nx, nu, nj, feedback;
  hipStream_t stream;
  const DeviceModel* d_model;
  const int *p_grid, *g_nodes, *g_kind, *g_mode;    // grid tables of the last setup
  const double *g_time, *x, *u, *K;                 // solution of the last run
  double* loop_x;                                   // [max_batch][nx]: start of bpmpc_solver_setup_commands(x0 = NULL) after a tick
};
// Throws (std::invalid_argument: no completed run since the last setup; the Unsupported error of solver.hip: the DDP solver).
SolverTickView solver_tick_view(bpmpc_solver* s);
// The tick wrote loop_x: the next setup_commands(x0 = NULL) starts from it (until the next rollout).
void solver_tick_done(bpmpc_solver* s);
int solver_device(const bpmpc_solver* s);
// ---- restarts (bpmpc_controller_restart): the solver's stream and model after the checks of bpmpc_solver_restart (SQP, batch of the last setup)
struct SolverRestartView {
  int device, nj;
  hipStream_t stream;
  const DeviceModel* d_model;
};
SolverRestartView solver_restart_view(bpmpc_solver* s, int batch);
// bpmpc_solver_restart without the API wrapper (throws)
void solver_restart(bpmpc_solver* s, int batch, const int* mask, const double* x_new, bool inputs_on_device);
// The status solver.hip returns for an exception it threw.
int solver_translate(const std::exception& e);

struct WbcTickView {
  int device, max_batch, n, nv, nj;
  double* sol;                                      // [max_batch][n]: the last QP solution of every robot (lastQpSol_)
  int* status;                                      // [max_batch]
};
WbcTickView wbc_tick_view(const bpmpc_wbc* w);
int wbc_translate(const std::exception& e);        // the status wbc.hip returns for an exception it threw
// k_wbc on device inputs, enqueued on `stream`; later work on the WBC handle's own stream waits for it.
void wbc_launch_on(bpmpc_wbc* w, int batch, const double* state_des, const double* input_des, const double* rbd_meas, const int* mode, hipStream_t stream);
// bpmpc_wbc_restart on a device mask, enqueued on `stream` with the same cross-stream rule
void wbc_restart_on(bpmpc_wbc* w, int batch, const int* mask, hipStream_t stream);
}  // namespace bpmpc
