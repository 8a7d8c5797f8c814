// The command batch (include/bpmpc.h: bpmpc_command_batch) as the solver's device-side setups see it: the handle, and the window of its stored
// target trajectories into the solver's tables, which launch_command_targets (solver.hip) enqueues in place of k_command_targets while a
// command batch is attached.  Everything else of the handle lives in command_batch.hip.
#pragma once
#include "solver.h"

// One TargetTrajectories per robot on the device; created on a solver, enqueues on its stream, destroyed before it.
struct bpmpc_command_batch {
  bpmpc_solver* solver = nullptr;
  int max_batch = 0, max_points = 0, nx = 0;
  int* status = nullptr;                                   // [max_batch][kCommandStatus]: applied, dropped, source, number of stored points
  double* times = nullptr;                                 // [max_batch][max_points]
  double* states = nullptr;                                // [max_batch][max_points][nx]
  // device copies of host inputs (inputs_on_device == 0)
  int* d_mask = nullptr;                                   // [max_batch]
  int* d_n = nullptr;                                      // [max_batch]
  double* d_t = nullptr;                                   // [max_batch]
  double* d_cmd = nullptr;                                 // [max_batch][4]
  double* d_x = nullptr;                                   // [max_batch][nx]
  double* d_times = nullptr;                               // [max_batch][max_points]
  double* d_states = nullptr;                              // [max_batch][max_points][nx]
  bpmpc::DeviceBuffers mem;
};

namespace bpmpc {

// s->commands windowed into p_tgt_t / p_tgt_x / p_tgt_n for the problems' t0 (p_t0, uploaded by the setup) and `horizon`; the verdicts go to
// s->tgt_flag, which accept_reference_grids reads back with the grid sizes.  Reads the stored trajectories only.
void launch_command_window(bpmpc_solver* s, int batch, double horizon);

}  // namespace bpmpc
