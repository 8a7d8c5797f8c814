// The policy buffer (include/bpmpc.h "Policy buffer", policy.hip): the reference's MPC_MRT_Interface between the solve and the control tick
// (bipedal_controllers/src/BipedalController.cpp:191-200 updatePolicy / evaluatePolicy, :332-350 advanceMpc).  Two slots of the solution and the
// grid row of every robot; a publish copies the solver's arrays into the slot the ticks do not read, an adoption makes that slot the one they
// read.  The controller (controller.cpp) runs its ticks on the buffer's stream and hands the tick kernel the pointers of the front slot.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bpmpc.h"
#include "device_handle.h"

struct bpmpc_solver;

namespace bpmpc {

// One slot: the arrays of TickArgs (kernels/tick.h) with the strides of the solver's (N = max_nodes), the grid tables one row per ROBOT
struct PolicySlot {
  double *x = nullptr, *u = nullptr, *K = nullptr;      // [max_batch][N + 1][NX], [max_batch][N][NU], [max_batch][N][NU][NX] (K: feedback only)
  double* g_time = nullptr;                             // [max_batch][N + 1]
  int *g_kind = nullptr, *g_mode = nullptr, *g_nodes = nullptr;      // [max_batch][N], [max_batch][N], [max_batch]
};

// k_policy_publish (policy.hip).  Robot b is TAKEN when mask[b] != 0 (mask NULL: every robot) and, with skip_failed, the status of its stats row
// is not 2: its live nodes travel from the solver's arrays (grid row p_grid[b]) to `back`, and its pending flag, t0 and status are set.  A robot
// that is not taken keeps its policy: in the `first` publish since an adoption its live nodes travel from `front` to `back`, so that the slot as
// a whole can become the front; in a later publish it is not touched.
struct PolicyPublishArgs {
  int batch, N, nx, feedback, skip_failed, first, wg_per_robot;
  const int* mask;                    // [batch] nullable
  const double* stats;                // [batch][kStatsStride] of the last run
  const int *p_grid, *g_nodes, *g_kind, *g_mode;
  const double *g_time, *x, *u, *K;   // the solver's solution and grid tables
  PolicySlot front, back;
  int *pending, *status_pend;         // [max_batch]
  double* t0_pend;                    // [max_batch]
};

}  // namespace bpmpc

struct bpmpc_policy {
  bpmpc_solver* s = nullptr;
  int device = 0, max_batch = 0, N = 0, nx = 0, nu = 0, feedback = 0;
  bpmpc::DeviceBuffers mem;           // every d_* and slot array below
  // the buffer's stream: adoptions and, for an attached controller, ticks, restarts' observations and joint-gain writes.  Foreign launches: what
  // the solver's stream does to the state those ticks share with it (tick_x read by setup_commands(x0 = NULL), written by a restart)
  bpmpc::StreamHandshake hs;
  hipEvent_t ev_publish = nullptr;    // the last publish on the solver's stream: an adoption waits for it
  hipEvent_t ev_adopt = nullptr;      // the last adoption on the buffer's stream: the next publish waits for it (ticks before it read its back slot)
  bpmpc::PolicySlot slot[2];
  int front = 0;                      // the slot ticks read.  One value for the batch: the tick kernel takes one set of pointers
  int* d_identity = nullptr;          // [max_batch] 0, 1, ..: the p_grid of a slot
  int *d_pending = nullptr, *d_generation = nullptr, *d_status = nullptr, *d_status_pend = nullptr, *d_mask = nullptr;      // [max_batch]
  double *d_t0 = nullptr, *d_t0_pend = nullptr;      // [max_batch]
  int attached = 0;                   // controllers that tick on this buffer (bpmpc_controller_attach_policy)
  int batch = 0;                      // of the last publish (0: none yet)
  bool outstanding = false;           // a publish that no adoption has taken over
  bool full_outstanding = false;      // ... one of them covered every robot unconditionally
  bool ready = false;                 // such a publish has been adopted: the front slot holds a policy for every robot of `batch`
  bool restart_hold = false;          // a controller restart since the last adoption: buffered ticks wait for the next one
};

namespace bpmpc {
// policy.hip
void launch_policy_publish(hipStream_t stream, int num_cus, const PolicyPublishArgs& a, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// The refusals of a buffered tick (controller.cpp): the initial policy, a restart without an adoption since, the batch of the published policy
void check_buffered_tick(const bpmpc_policy* p, int batch, const char* who);
}  // namespace bpmpc
