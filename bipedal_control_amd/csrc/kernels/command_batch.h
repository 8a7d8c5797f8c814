// Device-resident target trajectories (bpmpc_command_batch, include/bpmpc.h): one stored TargetTrajectories per robot kept in HBM between
// setups, changed only by the calls that play the reference's command messages - BipedalController::starting (BipedalController.cpp:145,153),
// TargetTrajectoriesPublisher (TargetTrajectoriesPublisher.h:48-87, .cpp:30-99) - and read by the device-side setups of the solver it is
// attached to.  Three kernels: a message to a stored target (the arithmetic is ref_command_target of reference_device.h, what k_command_targets
// runs), the masked store of given trajectories, and the window of the stored trajectories into the solver's p_tgt_* tables with the rule of the
// host path (setup in solver.hip).  Defined here for command_batch.hip, the one unit that launches them.
#pragma once
#include <hip/hip_runtime.h>

#include "reference_device.h"

namespace bpmpc {

constexpr int kCommandStatus = 4;       // per robot: messages applied, messages dropped, source of the stored target, number of stored points
enum CommandSource { kCommandNone = 0, kCommandStart = 1, kCommandVelocity = 2, kCommandGoal = 3, kCommandTrajectory = 4 };
constexpr int kCommandMinPoints = 2, kCommandMaxPoints = 64;

struct CommandStore {
  int max_points, nx;
  int* status;             // [max_batch][kCommandStatus]
  double* times;           // [max_batch][max_points]
  double* states;          // [max_batch][max_points][nx]
};

struct CommandMessageArgs {
  CommandTargetArgs c;     // the constants and c.goal; c.t0 / c.x0 / c.cmd_vel: the observation times, the observations, the message rows
  CommandStore store;
  const int* mask;         // NULL: every robot below c.batch
  int source;              // kCommandStart, kCommandVelocity or kCommandGoal
};

// One thread per robot.  start: the single point (t_obs, x_obs).  A velocity or goal message: ref_command_target from that observation, once; at
// t_obs == 0.0 it is dropped and counted (TargetTrajectoriesPublisher.h:49,75: the publisher has not seen an observation yet)
__global__ __launch_bounds__(64) void k_command_message(CommandMessageArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.c.batch || (a.mask && !a.mask[b])) return;
  const int nx = a.store.nx;
  const double t = a.c.t0[b];
  const double* x = a.c.x0 + (size_t)b * nx;
  int* st = a.store.status + (size_t)b * kCommandStatus;
  double* ts = a.store.times + (size_t)b * a.store.max_points;
  double* xs = a.store.states + (size_t)b * a.store.max_points * nx;
  if (a.source == kCommandStart) {
    ts[0] = t;
    for (int i = 0; i < nx; ++i) xs[i] = x[i];
    st[2] = kCommandStart; st[3] = 1;
    return;
  }
  if (t == 0.0) { st[1] += 1; return; }
  ref_command_target(a.c, t, x, a.c.cmd_vel + (size_t)b * 4, ts, xs);
  st[0] += 1; st[2] = a.source; st[3] = 2;
}

struct CommandStoreArgs {
  CommandStore store;
  int batch;
  const int* mask;         // NULL: every robot below batch
  const int* n_points;     // [batch]
  const double* times;     // [batch][max_points]
  const double* states;    // [batch][max_points][nx]
};

// One wavefront per robot: lane l copies entries l, l + 64, .. of the robot's used times and states (consecutive lanes, consecutive doubles).
// A count from the device is not validated by the host: it is held inside 0 .. max_points here so that no row is left
__global__ __launch_bounds__(64) void k_command_store(CommandStoreArgs a) {
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= a.batch || (a.mask && !a.mask[b])) return;
  const int P = a.store.max_points, nx = a.store.nx;
  const int n = min(max(a.n_points[b], 0), P);
  const double* ts = a.times + (size_t)b * P;
  const double* xs = a.states + (size_t)b * P * nx;
  double* dt = a.store.times + (size_t)b * P;
  double* dx = a.store.states + (size_t)b * P * nx;
  for (int i = l; i < n; i += 64) dt[i] = ts[i];
  for (int i = l; i < n * nx; i += 64) dx[i] = xs[i];
  if (l == 0) { int* st = a.store.status + (size_t)b * kCommandStatus; st[2] = kCommandTrajectory; st[3] = n; }
}

struct CommandWindowArgs {
  CommandStore store;      // read only
  int batch;
  double horizon;
  const double* t0;        // per problem
  double* tgt_t;           // [batch][kMaxTargetPoints]
  double* tgt_x;           // [batch][kMaxTargetPoints][nx]
  int* tgt_n;
  int* flag;               // per problem: 0 taken, < 0 the robot has no target, > 0 that many points in the window (more than kMaxTargetPoints)
};

// One thread per robot: the points the piecewise-linear interpolation can touch for query times in [t0, t0 + horizon] - the last one at or before
// the window, the ones inside, the first one behind it (the lower_bound rule of setup, solver.hip) - go to the solver's tables
__global__ __launch_bounds__(64) void k_command_window(CommandWindowArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.batch) return;
  const int P = a.store.max_points, nx = a.store.nx;
  const int n = min(a.store.status[(size_t)b * kCommandStatus + 3], P);
  if (n < 1) { a.flag[b] = -1; return; }
  const double* ts = a.store.times + (size_t)b * P;
  const double lo = a.t0[b], hi = a.t0[b] + a.horizon;
  const int i0 = max(0, ref_lower_bound(ts, n, lo) - 1);
  const int i1 = min(n - 1, ref_lower_bound(ts, n, hi));
  const int np = i1 - i0 + 1;
  if (np > kMaxTargetPoints) { a.flag[b] = np; return; }
  const double* xs = a.store.states + ((size_t)b * P + i0) * nx;
  double* ot = a.tgt_t + (size_t)b * kMaxTargetPoints;
  double* ox = a.tgt_x + (size_t)b * kMaxTargetPoints * nx;
  for (int i = 0; i < np; ++i) ot[i] = ts[i0 + i];
  for (int i = 0; i < np * nx; ++i) ox[i] = xs[i];
  a.tgt_n[b] = np;
  a.flag[b] = 0;
}

}  // namespace bpmpc
