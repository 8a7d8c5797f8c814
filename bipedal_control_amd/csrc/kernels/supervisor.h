// The per-robot supervisor on the device (include/bpmpc.h "Supervisor"): which controller drives which robot of a batch.
//   InitialJointPositionController::update   bipedal_controllers/src/InitialJointController.cpp:110-141   the INIT command and its clamp
//   SafetyChecker::check                     bipedal_controllers/include/bipedal_controllers/SafetyChecker.h:39-52   the tilt limit
//   stopRequest                              bipedal_controllers/src/BipedalController.cpp:232-236   RUN -> STOPPED
//
// Mapping: a group of 16 lanes owns a robot, four robots per wavefront.  Lane g carries joint g (g < nj <= 12) and, for g < 12, one of the
// twelve base entries of rbd, so every row - measurement, joint rows, latched joints, the five command rows - is read and written by
// consecutive lanes on consecutive words.  The per-robot scalars (state, cause, the two clocks, the parameter row) are read by every lane of
// the group from one address and written by lane 0.  Two reductions run inside the group with __shfl_xor of width 16: the OR of the lanes'
// "not finite" bits, and the OR of the lanes' "outside the settle tolerance" flags.  The five counters are formed per wavefront from ballots of
// the groups' leaders and added by lanes 0..4 with one vector atomicAdd.
//
// The arithmetic of a lane and of a robot is written once, as __host__ __device__ functions; supervise_group (the kernel) and
// bpmpc_supervisor_rows_host (supervisor.hip: a loop over the lanes between the same reductions) compile this text.  No multiply-add
// contraction: the ramp is q_latch + s (q_init - q_latch) with s = elapsed / ramp_time, each operation rounded once.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace bpmpc {

#define SUP_HD __host__ __device__ __forceinline__

constexpr int kSupParamStride = 8;
constexpr int kSupGroup = 16;                 // lanes of a robot
constexpr int kSupMaxJoints = 12;
constexpr int kSupCounts = 8;
enum SupState { kSupInit = 0, kSupRun = 1, kSupStopped = 2 };
enum SupParam { kSupTiltLimit, kSupMinBaseHeight, kSupRampTime, kSupSettlePosTol, kSupSettleVelTol, kSupSettleTime, kSupStopKd, kSupParamUsed };
enum SupBit { kSupBitRoll = 1, kSupBitPitch = 2, kSupBitHeight = 4, kSupBitMeasurement = 8, kSupBitCommand = 16, kSupBitRequest = 64 };

struct SupervisorArgs {
  int batch, nj, cmd_stride;                  // cmd_stride: of run_pos / run_vel / run_tau (nj, or 3 nj for a tick's joint_cmd); gains are [b][nj]
  double period;
  const double* rbd;                          // [batch][2 (6 + nj)]
  const double *run_pos, *run_vel, *run_tau, *run_kp, *run_kd;      // the RUN command; run_pos == nullptr: there is none
  const double* params;                       // [max_batch][kSupParamStride]
  const double *q_init, *kp_init, *kd_init, *lower, *upper;         // [max_batch][nj]
  int *state, *cause, *unsafe, *ready, *latch;                      // [max_batch]
  int* counts;                                // [kSupCounts]
  double *elapsed, *settled;                  // [max_batch]
  double* q_latch;                            // [max_batch][nj]
  double *pos_des, *vel_des, *tau_ff, *kp, *kd;                     // [max_batch][nj]
};

struct SupRobot { int state, cause, unsafe, ready, latch; double elapsed, settled; };
struct SupCommand { double pos, vel, tau, kp, kd; };

SUP_HD bool sup_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for a NaN and for +-infinity

// lane g's share of the measurement rb = [zyx, position, joints, angular velocity, linear velocity, joint velocities]: base entry g (g < 12)
// and joint g (g < nj).  Returns kSupBitMeasurement when one of them is not finite.
SUP_HD int sup_lane_measure(int g, int nj, const double* rb, double* q, double* v) {
  const int nv = 6 + nj;
  bool ok = true;
  if (g < 12) ok = sup_finite(g < 6 ? rb[g] : rb[nv + g - 6]);
  *q = 0.0; *v = 0.0;
  if (g < nj) {
    *q = rb[6 + g]; *v = rb[nv + 6 + g];
    ok = ok && sup_finite(*q) && sup_finite(*v);
  }
  return ok ? 0 : kSupBitMeasurement;
}

// lane g's entries of the RUN command (g < nj); returns kSupBitCommand when one of the five is not finite
SUP_HD int sup_lane_run_command(const double* pos, const double* vel, const double* tau, const double* kp, const double* kd, SupCommand* c) {
  c->pos = *pos; c->vel = *vel; c->tau = *tau; c->kp = *kp; c->kd = *kd;
  return sup_finite(c->pos) && sup_finite(c->vel) && sup_finite(c->tau) && sup_finite(c->kp) && sup_finite(c->kd) ? 0 : kSupBitCommand;
}

// the limit bits of a robot.  SafetyChecker's comparisons are kept as they are: strict, and false for a NaN
SUP_HD int sup_limit_bits(const double* prm, double roll, double pitch, double z) {
  int u = 0;
  if (fabs(roll) > prm[kSupTiltLimit]) u |= kSupBitRoll;
  if (fabs(pitch) > prm[kSupTiltLimit]) u |= kSupBitPitch;
  if (prm[kSupMinBaseHeight] > 0.0 && z < prm[kSupMinBaseHeight]) u |= kSupBitHeight;
  return u;
}

// steps 2 and 3: stopRequest, then the state's clock
SUP_HD void sup_transition(SupRobot& r, int unsafe, double period) {
  r.unsafe = unsafe;
  if (r.state == kSupRun && unsafe != 0) { r.state = kSupStopped; r.cause = unsafe; r.elapsed = 0.0; r.settled = 0.0; r.ready = 0; }
  r.elapsed += period;
}

// the ramp's fraction: 1 selects q_init itself
SUP_HD double sup_ramp(const double* prm, double elapsed) {
  const double T = prm[kSupRampTime];
  return (T == 0.0 || elapsed >= T) ? 1.0 : elapsed / T;
}

// step 4 for joint g of a robot in state r.state (after the transition): the command, the latched joint (INIT with the latch pending), and
// whether this joint breaks the settle test.  `run` is the lane's RUN command (read only in RUN).
SUP_HD bool sup_lane_command(const SupRobot& r, const double* prm, double s, double q, double v, const SupCommand& run, double q_init, double kp_init,
                             double kd_init, double lower, double upper, double* q_latch, SupCommand* c) {
#pragma clang fp contract(off)
  if (r.state == kSupRun) { *c = run; return false; }
  if (r.state == kSupStopped) {
    c->pos = sup_finite(q) ? q : 0.0; c->vel = 0.0; c->tau = 0.0; c->kp = 0.0; c->kd = prm[kSupStopKd];
    return false;
  }
  if (r.latch) *q_latch = sup_finite(q) ? q : q_init;
  double target = q_init;
  if (s != 1.0) { const double d = q_init - *q_latch; target = *q_latch + s * d; }
  // enforceJointLimits (InitialJointController.cpp:135-141): above the upper limit first
  if (target > upper) target = upper;
  else if (target < lower) target = lower;
  c->pos = target; c->vel = 0.0; c->tau = 0.0; c->kp = kp_init; c->kd = kd_init;
  return !(fabs(q - target) <= prm[kSupSettlePosTol] && fabs(v) <= prm[kSupSettleVelTol]);
}

// the end of step 4 for the robot: the settle clock and the ready flag of INIT, ready = 0 of STOPPED; RUN keeps what entering it set
SUP_HD void sup_finish(SupRobot& r, const double* prm, double s, bool a_joint_breaks, double period) {
  if (r.state == kSupInit) {
    r.latch = 0;
    const bool holds = s == 1.0 && r.unsafe == 0 && !a_joint_breaks;
    r.settled = holds ? r.settled + period : 0.0;
    r.ready = holds && r.settled >= prm[kSupSettleTime] ? 1 : 0;
  } else if (r.state == kSupStopped) r.ready = 0;
}

// bpmpc_supervisor_request for one robot
SUP_HD void sup_request(SupRobot& r, int target, int only_ready) {
  if (target == kSupRun && (r.state != kSupInit || (only_ready && r.ready != 1))) return;
  r.state = target; r.elapsed = 0.0; r.settled = 0.0; r.ready = 0;
  if (target == kSupStopped) r.cause = kSupBitRequest;
  else r.cause = 0;
  if (target == kSupInit) r.latch = 1;
}

#if defined(__HIPCC__)
__device__ __forceinline__ int sup_group_or(int x) {
  for (int m = 1; m < kSupGroup; m <<= 1) x |= __shfl_xor(x, m, kSupGroup);
  return x;
}

// one update of the robots of this wavefront (64 threads per workgroup, grid = ceil(batch / 4))
__device__ __forceinline__ void supervise_group(const SupervisorArgs& a) {
  constexpr int RPW = 64 / kSupGroup;
  const int sub = threadIdx.x / kSupGroup, g = threadIdx.x % kSupGroup, nj = a.nj;
  const int bq = blockIdx.x * RPW + sub;
  const bool valid = bq < a.batch;
  const size_t b = valid ? bq : 0;          // groups beyond the batch compute robot 0 and write nothing (the shuffles need every lane)
  const bool joint = g < nj;
  const size_t row = b * nj + (joint ? g : 0);

  const double* prm = a.params + b * kSupParamStride;
  const double* rb = a.rbd + b * 2 * (6 + nj);
  SupRobot r{a.state[b], a.cause[b], 0, a.ready[b], a.latch[b], a.elapsed[b], a.settled[b]};

  // step 1
  double q, v;
  int bits = sup_lane_measure(g, nj, rb, &q, &v);
  SupCommand run{0.0, 0.0, 0.0, 0.0, 0.0};
  if (r.state == kSupRun) {
    if (!a.run_pos) bits |= kSupBitCommand;
    else if (joint) {
      const size_t c = b * a.cmd_stride + g;
      bits |= sup_lane_run_command(a.run_pos + c, a.run_vel + c, a.run_tau + c, a.run_kp + row, a.run_kd + row, &run);
    }
  }
  const int unsafe = sup_group_or(bits) | sup_limit_bits(prm, rb[2], rb[1], rb[5]);

  // steps 2 to 4
  sup_transition(r, unsafe, a.period);
  const double s = sup_ramp(prm, r.elapsed);
  const bool latching = r.state == kSupInit && r.latch != 0;
  double ql = 0.0, qi = 0.0, kpi = 0.0, kdi = 0.0, lo = 0.0, up = 0.0;
  if (joint && r.state == kSupInit) {
    ql = a.q_latch[row]; qi = a.q_init[row]; kpi = a.kp_init[row]; kdi = a.kd_init[row]; lo = a.lower[row]; up = a.upper[row];
  }
  SupCommand c{0.0, 0.0, 0.0, 0.0, 0.0};
  bool breaks = false;
  if (joint) breaks = sup_lane_command(r, prm, s, q, v, run, qi, kpi, kdi, lo, up, &ql, &c);
  const bool any_breaks = sup_group_or(breaks ? 1 : 0) != 0;
  sup_finish(r, prm, s, any_breaks, a.period);

  if (valid && joint) {
    a.pos_des[row] = c.pos; a.vel_des[row] = c.vel; a.tau_ff[row] = c.tau; a.kp[row] = c.kp; a.kd[row] = c.kd;
    if (latching) a.q_latch[row] = ql;
  }
  const bool leader = valid && g == 0;
  if (leader) {
    a.state[b] = r.state; a.cause[b] = r.cause; a.unsafe[b] = r.unsafe; a.ready[b] = r.ready; a.latch[b] = r.latch;
    a.elapsed[b] = r.elapsed; a.settled[b] = r.settled;
  }

  // step 5: the wavefront's share of the counters, lanes 0..4 adding one each
  const int n_init = __popcll(__ballot(leader && r.state == kSupInit)), n_run = __popcll(__ballot(leader && r.state == kSupRun)),
            n_stop = __popcll(__ballot(leader && r.state == kSupStopped)), n_ready = __popcll(__ballot(leader && r.ready != 0)),
            n_unsafe = __popcll(__ballot(leader && r.unsafe != 0));
  const int lane = threadIdx.x;
  const int add = lane == 0 ? n_init : lane == 1 ? n_run : lane == 2 ? n_stop : lane == 3 ? n_ready : lane == 4 ? n_unsafe : 0;
  if (add != 0) atomicAdd(a.counts + lane, add);
}
#endif

}  // namespace bpmpc
