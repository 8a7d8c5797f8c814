// The controller tick on the device (BipedalController::update, bipedal_controllers/src/BipedalController.cpp:186-262) for a batch of robots:
//   observation   computeCentroidalStateFromRbdModel + yaw unwrap (:400-403): measured rbd state -> x_obs = [A(q) v / m, q]
//   policy        MRT_BASE::evaluatePolicy (:199) of the last solution at t: x* = LinearInterpolation of x, u* = uff(t) + K(t) x_obs
//                 (LinearController) or u(t) (FeedforwardController), planned mode = ModeSchedule::modeAtTime
//   safety        SafetyChecker::check (SafetyChecker.h:39-52): |pitch|, |roll| of the observation at most pi/3
// (the WBC between policy and commands is k_wbc, kernels/wbc.h; k_tick_commands only gathers its joint block).  The observation alone, for the
// robots of a restart, is k_restart_observe (restart_observe below).
//
// Mapping: the lane-per-coordinate layout of linearize_fast.h / rollout.h - lane g of a robot carries generalised coordinate g
// (q = [base position, Euler ZYX, joints], v = [base linear velocity, Euler rates, joint rates]), 16 lanes per robot at nj = 10, 32 at nj = 12,
// four or two robots per wavefront.  The centroidal momentum matrix is built column by column as in eval_lane: joint lanes compose their
// chain frames from the joint-local rotations in LDS, body lanes publish their inertia about the base origin, every lane sums the composite
// of the subtree its coordinate moves and forms column g; h = sum_g A_g v_g is a reduction over the robot's lanes.  Oracle:
// oracle/wbc_py.py measured_state / centroidal_momentum_matrix, oracle/reference_py.py time_segment / primal_solution_arrays /
// linear_controller_input / mode_at_time.
#pragma once
#include "kinematics.h"
#include "rollout.h"

namespace bpmpc {

struct TickArgs {
  int batch, N;                       // N = node stride of the solution arrays
  int feedback;                       // sqp.useFeedbackPolicy: 1 u* = uff(t) + K(t) x_obs, 0 u* = u(t)
  const int *p_grid, *g_nodes, *g_kind, *g_mode;
  const double *g_time, *x, *u, *K;   // solution of the last run: [batch][N + 1][NX], [batch][N][NU], [batch][N][NU][NX]
  const double* t;                    // [batch] query times
  const double* rbd;                  // [batch][2 (6 + NJ)] measured rigid-body state; nullptr: x_in is the state (evaluatePolicy alone)
  const double* x_in;                 // [batch][NX] (rbd == nullptr)
  double* yaw_last;                   // [batch] yaw of the previous observation (rbd != nullptr): read and updated
  double *x_obs, *x_loop;             // [batch][NX] observation (rbd != nullptr); x_loop nullable: a second copy (the solver's closed-loop start)
  int* safe;                          // [batch] (rbd != nullptr)
  double *x_opt, *u_opt;              // [batch][NX], [batch][NU]
  int* mode;                          // [batch]
};

template <int NJ>
struct TickLds {
  using C = LinFastCfg<NJ>;
  double T[C::NPW][NJ][9];            // joint-local rotations Rfix E(q) of every joint
  double comp[C::NPW][C::NB][10];     // per body: mass, first moment, inertia - about the base origin
  double xo[C::NPW][C::NX];           // the observation (the state K multiplies)
};

// [ROS angles, recalled] angles::normalize_angle: (-pi, pi]; shortest_angular_distance(from, to) = normalize_angle(to - from)
__device__ __forceinline__ double tick_normalize_angle(double a) {
  const double r = fmod(a + M_PI, 2.0 * M_PI);
  return r <= 0.0 ? r + M_PI : r - M_PI;
}

// The observation of one robot (BipedalController.cpp:397-403) into w.xo of its lane group: x_obs = [A(q) v / m, q] from the measured state rb,
// the yaw unwrapped against yl; the yaw lane also stores the unwrapped yaw to *yaw_out (nullable).  Every lane of the group takes part (DPP
// reductions); returns behind the LDS barrier that follows the writes of xo.
template <int NJ>
__device__ __forceinline__ void tick_observation(const DeviceModel& md, TickLds<NJ>& w, const double* rb, double yl, double* yaw_out) {
  using C = LinFastCfg<NJ>;
  constexpr int G = C::G, NB = C::NB, LPN = C::LPN;
  static_assert(C::G0 == 0, "one lane per coordinate");
  const int sub = threadIdx.x / LPN, g = threadIdx.x % LPN;
  double* xo = w.xo[sub];
  // ---- measured state (WbcBase::updateMeasured / CentroidalModelRbdConversions layout): q_g, v_g of this lane
  const double pb[3] = {rb[3], rb[4], rb[5]};
  double sy, cy, sp, cp, sr, cr;
  sincos(rb[0], &sy, &cy);
  sincos(rb[1], &sp, &cp);
  sincos(rb[2], &sr, &cr);
  double qg = 0.0, vg = 0.0;
  if (g < 3) { qg = rb[3 + g]; vg = rb[G + 3 + g]; }
  else if (g < 6) {
    qg = rb[g - 3];
    double rates[3];
    fused::euler_rates_from_world_omega(sy, cy, sp, cp, rb + G, rates);
    vg = g == 3 ? rates[0] : (g == 4 ? rates[1] : rates[2]);
  } else if (g < G) { qg = rb[g]; vg = rb[G + g]; }
  const bool is_joint = g >= 6 && g < G, is_body = g >= 5 && g < G;
  const int body = is_body ? g - 5 : 0;
  // ---- joint-local rotations, then the chain walk of every body lane (wbc_rbd_pass's composition, per lane)
  if (is_joint) {
    double sg, cg;
    sincos(qg, &sg, &cg);
    double E[9];
    fused::joint_rotation(md.Rfix[body], md.axis[body], sg, cg, E);
    for (int i = 0; i < 9; ++i) w.T[sub][body - 1][i] = E[i];
  }
  lds_wave_sync();
  double R[9], o[3] = {pb[0], pb[1], pb[2]};
  fused::rot_zyx(sy, cy, sp, cp, sr, cr, R);
  if (is_joint) {
    const int depth = md.depth[body];
    for (int d = 0; d < depth; ++d) {
      const int j = md.path[body][d];
      fused::chain_step(R, o, md.pfix[j], w.T[sub][j - 1]);
    }
  }
  // ---- inertia of the lane's body about the base origin (eval_lane's composite form)
  if (is_body) {
    double cw[3], dv[3], Iw[6];
    fused::point_on_body(R, o, md.com[body], cw);
    for (int i = 0; i < 3; ++i) dv[i] = cw[i] - pb[i];
    fused::world_inertia(R, md.inertia[body], Iw);
    const double m = md.mass[body], dd = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];
    double* cm = w.comp[sub][body];
    cm[0] = m; cm[1] = m * dv[0]; cm[2] = m * dv[1]; cm[3] = m * dv[2];
    cm[4] = Iw[0] + m * (dd - dv[0] * dv[0]); cm[5] = Iw[1] - m * dv[0] * dv[1]; cm[6] = Iw[2] - m * dv[0] * dv[2];
    cm[7] = Iw[3] + m * (dd - dv[1] * dv[1]); cm[8] = Iw[4] - m * dv[1] * dv[2]; cm[9] = Iw[5] + m * (dd - dv[2] * dv[2]);
  }
  lds_wave_sync();
  // ---- composite of the subtree moved by this coordinate (the base coordinates move the whole robot), column g of A
  double s[10];
  for (int c = 0; c < 10; ++c) s[c] = 0.0;
  {
    const unsigned mask = g < G ? md.subtree[body] : 0u;
    for (int m = 0; m < NB; ++m) {
      const double sel = ((mask >> m) & 1u) ? 1.0 : 0.0;
      for (int c = 0; c < 10; ++c) s[c] += sel * w.comp[sub][m][c];
    }
  }
  const double Mc = s[0];
  const double invM = Mc > 0.0 ? 1.0 / Mc : 0.0;
  const double Dv[3] = {s[1] * invM, s[2] * invM, s[3] * invM};
  const double DD = Dv[0] * Dv[0] + Dv[1] * Dv[1] + Dv[2] * Dv[2];
  const double Cc[3] = {pb[0] + Dv[0], pb[1] + Dv[1], pb[2] + Dv[2]};
  const double Ic[6] = {s[4] - Mc * (DD - Dv[0] * Dv[0]), s[5] + Mc * Dv[0] * Dv[1], s[6] + Mc * Dv[0] * Dv[2],
                        s[7] - Mc * (DD - Dv[1] * Dv[1]), s[8] + Mc * Dv[1] * Dv[2], s[9] - Mc * (DD - Dv[2] * Dv[2])};
  const double Mtot = node_bcast<C, 5>(Mc);          // lane 5 (roll) sees the whole robot
  const double com[3] = {node_bcast<C, 5>(Cc[0]), node_bcast<C, 5>(Cc[1]), node_bcast<C, 5>(Cc[2])};
  double ah[3] = {0.0, 0.0, 0.0};
  if (g < 3) { ah[0] = g == 0 ? 1.0 : 0.0; ah[1] = g == 1 ? 1.0 : 0.0; ah[2] = g == 2 ? 1.0 : 0.0; }
  else if (g == 3) ah[2] = 1.0;
  else if (g == 4) { ah[0] = -sy; ah[1] = cy; }
  else if (g == 5) { ah[0] = cy * cp; ah[1] = sy * cp; ah[2] = -sp; }
  else if (g < G) fused::mat3_vec(R, md.axis[body], ah);
  double Ac[6];
  if (g < 3) {
    for (int i = 0; i < 3; ++i) { Ac[i] = ah[i] * Mtot; Ac[3 + i] = 0.0; }
  } else {
    const double rC[3] = {Cc[0] - o[0], Cc[1] - o[1], Cc[2] - o[2]};
    double vC[3], t[3], Iw[3];
    fused::cross3(ah, rC, vC);
    const double dC[3] = {Cc[0] - com[0], Cc[1] - com[1], Cc[2] - com[2]};
    fused::cross3(dC, vC, t);
    fused::sym3_vec(Ic, ah, Iw);
    for (int i = 0; i < 3; ++i) { Ac[i] = Mc * vC[i]; Ac[3 + i] = Iw[i] + Mc * t[i]; }
  }
  // ---- h = A v (a reduction over the robot's lanes), normalised by the robot mass; q; the yaw unwrap of BipedalController.cpp:400-403
  double hn[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) hn[i] = node_allreduce_add<LPN>(g < G ? Ac[i] * vg : 0.0) / md.robot_mass;
  lds_wave_sync();                                   // earlier readers of xo (none in this launch; the order of the phases stays explicit)
  if (g < 6) xo[g] = lane_pick6(hn, g);
  if (g < G) {
    double qo = qg;
    if (g == 3) {
      qo = yl + tick_normalize_angle(qg - yl);
      if (yaw_out) *yaw_out = qo;
    }
    xo[6 + g] = qo;
  }
  lds_wave_sync();
}

template <int NJ>
__device__ __forceinline__ void tick_observe_policy(const DeviceModel& md, TickLds<NJ>& w, const TickArgs& a) {
  using C = LinFastCfg<NJ>;
  constexpr int G = C::G, NX = C::NX, NU = C::NU, LPN = C::LPN, NPW = C::NPW;
  const int sub = threadIdx.x / LPN, g = threadIdx.x % LPN;
  const int bq = blockIdx.x * NPW + sub;
  const bool valid = bq < a.batch;
  const int b = valid ? bq : 0;            // lane groups beyond the batch compute robot 0 and write nothing (the DPP reductions need every lane)
  double* xo = w.xo[sub];
  if (a.rbd) {
    tick_observation<NJ>(md, w, a.rbd + (size_t)b * 2 * G, a.yaw_last[b], valid ? a.yaw_last + b : nullptr);
    if (valid) {
      for (int c = g; c < NX; c += LPN) {
        a.x_obs[(size_t)b * NX + c] = xo[c];
        if (a.x_loop) a.x_loop[(size_t)b * NX + c] = xo[c];
      }
      if (g == 0) {
        constexpr double kMaxTilt = M_PI / 3.0;       // SafetyChecker::checkOrientation: the limit itself passes
        a.safe[b] = (fabs(xo[10]) > kMaxTilt || fabs(xo[11]) > kMaxTilt) ? 0 : 1;
      }
    }
  } else {
    for (int c = g; c < NX; c += LPN) xo[c] = a.x_in[(size_t)b * NX + c];
    lds_wave_sync();
  }
  // ---- MRT_BASE::evaluatePolicy at t of the last solution (toPrimalSolution: the input and gain of a pre-event node and of the terminal node
  // repeat the one before; LinearController bias uff_j = u_j - K_j x_j)
  const int N = a.N, grid = a.p_grid[b], n = a.g_nodes[grid];
  const double* tp = a.g_time + (size_t)grid * (N + 1);
  const int* kp = a.g_kind + (size_t)grid * N;
  int j;
  double al;
  time_segment(tp, n + 1, a.t[b], &j, &al);
  auto effective = [&](int k) { while (k > 0 && (k == n || kp[k] == 1)) --k; return k; };
  const int e0 = effective(j), e1 = effective(j + 1);
  const double* x0 = a.x + ((size_t)b * (N + 1) + j) * NX;
  const double* x1 = x0 + NX;
  if (!valid) return;
  for (int c = g; c < NX; c += LPN) a.x_opt[(size_t)b * NX + c] = al * x0[c] + (1.0 - al) * x1[c];
  const double* u0 = a.u + ((size_t)b * N + e0) * NU;
  const double* u1 = a.u + ((size_t)b * N + e1) * NU;
  for (int r = g; r < NU; r += LPN) {
    double out;
    if (a.feedback) {
      const double* K0 = a.K + (((size_t)b * N + e0) * NU + r) * NX;
      const double* K1 = a.K + (((size_t)b * N + e1) * NU + r) * NX;
      double f0 = u0[r], f1 = u1[r];
      for (int c = 0; c < NX; ++c) { f0 -= K0[c] * x0[c]; f1 -= K1[c] * x1[c]; }
      double kx = 0.0;
      for (int c = 0; c < NX; ++c) kx += (al * K0[c] + (1.0 - al) * K1[c]) * xo[c];
      out = (al * f0 + (1.0 - al) * f1) + kx;
    } else {
      out = al * u0[r] + (1.0 - al) * u1[r];
    }
    a.u_opt[(size_t)b * NU + r] = out;
  }
  // ModeSchedule::modeAtTime from the mode of the interval time_segment selected: an event time belongs to the interval that ends there
  // (the earlier mode); before the first node / after the last one the mode of the first / last interval (a clamp to the solution's span)
  if (g == 0) a.mode[b] = a.g_mode[(size_t)grid * N + j];
}

// joint commands of BipedalController.cpp:237-252: posDes = x*[12:], velDes = u*[12:], torque = the joint-torque block of the WBC solution;
// with the robot's joint gains (the kp / kd of HybridJointHandle::setCommand, :250-254) the torque the hardware layer forms from that five-tuple
// (bipedal_gazebo/src/BipedalHWSim.cpp:174-175): kp (posDes - q) + kd (velDes - v) + tau, q / v the joint entries of the measured rbd
struct TickCommandArgs {
  int batch;
  const double *x_opt, *u_opt, *sol, *rbd;      // [batch][NX], [batch][NU], [batch][n], [batch][2 (6 + NJ)]
  const double *kp, *kd;                        // [batch][NJ]
  double *cmd, *joint_torque;                   // [batch][3][NJ], [batch][NJ]
};

template <int NJ>
__device__ __forceinline__ void tick_commands(const TickCommandArgs& a) {
  constexpr int NX = 12 + NJ, NU = 12 + NJ, NV = 6 + NJ, NSOL = 6 + NJ + 12 + NJ;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.batch * NJ) return;
  const int b = idx / NJ, j = idx % NJ;
  double* c = a.cmd + (size_t)b * 3 * NJ;
  const double pos = a.x_opt[(size_t)b * NX + 12 + j], vel = a.u_opt[(size_t)b * NU + 12 + j], tau = a.sol[(size_t)b * NSOL + NSOL - NJ + j];
  c[j] = pos;
  c[NJ + j] = vel;
  c[2 * NJ + j] = tau;
  const double* rb = a.rbd + (size_t)b * 2 * NV;
  a.joint_torque[idx] = a.kp[idx] * (pos - rb[6 + j]) + a.kd[idx] * (vel - rb[NV + 6 + j]) + tau;
}

// The observation of a restart (BipedalController::starting, :126-127: the observation is zeroed, then set from the estimator): for every robot
// with mask[b] != 0 x_obs[b] and yaw_last[b] from rbd[b], the yaw unwrapped against 0 (wrapped to (-pi, pi]); other robots are not written.
// The tick's mapping and device functions; a wavefront without a restarted robot leaves at once.
struct RestartArgs {
  int batch;
  const int* mask;                    // [batch] non-zero: restart
  const double* rbd;                  // [batch][2 (6 + NJ)]
  double *yaw_last, *x_obs;           // [batch], [batch][NX]
};

template <int NJ>
__device__ __forceinline__ void restart_observe(const DeviceModel& md, TickLds<NJ>& w, const RestartArgs& a) {
  using C = LinFastCfg<NJ>;
  constexpr int G = C::G, NX = C::NX, LPN = C::LPN, NPW = C::NPW;
  const int sub = threadIdx.x / LPN, g = threadIdx.x % LPN;
  const int bq = blockIdx.x * NPW + sub;
  const bool mine = bq < a.batch && a.mask[bq] != 0;
  if (__ballot(mine) == 0) return;       // one wavefront per workgroup: it leaves as a whole
  const int b = bq < a.batch ? bq : 0;   // the other lane groups compute a robot in range and write nothing (the DPP reductions need every lane)
  tick_observation<NJ>(md, w, a.rbd + (size_t)b * 2 * G, 0.0, mine ? a.yaw_last + b : nullptr);
  if (mine)
    for (int c = g; c < NX; c += LPN) a.x_obs[(size_t)b * NX + c] = w.xo[sub][c];
}

}  // namespace bpmpc
