// Batched state estimation on the device (BipedalController::updateStateEstimation, bipedal_controllers/src/BipedalController.cpp:360-405): sensors
// of a batch of robots -> the measured rigid-body state the controller tick starts from.
//   StateEstimateBase::updateJointStates / updateImu / updateAngular / updateLinear   bipedal_estimation/src/StateEstimateBase.cpp:34-63
//   quatToZyx                                                                        bipedal_estimation/include/bipedal_estimation/StateEstimateBase.h:70-79
//   FromTopicStateEstimate::update                                                   bipedal_estimation/src/FromTopicEstimate.cpp:28-47
//   KalmanFilterEstimate                       declared in LinearKalmanFilter.h with its seven noise settings; src/LinearKalmanFilter.cpp is EMPTY in
//                                              the reference.  The filter below is the linear Kalman filter of the project that header cites
//                                              (qiayuanl/legged_control), recalled and unpinned; include/bpmpc.h "State estimation" is its specification.
//
// One wavefront per robot, one launch per update.  Mapping of the filter (n = 18 states, m = 28 observations):
//   front end      every lane forms zyx, R(zyx), the Euler rates and the world angular velocity (wave-uniform values); joint lanes write the joint
//                  slots of rbd and their joint-local rotations to LDS
//   predict        P- = A P A' + Q element by element over the wave; x- = A x + B a is column 18 of the same LDS tile
//   kinematics     lanes 0..3 walk the chain of their contact point (base at the origin): position and velocity -> y, and R's diagonal
//   S, C P-, r     C is never formed: row i of C x picks x[i % 3] - x[6 + i] (i < 12), x[3 + i % 3] (i < 24) or x[8 + 3 (i - 24)].  Lane l < 28 holds
//                  column l of S = C P- C' + R in registers, lane 28 + c column c of C P-, lane 46 the column C x- - y (the negative innovation)
//   solve          Gauss-Jordan without pivoting (S is symmetric positive definite) on those 47 register columns: at step k lane k publishes its
//                  column through LDS, every lane scales its entry of row k and eliminates the other 27 - fully unrolled, registers indexed statically
//   correct        lane 28 + c forms g = C' Z[:, c] (18 sums of at most five entries) and column c of P = P- - P- g; lane 46 the same for x
//   finish         P = (P + P') / 2, the xy reset, stores
// The arithmetic of one robot depends on nothing but that robot's data.
#pragma once
#include <hip/hip_runtime.h>

#include "../device_model.h"
#include "wbc.h"   // kinematics.h, lds_wave_sync, kWave

namespace bpmpc {

constexpr int kEstParamStride = 8;     // BPMPC_EST_PARAM_STRIDE
constexpr int kEstStates = 18, kEstObs = 28, kEstCols = kEstObs + kEstStates + 1;
constexpr double kEstGravity = 9.81;
constexpr double kEstXyResetDet = 1e-6;

// A parameter row: the settings of LinearKalmanFilter.h:45-51 in the order of their declaration
struct EstSettings {
  double foot_radius, imu_process_noise_position, imu_process_noise_velocity, foot_process_noise_position, foot_sensor_noise_position,
      foot_sensor_noise_velocity, foot_height_sensor_noise, reserved;
};
static_assert(sizeof(EstSettings) == kEstParamStride * sizeof(double), "EstSettings is a parameter row");

struct EstArgs {
  int batch, kind;                                  // kind: BPMPC_ESTIMATOR_FROM_TOPIC 0, BPMPC_ESTIMATOR_KALMAN 1
  double dt;
  const double *joint_pos, *joint_vel;              // [batch][NJ]
  const double *quat, *ang_local, *acc_local;       // [batch][4] x y z w, [batch][3], [batch][3] (nullable for kind 0)
  const int *contact, *mode;                        // [batch][4] or [batch]: exactly one (kind 1)
  const double* feet_heights;                       // [batch][4], nullable: 0
  const double *odom_pos, *odom_quat, *odom_lin, *odom_ang;   // kind 0
  const double* params;                             // [max_batch][kEstParamStride]
  double *x_hat, *cov;                              // [max_batch][18], [max_batch][18][18]: read and updated (kind 1)
  double* rbd;                                      // [max_batch][2 (6 + NJ)]
  int* xy_reset;                                    // [max_batch]
};

template <int NJ>
struct EstLds {
  double T[NJ][9];                          // joint-local rotations Rfix E(q)
  double P[kEstStates][kEstStates + 1];     // P (in), then the corrected P before it is symmetrised; column 18: x_hat
  double Pm[kEstStates][kEstStates + 1];    // P-, column 18: x-
  double col[2][kEstObs];                   // the pivot column of a Gauss-Jordan step (double buffered: one barrier per step)
  double y[kEstObs], Rd[kEstObs];
  double par[kEstParamStride];
  int flag[kNumContacts];
};

// StateEstimateBase.h:70-79, the clamp on one side only.  No contraction into fused multiply-adds: near the clamp the arguments of the two atan2
// are differences of products as small as cos(pitch), and a host evaluation of the header's expressions rounds every product
__device__ __forceinline__ void est_quat_to_zyx(const double* q, double* zyx) {
#pragma clang fp contract(off)
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double as = fmin(-2.0 * (x * z - w * y), .99999);
  zyx[0] = atan2(2.0 * (x * y + w * z), w * w + x * x - y * y - z * z);
  zyx[1] = asin(as);
  zyx[2] = atan2(2.0 * (y * z + w * x), w * w - x * x - y * y + z * z);
}

// the two state entries a row of C combines: (C x)[i] = x[est_c_first(i)] - (i < 12 ? x[6 + i] : 0)
__device__ __forceinline__ constexpr int est_c_first(int i) { return i < 12 ? i % 3 : (i < 24 ? 3 + i % 3 : 8 + 3 * (i - 24)); }

template <int NJ>
__device__ __forceinline__ void estimate_robot(const DeviceModel& md, EstLds<NJ>& w, const EstArgs& a, int b, int l) {
  constexpr int G = 6 + NJ, N = kEstStates, M = kEstObs;
  double* rbd = a.rbd + (size_t)b * 2 * G;
  const bool kalman = a.kind != 0;
  // ---- joints (updateJointStates), orientation and angular velocity (updateImu / FromTopicStateEstimate::update)
  double qj = 0.0, qdj = 0.0;
  if (l < NJ) {
    qj = a.joint_pos[(size_t)b * NJ + l];
    qdj = a.joint_vel[(size_t)b * NJ + l];
    rbd[6 + l] = qj;
    rbd[G + 6 + l] = qdj;
  }
  const double* qsrc = (kalman ? a.quat : a.odom_quat) + (size_t)b * 4;
  const double quat[4] = {qsrc[0], qsrc[1], qsrc[2], qsrc[3]};
  double zyx[3];
  est_quat_to_zyx(quat, zyx);
  double sz, cz, sy, cy, sx, cx;
  sincos(zyx[0], &sz, &cz);
  sincos(zyx[1], &sy, &cy);
  sincos(zyx[2], &sx, &cx);
  double rates[3] = {0.0, 0.0, 0.0}, wg[3];      // Euler rates (z, y, x), world angular velocity
  if (kalman) {
    const double* wl = a.ang_local + (size_t)b * 3;
    // getEulerAnglesZyxDerivativesFromLocalAngularVelocity, then getGlobalAngularVelocityFromEulerAnglesZyxDerivatives [OCS2-upstream, recalled]
    rates[0] = sx * wl[1] / cy + cx * wl[2] / cy;
    rates[1] = cx * wl[1] - sx * wl[2];
    rates[2] = wl[0] + sy * rates[0];
    wg[0] = -sz * rates[1] + cy * cz * rates[2];
    wg[1] = cz * rates[1] + cy * sz * rates[2];
    wg[2] = rates[0] - sy * rates[2];
  } else {
    for (int i = 0; i < 3; ++i) wg[i] = a.odom_ang[(size_t)b * 3 + i];
  }
  if (l < 3) {
    rbd[l] = l == 0 ? zyx[0] : (l == 1 ? zyx[1] : zyx[2]);
    rbd[G + l] = l == 0 ? wg[0] : (l == 1 ? wg[1] : wg[2]);
    if (!kalman) {
      rbd[3 + l] = a.odom_pos[(size_t)b * 3 + l];
      rbd[G + 3 + l] = a.odom_lin[(size_t)b * 3 + l];
    }
  }
  if (!kalman) return;

  // ---- the filter's state, this robot's settings and contact flags into LDS; the joint-local rotations
  const double dt = a.dt;
  double* xh = a.x_hat + (size_t)b * N;
  double* cov = a.cov + (size_t)b * N * N;
  for (int e = l; e < N * N; e += kWave) w.P[e / N][e % N] = cov[e];
  if (l < N) w.P[l][N] = xh[l];
  if (l < kEstParamStride) w.par[l] = a.params[(size_t)b * kEstParamStride + l];
  if (l < kNumContacts) {
    int f;
    if (a.contact) f = a.contact[(size_t)b * kNumContacts + l] != 0;
    else f = fused::stance_flag(a.mode[b], l);      // modeNumber2StanceLeg; a device value outside 0..3 counts as 0 (include/bpmpc.h)
    w.flag[l] = f;
  }
  if (l < NJ) {
    double sg, cg, E[9];
    sincos(qj, &sg, &cg);
    fused::joint_rotation(md.Rfix[l + 1], md.axis[l + 1], sg, cg, E);
    for (int i = 0; i < 9; ++i) w.T[l][i] = E[i];
    w.col[0][l] = qdj;                  // the joint rates, read by the contact lanes (col is free until the solve)
  }
  lds_wave_sync();

  double Rb[9];
  fused::rot_zyx(sz, cz, sy, cy, sx, cx, Rb);
  // ---- predict: P- = A P A' + Q, x- = A x + B accel
  for (int e = l; e < N * N; e += kWave) {
    const int r = e / N, c = e % N;
    double v = w.P[r][c];
    if (r < 3) v += dt * w.P[r + 3][c];
    if (c < 3) {
      double u = w.P[r][c + 3];
      if (r < 3) u += dt * w.P[r + 3][c + 3];
      v += dt * u;
    }
    if (r == c) {
      double qd;
      if (r < 3) qd = dt / 20.0 * w.par[1];
      else if (r < 6) qd = dt * kEstGravity / 20.0 * w.par[2];
      else qd = dt * w.par[3] * (w.flag[(r - 6) / 3] ? 1.0 : 100.0);
      v += qd;
    }
    w.Pm[r][c] = v;
  }
  if (l < N) {
    const double* al = a.acc_local + (size_t)b * 3;
    double acc[3];
    fused::mat3_vec(Rb, al, acc);
    acc[2] -= kEstGravity;
    double v = w.P[l][N];
    if (l < 3) {
      const double ac = l == 0 ? acc[0] : (l == 1 ? acc[1] : acc[2]);
      v += dt * w.P[l + 3][N] + 0.5 * dt * dt * ac;
    } else if (l < 6) {
      const double ac = l == 3 ? acc[0] : (l == 4 ? acc[1] : acc[2]);
      v += dt * ac;
    }
    w.Pm[l][N] = v;
  }
  // ---- kinematics of the contact points with the base at the origin (q = [0, zyx, joints], v = [0, Euler rates, joint rates]); y and R
  if (l < kNumContacts) {
    const int body = md.contact_body[l];
    const int depth = md.depth[body];
    double R[9], o[3] = {0.0, 0.0, 0.0}, om[3] = {wg[0], wg[1], wg[2]}, vo[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 9; ++i) R[i] = Rb[i];
    for (int d = 0; d < depth; ++d) {
      const int j = md.path[body][d];
      double t[3], t2[3], E[9], ah[3];
      fused::mat3_vec(R, md.pfix[j], t);      // the arm of this step, for the velocity of the joint's origin: om x (R pfix)
      fused::cross3(om, t, t2);
      for (int i = 0; i < 3; ++i) vo[i] += t2[i];
      for (int i = 0; i < 9; ++i) E[i] = w.T[j - 1][i];
      fused::chain_step(R, o, md.pfix[j], E);
      fused::mat3_vec(R, md.axis[j], ah);
      const double qd = w.col[0][j - 1];
      for (int i = 0; i < 3; ++i) om[i] += ah[i] * qd;
    }
    double t[3], t2[3], pt[3];
    fused::mat3_vec(R, md.contact_off[l], t);
    fused::cross3(om, t, t2);
    fused::point_on_body(R, o, md.contact_off[l], pt);
    const int f = w.flag[l];
    const double scale = f ? 1.0 : 100.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      w.y[3 * l + i] = -pt[i] + (i == 2 ? w.par[0] : 0.0);
      w.y[12 + 3 * l + i] = -(vo[i] + t2[i]);
      w.Rd[3 * l + i] = w.par[4];
      w.Rd[12 + 3 * l + i] = w.par[5] * scale;
    }
    w.y[24 + l] = a.feet_heights ? a.feet_heights[(size_t)b * kNumContacts + l] : 0.0;
    w.Rd[24 + l] = w.par[6] * scale;
  }
  lds_wave_sync();

  // ---- this lane's column of [S | C P- | C x- - y]
  const int c1 = l < M ? est_c_first(l) : (l < kEstCols ? l - M : 0);
  const int c2 = l < 12 ? 6 + l : -1;
  const bool is_rhs = l == kEstCols - 1;
  double W[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const int r1 = est_c_first(i);
    double v = w.Pm[r1][c1];
    if (i < 12) v -= w.Pm[6 + i][c1];
    if (c2 >= 0) {
      double u = w.Pm[r1][c2];
      if (i < 12) u -= w.Pm[6 + i][c2];
      v -= u;
    }
    if (is_rhs) v -= w.y[i];
    else if (l == i) v += w.Rd[i];
    W[i] = v;
  }
  // ---- Gauss-Jordan: after step k row k is scaled to a unit pivot and column k is eliminated from every other row
#pragma unroll
  for (int k = 0; k < M; ++k) {
    double* pc = w.col[k & 1];
    if (l == k) {
#pragma unroll
      for (int i = 0; i < M; ++i) pc[i] = W[i];
    }
    lds_wave_sync();
    const double t = W[k] * (1.0 / pc[k]);
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if (i == k) W[i] = t;
      else W[i] -= pc[i] * t;
    }
  }
  // ---- correct: lane 28 + c holds Z[:, c] = S^-1 (C P-)[:, c], lane 46 -S^-1 (y - C x-); g = C' Z; column = P-[:, c] - P- g
  if (l >= M && l < kEstCols) {
    double g[N];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      g[d] = W[d] + W[3 + d] + W[6 + d] + W[9 + d];
      g[3 + d] = W[12 + d] + W[15 + d] + W[18 + d] + W[21 + d];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) g[6 + i] = (i % 3 == 2 ? W[24 + i / 3] : 0.0) - W[i];
    const int c = l - M;
    for (int r = 0; r < N; ++r) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) s += w.Pm[r][j] * g[j];
      w.P[r][c] = w.Pm[r][c] - s;
    }
  }
  lds_wave_sync();
  // ---- P = (P + P') / 2, the xy reset, the outputs
  const double p00 = w.P[0][0], p11 = w.P[1][1], p01 = 0.5 * (w.P[0][1] + w.P[1][0]);
  const bool reset = p00 * p11 - p01 * p01 > kEstXyResetDet;
  for (int e = l; e < N * N; e += kWave) {
    const int r = e / N, c = e % N;
    double v = 0.5 * (w.P[r][c] + w.P[c][r]);
    if (reset) {
      if (r < 2 && c < 2) v = v / 10.0;
      else if (r < 2 || c < 2) v = 0.0;
    }
    cov[e] = v;
  }
  if (l < N) {
    const double v = w.P[l][N];
    xh[l] = v;
    if (l < 3) rbd[3 + l] = v;
    else if (l < 6) rbd[G + l] = v;
  }
  if (l == 0) a.xy_reset[b] = reset ? 1 : 0;
}

}  // namespace bpmpc
