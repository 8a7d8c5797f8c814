// k_plant_sense: the plant's sensor model (include/bpmpc.h "Plant", sensors), what a switched handle launches behind its step kernel, and the two
// small kernels that seed it and forget its history.  A translation unit of its own: k_plant_step and k_plant_stick_step are compiled as they
// were before the plant had a sensor model.
//
// One wavefront per robot; lane g owns draw z[g] of kernels/sensor_noise.h and the measured entry that draw belongs to:
//   lanes 0..2     angular_vel_local (the walk draws z[3..5] come from lanes 3..5 by lane exchange; these lanes also walk and store the gyro bias)
//   lanes 6..8     linear_accel_local (walk draws z[9..11] from lanes 9..11; the accelerometer bias)
//   lanes 12..15   quat: every lane reads z[12..14] by lane exchange and forms quat (x) dq; lane 12 + c stores component c
//   lanes 16 + j   joint_pos[j], quantised          lanes 32 + j   joint_vel[j]          lanes 48 + i   contact[i], u[i] of block 32
// Every lane computes its Philox block (g >> 1) and block 32 in registers: no LDS, no scratch.  The lane that forms an entry stores it into the
// ring slot n mod 9 and reads the same entry of slot max(n - delay, 0) mod 9 back for the sensed block, so no lane waits for another.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "kernel_launchers.h"
#include "plant.h"

namespace bpmpc {

template <int NJ>
__global__ __launch_bounds__(kWave) void k_plant_sense(PlantSenseArgs a) {
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= a.batch) return;
  static_assert(32 + NJ <= 48 && 16 + NJ <= 32, "one lane per joint draw");
  constexpr int W = sensor_sample_width(NJ);
  const size_t B = (size_t)a.max_batch;
  const double* par = a.params + (size_t)b * kSensorParamStride;
  const unsigned k0 = a.key[2 * b], k1 = a.key[2 * b + 1];
  const unsigned long long t = a.ticks[2 * b], n = a.ticks[2 * b + 1];

  // 1. draws
  const double z = sensor_gaussian(t, (unsigned)b, k0, k1, l);
  const Philox4 ub = sensor_block(t, (unsigned)b, kSensorUniformBlock, k0, k1);
  const double z_walk = __shfl(z, (l + 3) & (kWave - 1));
  const double dx = __shfl(z, 12), dy = __shfl(z, 13), dz = __shfl(z, 14);

  // the truth's sections (kernels/plant.h PlantOut), this robot's rows
  auto truth = [&](int section, int width) { return a.truth + B * plant_out_offset(section, NJ) + (size_t)b * width; };
  auto sensed = [&](int section, int width) { return a.sensed + B * sensor_sensed_offset(section, NJ) + (size_t)b * width; };

  int e = -1;              // this lane's entry of the measured sample; -1: none
  double value = 0.0;
  double* dst = nullptr;   // where the entry goes in the sensed block (contacts: as an int, below)
  int* dst_contact = nullptr;
  if (l < 3 || (l >= 6 && l < 9)) {
    // 2. bias walk, 3. gyro = w + bg + gyro_noise z[0..2]; acc = a + ba + accel_noise z[6..8]
    const bool gyro = l < 3;
    const int i = gyro ? l : l - 6;
    double* bias = a.bias + (size_t)b * 6 + (gyro ? 0 : 3) + i;
    const double walked = *bias + par[gyro ? kSensGyroBiasWalk : kSensAccelBiasWalk] * a.sqrt_period * z_walk;
    *bias = walked;
    value = truth(gyro ? kPlantAngLocal : kPlantAccLocal, 3)[i] + walked + par[gyro ? kSensGyroNoise : kSensAccelNoise] * z;
    e = 2 * NJ + (gyro ? 4 : 7) + i;
    dst = sensed(gyro ? kSensedAngLocal : kSensedAccLocal, 3) + i;
  } else if (l >= 12 && l < 16) {
    const int c = l - 12;
    const double* q = truth(kPlantQuat, 4);
    const double sigma = par[kSensOrientationNoise];
    value = q[c];
    if (sigma > 0.0) {
      // quat (x) dq, dq = (delta sin(|delta| / 2) / |delta|, cos(|delta| / 2)), delta = sigma z[12..14]; x y z w
      const double ex = sigma * dx, ey = sigma * dy, ez = sigma * dz;
      const double nrm = sqrt(ex * ex + ey * ey + ez * ez);
      const double s = nrm > 0.0 ? sin(0.5 * nrm) / nrm : 0.5;
      const double bx = ex * s, by = ey * s, bz = ez * s, bw = cos(0.5 * nrm);
      const double ax = q[0], ay = q[1], az = q[2], aw = q[3];
      const double px = aw * bx + bw * ax + (ay * bz - az * by);
      const double py = aw * by + bw * ay + (az * bx - ax * bz);
      const double pz = aw * bz + bw * az + (ax * by - ay * bx);
      const double pw = aw * bw - (ax * bx + ay * by + az * bz);
      const double len = sqrt(px * px + py * py + pz * pz + pw * pw);
      value = (c == 0 ? px : c == 1 ? py : c == 2 ? pz : pw) / len;
    }
    e = 2 * NJ + c;
    dst = sensed(kSensedQuat, 4) + c;
  } else if (l >= 16 && l < 16 + NJ) {
    const int j = l - 16;
    value = truth(kPlantJointPos, NJ)[j] + par[kSensJointPosNoise] * z;
    const double res = par[kSensJointPosResolution];
    if (res > 0.0) value = rint(value / res) * res;
    e = j;
    dst = sensed(kSensedJointPos, NJ) + j;
  } else if (l >= 32 && l < 32 + NJ) {
    const int j = l - 32;
    value = truth(kPlantJointVel, NJ)[j] + par[kSensJointVelNoise] * z;
    e = NJ + j;
    dst = sensed(kSensedJointVel, NJ) + j;
  } else if (l >= 48 && l < 48 + kNumContacts) {
    const int i = l - 48;
    const unsigned word = i == 0 ? ub.w[0] : i == 1 ? ub.w[1] : i == 2 ? ub.w[2] : ub.w[3];
    const bool closed = reinterpret_cast<const int*>(truth(kPlantContact, 2))[i] != 0;
    value = closed && !(sensor_uniform(word) < par[kSensContactDropout]) ? 1.0 : 0.0;
    e = 2 * NJ + 10 + i;
    dst_contact = reinterpret_cast<int*>(sensed(kSensedContact, 2)) + i;
  }

  // 4. ring: the sample into slot n mod 9; the sensed output is the sample with index max(n - delay, 0)
  if (e >= 0) {
    const unsigned long long delay = (unsigned long long)sensor_delay_of(par[kSensDelaySteps]);
    const int slot_in = (int)(n % kSensorRing), slot_out = (int)((n > delay ? n - delay : 0ull) % kSensorRing);
    double* ring = a.ring + (size_t)b * kSensorRing * W;
    ring[slot_in * W + e] = value;
    const double out = slot_out == slot_in ? value : ring[slot_out * W + e];
    if (dst) *dst = out;
    else *dst_contact = out != 0.0 ? 1 : 0;
  }
  // 5. counters
  if (l == 0) { a.ticks[2 * b] = t + 1; a.ticks[2 * b + 1] = n + 1; }
}

// One thread per robot
__global__ __launch_bounds__(256) void k_plant_seed_sensors(int batch, const int* mask, unsigned k0, unsigned k1, const double* params, unsigned* key,
                                                            unsigned long long* ticks, double* bias) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch || (mask && !mask[b])) return;
  const double* par = params + (size_t)b * kSensorParamStride;
  key[2 * b] = k0; key[2 * b + 1] = k1;
  ticks[2 * b] = 0; ticks[2 * b + 1] = 0;
  for (int i = 0; i < 3; ++i) {
    bias[(size_t)b * 6 + i] = par[kSensGyroBiasInit] * sensor_gaussian(kSensorTurnOnTick, (unsigned)b, k0, k1, i);
    bias[(size_t)b * 6 + 3 + i] = par[kSensAccelBiasInit] * sensor_gaussian(kSensorTurnOnTick, (unsigned)b, k0, k1, 3 + i);
  }
}

__global__ __launch_bounds__(256) void k_plant_forget_samples(int batch, const int* mask, unsigned long long* ticks) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch || (mask && !mask[b])) return;
  ticks[2 * b + 1] = 0;
}

void launch_plant_sense(int nj, hipStream_t stream, const PlantSenseArgs& a) {
  KL_NJ(nj, hipLaunchKernelGGL(k_plant_sense<NJ>, dim3(a.batch), dim3(kWave), 0, stream, a));
  HIP_CHECK(hipGetLastError());
}

void launch_plant_seed_sensors(hipStream_t stream, int batch, const int* mask, long seed, const double* params, unsigned* key, unsigned long long* ticks, double* bias) {
  const unsigned long long s = (unsigned long long)seed;
  hipLaunchKernelGGL(k_plant_seed_sensors, dim3((batch + 255) / 256), dim3(256), 0, stream, batch, mask, (unsigned)s, (unsigned)(s >> 32), params, key, ticks, bias);
  HIP_CHECK(hipGetLastError());
}

void launch_plant_forget_samples(hipStream_t stream, int batch, const int* mask, unsigned long long* ticks) {
  hipLaunchKernelGGL(k_plant_forget_samples, dim3((batch + 255) / 256), dim3(256), 0, stream, batch, mask, ticks);
  HIP_CHECK(hipGetLastError());
}

}  // namespace bpmpc
