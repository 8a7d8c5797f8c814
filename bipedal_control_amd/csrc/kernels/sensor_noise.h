// The random numbers of the plant's sensor model (include/bpmpc.h "Plant", sensors): a counter-based generator and the table that says which of
// its words becomes which draw.  One text for the device (k_plant_sense, k_plant_seed_sensors in plant_sense.hip) and for the host
// (bpmpc_plant_sensor_draw in capi.cpp), so that what is tested without a device is what the kernels run.
//
// Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011).  One round maps the counter
// (c0, c1, c2, c3) under the key (k0, k1) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)) with M0 = 0xD2511F53,
// M1 = 0xCD9E8D57; between two rounds the key grows by the Weyl constants (0x9E3779B9, 0xBB67AE85); ten rounds.
//   counter = (tick low word, tick high word, robot index in the batch, block)      key = (seed low word, seed high word)
// Draw table of one (tick, robot, key):
//   uniform of a word w    (w + 0.5) 2^-32, in (0, 1), exact in a double
//   z[g], g = 0..63        Gaussian by Box-Muller from block g >> 1: words (0, 1) for even g, (2, 3) for odd g;
//                          z = sqrt(-2 ln u1) cos(2 pi u2), |z| <= sqrt(2 ln 2^33) = 6.76
//   u[i], i = 0..3         the uniforms of the four words of block 32
//   turn-on draw           the same table at the tick with all 64 bits set
// Who uses which draw (kernels in plant_sense.hip): z[0..2] gyro noise, z[3..5] gyro bias walk, z[6..8] accelerometer noise, z[9..11]
// accelerometer bias walk, z[12..14] orientation noise, z[16 + j] joint position noise, z[32 + j] joint velocity noise, u[i] dropout of contact
// i; of the turn-on draw z[0..2] the initial gyro bias and z[3..5] the initial accelerometer bias.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace bpmpc {

constexpr int kSensorParamStride = 16;      // BPMPC_PLANT_SENSOR_PARAM_STRIDE
constexpr int kSensorParamUsed = 12;
constexpr int kSensorRing = 9;              // measured samples kept per robot: delay_steps 0..8
constexpr int kSensorMaxDelay = kSensorRing - 1;
constexpr int kSensorGaussians = 64, kSensorUniforms = 4, kSensorUniformBlock = 32;
constexpr unsigned long long kSensorTurnOnTick = ~0ull;

// the entries of a parameter row
enum SensorParam { kSensGyroNoise, kSensGyroBiasWalk, kSensGyroBiasInit, kSensAccelNoise, kSensAccelBiasWalk, kSensAccelBiasInit, kSensOrientationNoise,
                   kSensJointPosNoise, kSensJointPosResolution, kSensJointVelNoise, kSensContactDropout, kSensDelaySteps };

struct Philox4 { unsigned w[4]; };

__host__ __device__ inline unsigned sensor_mulhi(unsigned a, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (unsigned)(((unsigned long long)a * b) >> 32);
#endif
}

__host__ __device__ inline Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = sensor_mulhi(M0, c0), lo0 = M0 * c0, hi1 = sensor_mulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// block `block` of (tick, robot, key)
__host__ __device__ inline Philox4 sensor_block(unsigned long long tick, unsigned robot, unsigned block, unsigned k0, unsigned k1) {
  return philox4x32_10((unsigned)tick, (unsigned)(tick >> 32), robot, block, k0, k1);
}

__host__ __device__ inline double sensor_uniform(unsigned w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

// z[g] from the block g >> 1
__host__ __device__ inline double sensor_gaussian_of(const Philox4& block, int g) {
  const bool odd = (g & 1) != 0;      // selects, not an index: the words stay in registers
  const double u1 = sensor_uniform(odd ? block.w[2] : block.w[0]), u2 = sensor_uniform(odd ? block.w[3] : block.w[1]);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

__host__ __device__ inline double sensor_gaussian(unsigned long long tick, unsigned robot, unsigned k0, unsigned k1, int g) {
  return sensor_gaussian_of(sensor_block(tick, robot, (unsigned)(g >> 1), k0, k1), g);
}

// a device row cannot be inspected: the kernels read its delay through this
__host__ __device__ inline int sensor_delay_of(double delay_steps) {
  return delay_steps >= (double)kSensorMaxDelay ? kSensorMaxDelay : (delay_steps >= 1.0 ? (int)delay_steps : 0);      // NaN: 0
}

}  // namespace bpmpc
