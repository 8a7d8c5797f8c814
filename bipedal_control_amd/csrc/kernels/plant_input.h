// The rules of the plant's input model (include/bpmpc.h "Plant", inputs): what happens to a joint command and a base force on their way to the
// step kernel - latency, packet loss, pushes.  One text for the device (k_plant_input in plant_input.hip) and for the host (bpmpc_plant_input_draw
// and the row validation in capi.cpp), so that what is tested without a device is what the kernel runs.
//
// Times are compared as integer nanoseconds, ns(x) = llrint(x 1e9), as ros::Time / ros::Duration compare them in the reference's
// BipedalHWSim::writeSim (bipedal_gazebo/src/BipedalHWSim.cpp:160-176).  That ros::Duration(double) rounds to the nearest nanosecond is recalled
// behaviour of roscpp, not read from a source on this project's side.  P = max(1, ns(period)) is the control step.
//   delay steps    k = min(15, ns(delay) / P): writeSim drops buffered commands from the back while stamp + delay < time and applies the back, i.e.
//                  the oldest command whose age is at most delay
//   push window    W = max(1, ns(push_interval) / P) steps, D = min(W, max(1, ns(push_duration) / P)) of them pushed; window w = t / W, offset
//                  o = t mod W; the push starts at offset s = min(W - D, floor(u_s (W - D + 1))) and holds while s <= o < s + D
// Clamps (a device row cannot be inspected): an entry that is not a number or is negative counts as 0, dropout above 1 as 1, a time of 2^62 ns or
// more as 2^62 ns, k is capped at 15.
// Draw table, on the generator and the uniform of kernels/sensor_noise.h with two blocks the sensor model does not use:
//   block 64 at counter t (the tick)           word 0: u_drop, the loss draw
//   block 65 at counter w (the push window)    word 0: u_s, where the push starts; word 1: u_dir, its direction 2 pi u_dir about the world z axis
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "sensor_noise.h"

namespace bpmpc {

constexpr int kInputParamStride = 8;        // BPMPC_PLANT_INPUT_PARAM_STRIDE
constexpr int kInputParamUsed = 5;
constexpr int kInputRing = 16;              // arrived commands kept per robot: delays of 0..15 steps
constexpr int kInputMaxDelay = kInputRing - 1;
constexpr int kInputRows = 5;               // pos_des, vel_des, tau_ff, kp, kd
constexpr unsigned kInputLossBlock = 64, kInputPushBlock = 65;
constexpr long long kInputMaxNs = 1ll << 62;

// the entries of a parameter row
enum InputParam { kInDelay, kInDropout, kInPushForce, kInPushInterval, kInPushDuration };

// not a number, or negative: 0
__host__ __device__ inline double input_clamp(double x) { return x > 0.0 ? x : 0.0; }

// integer nanoseconds of a clamped time
__host__ __device__ inline long long input_ns(double seconds) {
  const double v = input_clamp(seconds) * 1e9;
  return v >= (double)kInputMaxNs ? kInputMaxNs : llrint(v);
}

// the control step in nanoseconds
__host__ __device__ inline long long input_period_ns(double period) {
  const long long p = input_ns(period);
  return p > 1 ? p : 1;
}

// k: control steps between a command and its torque
__host__ __device__ inline int input_delay_steps(double delay, long long P) {
  const long long k = input_ns(delay) / P;
  return k > kInputMaxDelay ? kInputMaxDelay : (int)k;
}

// u_drop < dropout, with dropout clamped to 0..1
__host__ __device__ inline bool input_lost(double u_drop, double dropout) {
  const double p = input_clamp(dropout);
  return u_drop < (p > 1.0 ? 1.0 : p);
}

struct InputPush { bool on; unsigned long long W, D; };

// the push schedule of a row: off unless push_force > 0 and ns(push_interval) > 0
__host__ __device__ inline InputPush input_push_windows(double push_force, double push_interval, double push_duration, long long P) {
  const long long interval = input_ns(push_interval);
  if (!(input_clamp(push_force) > 0.0) || interval <= 0) return InputPush{false, 1ull, 1ull};
  const long long W = interval / P > 1 ? interval / P : 1;
  const long long d = input_ns(push_duration) / P > 1 ? input_ns(push_duration) / P : 1;
  return InputPush{true, (unsigned long long)W, (unsigned long long)(d < W ? d : W)};
}

// s: the offset at which the push of a window starts
__host__ __device__ inline unsigned long long input_push_start(double u_s, unsigned long long W, unsigned long long D) {
  const unsigned long long s = (unsigned long long)floor(u_s * (double)(W - D + 1));
  return s > W - D ? W - D : s;
}

// the draws: u_drop of block 64 at the tick; u_s, u_dir of block 65 at the push window
__host__ __device__ inline double input_loss_draw(unsigned long long t, unsigned robot, unsigned k0, unsigned k1) {
  return sensor_uniform(sensor_block(t, robot, kInputLossBlock, k0, k1).w[0]);
}
__host__ __device__ inline void input_push_draw(unsigned long long w, unsigned robot, unsigned k0, unsigned k1, double* u_s, double* u_dir) {
  const Philox4 block = sensor_block(w, robot, kInputPushBlock, k0, k1);
  *u_s = sensor_uniform(block.w[0]);
  *u_dir = sensor_uniform(block.w[1]);
}

// component c (0: x, 1: y) of the unit push direction
__host__ __device__ inline double input_push_direction(double u_dir, int c) {
  const double angle = 6.283185307179586 * u_dir;
  return c == 0 ? cos(angle) : sin(angle);
}

}  // namespace bpmpc
