// k_plant_input: the plant's input model (include/bpmpc.h "Plant", inputs; the rules are kernels/plant_input.h), what a switched handle launches
// in front of its step kernel, and the two small kernels that seed it and forget its history.  A translation unit of its own: k_plant_step,
// k_plant_stick_step and k_plant_sense are compiled as they were before the plant had an input model.
//
// One wavefront per robot:
//   lanes r NJ + j, r < 5   entry (row r, joint j) of the command, rows pos_des, vel_des, tau_ff, kp, kd: the lane reads it with the caller's
//                           stride, writes it (or, for a lost packet, the entry of slot n - 1) into ring slot n mod 16 and reads its own entry of
//                           slot max(n - k, 0) mod 16 back for the applied rows, so no lane waits for another
//   lanes 60..62            component x, y, z of the applied base force
//   lane 63                 delay_steps, lost, pushing and the counters
// Every lane computes the draws it needs in registers: no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "kernel_launchers.h"
#include "plant.h"

namespace bpmpc {

template <int NJ>
__global__ __launch_bounds__(kWave) void k_plant_input(PlantInputArgs a) {
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= a.batch) return;
  static_assert(kInputRows * NJ <= 60, "one lane per command entry below the force lanes");
  constexpr int W = kInputRows * NJ;      // doubles of one ring slot
  const double* par = a.params + (size_t)b * kInputParamStride;
  const unsigned k0 = a.key[2 * b], k1 = a.key[2 * b + 1];
  const unsigned long long t = a.ticks[2 * b], n = a.ticks[2 * b + 1];

  // 1. loss
  const bool lost = n > 0 && input_lost(input_loss_draw(t, (unsigned)b, k0, k1), par[kInDropout]);
  // 2. delay
  const int k = input_delay_steps(par[kInDelay], a.period_ns);

  if (l < W) {
    const int r = l / NJ, j = l - r * NJ;
    const double* src = r == 0 ? a.pos_des : r == 1 ? a.vel_des : r == 2 ? a.tau_ff : r == 3 ? a.kp : a.kd;
    const size_t stride = r < 3 ? (size_t)a.cmd_stride : (size_t)NJ;
    double* ring = a.ring + (size_t)b * kInputRing * W;
    const int slot_in = (int)(n % kInputRing), slot_out = (int)((n > (unsigned long long)k ? n - k : 0ull) % kInputRing);
    const double arrived = lost ? ring[(int)((n - 1) % kInputRing) * W + l] : src[(size_t)b * stride + j];
    ring[slot_in * W + l] = arrived;
    a.applied[((size_t)r * a.max_batch + b) * NJ + j] = slot_out == slot_in ? arrived : ring[slot_out * W + l];
  } else if (l >= 60) {
    // 3. push
    const InputPush push = input_push_windows(par[kInPushForce], par[kInPushInterval], par[kInPushDuration], a.period_ns);
    bool pushing = false;
    double u_s = 0.0, u_dir = 0.0;
    if (push.on) {
      input_push_draw(t / push.W, (unsigned)b, k0, k1, &u_s, &u_dir);
      const unsigned long long o = t % push.W, s = input_push_start(u_s, push.W, push.D);
      pushing = s <= o && o < s + push.D;
    }
    if (l < 63) {
      const int c = l - 60;
      const double f = a.base_force ? a.base_force[(size_t)b * 3 + c] : 0.0;
      a.force[(size_t)b * 3 + c] = pushing && c < 2 ? f + input_clamp(par[kInPushForce]) * input_push_direction(u_dir, c) : f;
    } else {
      // 4. what the step did, and the counters
      a.flags[b] = k; a.flags[a.max_batch + b] = lost ? 1 : 0; a.flags[2 * a.max_batch + b] = pushing ? 1 : 0;
      a.ticks[2 * b] = t + 1; a.ticks[2 * b + 1] = n + 1;
    }
  }
}

// One thread per robot
__global__ __launch_bounds__(256) void k_plant_seed_inputs(int batch, const int* mask, unsigned k0, unsigned k1, unsigned* key, unsigned long long* ticks) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch || (mask && !mask[b])) return;
  key[2 * b] = k0; key[2 * b + 1] = k1;
  ticks[2 * b] = 0; ticks[2 * b + 1] = 0;
}

__global__ __launch_bounds__(256) void k_plant_forget_commands(int batch, const int* mask, unsigned long long* ticks) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch || (mask && !mask[b])) return;
  ticks[2 * b + 1] = 0;
}

void launch_plant_input(int nj, hipStream_t stream, const PlantInputArgs& a) {
  KL_NJ(nj, hipLaunchKernelGGL(k_plant_input<NJ>, dim3(a.batch), dim3(kWave), 0, stream, a));
  HIP_CHECK(hipGetLastError());
}

void launch_plant_seed_inputs(hipStream_t stream, int batch, const int* mask, long seed, unsigned* key, unsigned long long* ticks) {
  const unsigned long long s = (unsigned long long)seed;
  hipLaunchKernelGGL(k_plant_seed_inputs, dim3((batch + 255) / 256), dim3(256), 0, stream, batch, mask, (unsigned)s, (unsigned)(s >> 32), key, ticks);
  HIP_CHECK(hipGetLastError());
}

void launch_plant_forget_commands(hipStream_t stream, int batch, const int* mask, unsigned long long* ticks) {
  hipLaunchKernelGGL(k_plant_forget_commands, dim3((batch + 255) / 256), dim3(256), 0, stream, batch, mask, ticks);
  HIP_CHECK(hipGetLastError());
}

}  // namespace bpmpc
