// The kinematic primitives of the side handles (WBC, controller tick, telemetry, estimator, plan geometry, plant), written once in
// kinematics_body.h and compiled in two flavours:
//   fused::   the compiler's default contraction - a * b + c may become one fused multiply-add
//   exact::   contract(off) - every product is rounded, as a host evaluation of the same text does (the plan geometry's host twin)
// Contraction follows the called function, not the body it is inlined into: the namespace at a call site is the choice (DESIGN.md section 4,
// "Kinematic primitives").  The kernels of the solve keep lane_model.h, which g++ compiles for tests/hostemu.
#pragma once
#include <hip/hip_runtime.h>

#define KIN_FN __host__ __device__ __forceinline__
namespace bpmpc {
namespace fused {
#define KIN_FP
#include "kinematics_body.h"
#undef KIN_FP
}  // namespace fused
namespace exact {
#define KIN_FP _Pragma("clang fp contract(off)")
#include "kinematics_body.h"
#undef KIN_FP
}  // namespace exact
}  // namespace bpmpc
#undef KIN_FN
