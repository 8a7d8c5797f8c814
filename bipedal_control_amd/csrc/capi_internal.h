// The error model of the C ABI (include/bpmpc.h), shared by every unit of libbpmpc.so that has entry points: exceptions inside, a status code
// and bpmpc_last_error() outside.
#pragma once
#include <hip/hip_runtime.h>

#include <exception>
#include <string>
#include <type_traits>

#include "../../include/bpmpc.h"
#include "errors.h"
#include "robot_model.h"

namespace bpmpc {
void set_last_error(const std::string& message);
const RobotModel& model_of(const bpmpc_model* handle);

#define HIP_CHECK(expr)                                                                                     \
  do {                                                                                                      \
    hipError_t err_ = (expr);                                                                               \
    if (err_ != hipSuccess) throw DeviceError(std::string(#expr) + ": " + hipGetErrorString(err_));         \
  } while (0)

// Sets bpmpc_last_error() to e.what() and returns the status of e's class (errors.h; std::invalid_argument, std::length_error), `fallback` for
// any other exception: BPMPC_ERR_IO for the solver, WBC, gait batch and model entry points, BPMPC_ERR_DEVICE for the controller's.
int translate(const std::exception& e, int fallback);

// An entry point's body under the error model: what it returns (BPMPC_OK for a body without a result), or the status of what it throws.
template <typename F>
int guarded(int fallback, F&& body) {
  try {
    if constexpr (std::is_void_v<std::invoke_result_t<F&>>) { body(); return BPMPC_OK; }
    else return body();
  } catch (const std::exception& e) { return translate(e, fallback); }
}
}  // namespace bpmpc
