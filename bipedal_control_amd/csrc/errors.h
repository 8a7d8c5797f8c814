// The exception classes of the C ABI's error model (translate, capi_internal.h, maps them to status codes).  No HIP header: the host-only
// units throw them too, and some of those are also compiled with a plain C++ compiler.
#pragma once
#include <stdexcept>

namespace bpmpc {

struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };   // a HIP call failed: BPMPC_ERR_DEVICE
// a setting or solver variant this engine does not implement (a task.info key, the DDP solver on an SQP-only path): BPMPC_ERR_UNSUPPORTED
struct Unsupported : std::runtime_error { using std::runtime_error::runtime_error; };

}  // namespace bpmpc
