// The masked per-robot row write of device_handle.h: the parameter rows of the WBC and the estimator, the joint gains of the controller.
#include "device_handle.h"

namespace bpmpc {

// One thread per entry of [batch][width]; the second pair is written when it has a destination.
__global__ __launch_bounds__(256) void k_write_rows(int batch, int width, int used, const int* mask, int n_rows, const double* src_a, double* dst_a,
                                                    const double* src_b, double* dst_b) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)batch * width) return;
  const int b = (int)(i / width), e = (int)(i % width);
  if (mask && !mask[b]) return;
  const size_t s = (size_t)(n_rows == 1 ? 0 : b) * width + e;
  dst_a[i] = e < used ? src_a[s] : 0.0;
  if (dst_b) dst_b[i] = e < used ? src_b[s] : 0.0;
}

void write_rows(hipStream_t stream, int batch, int width, int used, const int* mask, int n_rows, const RowPair& a, const RowPair& b) {
  hipLaunchKernelGGL(k_write_rows, dim3((unsigned)(((size_t)batch * width + 255) / 256)), dim3(256), 0, stream, batch, width, used, mask, n_rows, a.src, a.dst, b.src, b.dst);
  HIP_CHECK(hipGetLastError());
}

}  // namespace bpmpc
