// Small transfers between the host and the device buffers of a solver handle in ONE copy (solver.h: CopyTable, upload_batch, Downloads).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "solver.h"

namespace {

__global__ __launch_bounds__(256) void k_copy_table(CopyTable t) {
  const int e = blockIdx.y;
  const unsigned* src = static_cast<const unsigned*>(t.src[e]);
  unsigned* dst = static_cast<unsigned*>(t.dst[e]);
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < t.words[e]; i += gridDim.x * 256) dst[i] = src[i];
}

// one piece host -> device through the pinned arena (pin_up.reset() by the caller, once nothing of the previous call is in flight)
void upload_pinned(bpmpc_solver* s, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return;
  void* stage = s->pin_up.take(bytes);
  if (stage) std::memcpy(stage, src, bytes);
  HIP_CHECK(hipMemcpyAsync(dst, stage ? stage : src, bytes, hipMemcpyHostToDevice, s->stream));
}
inline size_t piece_span(size_t bytes) { return (bytes + 15) & ~size_t(15); }

}  // namespace

namespace bpmpc {

void launch_copy_table(bpmpc_solver* s, const CopyTable& t) {
  if (t.n == 0) return;
  unsigned most = 0;
  for (int i = 0; i < t.n; ++i) most = std::max(most, t.words[i]);
  hipLaunchKernelGGL(k_copy_table, dim3(std::min(64u, (most + 255) / 256), t.n), dim3(256), 0, s->stream, t);
  HIP_CHECK(hipGetLastError());
}
void upload_batch(bpmpc_solver* s, const TransferPiece* pc, int n) {
  size_t total = 0;
  int live = 0;
  bool words = true;
  for (int i = 0; i < n; ++i) if (pc[i].bytes) { total += piece_span(pc[i].bytes); ++live; words = words && pc[i].bytes % 4 == 0; }
  char* pin = (words && live >= 2 && live <= CopyTable::kMax && total <= s->xfer_cap) ? static_cast<char*>(s->pin_up.take(total)) : nullptr;
  if (!pin) {                                             // no room in the arena (its first cycle): piece by piece
    for (int i = 0; i < n; ++i) upload_pinned(s, pc[i].device, pc[i].host_src, pc[i].bytes);
    return;
  }
  CopyTable t{};
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    if (!pc[i].bytes) continue;
    std::memcpy(pin + off, pc[i].host_src, pc[i].bytes);
    t.dst[t.n] = pc[i].device; t.src[t.n] = s->xfer + off; t.words[t.n] = (unsigned)(pc[i].bytes / 4); ++t.n;
    off += piece_span(pc[i].bytes);
  }
  HIP_CHECK(hipMemcpyAsync(s->xfer, pin, off, hipMemcpyHostToDevice, s->stream));
  launch_copy_table(s, t);
}
void Downloads::enqueue(bpmpc_solver* s) {
  s->pin_down.reset();
  size_t total = 0;
  int live = 0;
  for (const Item& it : items) if (it.pc.bytes <= kPackLimit && it.pc.bytes % 4 == 0) { total += piece_span(it.pc.bytes); ++live; }
  char* pin = (live >= 2 && live <= CopyTable::kMax && total <= s->xfer_cap) ? static_cast<char*>(s->pin_down.take(total)) : nullptr;
  if (pin) {
    CopyTable t{};
    size_t off = 0;
    for (Item& it : items) {
      if (!(it.pc.bytes <= kPackLimit && it.pc.bytes % 4 == 0)) continue;
      t.dst[t.n] = s->xfer + off; t.src[t.n] = it.pc.device; t.words[t.n] = (unsigned)(it.pc.bytes / 4); ++t.n;
      it.pin = pin + off;
      off += piece_span(it.pc.bytes);
    }
    launch_copy_table(s, t);
    HIP_CHECK(hipMemcpyAsync(pin, s->xfer, off, hipMemcpyDeviceToHost, s->stream));
  }
  for (Item& it : items) {
    if (it.pin) continue;
    void* own = it.pc.bytes <= (size_t(4) << 20) ? s->pin_down.take(it.pc.bytes) : nullptr;      // small results land in pinned memory, large ones in the caller's arrays
    HIP_CHECK(hipMemcpyAsync(own ? own : it.pc.host_dst, it.pc.device, it.pc.bytes, hipMemcpyDeviceToHost, s->stream));
    it.pin = own;
  }
}

}  // namespace bpmpc
