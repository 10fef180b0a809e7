// pop_clone.hip — the device copy of gcrl_pop_clone (agent_pop.inc): every state allocation of every (source, destination) pair of a
// call, and with GCRL_CLONE_RING the pairs' replay rings, in ONE launch.  The host fills a device table of {src, dst, bytes} segments
// (pbt_host.h); workgroup (x, y) copies chunk x of segment y.  No waits between workgroups, no atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "common.h"
#include "pbt_host.h"
#include "pop.h"

namespace gcrl {
namespace {

constexpr int kCloneThreads = 256;

// 16-byte loads and stores in a grid-stride loop over the segment; what does not fill 16 bytes (and a segment whose addresses are not
// 16-byte aligned: never the engine's own allocations) goes byte by byte
__global__ __launch_bounds__(kCloneThreads) void pop_clone_kernel(const CloneSeg* __restrict__ tab) {
  const CloneSeg s = tab[blockIdx.y];
  const unsigned long long bytes = s.bytes;
  const bool aligned = ((reinterpret_cast<unsigned long long>(s.src) | reinterpret_cast<unsigned long long>(s.dst)) & 15ull) == 0;
  const unsigned long long n16 = aligned ? bytes >> 4 : 0;
  const unsigned long long stride = (unsigned long long)gridDim.x * kCloneThreads;
  const unsigned long long t = (unsigned long long)blockIdx.x * kCloneThreads + threadIdx.x;
  const uint4* __restrict__ src = static_cast<const uint4*>(s.src);
  uint4* __restrict__ dst = static_cast<uint4*>(s.dst);
  for (unsigned long long i = t; i < n16; i += stride) dst[i] = src[i];
  const unsigned char* __restrict__ sb = static_cast<const unsigned char*>(s.src);
  unsigned char* __restrict__ db = static_cast<unsigned char*>(s.dst);
  for (unsigned long long i = (n16 << 4) + t; i < bytes; i += stride) db[i] = sb[i];
}

}  // namespace

int launch_pop_clone(hipStream_t st, const void* tab, int segments, unsigned chunks) {
  if (segments < 1) return GCRL_OK;
  hipLaunchKernelGGL(pop_clone_kernel, dim3(chunks, (unsigned)segments), dim3(kCloneThreads), 0, st, static_cast<const CloneSeg*>(tab));
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl
