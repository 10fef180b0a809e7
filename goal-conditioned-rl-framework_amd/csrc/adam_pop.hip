// adam_pop.hip — population forms of the optimiser launches (agent.hip gcrl_pop_*): adam_pop_kernel and adam_pair_pop_kernel run
// the same device functions and kernel bodies as ops.hip's adam_kernel and adam_pair_kernel, each member on its own arguments.  (A
// translation unit of their own: beside them in ops.hip the per-net step was no longer inlined into the single-agent kernels.)
#include "adam_math.h"
#include "ops.h"
#include "pop.h"

namespace gcrl {
namespace {

#include "adam_device.inc"

// member blockIdx.z runs its own arguments tab[blockIdx.z] on the workgroups (blockIdx.x, blockIdx.y) of its single-agent launch (the
// members' grids are equal, so each member's rider workgroup is the last blockIdx.x, as in adam_kernel)
__global__ __launch_bounds__(256) void adam_pop_kernel(const AdamArgs* __restrict__ tab) {
  const AdamArgs& a = tab[blockIdx.z];
#include "adam_kernel_body.inc"
}

// member blockIdx.z runs its own pair tab[blockIdx.z]
__global__ __launch_bounds__(256) void adam_pair_pop_kernel(const AdamPairArgs* __restrict__ tab) {
  const AdamArgs& a0 = tab[blockIdx.z].a0;
  const AdamArgs& a1 = tab[blockIdx.z].a1;
#include "adam_pair_body.inc"
}

}  // namespace

int launch_adam_pop(hipStream_t st, const void* tab, int members, dim3 grid) {
  GCRL_CHECK_ARG(members >= 1 && members <= 65535 && grid.y >= 1 && grid.y <= kMaxCritics && grid.z == 1, "adam population: bad launch");
  hipLaunchKernelGGL(adam_pop_kernel, dim3(grid.x, grid.y, (unsigned)members), dim3(256), 0, st, static_cast<const AdamArgs*>(tab));
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int launch_adam_pair_pop(hipStream_t st, const void* tab, int members, dim3 grid) {
  GCRL_CHECK_ARG(members >= 1 && members <= 65535 && grid.y == 2 && grid.z == 1, "adam_pair population: bad launch");
  hipLaunchKernelGGL(adam_pair_pop_kernel, dim3(grid.x, 2, (unsigned)members), dim3(256), 0, st, static_cast<const AdamPairArgs*>(tab));
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl
