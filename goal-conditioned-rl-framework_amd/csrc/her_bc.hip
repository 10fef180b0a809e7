// her_bc.hip — Q-filtered behaviour cloning on the prior-data rows of a batch (bc_weight / q_filter).
//
// Prior-data replay (her_prior.hip) leaves Bd demonstration rows at rows [B - Bd, B) of every batch.  On an actor step of DDPG / TD3
// the actor loss gains  bc_weight * (1 / Bd) * sum_{b >= B - Bd} mask_b * sum_j (pi_bj - a_bj)^2  (Nair et al., ICRA 2018): mask_b = 1
// without the Q-filter, else Q0(s_b, a_b) > Q0(s_b, pi_b), strictly — a NaN on either side rejects the row.  The denominator is always
// Bd.  The engine's layer-per-launch actor step has everything the term needs once the critic's input-gradient chain has run:
//   bc_qfilter_kernel   ONE workgroup.  Demonstration row i = t, t + 256, ... of thread t: the mask from q_a / q_pi, the row's squared
//       distance over its A <= 16 action columns (pi from spa, a from sa, same columns of the step's batch slot), and for an ACCEPTED
//       row  dact[b][j] += (c * (pi - a)) * (1 - pi * pi),  c = fp32(2 * bc_weight / Bd) — the term's gradient w.r.t. the pre-tanh
//       action, on top of what the critic's last dX problem left there with its tanh derivative applied.  A rejected row is not
//       touched (adding 0.0 would turn a -0.0 into +0.0), nor are the columns from A on.  The two metric words: the accepted rows'
//       distances summed per thread in row order, then a xor-butterfly over the wave (offsets 32 .. 1), then the four waves' words from
//       LDS in wave order, times fp32(bc_weight / Bd); the accepted count, exact, over Bd.
// Every rounding is restated in numpy in tests/her_bc_ref.py, which is the definition (-ffp-contract=off: no product is fused).
//
// A translation unit of its own: every other unit's kernels keep their code, byte for byte.  No atomics, no waits between
// workgroups, no per-thread scratch; every address comes from the kernel arguments and the step's control record.
#include "her_bc.h"

namespace {

__global__ __launch_bounds__(gcrl::kBcThreads) void bc_qfilter_kernel(gcrl::BcArgs p) {
  __shared__ float w_sum[gcrl::kBcThreads / 64];
  __shared__ int w_cnt[gcrl::kBcThreads / 64];
  const gcrl::StepCtrl c = *p.cur;
  const long long x0 = (long long)c.batch_slot * p.slot_x + p.col0;
  const float* __restrict__ pi_rows = p.spa + x0;
  const float* __restrict__ a_rows = p.sa + x0;
  const int row0 = p.B - p.Bd;
  float acc = 0.f;
  int cnt = 0;
  for (int i = threadIdx.x; i < p.Bd; i += gcrl::kBcThreads) {
    const int b = row0 + i;
    const bool keep = p.q_a ? (p.q_a[b] > p.q_pi[b]) : true;
    if (p.mask) p.mask[b] = keep ? 1.f : 0.f;
    if (!keep) continue;
    const float* __restrict__ pr = pi_rows + (long long)b * p.ldx;
    const float* __restrict__ ar = a_rows + (long long)b * p.ldx;
    float* __restrict__ g = p.dact + (long long)b * p.ld_dact;
    float s = 0.f;
    for (int j = 0; j < p.A; ++j) {
      const float pi = pr[j];
      const float d = pi - ar[j];
      s = s + d * d;
      g[j] = g[j] + (p.c * d) * (1.f - pi * pi);
    }
    acc = acc + s;
    cnt += 1;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    acc = acc + __shfl_xor(acc, off, 64);
    cnt += __shfl_xor(cnt, off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { w_sum[wave] = acc; w_cnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = w_sum[0];
    int n = w_cnt[0];
    for (int w = 1; w < gcrl::kBcThreads / 64; ++w) { total = total + w_sum[w]; n += w_cnt[w]; }
    float* met = p.metrics + (long long)c.metrics_slot * gcrl::kMetricFloats;
    met[gcrl::MET_BC_LOSS] = p.w_bd * total;
    met[gcrl::MET_BC_PASS] = __fdiv_rn((float)n, (float)p.Bd);
  }
}

}  // namespace

namespace gcrl {

bool bc_args_ok(const BcArgs& a) {
  return a.cur && a.spa && a.sa && a.q_pi && a.dact && a.metrics && a.B >= 1 && a.B <= (1 << 24) && a.Bd >= 1 && a.Bd <= a.B && a.A >= 1 &&
         a.A <= 16 && a.col0 >= 0 && a.col0 + a.A <= a.ldx && a.ld_dact >= a.A && a.slot_x >= (long long)a.B * a.ldx;
}

int launch_bc_qfilter(hipStream_t st, const BcArgs& a) {
  GCRL_CHECK_ARG(bc_args_ok(a), "bc_qfilter: bc_weight: bad arguments (B=%d Bd=%d A=%d ldx=%d col0=%d ld_dact=%d)", a.B, a.Bd, a.A, a.ldx, a.col0,
                 a.ld_dact);
  hipLaunchKernelGGL(bc_qfilter_kernel, dim3(1), dim3(kBcThreads), 0, st, a);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl
