// rowchain.hip — the DDPG critic phase (K) and actor phase (P) as row-block chains: one launch
// walks each block of 4/8/16 batch rows through every forward and input-gradient pass of the
// phase (rowchain.h), leaving only the batch-contracting dW GEMMs and the optimiser to follow.
//
//   K (src/agent.py:1311-1317, critic_update):  target actor -> target critic -> TD target y;
//       online critic on [s|a] (activations saved) -> q; dq = 2(q-y)/B; critic input-gradient
//       chain, every layer's pre-activation gradient saved for dW.
//   P (src/agent.py:1288-1300, actor_update):  actor on s (saved) -> a = tanh(.); critic on
//       [s|a] -> q2 (= -loss*B); critic input-gradient chain down to the action columns;
//       d(pre-tanh) = da*(1-a^2); actor gradient chain, saved for dW.
#include "rowchain.h"
#include "norm_math.h"
#include "meet.h"
#include "sac_select.h"
#include "pop.h"

#include <algorithm>
#include <array>
#include <cstdlib>
#include <map>
#include <mutex>
#include <type_traits>

namespace gcrl {
namespace {

template <int RG>
__device__ inline void load_rows(float* X, int ldl, const float* src, long long ld_src, int ncols, int jpad, int rv) {
  constexpr int R = 4 * RG;
  for (int i = threadIdx.x; i < R * jpad; i += kRowThreads) {
    const int r = i / jpad, c = i - r * jpad;
    X[r * ldl + c] = (r < rv && c < ncols) ? src[(long long)r * ld_src + c] : 0.f;
  }
}

// hidden layers 0..L-1 of `net` on the rows in X0 (jpad0 columns, zero padded); returns the LDS
// buffer holding the last hidden activation.  save: [L][B][H] global, row r0 of the block.
template <int RG>
__device__ inline float* mlp_hidden(const RowNet& net, const float* X0, float* X1, float* X2, int ldl, float* part,
                                    float* save, long long BH, long long row0, int rv, float* last_out = nullptr) {
  const float* in = X0;
  float* out = X1;
  const bool chained = RG == 1 && net.H <= kRowChunk;   // one barrier per layer (rows_linear); measured slower at 8 rows
  for (int l = 0; l < net.L; ++l) {
    if (last_out && l == net.L - 1) out = last_out;   // e.g. kept aside while the ping-pong buffers are reused
    rows_linear<RG>(in, ldl, l == 0 ? net.jpad0 : net.H, net.Wt + net.wt[l], net.H, net.H, net.P + net.b[l], EPI_LEAKY,
                    part, out, ldl, save ? save + l * BH + row0 * net.H : nullptr, net.H, rv, nullptr, 0, MUL_NONE,
                    chained, l & 1);
    in = out;
    out = (out == X1) ? X2 : X1;
  }
  if (chained) __syncthreads();   // the callers read the result across waves
  return (float*)in;
}

// G <- (upstream[r][o] . Whead[o][k]) * act'(h[r][k]) in place over h (LDS), n_up <= 16 head outputs.
// A thread owns four consecutive k (16-byte LDS accesses; H % 4 == 0): one pass for 4 rows x 256 columns (round 4: the
// element-per-thread loop was four dependent rounds of LDS reads, 0.8-1.9 us per call by the kernel's own clock stamps).
// q_out (optional, n_up == 1): ALSO the head's forward value q[r] = sum_k h[r][k] * Whead[k] + q_bias -> q_out[r * 16], formed
// from the same reads — for callers whose upstream gradient does not depend on it (DDPG's actor phase: d(-mean Q)/dq = -1/B),
// which saves the separate head pass.  Needs the H / 4 threads of a row inside one wavefront (H = 64, 128, 256).
template <int RG>
__device__ inline void head_backward(float* h, int ldl, int H, const float* Wh, int n_up, const float* up /* LDS [R][16] */,
                                     float* save, int rv, float* q_out = nullptr, float q_bias = 0.f) {
  constexpr int R = 4 * RG;
  const int H4 = H >> 2;
  for (int i = threadIdx.x; i < R * H4; i += kRowThreads) {
    const int r = i / H4, k = (i - r * H4) << 2;
    const v4f hv = *(const v4f*)(h + r * ldl + k);
    v4f s = (v4f){0.f, 0.f, 0.f, 0.f};
    for (int o = 0; o < n_up; ++o) s += up[r * 16 + o] * *(const v4f*)(Wh + (long long)o * H + k);
    v4f g;
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = s[q] * act_deriv(hv[q], MUL_DLEAKY);
    if (q_out) {   // (uniform) the rows of a wave: 64 / H4 of them, H4 lanes each
      const v4f w = *(const v4f*)(Wh + k);
      float qs = ((hv[0] * w[0] + hv[1] * w[1]) + hv[2] * w[2]) + hv[3] * w[3];
      for (int off = H4 >> 1; off > 0; off >>= 1) qs += __shfl_xor(qs, off, 64);
      if ((i - r * H4) == 0) q_out[r * 16] = qs + q_bias;
    }
    *(v4f*)(h + r * ldl + k) = g;
    if (save && r < rv) *(v4f*)(save + (long long)r * H + k) = g;
  }
}
__device__ inline bool head_fusable(int H) { return H == 64 || H == 128 || H == 256; }

// pre-activation gradients of hidden layers L-2..0 from the one of layer L-1 (in G, LDS)
template <int RG>
__device__ inline float* grad_chain(const RowNet& net, float* G, float* X1, float* X2, int ldl, float* part,
                                    const float* hsaved, float* gsave, long long BH, long long row0, int rv) {
  float* in = G;
  const bool chained = RG == 1 && net.H <= kRowChunk;
  for (int l = net.L - 1; l >= 1; --l) {
    float* out = (in == X1) ? X2 : X1;
    rows_linear<RG>(in, ldl, net.H, net.P + net.w[l], net.H, net.H, nullptr, EPI_NONE, part, out, ldl,
                    gsave ? gsave + (l - 1) * BH + row0 * net.H : nullptr, net.H, rv,
                    hsaved + (l - 1) * BH + row0 * net.H, net.H, MUL_DLEAKY, chained, l & 1);
    in = out;
  }
  if (chained) __syncthreads();
  return in;
}

// LDS-multiplier form (rowchain.h rowchain_lds_bytes_mul) of the two walks above, for a net whose backward chain runs in the same workgroup:
// layer l < L-1 leaves its output in rows of its own, keep + l * R * ldl, layer L-1 in `last`, and the chain multiplies by act' of the kept
// rows instead of loading the global save back.  Same passes, same operands, same order: act_deriv sees the fp32 value the save holds.
// Chained passes need no barrier for it: in both directions N = H, so a wave's (row, column) items of the epilogue are the same
// (rows_linear: cb, q4) and it reads back as multiplier exactly what it wrote as output; the unchained form ends every pass with a barrier.
// Rows >= rv hold finite values (biases walked through zero inputs) that nothing reads: rows_linear takes a multiplier for valid rows only.
template <int RG>
__device__ inline float* mlp_hidden_keep(const RowNet& net, const float* X0, float* keep, float* last, int ldl, float* part,
                                         float* save, long long BH, long long row0, int rv) {
  constexpr int R = 4 * RG;
  const float* in = X0;
  const bool chained = RG == 1 && net.H <= kRowChunk;
  for (int l = 0; l < net.L; ++l) {
    float* out = l == net.L - 1 ? last : keep + l * R * ldl;
    rows_linear<RG>(in, ldl, l == 0 ? net.jpad0 : net.H, net.Wt + net.wt[l], net.H, net.H, net.P + net.b[l], EPI_LEAKY,
                    part, out, ldl, save ? save + l * BH + row0 * net.H : nullptr, net.H, rv, nullptr, 0, MUL_NONE,
                    chained, l & 1);
    in = out;
  }
  if (chained) __syncthreads();
  return last;
}
template <int RG>
__device__ inline float* grad_chain_keep(const RowNet& net, float* G, float* X1, float* X2, int ldl, float* part,
                                         const float* keep, float* gsave, long long BH, long long row0, int rv) {
  constexpr int R = 4 * RG;
  float* in = G;
  const bool chained = RG == 1 && net.H <= kRowChunk;
  for (int l = net.L - 1; l >= 1; --l) {
    float* out = (in == X1) ? X2 : X1;
    rows_linear<RG>(in, ldl, net.H, net.P + net.w[l], net.H, net.H, nullptr, EPI_NONE, part, out, ldl,
                    gsave ? gsave + (l - 1) * BH + row0 * net.H : nullptr, net.H, rv,
                    keep + (l - 1) * R * ldl, ldl, MUL_DLEAKY, chained, l & 1);
    in = out;
  }
  if (chained) __syncthreads();
  return in;
}

// Stream form (rowchain.h WStream) of the four walks above, 4 rows per workgroup and H <= kRowChunk (always chained): every pass requests
// the first stage of the next layer's matrix, the walk's last pass the caller's `nx` (TAIL, HASB_N: its kind, whether it has a bias).
// KEEP: the LDS-multiplier form's buffers (A1 = keep rows, `last` = the last layer's rows); else the ping-pong pair A1 / A2, the last
// layer into `last` when given.  KS: H / 4 at a dispatched H (the caller's branch: no join of branches while the stream is live), 0: any H.
// The walk's first pass is always requested by somebody before it.  A walk needs L >= 2 (the launcher's rule).
template <int KS, bool KEEP, int TAIL, bool HASB_N>
__device__ __forceinline__ float* mlp_hidden_st(WStream<8>& ws, const RowNet& net, const float* X0, float* A1, float* A2, float* last, int ldl,
                                                float* part, float* save, long long BH, long long row0, int rv, const WNext& nx) {
  constexpr int R = 4;
  const int H = net.H, L = net.L;
  auto out_of = [&](int l) -> float* {
    if (KEEP) return l == L - 1 ? last : A1 + l * R * ldl;
    return (last && l == L - 1) ? last : ((l & 1) ? A2 : A1);
  };
  auto next_of = [&](int l) { return WNext{net.Wt + net.wt[l + 1], H, H, H, net.P + net.b[l + 1]}; };
  auto save_of = [&](int l) -> float* { return save ? save + l * BH + row0 * H : nullptr; };
  rows_linear_stream<KS, true, TAIL_FULL, true, true>(ws, X0, ldl, net.jpad0, net.Wt + net.wt[0], H, H, net.P + net.b[0], EPI_LEAKY, part, out_of(0), ldl,
                                            save_of(0), H, rv, nullptr, 0, MUL_NONE, 0, next_of(0));
  for (int l = 1; l < L - 1; ++l)
    rows_linear_stream<KS, false, TAIL_FULL, true, true>(ws, out_of(l - 1), ldl, H, net.Wt + net.wt[l], H, H, net.P + net.b[l], EPI_LEAKY, part, out_of(l), ldl,
                                              save_of(l), H, rv, nullptr, 0, MUL_NONE, l & 1, next_of(l));
  rows_linear_stream<KS, false, TAIL, true, HASB_N>(ws, out_of(L - 2), ldl, H, net.Wt + net.wt[L - 1], H, H, net.P + net.b[L - 1], EPI_LEAKY, part, out_of(L - 1), ldl,
                                         save_of(L - 1), H, rv, nullptr, 0, MUL_NONE, (L - 1) & 1, nx);
  __syncthreads();   // the callers read the result across waves
  return out_of(L - 1);
}
// mulbase: KEEP: the kept rows (LDS); else the global saves [L][B][H].  The walk's first pass is always requested by the caller's side
// (the forward walk's last pass, or the head section's predecessor).
template <int KS, bool KEEP, int TAIL, bool HASB_N>
__device__ __forceinline__ float* grad_chain_st(WStream<8>& ws, const RowNet& net, float* G, float* X1, float* X2, int ldl, float* part,
                                                const float* mulbase, float* gsave, long long BH, long long row0, int rv, const WNext& nx) {
  constexpr int R = 4;
  const int H = net.H;
  float* in = G;
  auto mul_of = [&](int l) -> const float* { return KEEP ? mulbase + (l - 1) * R * ldl : mulbase + (l - 1) * BH + row0 * H; };
  auto save_of = [&](int l) -> float* { return gsave ? gsave + (l - 1) * BH + row0 * H : nullptr; };
  const long long ld_mul = KEEP ? ldl : H;
  for (int l = net.L - 1; l >= 2; --l) {
    float* out = (in == X1) ? X2 : X1;
    rows_linear_stream<KS, false, TAIL_FULL, false, false>(ws, in, ldl, H, net.P + net.w[l], H, H, nullptr, EPI_NONE, part, out, ldl, save_of(l), H, rv,
                                                mul_of(l), ld_mul, MUL_DLEAKY, l & 1, WNext{net.P + net.w[l - 1], H, H, H, nullptr});
    in = out;
  }
  float* out = (in == X1) ? X2 : X1;
  rows_linear_stream<KS, false, TAIL, false, HASB_N>(ws, in, ldl, H, net.P + net.w[1], H, H, nullptr, EPI_NONE, part, out, ldl, save_of(1), H, rv,
                                          mul_of(1), ld_mul, MUL_DLEAKY, 1, nx);
  __syncthreads();
  return out;
}

// stage `n` floats of global memory into LDS (all threads)
// Prologue staging in two phases — every global load of the block's inputs is requested (into registers)
// before the first LDS store waits for any of them: the phases used to alternate per region and the
// prologue was seven memory round trips (4.9 us) long.
template <int N>
struct Staged { float v[N]; };

template <int N>
__device__ inline void seg_load(Staged<N>& s, const float* src, int n) {
#pragma unroll
  for (int u = 0; u < N; ++u) { const int i = threadIdx.x + u * kRowThreads; s.v[u] = i < n ? src[i] : 0.f; }
}
template <int N>
__device__ inline void seg_store(const Staged<N>& s, float* dst, const float* src, int n) {
#pragma unroll
  for (int u = 0; u < N; ++u) { const int i = threadIdx.x + u * kRowThreads; if (i < n) dst[i] = s.v[u]; }
  for (int i = threadIdx.x + N * kRowThreads; i < n; i += kRowThreads) dst[i] = src[i];   // oversize regions: the rest directly
}
template <int RG, int N>
__device__ inline void rows_load(Staged<N>& s, const float* src, long long ld_src, int ncols, int jpad, int rv) {
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int i = threadIdx.x + u * kRowThreads, r = i / jpad, c = i - r * jpad;
    s.v[u] = (i < 4 * RG * jpad && r < rv && c < ncols) ? src[(long long)r * ld_src + c] : 0.f;
  }
}
template <int RG, int N>
__device__ inline void rows_store(const Staged<N>& s, float* X, int ldl, const float* src, long long ld_src, int ncols, int jpad, int rv) {
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const int i = threadIdx.x + u * kRowThreads, r = i / jpad, c = i - r * jpad;
    if (i < 4 * RG * jpad) X[r * ldl + c] = s.v[u];
  }
  for (int i = threadIdx.x + N * kRowThreads; i < 4 * RG * jpad; i += kRowThreads) {
    const int r = i / jpad, c = i - r * jpad;
    X[r * ldl + c] = (r < rv && c < ncols) ? src[(long long)r * ld_src + c] : 0.f;
  }
}

// (eight loads in flight per thread before the first LDS store: one memory round trip per 2048 floats)
__device__ inline void stage(float* dst, const float* src, int n) {
  for (int i0 = threadIdx.x; i0 < n; i0 += 8 * kRowThreads) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int i = i0 + u * kRowThreads; v[u] = i < n ? src[i] : 0.f; }
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int i = i0 + u * kRowThreads; if (i < n) dst[i] = v[u]; }
  }
}

// LM: the LDS-multiplier form (mlp_hidden_keep; only the fused DDPG launch's two-role critic phase asks for it: phase 0, part 3)
template <int RG, bool HF = false, bool LM = false>
__device__ __forceinline__ void rowchain_split_body(const RowChainArgs& a, int phase, int part, int bid, const HeadsFold& hfr = HeadsFold{});

// ---- L2-warming riders of the single-agent stream launch (rowchain_ddpg_kernel_stream; round 38) ----
// L2 contents do not survive a kernel boundary, and the optimiser launch in front has just written every weight through to the memory
// side: the first touch of a matrix on an XCD is a miss that the XCD's role workgroups, running in lockstep, all wait behind.  The launch
// leaves CUs idle (192 workgroups on 256 CUs at the headline shape), so it grows by a.reserved0 workgroups with its LAST indices — under
// round-robin dispatch rider r lands on XCD (first rider's index + r) % 8 — that only LOAD, and discard, the H x H matrices the roles will
// stream, in the order of first need.  A rider uses no LDS and no barrier, stores nothing, stamps nothing, waits for nothing another
// workgroup writes, and returns once its loads are back: it cannot change a bit of the result, and a wrong guess about its placement
// costs speed only.  With 8 k riders, k of them share an XCD and each takes every k-th 4 KB piece of a matrix.
__device__ __forceinline__ void rc_warm_matrix(const float* M, int nfloats, int part, int share) {
  const __amdgpu_buffer_rsrc_t rs = bounded_rsrc(M, nfloats);   // a piece past the matrix's end reads zeros and moves nothing
  const int bytes = nfloats * 4;
  constexpr int U = 16;                                         // loads of a thread in flight: 64 KB per rider
  const int step = kRowThreads * 16;                            // a workgroup-wide 16-byte load covers 4 KB: whole lines
  const int mine = part * step + (int)threadIdx.x * 16;
  for (int base = 0; base < bytes; base += share * step * U) {
    v4u w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, base + u * share * step + mine, 0, 0);
#pragma unroll
    for (int u = 0; u < U; ++u) asm volatile("" ::"v"(w[u]));   // the loads stay alive without a store
  }
}
__device__ __forceinline__ void rc_warm_rider(const RowChainArgs& a, int rid) {
  const int nw = a.reserved0;
  const int share = (nw >= 8 && nw % 8 == 0) ? nw / 8 : 1, part = share > 1 ? rid / 8 : 0;
  const int H = a.critic[0].H, L = a.critic[0].L, HH = H * H;
  const bool k = a.nblk_k > 0, p = a.nblk_p > 0;
  // the [in][out] copies of layers >= 1: the three roles walk actor, critic and target actor side by side; the target critic follows
  for (int l = 1; l < L; ++l) {
    if (p) rc_warm_matrix(a.actor.Wt + a.actor.wt[l], HH, part, share);
    rc_warm_matrix(a.critic[0].Wt + a.critic[0].wt[l], HH, part, share);
    if (k) rc_warm_matrix(a.tactor.Wt + a.tactor.wt[l], HH, part, share);
  }
  if (k) for (int l = 1; l < L; ++l) rc_warm_matrix(a.tcritic[0].Wt + a.tcritic[0].wt[l], HH, part, share);
  // the torch-layout matrices of the dX chains, last layer first: the critic's (online role, then the actor phase), then the actor's
  for (int l = L - 1; l >= 1; --l) rc_warm_matrix(a.critic[0].P + a.critic[0].w[l], HH, part, share);
  if (p) for (int l = L - 1; l >= 1; --l) rc_warm_matrix(a.actor.P + a.actor.w[l], HH, part, share);
}

#ifndef RC_STAMP
#define RC_STAMP(i)   // (tools/rc_stamps_build.py: device-clock stamps of the development build)
#endif
// LM = false: the global-multiplier form (the chain's act' multipliers are loaded back from the global saves); true: from LDS
template <int RG, bool LM>
__global__ __launch_bounds__(kRowThreads) void rowchain_ddpg_kernel(RowChainArgs a) {
  kernarg_warm_once<sizeof(RowChainArgs)>();
  constexpr bool ST = false;
  constexpr bool WR = false;
#include "rowchain_ddpg_body.inc"
}
// the stream form (rowchain.h WStream) of the launch at 4 rows per workgroup: the same body, its chained passes carry the weight stream
template <bool LM>
__global__ __launch_bounds__(kRowThreads) void rowchain_ddpg_kernel_stream(RowChainArgs args) {
  kernarg_warm_once<sizeof(RowChainArgs)>();
  // the arguments are read in place, as the population kernel reads its table: with this body's larger number of walks hipcc otherwise
  // copies the by-value record to per-thread scratch (1.8 KB) and indexes it there.  `args` is the kernel's only parameter, so it is
  // what the kernarg segment begins with (offset 0; implicit arguments follow the explicit ones): the same bytes, read where they lie.
  const RowChainArgs& a = *(const RowChainArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  constexpr int RG = 1;
  constexpr bool ST = true;
  constexpr bool WR = true;   // the L2-warming riders (rc_warm_rider above): this kernel only
#include "rowchain_ddpg_body.inc"
}

// population form (agent.hip gcrl_pop_*): member blockIdx.y runs its own arguments tab[blockIdx.y] on the workgroups blockIdx.x of
// its single-agent launch; every pointer of a member's arguments is that member's own
template <int RG, bool LM>
__global__ __launch_bounds__(kRowThreads) void rowchain_ddpg_pop_kernel(const RowChainArgs* __restrict__ tab) {
  const RowChainArgs& a = tab[blockIdx.y];
  constexpr bool ST = false;
  constexpr bool WR = false;
#include "rowchain_ddpg_body.inc"
}
template <bool LM>
__global__ __launch_bounds__(kRowThreads) void rowchain_ddpg_pop_kernel_stream(const RowChainArgs* __restrict__ tab) {
  const RowChainArgs& a = tab[blockIdx.y];
  constexpr int RG = 1;
  constexpr bool ST = true;
  constexpr bool WR = false;
#include "rowchain_ddpg_body.inc"
}

// ---- role-parallel form (rowchain.h: launch_rowchain_split) -------------------------------------------------
// part 3: the role workgroups of a row block meet (meet.h: every wave drains its agent-scope stores before the arrival; one
// monotonic 64-bit counter per row block and phase; those that need the others' values wait, bounded).  Returns false on a timed-out wait.
__device__ inline bool rc_meet(unsigned int* words, int arrivals, bool wait, unsigned int* s_flag, unsigned int* status) {
  return meet(reinterpret_cast<unsigned long long*>(words), (unsigned)arrivals, wait, s_flag, status, MEET_ERR_ROWCHAIN);
}
__device__ inline void st_agent(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline float ld_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the two heads of the BatchNorm actor on the rows in `hrows` (global [.][H], this block's rows: contiguous) and the sampling (rowchain.h HeadsFold):
// action -> X0's action columns, log-prob terms -> sm3; mu / ls_raw stay in sm / sm2; eps / std -> es[r * 16 + o] / es[R * 16 + r * 16 + o].
// hw_m: LDS room for 2 * A * H floats; es: 2 * R * 16 floats.  Two steps, like the kernels' other prologue staging: heads_request puts every
// global load in flight (into registers) BEFORE the caller's own staging waits for anything — requested after it, the three regions were three more
// dependent round trips in front of the first layer pass (measured: the fold gained 2 us of the launch's 11).
struct HeadsStaged { Staged<4> wm, wl, h; float bm, bl; };
template <int RG>
__device__ __forceinline__ void heads_request(HeadsStaged& g, const HeadsFold& f, const float* hrows, int H, int A, int rv) {
  seg_load(g.wm, f.P + f.w_mean, A * H);
  seg_load(g.wl, f.P + f.w_ls, A * H);
  seg_load(g.h, hrows, rv * H);
  const int tid = threadIdx.x;
  g.bm = tid < A ? f.P[f.b_mean + tid] : 0.f;
  g.bl = tid < A ? f.P[f.b_ls + tid] : 0.f;
}
template <int RG>
__device__ __forceinline__ void heads_sample_rows(const HeadsStaged& g, const HeadsFold& f, const float* hrows, const float* eps, int rng_stream, unsigned long long seed,
                                         const StepCtrl& c, float* X0, float* X1, int ldl, int H, int S, int A, long long row0, int rv,
                                         float* hw_m, float* hb, float* sm, float* sm2, float* sm3, float* es) {
  constexpr int R = 4 * RG;
  const int tid = threadIdx.x;
  seg_store(g.wm, hw_m, f.P + f.w_mean, A * H);
  seg_store(g.wl, hw_m + A * H, f.P + f.w_ls, A * H);
  const bool one_pass = 2 * A <= 16;   // both heads as ONE 2A-output pass (weights and biases are contiguous in LDS: mean rows, then log_std rows)
  if (tid < A) { hb[32 + tid] = g.bm; hb[(one_pass ? 32 + A : 48) + tid] = g.bl; }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = tid + u * kRowThreads, r = i / H, kk = i - r * H;
    if (i < R * H) X1[r * ldl + kk] = g.h.v[u];             // (rows >= rv: zeros, seg_load's bound)
  }
  for (int i = tid + 4 * kRowThreads; i < R * H; i += kRowThreads) {
    const int r = i / H, kk = i - r * H;
    X1[r * ldl + kk] = r < rv ? hrows[(long long)r * H + kk] : 0.f;
  }
  __syncthreads();
  if (one_pass) {
    rows_head<RG>(X1, ldl, H, hw_m, H, hb + 32, 2 * A, EPI_NONE, sm);
    __syncthreads();
    if (tid < R * A) { const int r = tid / A, o = tid - r * A; sm2[r * 16 + o] = sm[r * 16 + A + o]; }   // (the callers read log_std's outputs from sm2)
  } else {
    rows_head<RG>(X1, ldl, H, hw_m, H, hb + 32, A, EPI_NONE, sm);
    rows_head<RG>(X1, ldl, H, hw_m + A * H, H, hb + 48, A, EPI_NONE, sm2);
  }
  __syncthreads();
  if (tid < R * A) {
    const int r = tid / A, o = tid - r * A;
    float t = 0.f;
    if (r < rv) {
      const TgElem e = tanh_gauss_elem_raw(eps, seed, rng_stream, c, sm[r * 16 + o], sm2[r * 16 + o], (row0 + r) * A + o);
      t = e.t;
      sm3[r * 16 + o] = e.term;
      es[r * 16 + o] = e.e; es[R * 16 + r * 16 + o] = e.sd;
    }
    X0[r * ldl + S + o] = t;
  }
  __syncthreads();
}
// what the actor's backward and the actor loss read of actor.sample(states), from heads_sample_rows' LDS results (one role per row block calls it)
template <int RG>
__device__ __forceinline__ void heads_write_cur(const HeadsFold& f, const float* X0, int ldl, int S, int A, int Apad, long long row0, int rv,
                                       const float* sm, const float* sm2, const float* sm3, const float* es);
__device__ inline float logp_row(const float* sm3, int r, int A) {
  float lp = 0.f;
  for (int j = 0; j < A; ++j) lp = __fadd_rn(lp, sm3[r * 16 + j]);   // in action order, as the sampling launch adds
  return lp;
}

template <int RG>
__device__ __forceinline__ void heads_write_cur(const HeadsFold& f, const float* X0, int ldl, int S, int A, int Apad, long long row0, int rv,
                                       const float* sm, const float* sm2, const float* sm3, const float* es) {
  constexpr int R = 4 * RG;
  const int tid = threadIdx.x;
  if (tid < R * A) {
    const int r = tid / A, o = tid - r * A;
    if (r < rv) {
      const long long i = (row0 + r) * A + o;
      f.pi[(row0 + r) * Apad + o] = X0[r * ldl + S + o];
      f.save_eps[i] = es[r * 16 + o]; f.save_std[i] = es[R * 16 + r * 16 + o];
      f.head[(row0 + r) * 2 * Apad + o] = sm[r * 16 + o];
      f.head[(row0 + r) * 2 * Apad + Apad + o] = sm2[r * 16 + o];
    }
  }
  if (tid < rv) f.logp[row0 + tid] = logp_row(sm3, tid, A);
}

// HF: the instantiation of rowchain_split_heads_kernel (the record is a kernel argument: read in place, never through a pointer that could be null —
// with `const HeadsFold*` and run-time null checks hipcc copied the 192-byte record to per-thread scratch once a third use site appeared)
template <int RG, bool HF, bool LM>
__device__ __forceinline__ void rowchain_split_body(const RowChainArgs& a, int phase, int part, int bid, const HeadsFold& hfr) {
  const HeadsFold* const hf = &hfr;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int R = 4 * RG;
  const int ldl = a.ldl, H = a.critic[0].H, S = a.S, A = a.A, B = a.B, C = a.C;
  float* X0 = lds;
  float* X1 = X0 + R * ldl;
  float* X2 = X1 + R * ldl;
  float* XS = X2 + R * ldl;
  float* part_ = XS + R * ldl;
  float* sm = part_ + R * 16 + (RG == 1 ? 2 : 1) * 4 * R * kRowChunk;
  float* sm2 = sm + R * 16;
  float* sm3 = sm2 + R * 16;
  float* hw = sm3 + R * 16;
  float* hb = hw + max(max(2 * A + 1, A + 2 * C), C * (A + 1)) * H;
  [[maybe_unused]] float* KP = hb + 96;   // LM: the online critic's kept layers, [L - 1][R][ldl]
  const int nblk = (B + R - 1) / R;
  const int role = bid / nblk;
  const int blk = bid - role * nblk;
  const bool fold = HF && hfr.on != 0;

  const long long row0 = (long long)blk * R;
  const int rv = min(R, B - (int)row0);
  const long long BH = (long long)B * H;
  const int tid = threadIdx.x;
  const StepCtrl c = phase == 0 ? *a.cur_k : *a.cur_p;
  if (fold && phase == 0 && part != 2 && role == 2 * C) {
    // the launch's extra workgroups (highest indices, waiting for nobody: they start as role workgroups finish and run beside the online roles'
    // backward passes): with cur_in_k one per row block forms pi(s) and what phase 1 and the actor's backward read of it — in the online role's
    // own workgroup the same work sat on the launch's critical path (34.4 us against 32.2) —; block 0 also applies BatchNorm's running statistics
    // (input 0's batch, then input 1's)
    if (hf->cur_in_k) {
      HeadsStaged hst;
      heads_request<RG>(hst, *hf, hf->h_cur + row0 * H, H, A, rv);
      heads_sample_rows<RG>(hst, *hf, hf->h_cur + row0 * H, hf->eps_cur, 2, a.seed, c, X0, X1, ldl, H, S, A, row0, rv, hw, hb, sm, sm2, sm3, part_);
      heads_write_cur<RG>(*hf, X0, ldl, S, A, a.Apad, row0, rv, sm, sm2, sm3, part_);
    }
    if (blk == 0 && hf->run.layers) bn_running_update(hf->run);
    return;
  }
  const bool merged = part == 3;                 // parts 1 and 2 in this launch (rowchain.h)
  __shared__ unsigned int s_flag;
  unsigned int* meet = merged ? a.bar + ((long long)phase * nblk + blk) * 32 : nullptr;
  bool met = true;
  if (phase == 0 && part != 2 && bid == 0 && tid == 0) { a.cb->cur_b = a.cb->cur; a.cb->prev_b = a.cb->prev; }

  if (phase == 0 && part != 2 && role < C) {
    // ---- target critic `role` on [ns | a'] (a' given: SAC; else the target actor runs first: TD3)
    const int k = role;
    const float* ns_rows = a.nsa + (long long)c.batch_slot * a.slot_x + row0 * a.ldx;
    const int jp_ns = max(a.tactor.jpad0, a.tcritic[0].jpad0), nc_ns = (a.given_next && !fold) ? S + A : S;
    float* hw_ta = hw; float* hw_tc = hw + (fold ? 2 * A : A) * H;
    HeadsStaged hst;
    if (fold) heads_request<RG>(hst, *hf, hf->h_next + row0 * H, H, A, rv);
    load_rows<RG>(X0, ldl, ns_rows, a.ldx, nc_ns, jp_ns, rv);
    stage(hw_tc, a.tcritic[k].P + a.tcritic[k].w[a.tcritic[k].L], H);
    if (tid == 0) hb[16] = a.tcritic[k].P[a.tcritic[k].b[a.tcritic[k].L]];
    if (!a.given_next) {
      stage(hw_ta, a.tactor.P + a.tactor.w[a.tactor.L], A * H);
      if (tid < A) hb[tid] = a.tactor.P[a.tactor.b[a.tactor.L] + tid];
      if (a.target_kind == TGT_MIN && tid < R * A) {
        const int r = tid / A, o = tid - r * A;
        const long long i = (row0 + r) * A + o;
        float e = 0.f;
        if (r < rv) e = a.noise ? a.noise[i] : hash_normal(a.seed, (((unsigned long long)c.rng_hi << 32) | c.rng_lo) + (unsigned long long)i);
        part_[tid] = fminf(fmaxf(__fmul_rn(e, a.policy_noise), -a.noise_clamp), a.noise_clamp);
      }
    }
    if (fold) {   // a' = actor.sample(next_state) for these rows; role 0 publishes logp_next (the online roles read it after the meeting)
      heads_sample_rows<RG>(hst, *hf, hf->h_next + row0 * H, hf->eps_next, 1, a.seed, c, X0, X1, ldl, H, S, A, row0, rv, hw, hb, sm, sm2, sm3, part_);
      if (k == 0 && tid < rv) st_agent(hf->logp_next + row0 + tid, logp_row(sm3, tid, A));
    }
    __syncthreads();
    float* h;
    if (!a.given_next) {
      h = mlp_hidden<RG>(a.tactor, X0, X1, X2, ldl, part_ + R * 16, nullptr, BH, row0, rv);
      rows_head<RG>(h, ldl, H, hw_ta, H, hb, A, EPI_TANH, sm);
      __syncthreads();
      if (tid < R * A) {
        const int r = tid / A, o = tid - r * A;
        float act = sm[r * 16 + o];
        if (a.target_kind == TGT_MIN) act = fminf(fmaxf(__fadd_rn(act, part_[tid]), -1.0f), 1.0f);
        X0[r * ldl + S + o] = act;
      }
      __syncthreads();
    }
    h = mlp_hidden<RG>(a.tcritic[k], X0, X1, X2, ldl, part_ + R * 16, nullptr, BH, row0, rv);
    rows_head<RG>(h, ldl, H, hw_tc, H, hb + 16, 1, EPI_NONE, sm);
    __syncthreads();
    if (tid < rv) st_agent(a.qt + (long long)k * B + row0 + tid, sm[tid * 16]);
    if (merged) {                                                    // (the target roles only report in)
      if (a.producers_first) meet_produce(reinterpret_cast<unsigned long long*>(meet));
      else rc_meet(meet, 2 * C, false, &s_flag, a.status);
    }
    return;
  }
  int k2 = role;                                 // the critic whose backward part runs in this workgroup
  if (phase == 0 && part != 2) {
    // ---- online critic `role - C` on [s | a]: forward, activations saved
    const int k = role - C;
    const float* sa_rows = a.sa + (long long)c.batch_slot * a.slot_x + row0 * a.ldx;
    load_rows<RG>(LM ? X0 : XS, ldl, sa_rows, a.ldx, S + A, a.critic[0].jpad0, rv);   // (LM: XS takes the last layer's output)
    stage(hw, a.critic[k].P + a.critic[k].w[a.critic[k].L], H);
    if (tid == 0) hb[18] = a.critic[k].P[a.critic[k].b[a.critic[k].L]];
    __syncthreads();
    float* h;
    if constexpr (LM) h = mlp_hidden_keep<RG>(a.critic[k], X0, KP, XS, ldl, part_ + R * 16, a.hC + (long long)k * a.critic[k].L * BH, BH, row0, rv);
    else h = mlp_hidden<RG>(a.critic[k], XS, X1, X2, ldl, part_ + R * 16, a.hC + (long long)k * a.critic[k].L * BH, BH, row0, rv);
    rows_head<RG>(h, ldl, H, hw, H, hb + 18, 1, EPI_NONE, sm);
    __syncthreads();
    if (tid < rv) a.q[(long long)k * B + row0 + tid] = sm[tid * 16];
    if (!merged) return;
    // both target critics' outputs of these rows are out
    if (a.producers_first)
      met = meet_consume(reinterpret_cast<unsigned long long*>(meet), reinterpret_cast<unsigned long long*>(meet) + 2 + k, (unsigned)C, &s_flag, a.status, MEET_ERR_ROWCHAIN);
    else met = rc_meet(meet, 2 * C, true, &s_flag, a.status);
    k2 = k;
  }
  if (phase == 0) {
    // ---- part 2: TD target, loss gradient and input-gradient chain of critic `k2`
    const int k = k2;
    const int L = a.critic[k].L;
    const float* hs = a.hC + (long long)k * L * BH;
    const float* hsrc = hs + (L - 1) * BH + row0 * H;
    stage(hw, a.critic[k].P + a.critic[k].w[L], H);
    if constexpr (!LM)   // (LM: the forward part of this launch left the activation in XS)
      for (int i = tid; i < R * H; i += kRowThreads) {
        const int r = i / H, kk = i - r * H;
        XS[r * ldl + kk] = r < rv ? hsrc[(long long)r * H + kk] : 0.f;
      }
    if (tid < R) {
      const int r = tid;
      float g = 0.f;
      if (r < rv) {
        const float rew = a.rbuf[(long long)c.batch_slot * a.slot_rd + row0 + r], dn = a.dbuf[(long long)c.batch_slot * a.slot_rd + row0 + r];
        const float t0 = ld_agent(a.qt + row0 + r), t1 = C > 1 ? ld_agent(a.qt + (long long)B + row0 + r) : t0;
        float tq = a.target_kind == TGT_DDPG ? t0 : fminf(t0, t1);
        if (a.target_kind == TGT_MIN_ENT) tq = __fsub_rn(tq, __fmul_rn(a.alpha, fold ? ld_agent(a.logp_next + row0 + r) : a.logp_next[row0 + r]));
        float y = __fadd_rn(rew, __fmul_rn(__fmul_rn(a.gamma, __fsub_rn(1.0f, dn)), tq));
        if (a.target_kind == TGT_DDPG) y = fminf(fmaxf(y, a.clamp_lo), 0.0f);
        const float q = a.q[(long long)k * B + row0 + r];
        const float diff = __fsub_rn(q, y);
        if (a.loss_kind == LOSS_MSE) g = (2.0f / (float)B) * diff;
        else { const float n1 = 1.0f / (float)B; g = (diff < -1.0f) ? -n1 : (diff > 1.0f ? n1 : n1 * diff); }
        if (!met) g = __builtin_nanf("");          // a timed-out meeting must not pass for a result
        if (k == 0) a.y[row0 + r] = y;
        a.dq[(long long)k * B + row0 + r] = g;
      }
      sm2[r * 16] = g;
    }
    __syncthreads();
    float* gsave = a.gC + (long long)k * L * BH;
    head_backward<RG>(XS, ldl, H, hw, 1, sm2, gsave + (L - 1) * BH + row0 * H, rv);
    __syncthreads();
    if constexpr (LM) grad_chain_keep<RG>(a.critic[k], XS, X1, X2, ldl, part_ + R * 16, KP, gsave, BH, row0, rv);
    else grad_chain<RG>(a.critic[k], XS, X1, X2, ldl, part_ + R * 16, hs, gsave, BH, row0, rv);
    return;
  }
  if (part != 2) {
    // ---- P, part 1: critic `role` forward on [s | pi(s)]
    const int k = role;
    const float* s_rows = a.sa + (long long)c.batch_slot * a.slot_x + row0 * a.ldx;
    const int jpad = a.critic[0].jpad0;
    HeadsStaged hst;
    if (fold) heads_request<RG>(hst, *hf, hf->h_cur + row0 * H, H, A, rv);
    for (int i = tid; i < R * jpad; i += kRowThreads) {
      const int r = i / jpad, cc = i - r * jpad;
      float v = 0.f;
      if (r < rv) {
        if (cc < S) v = s_rows[(long long)r * a.ldx + cc];
        else if (cc < S + A && !fold) v = a.pi[(row0 + r) * a.Apad + (cc - S)];
      }
      if (!fold || cc < S || cc >= S + A) X0[r * ldl + cc] = v;
    }
    stage(hw, a.critic[k].P + a.critic[k].w[a.critic[k].L], H);
    if (tid == 0) hb[0] = a.critic[k].P[a.critic[k].b[a.critic[k].L]];
    if (fold) {   // pi(s) = actor.sample(states) for these rows; role 0 writes what the actor's backward and the actor loss read
      float* hw_m = hw + H;
      heads_sample_rows<RG>(hst, *hf, hf->h_cur + row0 * H, hf->eps_cur, 2, a.seed, c, X0, X1, ldl, H, S, A, row0, rv, hw_m, hb, sm, sm2, sm3, part_);
      if (k == 0) heads_write_cur<RG>(*hf, X0, ldl, S, A, a.Apad, row0, rv, sm, sm2, sm3, part_);
    }
    __syncthreads();
    float* h = mlp_hidden<RG>(a.critic[k], X0, X1, X2, ldl, part_ + R * 16, a.hC2 + (long long)k * a.critic[k].L * BH, BH, row0, rv);
    rows_head<RG>(h, ldl, H, hw, H, hb, 1, EPI_NONE, sm);
    __syncthreads();
    if (tid < rv) st_agent(a.q2 + (long long)k * B + row0 + tid, sm[tid * 16]);
    if (!merged) return;
    met = rc_meet(meet, C, true, &s_flag, a.status);                   // the other critic's Q of these rows is out
  }
  {
    // ---- P, part 2: d(-mean min(q1, q2))/dq_k, input-gradient chain of critic `role` down to the action columns
    const int k = role;
    const int L = a.critic[k].L;
    const float* hs = a.hC2 + (long long)k * L * BH;
    const float* hsrc = hs + (L - 1) * BH + row0 * H;
    float* hw_da = hw + H;
    stage(hw, a.critic[k].P + a.critic[k].w[L], H);
    stage(hw_da, a.critic[k].Wt + a.critic[k].wt[0] + (long long)S * H, A * H);
    for (int i = tid; i < R * H; i += kRowThreads) {
      const int r = i / H, kk = i - r * H;
      XS[r * ldl + kk] = r < rv ? hsrc[(long long)r * H + kk] : 0.f;
    }
    if (tid < R) {
      const int r = tid;
      float g = 0.f;
      if (r < rv) {
        const float q0 = ld_agent(a.q2 + row0 + r), q1 = C > 1 ? ld_agent(a.q2 + (long long)B + row0 + r) : INFINITY;
        const float gb = -1.0f / (float)B;
        const float w0 = q0 < q1 ? 1.f : (q0 == q1 ? 0.5f : 0.f);
        g = k == 0 ? gb * w0 : gb * (1.f - w0);
        if (!met) g = __builtin_nanf("");
      }
      sm2[r * 16] = g;
    }
    __syncthreads();
    head_backward<RG>(XS, ldl, H, hw, 1, sm2, nullptr, rv);
    __syncthreads();
    float* g0 = grad_chain<RG>(a.critic[k], XS, X1, X2, ldl, part_ + R * 16, hs, nullptr, BH, row0, rv);
    rows_head<RG>(g0, ldl, H, hw_da, H, nullptr, A, EPI_NONE, sm);
    __syncthreads();
    if (tid < R * A) {
      const int r = tid / A, o = tid - r * A;
      if (r < rv) a.dz[((long long)k * B + row0 + r) * a.Apad + o] = sm[r * 16 + o];
    }
  }
}

template <int RG>
__global__ __launch_bounds__(kRowThreads) void rowchain_split_kernel(RowChainArgs a, int phase, int part) {
  kernarg_warm<sizeof(RowChainArgs) + 8>();
  rowchain_split_body<RG>(a, phase, part, (int)blockIdx.x);
}
template <int RG>
__global__ __launch_bounds__(kRowThreads) void rowchain_split_heads_kernel(RowChainArgs a, int phase, int part, HeadsFold hf) {
  kernarg_warm<sizeof(RowChainArgs) + 8 + sizeof(HeadsFold)>();
  rowchain_split_body<RG, true>(a, phase, part, (int)blockIdx.x, hf);
}

// population forms (pop.h): member blockIdx.y runs its own launch — arguments, phase, part and, for the heads form, the HeadsFold record, all
// from the device table — on the workgroups blockIdx.x of its single-agent launch.  The body reads the records in place (references into the
// table: uniform loads, no copy); a member's meeting counters, exchange words and status word are its own, so its workgroups meet only each other.
struct RowSplitPop { RowChainArgs a; int phase, part; HeadsFold hf; };
template <int RG>
__global__ __launch_bounds__(kRowThreads) void rowchain_split_pop_kernel(const RowSplitPop* __restrict__ tab) {
  const RowSplitPop& e = tab[blockIdx.y];
  rowchain_split_body<RG>(e.a, e.phase, e.part, (int)blockIdx.x);
}
template <int RG>
__global__ __launch_bounds__(kRowThreads) void rowchain_split_heads_pop_kernel(const RowSplitPop* __restrict__ tab) {
  const RowSplitPop& e = tab[blockIdx.y];
  rowchain_split_body<RG, true>(e.a, e.phase, e.part, (int)blockIdx.x, e.hf);
}

// `row_at(i)`: element i of the launch's input rows ([n][ld_obs] flattened); `noise_at(t)`: exploration noise of action element t —
// functors, so that the inline form reads the kernel-argument segment by plain indexed loads (a POINTER into a by-value argument
// struct made hipcc copy the whole struct into every thread's scratch: 36 us for this kernel, round 4).  SYS: the float64 actions
// go out as system-scope (write-through) stores, for a host that polls a flag behind them.
template <bool SYS, typename RowAt, typename NoiseAt>
__device__ inline void rowchain_act_body(const RowActArgs& a, RowAt row_at, NoiseAt noise_at, bool has_noise, double* out64, float* lds) {
  constexpr int R = 4;
  const int ldl = a.ldl, H = a.actor.H, A = a.A, tid = threadIdx.x;
  float* X0 = lds;
  float* X1 = X0 + R * ldl;
  float* X2 = X1 + R * ldl;
  float* part = X2 + R * ldl;                 // two exchange buffers (chained layers)
  float* sm = part + 2 * 4 * R * kRowChunk;
  float* hw = sm + R * 16;
  float* hb = hw + A * H;
  const long long row0 = (long long)blockIdx.x * R;
  const int rv = min(R, a.n - (int)row0);
  const float* src_h = a.actor.P + a.actor.w[a.actor.L];
  const int jp = a.actor.jpad0;
  constexpr int NX = 2;                        // staged elements per thread: rows of up to 128 floats; wider rows take the loop below
  float s_x[NX];
  Staged<8> s_h;
#pragma unroll
  for (int u = 0; u < NX; ++u) {
    const int i = tid + u * kRowThreads, r = i / jp, c = i - r * jp;
    s_x[u] = (i < R * jp && r < rv && c < a.S) ? row_at((row0 + r) * a.ld_obs + c) : 0.f;
  }
  seg_load(s_h, src_h, A * H);
  const float v_hb = tid < A ? a.actor.P[a.actor.b[a.actor.L] + tid] : 0.f;
  // An acting launch is a few workgroups long after the last optimiser launch: every layer's weights come from HBM, one
  // dependent ~2 us round trip per layer pass.  Touch one float of every 128-byte line of the LATER layers' [in][out] copies now
  // (fire and forget: the values are only consumed by a never-taken branch at the end), so that their passes find them in L2.
  float pf = 0.f;
  {
    const float* wl = a.actor.Wt + a.actor.wt[a.actor.L > 1 ? 1 : 0];
    const long long nfl = a.actor.L > 1 ? (long long)(a.actor.L - 1) * H * H : 0;
    if (nfl <= 64 * 1024)
      for (long long i = (long long)tid * 32; i < nfl; i += (long long)kRowThreads * 32) pf += wl[i];
  }
  // fused acting entry: the rows are raw; normalise this thread's elements on their way into LDS
  if (a.nz_mean || a.nzg_mean) {
#pragma unroll
    for (int u = 0; u < NX; ++u) {
      const int i = tid + u * kRowThreads, r = i / jp, c = i - r * jp;
      if (i < R * jp && r < rv && c < a.S) {
        const bool ob = c < a.D;
        const double* m = ob ? a.nz_mean : a.nzg_mean;
        if (m) {
          const int j = ob ? c : c - a.D;
          const double* v = ob ? a.nz_var : a.nzg_var;
          const double clip = ob ? a.nz_clip : a.nzg_clip;
          const int md = ob ? a.nz_mode : a.nzg_mode;
          s_x[u] = norm_apply(s_x[u], m[j], norm_den(v[j], (md & NORM_F32) != 0), clip, norm_apply_f32(md));
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < NX; ++u) {
    const int i = tid + u * kRowThreads, r = i / jp, c = i - r * jp;
    if (i < R * jp) X0[r * ldl + c] = s_x[u];
  }
  for (int i = tid + NX * kRowThreads; i < R * jp; i += kRowThreads) {   // (rows wider than 128 floats: never with fused normalisation)
    const int r = i / jp, c = i - r * jp;
    X0[r * ldl + c] = (r < rv && c < a.S) ? row_at((row0 + r) * a.ld_obs + c) : 0.f;
  }
  seg_store(s_h, hw, src_h, A * H);
  if (tid < A) hb[tid] = v_hb;
  __syncthreads();
  float* h = mlp_hidden<1>(a.actor, X0, X1, X2, ldl, part, nullptr, 0, row0, rv);
  rows_head<1>(h, ldl, H, hw, H, hb, A, EPI_TANH, sm);
  __syncthreads();
  if (tid < R * A) {
    const int r = tid / A, o = tid - r * A;
    if (r < rv) {
      const float y = sm[r * 16 + o];
      if (!a.post) a.out[(row0 + r) * a.ld_out + o] = y;
      else {
        const long long t = (row0 + r) * A + o;
        double v = (double)y;
        if (a.post != 3) {
          v = (double)tanhf(y);
          if (a.post == 1 && has_noise) v += noise_at(t);
          v = fmin(fmax(v, -1.0), 1.0);
        }
        if (SYS) __hip_atomic_store(out64 + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else out64[t] = v;
      }
    }
  }
  if (pf == 1.2345678e-30f && a.post) out64[0] = (double)pf;   // (keeps the prefetch loads alive; never true in practice, harmless if it were)
}

__global__ __launch_bounds__(kRowThreads) void rowchain_act_kernel(RowActArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  rowchain_act_body<false>(a, [&](long long i) { return a.obs[i]; }, [&](long long t) { return a.noise[t]; }, a.noise != nullptr, a.out64, lds);
}

// rows and noise inside the kernel arguments, actions and a completion flag per workgroup to host-visible memory (rowchain.h)
__global__ __launch_bounds__(kRowThreads) void rowchain_act_inline_kernel(RowActInline a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  rowchain_act_body<true>(a.base, [&](long long i) { return a.obs_inl[i]; }, [&](long long t) { return a.noise_inl[t]; }, a.with_noise != 0, a.out_host, lds);
  // this workgroup's rows are out as write-through stores: drain them, then raise its flag (system scope: the host polls it)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(a.flag_host + blockIdx.x, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// population form (rowchain.h RowActPop): member blockIdx.y on its own arguments tab[blockIdx.y] and its own slices of the rows, the
// noise and the actions — the same body text as the inline kernel, so each member's rows go through its own arithmetic in its own order
__global__ __launch_bounds__(kRowThreads) void rowchain_act_pop_kernel(RowActPop c) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const unsigned int m = blockIdx.y;
  if (!((c.live >> m) & 1u)) return;   // skipped member: nothing read, nothing written
  const RowActArgs& a = c.tab[m];      // (a reference into the device table: uniform loads, no copy of the struct)
  const float* rows = c.rows + (size_t)m * c.stride_n * a.ld_obs;
  const double* noise = c.noise + (size_t)m * c.stride_n * a.A;
  double* out = c.out + (size_t)m * c.stride_n * a.A;
  rowchain_act_body<true>(a, [&](long long i) { return __hip_atomic_load(rows + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); },
                          [&](long long t) { return __hip_atomic_load(noise + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); },
                          ((c.noisy >> m) & 1u) != 0, out, lds);
  // this workgroup's rows are out as write-through stores: drain them, then raise its flag (system scope: the host polls it)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && c.flags) __hip_atomic_store(c.flags + (size_t)m * gridDim.x + blockIdx.x, c.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Wt[wt[l] + k*H + o] = P[w[l] + o*in_l + k]; layer 0 rows in..jpad0-1 are zero
__global__ void wt_rebuild_kernel(RowNet net, float* Wt) {
  const int l = blockIdx.y;
  const int in = l == 0 ? net.in : net.H, J = l == 0 ? net.jpad0 : net.H, H = net.H;
  const long long n = (long long)J * H;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i / H), o = (int)(i - (long long)k * H);
    Wt[net.wt[l] + i] = k < in ? net.P[net.w[l] + (long long)o * in + k] : 0.f;
  }
}

}  // namespace

size_t rowchain_lds_bytes(int rg, int ldl, int A, int H, int C) {
  const int R = 4 * rg;
  return (size_t)(4 * R * ldl + (rg == 1 ? 2 : 1) * 4 * R * kRowChunk + 4 * R * 16 + std::max(std::max(2 * A + 1, A + 2 * C), C * (A + 1)) * H + 96) * sizeof(float);   // (the trailing floats: head biases — hb[0 .. 64))
}

size_t rowchain_lds_bytes_mul(int rg, int ldl, int A, int H, int C, int L, bool actor_phase) {
  return rowchain_lds_bytes(rg, ldl, A, H, C) + (size_t)(actor_phase ? 2 : 1) * std::max(L - 1, 0) * 4 * rg * ldl * sizeof(float);
}

namespace {
// workgroups of `kernel` a CU holds at this much dynamic LDS (meet_capacity's count, abi_misc.hip: the occupancy query, then LDS in 1 KB
// granules with one held back); 0 when the query fails
int rc_resident_per_cu(const void* kernel, size_t lds) {
  int per_cu = 0;
  if (lds > 64 * 1024 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kRowThreads, lds) != hipSuccess) { (void)hipGetLastError(); return 0; }
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, kernel) == hipSuccess) {
    const size_t g = ((fa.sharedSizeBytes + lds + 1023) / 1024) * 1024;
    if (g > 0) per_cu = (int)std::min<long long>(per_cu, (long long)((160 * 1024 - 1024) / g));
  }
  return std::max(per_cu, 0);
}
}  // namespace

bool rowchain_lds_mul_ok(int rg, int ldl, int A, int H, int C, int L, bool actor_phase, long long wgs) {
  if (L < 2 || wgs < 1 || !(rg == 1 || rg == 2 || rg == 4)) return false;
  const size_t lds_old = rowchain_lds_bytes(rg, ldl, A, H, C), lds_new = rowchain_lds_bytes_mul(rg, ldl, A, H, C, L, actor_phase);
  if (lds_new > 160 * 1024) return false;
  // (the device is asked once per shape — agent creation does it, gcrl_agent_rowchain_form's rule —: the occupancy queries are host work a
  // launch should not repeat, least of all inside a stream capture)
  static std::mutex mu;
  static std::map<std::array<long long, 3>, std::array<long long, 2>> known;   // -> workgroups the device holds at once: old form, new form
  const std::array<long long, 3> key = {(long long)rg, (long long)lds_old, (long long)lds_new};
  std::lock_guard<std::mutex> lock(mu);
  auto it = known.find(key);
  // never fewer of the launch's workgroups resident at once than it has today (a launch smaller than the chip has all of them either way)
  auto rule = [&](const std::array<long long, 2>& cap) { return std::min(wgs, cap[1]) >= 1 && std::min(wgs, cap[1]) >= std::min(wgs, cap[0]); };
  if (it != known.end()) return rule(it->second);
  const void* k_old = rg == 1 ? (const void*)rowchain_ddpg_kernel<1, false> : (rg == 2 ? (const void*)rowchain_ddpg_kernel<2, false> : (const void*)rowchain_ddpg_kernel<4, false>);
  const void* k_new = rg == 1 ? (const void*)rowchain_ddpg_kernel<1, true> : (rg == 2 ? (const void*)rowchain_ddpg_kernel<2, true> : (const void*)rowchain_ddpg_kernel<4, true>);
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { (void)hipGetLastError(); cus = 0; }
  const std::array<long long, 2> cap = {(long long)cus * rc_resident_per_cu(k_old, lds_old), (long long)cus * rc_resident_per_cu(k_new, lds_new)};
  known.emplace(key, cap);
  return rule(cap);
}

// the merged (part 3) launches wait inside the kernel: all 2C x nblk workgroups of the larger one must be resident at once
bool rowchain_merge_ok(int rg, int ldl, int A, int H, int C, int B) {
  const size_t lds = rowchain_lds_bytes(rg, ldl, A, H, C);
  if (lds > 160 * 1024) return false;
  const void* k = rg == 1 ? (const void*)rowchain_split_kernel<1> : (rg == 2 ? (const void*)rowchain_split_kernel<2> : (const void*)rowchain_split_kernel<4>);
  if (lds > 64 * 1024 && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
  const long long nblk = (B + 4 * rg - 1) / (4 * rg);
  // (the form with the actor's heads inside — SAC, rowchain.h HeadsFold — is another kernel with its own register count: both must fit)
  const void* kh = rg == 1 ? (const void*)rowchain_split_heads_kernel<1> : (rg == 2 ? (const void*)rowchain_split_heads_kernel<2> : (const void*)rowchain_split_heads_kernel<4>);
  if (lds > 64 * 1024 && hipFuncSetAttribute(kh, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
  // (its extra workgroup has the launch's LAST index and waits for nobody: it may start once a role workgroup has finished)
  return 2LL * C * nblk <= meet_capacity(k, kRowThreads, lds) && 2LL * C * nblk <= meet_capacity(kh, kRowThreads, lds);
}

// the stream form's shapes: the plain DDPG launch at 4 rows per workgroup, chained passes (H <= kRowChunk), walks of two layers or more
bool rowchain_stream_ok(const RowChainArgs& a, int rg) {
  const int H = a.critic[0].H, L = a.critic[0].L;
  return rg == 1 && a.C == 1 && !a.p_critic_only && !a.given_next && a.target_kind == TGT_DDPG && H <= kRowChunk && L >= 2 &&
         a.actor.H == H && a.tactor.H == H && a.tcritic[0].H == H && a.actor.L == L && a.tactor.L == L && a.tcritic[0].L == L;
}

int launch_rowchain_ddpg(hipStream_t st, const RowChainArgs& a, int rg, bool lds_mul, bool stream) {
  GCRL_CHECK_ARG(rg == 1 || rg == 2 || rg == 4, "rowchain: rows per block must be 4, 8 or 16");
  GCRL_CHECK_ARG(a.critic[0].H % 4 == 0 && a.ldl % 4 == 0 && a.A <= 16 && a.C >= 1 && a.C <= 2,
                 "rowchain: unsupported shape (H=%d, A=%d, C=%d)", a.critic[0].H, a.A, a.C);
  // the form: multipliers from LDS where that fits and costs no resident workgroup (rowchain.h); the SAC form keeps the global saves
  const int L = std::max(a.actor.L, a.critic[0].L);
  const int grid = (a.k_split ? 2 : 1) * a.nblk_k + a.nblk_p;
  const bool lm = lds_mul && !a.p_critic_only && a.actor.L == a.critic[0].L && rowchain_lds_mul_ok(rg, a.ldl, a.A, a.critic[0].H, a.C, L, a.nblk_p > 0, grid);
  const size_t lds = lm ? rowchain_lds_bytes_mul(rg, a.ldl, a.A, a.critic[0].H, a.C, L, a.nblk_p > 0) : rowchain_lds_bytes(rg, a.ldl, a.A, a.critic[0].H, a.C);
  GCRL_CHECK_ARG(lds <= 160 * 1024, "rowchain: %zu bytes of LDS needed", lds);
  GCRL_CHECK_ARG(!a.k_split || (a.bar && a.qt && a.producers_first && a.C == 1), "rowchain: the two-role critic phase needs its meeting counters");
  if (grid < 1) return GCRL_OK;
  const bool sf = stream && rowchain_stream_ok(a, rg);   // the stream form of the chained passes (rowchain.h WStream)
  if (PopRec* r = pop_recording())   // a population step is being recorded (pop.h)
    return pop_record(r, POP_ROWCHAIN, rg | (lm ? 16 : 0) | (sf ? 32 : 0), dim3(grid), lds, &a, sizeof(a), [ac = a, rg, lds_mul, stream](hipStream_t s) { return launch_rowchain_ddpg(s, ac, rg, lds_mul, stream); });
  // the L2-warming riders (rc_warm_rider): a.reserved0 more workgroups behind the roles', the single-agent stream kernel's only
  const int nw = sf ? a.reserved0 : 0;
  auto go = [&](auto kern) -> int {
    static thread_local size_t raised = 0;   // (per kernel: a generic lambda's statics belong to its instantiation)
    if (lds > 64 * 1024 && lds > raised) {
      GCRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      raised = lds;
    }
    hipLaunchKernelGGL(kern, dim3(grid + nw), dim3(kRowThreads), lds, st, a);
    GCRL_HIP(hipGetLastError());
    return GCRL_OK;
  };
  if (sf) return lm ? go(rowchain_ddpg_kernel_stream<true>) : go(rowchain_ddpg_kernel_stream<false>);
  if (lm) {
    if (rg == 1) return go(rowchain_ddpg_kernel<1, true>);
    if (rg == 2) return go(rowchain_ddpg_kernel<2, true>);
    return go(rowchain_ddpg_kernel<4, true>);
  }
  if (rg == 1) return go(rowchain_ddpg_kernel<1, false>);
  if (rg == 2) return go(rowchain_ddpg_kernel<2, false>);
  return go(rowchain_ddpg_kernel<4, false>);
}

int launch_rowchain_split(hipStream_t st, const RowChainArgs& a, int rg, int phase, int part, const HeadsFold* hf) {
  GCRL_CHECK_ARG(rg == 1 || rg == 2 || rg == 4, "rowchain: rows per block must be 4, 8 or 16");
  GCRL_CHECK_ARG(a.critic[0].H % 4 == 0 && a.ldl % 4 == 0 && a.A <= 16 && a.C >= 1 && a.C <= 2 && (phase == 0 || phase == 1) &&
                     (part >= 1 && part <= 3) && (part != 3 || a.bar) && (phase == 0 || a.p_critic_only) && a.qt,
                 "rowchain split: unsupported shape (H=%d, A=%d, C=%d, phase %d part %d)", a.critic[0].H, a.A, a.C, phase, part);
  const size_t lds = rowchain_lds_bytes(rg, a.ldl, a.A, a.critic[0].H, a.C);
  GCRL_CHECK_ARG(lds <= 160 * 1024, "rowchain: %zu bytes of LDS needed", lds);
  const int nblk = (a.B + 4 * rg - 1) / (4 * rg);
  const int roles = (phase == 0 && part != 2) ? 2 * a.C : a.C;
  // part 3: every workgroup of the launch must be resident at once (rowchain_merge_ok: the kernel's occupancy at this LDS size
  // on a device the process has to itself)
  GCRL_CHECK_ARG(part != 3 || (phase == 0 && a.producers_first && !meet_device_shared()) || rowchain_merge_ok(rg, a.ldl, a.A, a.critic[0].H, a.C, a.B),
                 "rowchain split: %d workgroups of %zu bytes of LDS cannot all be resident (or the device is shared)", roles * nblk, lds);
  if (PopRec* r = pop_recording()) {   // a population step is being recorded (pop.h)
    GCRL_CHECK_ARG(!(hf && hf->on) || (a.given_next && a.p_critic_only && part != 2 && a.A <= 16), "rowchain split: the folded heads need the SAC form (given_next, critic-only actor phase)");
    RowSplitPop e;
    std::memset(&e, 0, sizeof(e));
    // (byte copies of records their builders zeroed first, padding included: the device tables are cached by content)
    std::memcpy(&e.a, &a, sizeof(a)); e.phase = phase; e.part = part;
    const bool heads = hf && hf->on;
    if (heads) std::memcpy(&e.hf, hf, sizeof(*hf));
    const int grid = roles * nblk + ((heads && phase == 0) ? (hf->cur_in_k ? nblk : (hf->run.layers ? 1 : 0)) : 0);
    return pop_record(r, heads ? POP_RC_SPLIT_HEADS : POP_RC_SPLIT, rg | (part << 4) | (phase << 8), dim3(grid), lds, &e, sizeof(e),
                      [e, rg, heads](hipStream_t s) { return launch_rowchain_split(s, e.a, rg, e.phase, e.part, heads ? &e.hf : nullptr); });
  }
  auto go = [&](auto kern) -> int {
    static thread_local size_t raised = 0;
    if (lds > 64 * 1024 && lds > raised) {
      GCRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      raised = lds;
    }
    hipLaunchKernelGGL(kern, dim3(roles * nblk), dim3(kRowThreads), lds, st, a, phase, part);
    GCRL_HIP(hipGetLastError());
    return GCRL_OK;
  };
  if (hf && hf->on) {   // the BatchNorm actor's heads and sampling inside the launch (rowchain.h HeadsFold); phase 0 carries the running-statistics workgroup
    GCRL_CHECK_ARG(a.given_next && a.p_critic_only && part != 2 && a.A <= 16, "rowchain split: the folded heads need the SAC form (given_next, critic-only actor phase)");
    const int grid = roles * nblk + (phase == 0 ? (hf->cur_in_k ? nblk : (hf->run.layers ? 1 : 0)) : 0);
    auto goh = [&](auto kern) -> int {
      static thread_local size_t raised = 0;
      if (lds > 64 * 1024 && lds > raised) {
        GCRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        raised = lds;
      }
      hipLaunchKernelGGL(kern, dim3(grid), dim3(kRowThreads), lds, st, a, phase, part, *hf);
      GCRL_HIP(hipGetLastError());
      return GCRL_OK;
    };
    if (rg == 1) return goh(rowchain_split_heads_kernel<1>);
    if (rg == 2) return goh(rowchain_split_heads_kernel<2>);
    return goh(rowchain_split_heads_kernel<4>);
  }
  if (rg == 1) return go(rowchain_split_kernel<1>);
  if (rg == 2) return go(rowchain_split_kernel<2>);
  return go(rowchain_split_kernel<4>);
}

int launch_rowchain_act(hipStream_t st, const RowActArgs& a) {
  GCRL_CHECK_ARG(a.actor.H % 4 == 0 && a.ldl % 4 == 0 && a.A <= 16 && a.n >= 1, "rowchain act: unsupported shape");
  GCRL_CHECK_ARG(!(a.nz_mean || a.nzg_mean) || 4 * a.actor.jpad0 <= 2 * kRowThreads, "rowchain act: fused normalisation supports state_dim <= 128");
  const size_t lds = (size_t)(3 * 4 * a.ldl + 2 * 4 * 4 * kRowChunk + 4 * 16 + a.A * a.actor.H + 32) * sizeof(float);
  GCRL_CHECK_ARG(lds <= 160 * 1024, "rowchain act: %zu bytes of LDS needed", lds);
  static thread_local size_t raised = 0;
  if (lds > 64 * 1024 && lds > raised) {
    GCRL_HIP(hipFuncSetAttribute((const void*)rowchain_act_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = lds;
  }
  hipLaunchKernelGGL(rowchain_act_kernel, dim3((a.n + 3) / 4), dim3(kRowThreads), lds, st, a);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int launch_rowchain_act_inline(hipStream_t st, const RowActInline& a) {
  const RowActArgs& b = a.base;
  GCRL_CHECK_ARG(b.actor.H % 4 == 0 && b.ldl % 4 == 0 && b.A <= 16 && b.n >= 1 && b.post != 0 && a.out_host && a.flag_host, "rowchain act (inline): unsupported shape");
  GCRL_CHECK_ARG(b.n * b.ld_obs <= kActInlineFloats && b.n * b.A <= kActInlineNoise, "rowchain act (inline): %d rows do not fit the kernel arguments", b.n);
  GCRL_CHECK_ARG(!(b.nz_mean || b.nzg_mean) || 4 * b.actor.jpad0 <= 2 * kRowThreads, "rowchain act: fused normalisation supports state_dim <= 128");
  const size_t lds = (size_t)(3 * 4 * b.ldl + 2 * 4 * 4 * kRowChunk + 4 * 16 + b.A * b.actor.H + 32) * sizeof(float);
  GCRL_CHECK_ARG(lds <= 160 * 1024, "rowchain act: %zu bytes of LDS needed", lds);
  static thread_local size_t raised = 0;
  if (lds > 64 * 1024 && lds > raised) {
    GCRL_HIP(hipFuncSetAttribute((const void*)rowchain_act_inline_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = lds;
  }
  hipLaunchKernelGGL(rowchain_act_inline_kernel, dim3((b.n + 3) / 4), dim3(kRowThreads), lds, st, a);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int launch_rowchain_act_pop(hipStream_t st, const RowActPop& c, int members, int n, int ldl, int A, int H) {
  GCRL_CHECK_ARG(c.tab && c.rows && c.noise && c.out && members >= 1 && members <= 32 && n >= 1 && n <= c.stride_n, "rowchain act (population): bad launch");
  GCRL_CHECK_ARG(H % 4 == 0 && ldl % 4 == 0 && A >= 1 && A <= 16, "rowchain act (population): unsupported shape");
  const size_t lds = (size_t)(3 * 4 * ldl + 2 * 4 * 4 * kRowChunk + 4 * 16 + A * H + 32) * sizeof(float);
  GCRL_CHECK_ARG(lds <= 160 * 1024, "rowchain act: %zu bytes of LDS needed", lds);
  static thread_local size_t raised = 0;
  if (lds > 64 * 1024 && lds > raised) {
    GCRL_HIP(hipFuncSetAttribute((const void*)rowchain_act_pop_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = lds;
  }
  hipLaunchKernelGGL(rowchain_act_pop_kernel, dim3((n + 3) / 4, (unsigned)members), dim3(kRowThreads), lds, st, c);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

// sub: rows per block / 4, + 16 for the LDS-multiplier form, + 32 for the stream form (the members' own launches chose them: launch_rowchain_ddpg, same shape, same LDS)
int launch_rowchain_ddpg_pop(hipStream_t st, const void* tab, int members, int sub, dim3 grid, size_t lds) {
  const int rg = sub & 15;
  const bool lm = (sub & 16) != 0, sf = (sub & 32) != 0;
  GCRL_CHECK_ARG(rg == 1 || rg == 2 || rg == 4, "rowchain population: rows per block must be 4, 8 or 16");
  GCRL_CHECK_ARG(members >= 1 && members <= 65535 && grid.y == 1 && grid.z == 1 && lds <= 160 * 1024, "rowchain population: bad launch");
  const RowChainArgs* t = static_cast<const RowChainArgs*>(tab);
  const dim3 g(grid.x, (unsigned)members);
  auto go = [&](auto kern) -> int {
    if (lds > 64 * 1024) GCRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, g, dim3(kRowThreads), lds, st, t);
    GCRL_HIP(hipGetLastError());
    return GCRL_OK;
  };
  if (sf) {
    GCRL_CHECK_ARG(rg == 1, "rowchain population: the stream form runs 4 rows per block");
    return lm ? go(rowchain_ddpg_pop_kernel_stream<true>) : go(rowchain_ddpg_pop_kernel_stream<false>);
  }
  if (lm) {
    if (rg == 1) return go(rowchain_ddpg_pop_kernel<1, true>);
    if (rg == 2) return go(rowchain_ddpg_pop_kernel<2, true>);
    return go(rowchain_ddpg_pop_kernel<4, true>);
  }
  if (rg == 1) return go(rowchain_ddpg_pop_kernel<1, false>);
  if (rg == 2) return go(rowchain_ddpg_pop_kernel<2, false>);
  return go(rowchain_ddpg_pop_kernel<4, false>);
}

int launch_rowchain_split_pop(hipStream_t st, const void* tab, int members, int sub, bool heads, dim3 grid, size_t lds) {
  const int rg = sub & 15;
  GCRL_CHECK_ARG(rg == 1 || rg == 2 || rg == 4, "rowchain split (population): rows per block must be 4, 8 or 16");
  GCRL_CHECK_ARG(tab && members >= 1 && members <= 65535 && grid.y == 1 && grid.z == 1 && lds <= 160 * 1024, "rowchain split (population): bad launch");
  const RowSplitPop* t = static_cast<const RowSplitPop*>(tab);
  const dim3 g(grid.x, (unsigned)members);
  auto go = [&](auto kern) -> int {
    static thread_local size_t raised = 0;   // (per kernel: a generic lambda's statics belong to its instantiation)
    if (lds > 64 * 1024 && lds > raised) {
      GCRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      raised = lds;
    }
    hipLaunchKernelGGL(kern, g, dim3(kRowThreads), lds, st, t);
    GCRL_HIP(hipGetLastError());
    return GCRL_OK;
  };
  if (heads) {
    if (rg == 1) return go(rowchain_split_heads_pop_kernel<1>);
    if (rg == 2) return go(rowchain_split_heads_pop_kernel<2>);
    return go(rowchain_split_heads_pop_kernel<4>);
  }
  if (rg == 1) return go(rowchain_split_pop_kernel<1>);
  if (rg == 2) return go(rowchain_split_pop_kernel<2>);
  return go(rowchain_split_pop_kernel<4>);
}

// part 3 of a population: `members` times the 2C x nblk role workgroups resident at once by the population kernels' occupancy at this LDS size
void rowchain_pop_merge_terms(int rg, int ldl, int A, int H, int C, int B, int members, long long* want, long long* cap) {
  const size_t lds = rowchain_lds_bytes(rg, ldl, A, H, C);
  *want = 0; *cap = 0;
  if (lds > 160 * 1024 || members < 1) return;
  const void* k = rg == 1 ? (const void*)rowchain_split_pop_kernel<1> : (rg == 2 ? (const void*)rowchain_split_pop_kernel<2> : (const void*)rowchain_split_pop_kernel<4>);
  const void* kh = rg == 1 ? (const void*)rowchain_split_heads_pop_kernel<1> : (rg == 2 ? (const void*)rowchain_split_heads_pop_kernel<2> : (const void*)rowchain_split_heads_pop_kernel<4>);
  if (lds > 64 * 1024 && (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
                          hipFuncSetAttribute(kh, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)) return;
  const long long nblk = (B + 4 * rg - 1) / (4 * rg);
  *want = (long long)members * 2 * C * nblk;
  *cap = std::min(meet_capacity(k, kRowThreads, lds), meet_capacity(kh, kRowThreads, lds));
}

int launch_wt_rebuild(hipStream_t st, const RowNet& net, float* Wt) {
  // a population step is being recorded (pop.h): no population form, issued member by member
  if (PopRec* r = pop_recording()) return pop_defer(r, [net, Wt](hipStream_t s) { return launch_wt_rebuild(s, net, Wt); });
  hipLaunchKernelGGL(wt_rebuild_kernel, dim3(64, net.L), dim3(256), 0, st, net, Wt);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl
