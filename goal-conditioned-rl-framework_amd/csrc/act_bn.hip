// act_bn.hip — the fused acting launch of the BatchNorm actor (act_bn.h).
//
// A workgroup of 512 threads owns 4 rows.  A layer y = x W^T reads W as stored, [out][in]: eight neighbouring lanes own one output
// column and walk its weight row in 16-byte pieces (the eight pieces of a 128-byte line in one instruction), every lane holding the
// partial sums of all 4 rows; a three-step exchange inside the eight lanes finishes the sums, and lanes 0..3 of the group apply the
// bias, the BatchNorm-eval formula and the ReLU (sac_select.h: the arithmetic of bn_relu_eval) for row 0..3 and store to LDS.  Four
// columns per lane group are in flight at once: with 8 waves that is the ~64 vector-memory instructions a CU keeps in flight
// (DESIGN.md 4e).  ActBnArgs::warm makes each pass first touch one float of every 128-byte line of the NEXT pass's weights
// (warm_lines); measured, that is slower at both benchmark shapes (52 vs 58 us per call at H = 512), so the host never sets it.
#include "act_bn.h"
#include "common.h"
#include "norm_math.h"
#include "sac_select.h"

#include <algorithm>
#include <cstdint>

namespace gcrl {
namespace {

constexpr int R = kActBnRows;
constexpr int kGroups = kActBnThreads / 8;   // lane groups = output columns per round and per unrolled column
constexpr int kHeadLd = 32;                  // floats per row of the heads' outputs (mu | log_std: 2 x action_dim <= 32)

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // a weight row starts wherever the parameter vector puts it

__device__ inline float pick4(const float (&v)[R], int r) { return r == 0 ? v[0] : (r == 1 ? v[1] : (r == 2 ? v[2] : v[3])); }

// acc[u][r] = sum_k X[r][k] * w[u][k] for the lane group's U weight rows; every lane of the group ends up with the full sums.
// V = 4: K is a multiple of 4, 16-byte pieces; V = 1: any K, one float per lane and step.
template <int V, int U>
__device__ inline void group_dots(const float* X, int ldl, int K, const float* const (&w)[U], float (&acc)[U][R]) {
  const int sub = threadIdx.x & 7;
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[u][r] = 0.f;
  if (V == 4) {
#pragma unroll 2
    for (int k = sub * 4; k < K; k += 32) {
      f4u wv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) wv[u] = *reinterpret_cast<const f4u*>(w[u] + k);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float4 x = *reinterpret_cast<const float4*>(X + r * ldl + k);
#pragma unroll
        for (int u = 0; u < U; ++u)
          acc[u][r] = fmaf(x.w, wv[u][3], fmaf(x.z, wv[u][2], fmaf(x.y, wv[u][1], fmaf(x.x, wv[u][0], acc[u][r]))));
      }
    }
  } else {
#pragma unroll 2
    for (int k = sub; k < K; k += 8) {
      float wv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) wv[u] = w[u][k];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float x = X[r * ldl + k];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u][r] = fmaf(x, wv[u], acc[u][r]);
      }
    }
  }
#pragma unroll
  for (int off = 1; off < 8; off <<= 1)
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[u][r] += __shfl_xor(acc[u][r], off, 64);
}

// one hidden block: Xout[r][j] = relu(bn_eval(X[r] . W[j] + b[j])) for j < H
template <int V>
__device__ inline void hidden_layer(const float* X, float* Xout, int ldl, int K, int H, const float* W, const float* b, const float* g,
                                    const float* be, const float* rm, const float* rv) {
  constexpr int U = 4;
  const int sub = threadIdx.x & 7, cg = threadIdx.x >> 3;
  for (int jb = 0; jb < H; jb += kGroups * U) {
    const float* w[U];
    float vb[U], vg[U], vbe[U], vrm[U], vrv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int jc = min(jb + cg + u * kGroups, H - 1);   // (groups past the last column redo it and store nothing)
      w[u] = W + (long long)jc * K;
      vb[u] = b[jc]; vg[u] = g[jc]; vbe[u] = be[jc]; vrm[u] = rm[jc]; vrv[u] = rv[jc];
    }
    float acc[U][R];
    group_dots<V, U>(X, ldl, K, w, acc);
    if (sub < R) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = jb + cg + u * kGroups;
        if (j < H) Xout[sub * ldl + j] = bn_relu_eval_elem(pick4(acc[u], sub) + vb[u], vrm[u], vrv[u], vg[u], vbe[u]);
      }
    }
  }
}

// the two heads: sm[r][j] = X[r] . Wmu[j] + bmu[j] (j < A), sm[r][A + j] = X[r] . Wls[j] + bls[j]
template <int V>
__device__ inline void heads(const float* X, float* sm, int ldl, int H, int A, const float* Wmu, const float* bmu, const float* Wls, const float* bls) {
  const int sub = threadIdx.x & 7, cg = threadIdx.x >> 3;
  for (int jb = 0; jb < 2 * A; jb += kGroups) {
    const int jc = min(jb + cg, 2 * A - 1);
    const float* w[1] = {jc < A ? Wmu + (long long)jc * H : Wls + (long long)(jc - A) * H};
    const float vb = jc < A ? bmu[jc] : bls[jc - A];
    float acc[1][R];
    group_dots<V, 1>(X, ldl, H, w, acc);
    if (sub < R && jb + cg < 2 * A) sm[sub * kHeadLd + jc] = pick4(acc[0], sub) + vb;
  }
}

// One float of every 128-byte line of P[lo, hi): the lines are on their way into the L2 when a later pass asks for them.  Sixteen
// independent loads per thread and round; their values are handed to an empty asm statement, which is what keeps the loads: the
// thread waits for a round's loads there (loads return in order, so a pass that follows waits for them as well — the touches are
// therefore issued one pass ahead and never the whole network in front of the first layer).  Regions above 4 MB are left alone.
__device__ inline void warm_lines(const float* P, long long lo, long long hi) {
  constexpr int Q = 16;
  if (hi - lo > (1LL << 20)) return;
  for (long long i0 = lo + (long long)threadIdx.x * 32; i0 < hi; i0 += (long long)Q * kActBnThreads * 32) {
    float v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const long long i = i0 + (long long)q * kActBnThreads * 32;
      v[q] = P[i < hi ? i : hi - 1];
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) asm volatile("" ::"v"(v[q]));
  }
}

// `row_at(i)`: element i of the launch's raw rows ([n][S] flattened); `eps_at(t)`: the eps of action element t — functors, so that the
// inline form reads the kernel-argument segment by plain indexed loads (a pointer into a by-value argument struct would make hipcc copy
// the struct into every thread's scratch).  SYS: the actions leave as system-scope (write-through) stores for a host that polls a flag.
template <bool SYS, typename RowAt, typename EpsAt>
__device__ inline void act_bn_body(const ActBnArgs& a, RowAt row_at, EpsAt eps_at, bool has_eps, double* out64, float* lds) {
  const int tid = threadIdx.x, S = a.S, H = a.H, L = a.L, A = a.A, ldl = a.ldl;
  float* X0 = lds;
  float* X1 = X0 + R * ldl;
  float* sm = X1 + R * ldl;
  const long long row0 = (long long)blockIdx.x * R;
  const int rv = min(R, a.n - (int)row0);
  // normalize_state_batch: the same three regimes, clip and float32 / float64 rules as the row-chain act kernel's prologue
  for (int i = tid; i < R * S; i += kActBnThreads) {
    const int r = i / S, c = i - r * S;
    float x = 0.f;
    if (r < rv) {
      x = row_at((row0 + r) * S + c);
      const bool ob = c < a.D;
      const double* m = ob ? a.nz_mean : a.nzg_mean;
      if (m) {
        const int j = ob ? c : c - a.D;
        const double* v = ob ? a.nz_var : a.nzg_var;
        const double clip = ob ? a.nz_clip : a.nzg_clip;
        const int md = ob ? a.nz_mode : a.nzg_mode;
        x = norm_apply(x, m[j], norm_den(v[j], (md & NORM_F32) != 0), clip, norm_apply_f32(md));
      }
    }
    X0[r * ldl + c] = x;
  }
  // per-layer offsets in the parameter vector (agent.hip make_net): W [H][K], b, gamma, beta; then Wmu [A][H], bmu, Wls [A][H], bls
  const long long n0 = (long long)S * H + 3LL * H, nl = (long long)H * H + 3LL * H;
  const long long head0 = n0 + (long long)(L - 1) * nl, total = head0 + 2LL * ((long long)A * H + A);
  __syncthreads();
  const float* in = X0;
  float* out = X1;
  for (int l = 0; l < L; ++l) {
    const int K = l == 0 ? S : H;
    const float* W = a.P + (l == 0 ? 0 : n0 + (long long)(l - 1) * nl);
    const float* b = W + (long long)K * H;
    const float* rm = a.rmean + (long long)l * H;
    const float* rvr = a.rvar + (long long)l * H;
    // the next pass's weights (the next hidden block, or the heads) towards this XCD's L2 while this pass streams its own
    if (a.warm) warm_lines(a.P, l == 0 ? n0 : n0 + (long long)l * nl, l + 1 < L ? n0 + (long long)(l + 1) * nl : total);
    if ((K & 3) == 0) hidden_layer<4>(in, out, ldl, K, H, W, b, b + H, b + 2 * H, rm, rvr);
    else hidden_layer<1>(in, out, ldl, K, H, W, b, b + H, b + 2 * H, rm, rvr);
    __syncthreads();
    float* t = const_cast<float*>(in); in = out; out = t;
  }
  {
    const float* Wmu = a.P + head0;
    const float* bmu = Wmu + (long long)A * H;
    const float* Wls = bmu + A;
    const float* bls = Wls + (long long)A * H;
    if ((H & 3) == 0) heads<4>(in, sm, ldl, H, A, Wmu, bmu, Wls, bls);
    else heads<1>(in, sm, ldl, H, A, Wmu, bmu, Wls, bls);
  }
  __syncthreads();
  if (tid < R * A) {
    const int r = tid / A, o = tid - r * A;
    if (r < rv) {
      const long long t = (row0 + r) * A + o;
      const float mu = sm[r * kHeadLd + o];
      // select_action (src/agent.py: eval_action -> tanh(mean), else actor.sample's action), as float64 like .cpu().numpy() upcast by the trainer
      const float act = has_eps ? tanh_gauss_elem_with([&]() { return eps_at(t); }, mu, sm[r * kHeadLd + A + o]).t : tanh_gauss_mean(mu);
      const double v = (double)act;
      if (SYS) __hip_atomic_store(out64 + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      else out64[t] = v;
    }
  }
}

__global__ __launch_bounds__(kActBnThreads) void act_bn_kernel(ActBnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  act_bn_body<false>(a, [&](long long i) { return a.rows[i]; }, [&](long long t) { return a.eps[t]; }, a.eps != nullptr, a.out64, lds);
}

// rows and eps inside the kernel arguments, actions and a completion flag per workgroup to host-visible memory (act_bn.h)
__global__ __launch_bounds__(kActBnThreads) void act_bn_inline_kernel(ActBnInline a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  act_bn_body<true>(a.base, [&](long long i) { return a.obs_inl[i]; }, [&](long long t) { return (float)a.eps_inl[t]; }, a.with_eps != 0, a.out_host, lds);
  // this workgroup's rows are out as write-through stores: drain them, then raise its flag (system scope: the host polls it)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(a.flag_host + blockIdx.x, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Population forms (act_bn.h ActBnPop): member blockIdx.y on its own arguments tab[blockIdx.y] and its own slices of the rows, the eps
// and the actions — the same body, so each member's rows go through its own arithmetic in its own order.  `a` is a COPY of the table
// entry made before anything else: uniform addresses and nothing stored yet, so the whole struct arrives by scalar loads and stays in
// scalar registers (a reference into the table left the loads behind the first barrier as vector loads: 174 vector registers against 129).
// Fast form: the block is pinned, mapped, coherent host memory — rows and eps by system-scope loads (a later call cannot read an
// earlier call's rows), actions as system-scope stores, then one flag per (member, workgroup).
__global__ __launch_bounds__(kActBnThreads) void act_bn_pop_kernel(ActBnPop c) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const unsigned int m = blockIdx.y;
  const ActBnArgs a = c.tab[m];
  const float* rows = c.rows + (size_t)m * c.stride_n * a.S;
  const double* eps = c.eps + (size_t)m * c.stride_n * a.A;
  double* out = c.out + (size_t)m * c.stride_n * a.A;
  act_bn_body<true>(a, [&](long long i) { return __hip_atomic_load(rows + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); },
                    [&](long long t) { return (float)__hip_atomic_load(eps + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); },
                    c.with_eps != 0, out, lds);
  // this workgroup's rows are out as write-through stores: drain them, then raise its flag (system scope: the host polls it)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(c.flags + (size_t)m * gridDim.x + blockIdx.x, c.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Staged form: device buffers the host entry copies into and out of — plain loads and stores, no flags.
__global__ __launch_bounds__(kActBnThreads) void act_bn_pop_staged_kernel(ActBnPop c) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const unsigned int m = blockIdx.y;
  const ActBnArgs a = c.tab[m];
  const float* rows = c.rows + (size_t)m * c.stride_n * a.S;
  const double* eps = c.eps + (size_t)m * c.stride_n * a.A;
  double* out = c.out + (size_t)m * c.stride_n * a.A;
  act_bn_body<false>(a, [&](long long i) { return rows[i]; }, [&](long long t) { return (float)eps[t]; }, c.with_eps != 0, out, lds);
}

int check_shape(const ActBnArgs& a, size_t* lds) {
  GCRL_CHECK_ARG(a.P && a.rmean && a.rvar && a.n >= 1 && a.S >= 1 && a.H >= 1 && a.L >= 1 && a.A >= 1 && a.A <= 16 && a.D >= 0 && a.D <= a.S,
                 "act_bn: unsupported shape (S=%d, H=%d, L=%d, A=%d, n=%d)", a.S, a.H, a.L, a.A, a.n);
  GCRL_CHECK_ARG(a.ldl % 4 == 0 && a.ldl >= std::max(a.S, a.H), "act_bn: LDS row of %d floats for S=%d, H=%d", a.ldl, a.S, a.H);
  *lds = (size_t)(2 * R * a.ldl + R * kHeadLd) * sizeof(float);
  GCRL_CHECK_ARG(*lds <= 160 * 1024, "act_bn: %zu bytes of LDS needed", *lds);
  return GCRL_OK;
}

}  // namespace

int launch_act_bn(hipStream_t st, const ActBnArgs& a) {
  size_t lds = 0;
  if (int rc = check_shape(a, &lds)) return rc;
  GCRL_CHECK_ARG(a.rows && a.out64, "act_bn: null rows or actions");
  static thread_local size_t raised = 0;
  if (lds > 64 * 1024 && lds > raised) {
    GCRL_HIP(hipFuncSetAttribute((const void*)act_bn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = lds;
  }
  hipLaunchKernelGGL(act_bn_kernel, dim3((a.n + R - 1) / R), dim3(kActBnThreads), lds, st, a);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int launch_act_bn_inline(hipStream_t st, const ActBnInline& a) {
  const ActBnArgs& b = a.base;
  size_t lds = 0;
  if (int rc = check_shape(b, &lds)) return rc;
  GCRL_CHECK_ARG(a.out_host && a.flag_host, "act_bn (inline): null actions or flags");
  GCRL_CHECK_ARG(b.n * b.S <= kActInlineFloats && b.n * b.A <= kActInlineNoise, "act_bn (inline): %d rows do not fit the kernel arguments", b.n);
  static thread_local size_t raised = 0;
  if (lds > 64 * 1024 && lds > raised) {
    GCRL_HIP(hipFuncSetAttribute((const void*)act_bn_inline_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = lds;
  }
  hipLaunchKernelGGL(act_bn_inline_kernel, dim3((b.n + R - 1) / R), dim3(kActBnThreads), lds, st, a);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int launch_act_bn_pop(hipStream_t st, const ActBnPop& c, const ActBnArgs& shape, int members) {
  size_t lds = 0;
  if (int rc = check_shape(shape, &lds)) return rc;   // (the members share their shapes: one check)
  GCRL_CHECK_ARG(c.tab && c.rows && c.out && (c.eps || !c.with_eps) && members >= 1 && members <= 65535 && shape.n <= c.stride_n,
                 "act_bn (population): bad launch (%d members, %d rows of %d per member)", members, shape.n, c.stride_n);
  const bool fast = c.flags != nullptr;
  static thread_local size_t raised[2] = {0, 0};
  if (lds > 64 * 1024 && lds > raised[fast]) {
    GCRL_HIP(hipFuncSetAttribute(fast ? (const void*)act_bn_pop_kernel : (const void*)act_bn_pop_staged_kernel,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised[fast] = lds;
  }
  const dim3 grid((shape.n + R - 1) / R, (unsigned)members);
  if (fast) hipLaunchKernelGGL(act_bn_pop_kernel, grid, dim3(kActBnThreads), lds, st, c);
  else hipLaunchKernelGGL(act_bn_pop_staged_kernel, grid, dim3(kActBnThreads), lds, st, c);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl
