// her_nstep.hip — n-step returns for a ring in sample-time relabelling mode (gcrl_her_set_nstep, n_step = N in 2..8): gathers
// that fold the next m - 1 transitions of a drawn row into its reward and its done flag while the batch is assembled.  They rest
// on her_ring.h's invariant (an episode's rows lie contiguously, in step order, and `remaining` counts the ones that follow).
// The rule is restated in numpy in tests/her_nstep_ref.py, which is its definition; for row p, with f as her_relabel.hip picks it:
//     m = min(N, rem + 1)   last = p + m - 1   s, a <- record p   ns <- record last   (goal slots <- ag[p + f] when f > 0)
//     r_j (j < m) = f > 0 ? reward(ag[p + j], ag[p + f]) : r[p + j]        d_last = f > 0 ? 0 : d[last]
//     r <- r_0 + g (r_1 + g (.. r_{m-1}))     d <- m == 1 ? d_last : 1 - g^(m-1) (1 - d_last)       (fp32, one rounding per operation)
// Every TD site forms y = r + g (1 - d) q' with d read as a float, so the engine's kernels take the n-step target
// R + g^m (1 - d_last) q' from these two outputs unchanged.
//
// A translation unit of its own: the kernels of her_ring.hip and her_relabel.hip keep their code, byte for byte; a ring with
// n_step == 1 keeps launching them.
#include "her_ring.h"

#include <algorithm>

namespace {

constexpr int kMaxG = 8;
constexpr int kMaxN = 8;            // n_step <= 8: the (row, step) pairs of a wave's 16 rows are at most two per lane
constexpr int kTailW = 12;          // floats of a record from o_r on that the gather keeps: r, d, ag (<= 8), remaining

// the relabel decision, as her_relabel.hip takes it (that unit is left as it is; tests/her_relabel_ref.py defines both)
struct NstepRule {
  unsigned long long seed, ctr;   // ctr: rows gathered from this ring in sample mode before the launch's row 0
  int k, rem_max;                 // rem_max = min(flush_len, cap) - 1: every address formed stays inside the ring whatever a tail holds
  int reward_kind;
  float thr;
  int N;                          // n_step
  float g32;                      // float32(gamma)
};

__device__ inline int clamp_rem(const NstepRule& q, float rem_f) {
  return (int)fminf(fmaxf(rem_f, 0.f), (float)q.rem_max);   // [0, rem_max] whatever the tail holds (NaN -> 0)
}

// clamped remaining -> future offset f in [1, rem], or 0: the row stays as stored
__device__ inline int nstep_pick(const NstepRule& q, long long row, int rem) {
  if (rem <= 0) return 0;
  const unsigned long long c = q.ctr + (unsigned long long)row;
  if (gcrl::hash_below(q.seed, gcrl::kRelabelStream, 2ull * c, (uint32_t)(q.k + 1)) == 0) return 0;
  return 1 + (int)gcrl::hash_below(q.seed, gcrl::kRelabelStream, 2ull * c + 1ull, (uint32_t)rem);
}

__device__ inline uint32_t wrap_slot(uint32_t slot, int off, long long cap) {   // slot < cap, 0 <= off < cap
  unsigned long long x = (unsigned long long)slot + (unsigned long long)off;
  if (x >= (unsigned long long)cap) x -= (unsigned long long)cap;
  return (uint32_t)x;
}

// compute_reward(ag_i, ag_f): -||ag_i - ag_f||_2 or its threshold, fp32, one rounding per operation (her_flush_kernel's arithmetic)
__device__ inline float goal_reward(const NstepRule& q, const float* ag_i, const float* ag_f, int G) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxG; ++c)
    if (c < G) { const float df = __fsub_rn(ag_i[c], ag_f[c]); acc = __fadd_rn(acc, __fmul_rn(df, df)); }
  const float dist = sqrtf(acc);
  return (q.reward_kind == GCRL_REWARD_SPARSE) ? ((dist > q.thr) ? -1.0f : -0.0f) : -dist;
}

// d' of a window of m rows that ends on d_last
__device__ inline float fold_done(float d_last, int m, float g32) {
  if (m <= 1) return d_last;                      // bit for bit
  float gp = 1.0f;
  for (int i = 1; i < m; ++i) gp = __fmul_rn(gp, g32);
  return __fsub_rn(1.0f, __fmul_rn(gp, __fsub_rn(1.0f, d_last)));
}

// ---------------------------------------------------------------- gather (update engine)
struct GatherNstepArgs {
  const float* ring;
  const uint32_t* idx;   // null: computed per row from `gen`
  gcrl::IdxGen gen;
  long long n, head, cap;
  int SA4, S4, RS, ldx;   // ldx == SA4
  float *sa, *nsa, *spa, *r, *d;
  const uint4* cp_src; uint4* cp_dst; int cp_n16;
  int S, G;
  NstepRule rule;
};

typedef float gcrl_f4 __attribute__((ext_vector_type(4)));
__device__ inline void store4_nt(float* p, float4 v) {
  gcrl_f4 t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<gcrl_f4*>(p));
}

// her_gather_relabel_kernel's shape (her_relabel.hip) with a second round of loads.  One wave owns 16 consecutive batch rows:
//   (1) 16 indices in one coalesced load (or the keyed permutation per lane), ring wrap by compare-and-subtract;
//   (2) all 16 records in flight, 16 lanes x 16 B per record, up to the quad that holds `remaining`; they land in the wave-private
//       LDS tile [sa 16 x SA4 | nsa 16 x SA4 | r 16 | d 16 | tails 16 x (N + 1) x 12]; slot 0 of a row's tails is its own
//       (the record from o_r on: r, d, ag, remaining);
//   (3) lane l < 16 decides row l: f by the counter hash, m = min(N, rem + 1), last = p + m - 1; the wave reads them by __shfl;
//   (4) the second round, issued by all 64 lanes and in flight as a whole before anything of it is consumed: the ns group of record
//       `last` of every row with m > 1 (16 lanes x 16 B per record, over the tile's nsa rows) and the tails [r, d, ag] of rows
//       p + 1 .. p + m - 1 (slots 1 .. m - 1) and of p + f (slot N), one to three 16-byte loads each, the (row, slot) pairs spread
//       over the lanes: at most 8 + 6 loads per lane;
//   (5) lane l < 16 folds its row's rewards by Horner's rule from the last one, folds d, patches the goal slots in the tile, and
//   (6) the tile leaves as contiguous 16-byte non-temporal stores.  The launch's last, partial wave takes the same path with its
//       stores guarded by row.
// Every slot formed is p + an offset <= rem_max < cap brought back into the ring by compare-and-subtract.  The tile is private to
// the wave and a wave's LDS operations execute in order: no barrier between the stages, only the compiler is held back.  No waits
// between workgroups, no atomics, no per-thread scratch (the per-step values live in the tile).
template <bool kHead>
__global__ __launch_bounds__(256) void her_gather_nstep_kernel(GatherNstepArgs p) {
  extern __shared__ float nstep_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane >> 4, v4 = lane & 15;
  if (kHead)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.cp_n16; i += gridDim.x * 256) p.cp_dst[i] = p.cp_src[i];
  const int SA4 = p.SA4, S4 = p.S4, o_r = SA4 + S4, G = p.G, N = p.rule.N;
  const int o_last = o_r + ((2 + G) & ~3);                  // the quad that holds `remaining` (column o_r + 2 + G)
  const int nq = 4 * SA4;                                   // 16-byte quads of a [16][SA4] tile
  const int tw = (N + 1) * kTailW;                          // floats of one row's tails
  float* tile = nstep_lds + (size_t)w * (8 * nq + 32 + 16 * tw);
  float* t_ns = tile + 4 * nq;
  float* t_rd = tile + 8 * nq;
  float* t_tail = t_rd + 32;
  const long long r0 = ((long long)blockIdx.x * 4 + w) * 16;
  if (r0 >= p.n) return;
  uint32_t ph32 = 0;
  if (lane < 16 && r0 + lane < p.n) {
    unsigned long long phys = (unsigned long long)p.head + (p.idx ? p.idx[r0 + lane] : gcrl::idxgen_at(p.gen, r0 + lane));
    if (phys >= (unsigned long long)p.cap) phys -= (unsigned long long)p.cap;    // head, index < cap
    ph32 = (uint32_t)phys;
  }
  const bool full = r0 + 16 <= p.n;
  for (int cc = 0; cc <= o_last; cc += 64) {
    const int c0 = cc + v4 * 4;
    const bool useful = c0 <= o_last;
    float4 val[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t ph = __shfl(ph32, u * 4 + sub, 64);
      val[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (useful && r0 + u * 4 + sub < p.n) val[u] = *reinterpret_cast<const float4*>(p.ring + (size_t)ph * p.RS + c0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int rl = u * 4 + sub;
      if (!useful) continue;
      if (c0 < SA4) *reinterpret_cast<float4*>(tile + rl * SA4 + c0) = val[u];
      else if (c0 < o_r) *reinterpret_cast<float4*>(t_ns + rl * SA4 + (c0 - SA4)) = val[u];
      else *reinterpret_cast<float4*>(t_tail + rl * tw + (c0 - o_r)) = val[u];
    }
  }
  const int zq = (SA4 - S4) >> 2;          // quads of an nsa row beyond the record's ns group
  if (v4 < zq) {
#pragma unroll
    for (int u = 0; u < 4; ++u) *reinterpret_cast<float4*>(t_ns + (u * 4 + sub) * SA4 + S4 + v4 * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __builtin_amdgcn_wave_barrier();
  // ---- (3) the decision: lane l < 16 owns row l (a row past the launch's end: f = 0, m = 1, nothing further is loaded for it)
  int f = 0, m = 1;
  uint32_t last32 = ph32, fut32 = ph32;
  if (lane < 16 && r0 + lane < p.n) {
    const int rem = clamp_rem(p.rule, t_tail[lane * tw + 2 + G]);
    f = nstep_pick(p.rule, r0 + lane, rem);
    m = min(N, rem + 1);
    last32 = wrap_slot(ph32, m - 1, p.cap);
    fut32 = wrap_slot(ph32, f, p.cap);
  }
  // ---- (4) the second round of loads
  float4 nv[2][4];
  bool nuse[2][4];
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {          // S4 <= 128 (the host refuses wider rows: the tile would not fit)
    const int c0 = SA4 + ps * 64 + v4 * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t ls = __shfl(last32, u * 4 + sub, 64);
      const int mm = __shfl(m, u * 4 + sub, 64);
      nuse[ps][u] = c0 < o_r && mm > 1;
      nv[ps][u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (nuse[ps][u]) nv[ps][u] = *reinterpret_cast<const float4*>(p.ring + (size_t)ls * p.RS + c0);
    }
  }
  const uint32_t ph_b = __shfl(ph32, v4, 64), fut_b = __shfl(fut32, v4, 64);   // this lane's tail pairs belong to row v4
  const int f_b = __shfl(f, v4, 64), m_b = __shfl(m, v4, 64);
  float4 tv[2][3];
  bool tuse[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int j = 1 + sub + 4 * t;          // tail slot 1 .. 8: j < N is row p + j, j == N the future row
    tuse[t] = j < N ? j < m_b : (j == N && f_b > 0);
    const uint32_t slot = j < N ? wrap_slot(ph_b, tuse[t] ? j : 0, p.cap) : fut_b;
    const float* src = p.ring + (size_t)slot * p.RS + o_r;                    // (16-byte aligned: o_r and RS are multiples of 4)
    tv[t][0] = tv[t][1] = tv[t][2] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tuse[t]) {
      tv[t][0] = *reinterpret_cast<const float4*>(src);
      if (G > 2) tv[t][1] = *reinterpret_cast<const float4*>(src + 4);        // o_r + 7 < RS
      if (G > 6) tv[t][2] = *reinterpret_cast<const float4*>(src + 8);        // o_r + 11 < RS
    }
  }
#pragma unroll
  for (int ps = 0; ps < 2; ++ps)
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (nuse[ps][u]) *reinterpret_cast<float4*>(t_ns + (u * 4 + sub) * SA4 + ps * 64 + v4 * 4) = nv[ps][u];
#pragma unroll
  for (int t = 0; t < 2; ++t)
    if (tuse[t]) {
      float* dst = t_tail + v4 * tw + (1 + sub + 4 * t) * kTailW;
      *reinterpret_cast<float4*>(dst) = tv[t][0];
      *reinterpret_cast<float4*>(dst + 4) = tv[t][1];
      *reinterpret_cast<float4*>(dst + 8) = tv[t][2];
    }
  __builtin_amdgcn_wave_barrier();
  // ---- (5) the fold and the patch: lane l < 16 owns row l
  if (lane < 16) {
    const float* tl = t_tail + lane * tw;
    const float* fa = tl + N * kTailW + 2;              // the future row's achieved goal (read when f > 0 only)
    float acc = 0.f;
    for (int j = m - 1; j >= 0; --j) {
      const float* tj = tl + j * kTailW;
      const float rj = f > 0 ? goal_reward(p.rule, tj + 2, fa, G) : tj[0];
      acc = j == m - 1 ? rj : __fadd_rn(rj, __fmul_rn(p.rule.g32, acc));
    }
    const float d_last = f > 0 ? 0.f : tl[(m - 1) * kTailW + 1];
    if (f > 0) {
      float* gs = tile + lane * SA4 + (p.S - G);
      float* gn = t_ns + lane * SA4 + (p.S - G);
#pragma unroll
      for (int q = 0; q < kMaxG; ++q)
        if (q < G) { const float x = fa[q]; gs[q] = x; gn[q] = x; }
    }
    t_rd[lane] = acc;
    t_rd[16 + lane] = fold_done(d_last, m, p.rule.g32);
  }
  __builtin_amdgcn_wave_barrier();
  // ---- (6) stores
  float* sa = p.sa + r0 * p.ldx;
  float* nsa = p.nsa + r0 * p.ldx;
  const int rows = full ? 16 : (int)(p.n - r0);
  if (p.spa) {                              // layer-per-launch schedules only: spa = [s | ..], the S4 leading columns of the sa row
    const int sq = S4 >> 2;
    for (int q = lane; q < rows * sq; q += 64) {
      const int rl = q / sq, cq = q - rl * sq;
      *reinterpret_cast<float4*>(p.spa + (r0 + rl) * p.ldx + cq * 4) = *reinterpret_cast<const float4*>(tile + rl * SA4 + cq * 4);
    }
  }
  if (full) {
    const bool rd_vec = ((reinterpret_cast<size_t>(p.r) | reinterpret_cast<size_t>(p.d)) & 15) == 0;
    const int Q = 2 * nq + (rd_vec ? 8 : 0);
    for (int q = lane; q < Q; q += 64) {
      const float4 v = *reinterpret_cast<const float4*>(tile + q * 4);
      float* dst = q < nq ? sa + q * 4 : q < 2 * nq ? nsa + (q - nq) * 4 : q < 2 * nq + 4 ? p.r + r0 + (q - 2 * nq) * 4 : p.d + r0 + (q - 2 * nq - 4) * 4;
      store4_nt(dst, v);
    }
    if (!rd_vec && lane < 32) (lane < 16 ? p.r : p.d)[r0 + (lane & 15)] = t_rd[lane];
  } else {
    const int rq = rows * (SA4 >> 2);       // quads of the live rows of one matrix (rows are contiguous in the tile and in memory)
    for (int q = lane; q < 2 * rq; q += 64) {
      const bool second = q >= rq;
      const int qq = second ? q - rq : q;
      const float4 v = *reinterpret_cast<const float4*>((second ? t_ns : tile) + qq * 4);
      store4_nt((second ? nsa : sa) + qq * 4, v);
    }
    if (lane < 32 && (lane & 15) < rows) (lane < 16 ? p.r : p.d)[r0 + (lane & 15)] = t_rd[lane];
  }
}

// ---------------------------------------------------------------- gather (public sample): five dense outputs
struct GatherNstepPubArgs {
  const float* ring;
  const uint32_t* idx;
  gcrl::IdxGen gen;
  long long n, head, cap;
  int S, A, G, SA4, S4, RS;
  float *out_s, *out_a, *out_r, *out_ns, *out_d;
  int ld_s, ld_a, ld_ns;
  NstepRule rule;
};

// a 16-lane group per row, 16 rows per block per pass; every lane of a group takes the row's decision and folds its window
// itself (the same addresses: one fetch) and routes its columns to the outputs.  Not a hot path: any record width, no LDS.
__global__ __launch_bounds__(256) void her_gather_nstep_pub_kernel(GatherNstepPubArgs p) {
  const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
  const int o_ns = p.SA4, o_r = p.SA4 + p.S4, RW = o_r + 2, G = p.G, S = p.S;
  for (long long row = (long long)blockIdx.x * 16 + grp; row < p.n; row += (long long)gridDim.x * 16) {
    unsigned long long phys = (unsigned long long)p.head + (p.idx ? p.idx[row] : gcrl::idxgen_at(p.gen, row));
    if (phys >= (unsigned long long)p.cap) phys %= (unsigned long long)p.cap;
    const uint32_t ph = (uint32_t)phys;
    const float* rec = p.ring + (size_t)ph * p.RS;
    const int rem = clamp_rem(p.rule, rec[RW + G]);
    const int f = nstep_pick(p.rule, row, rem);
    const int m = min(p.rule.N, rem + 1);
    const float* recl = p.ring + (size_t)wrap_slot(ph, m - 1, p.cap) * p.RS;
    const float* recf = p.ring + (size_t)wrap_slot(ph, f, p.cap) * p.RS;
    float acc = 0.f;
    for (int j = m - 1; j >= 0; --j) {
      const float* rj_rec = p.ring + (size_t)wrap_slot(ph, j, p.cap) * p.RS;
      float rj = rj_rec[o_r];
      if (f > 0) {
        float s2 = 0.f;
        for (int q = 0; q < G; ++q) { const float df = __fsub_rn(rj_rec[RW + q], recf[RW + q]); s2 = __fadd_rn(s2, __fmul_rn(df, df)); }
        const float dist = sqrtf(s2);
        rj = (p.rule.reward_kind == GCRL_REWARD_SPARSE) ? ((dist > p.rule.thr) ? -1.0f : -0.0f) : -dist;
      }
      acc = j == m - 1 ? rj : __fadd_rn(rj, __fmul_rn(p.rule.g32, acc));
    }
    const float done = fold_done(f > 0 ? 0.f : recl[o_r + 1], m, p.rule.g32);
    for (int c = gl; c < RW; c += 16) {
      if (c < S) {
        float v = rec[c];
        if (f > 0 && c >= S - G) v = recf[RW + (c - (S - G))];
        p.out_s[row * p.ld_s + c] = v;
      } else if (c < S + p.A) p.out_a[row * p.ld_a + (c - S)] = rec[c];
      else if (c >= o_ns && c < o_ns + S) {
        const int cn = c - o_ns;
        float v = recl[c];
        if (f > 0 && cn >= S - G) v = recf[RW + (cn - (S - G))];
        p.out_ns[row * p.ld_ns + cn] = v;
      } else if (c == o_r) p.out_r[row] = acc;
      else if (c == o_r + 1) p.out_d[row] = done;
    }
  }
}

NstepRule make_rule(const gcrl_her* h, uint64_t ctr, float g32) {
  NstepRule q;
  q.seed = h->cfg.seed;
  q.ctr = ctr;
  q.k = h->cfg.k_future;
  q.rem_max = (int)std::min<int64_t>(h->cfg.flush_len, h->cfg.capacity) - 1;
  q.reward_kind = h->cfg.reward_kind;
  q.thr = h->cfg.reward_threshold;
  q.N = h->n_step;
  q.g32 = g32;
  return q;
}

}  // namespace

namespace gcrl {

int her_nstep_gather_update(gcrl_her* h, const uint32_t* idx, uint64_t ctr, float g32, int64_t n, float* sa, float* nsa, float* spa, int ldx,
                            float* r, float* d, hipStream_t st, const void* cp_src, void* cp_dst, size_t cp_bytes) {
  if (h->goal_strategy != GCRL_GOAL_FUTURE)   // final / episode: her_strategy.hip
    return her_goal_gather_update(h, idx, ctr, g32, n, sa, nsa, spa, ldx, r, d, st, cp_src, cp_dst, cp_bytes);
  if (h->n_step < 2 || h->n_step > kMaxN) return fail(GCRL_ERR_STATE, "her_gather_update: n_step: %d outside 2..%d for the n-step gather", h->n_step, kMaxN);
  GatherNstepArgs ga{h->ring, idx, h->last_gen, n, h->head, h->cfg.capacity, h->SA4, h->S4, h->RS, ldx, sa, nsa, spa, r, d,
                     (const uint4*)cp_src, (uint4*)cp_dst, (int)(cp_bytes / 16), h->S, h->G, make_rule(h, ctr, g32)};
  const int blocks = (int)((n + 63) / 64);
  const size_t lds = 4 * ((size_t)32 * h->SA4 + 32 + 16 * (size_t)(h->n_step + 1) * kTailW) * sizeof(float);
  if (lds > 64 * 1024 || h->S4 > 128)
    return fail(GCRL_ERR_ARG, "her_gather_update: n_step: a batch row of %d floats with the tails of n_step = %d does not fit the gather's tile", h->SA4, h->n_step);
  if (cp_bytes) hipLaunchKernelGGL(her_gather_nstep_kernel<true>, dim3(blocks), dim3(256), lds, st, ga);
  else hipLaunchKernelGGL(her_gather_nstep_kernel<false>, dim3(blocks), dim3(256), lds, st, ga);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int her_nstep_sample(gcrl_her* h, const uint32_t* idx_dev, uint64_t ctr, float g32, int64_t n, float* out_s, int ld_s, float* out_a, int ld_a,
                     float* out_r, float* out_ns, int ld_ns, float* out_d, hipStream_t st) {
  if (h->goal_strategy != GCRL_GOAL_FUTURE) return her_goal_sample(h, idx_dev, ctr, g32, n, out_s, ld_s, out_a, ld_a, out_r, out_ns, ld_ns, out_d, st);
  if (h->n_step < 2 || h->n_step > kMaxN) return fail(GCRL_ERR_STATE, "gcrl_her_sample: n_step: %d outside 2..%d for the n-step gather", h->n_step, kMaxN);
  GatherNstepPubArgs ga{h->ring, idx_dev, h->last_gen, (long long)n, h->head, h->cfg.capacity, h->S, h->A, h->G, h->SA4, h->S4, h->RS,
                        out_s, out_a, out_r, out_ns, out_d, ld_s, ld_a, ld_ns, make_rule(h, ctr, g32)};
  const int blocks = (int)std::min<long long>((n + 15) / 16, 8192);
  hipLaunchKernelGGL(her_gather_nstep_pub_kernel, dim3(blocks), dim3(256), 0, st, ga);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl

extern "C" {

int gcrl_her_set_nstep(gcrl_her* h, int n_step, double gamma) {
  GCRL_CHECK_ARG(h, "gcrl_her_set_nstep: null handle");
  GCRL_CHECK_ARG(n_step >= 1 && n_step <= kMaxN, "gcrl_her_set_nstep: n_step: %d outside 1..%d", n_step, kMaxN);
  if (n_step > 1 && h->relabel_mode != GCRL_RELABEL_SAMPLE)
    return gcrl::fail(GCRL_ERR_STATE, "gcrl_her_set_nstep: n_step: %d-step returns are formed by the sample-time relabelling gather; this ring was "
                                      "created with GCRL_RELABEL_PUSH", n_step);
  h->n_step = n_step;
  h->nstep_gamma = gamma;
  return GCRL_OK;
}

int gcrl_her_get_nstep(const gcrl_her* h, double* gamma) {
  if (!h) return -1;
  if (gamma) *gamma = h->nstep_gamma;
  return h->n_step;
}

}  // extern "C"
