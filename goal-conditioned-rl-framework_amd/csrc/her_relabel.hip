// her_relabel.hip — the ring's sample-time relabelling mode (relabel = "sample", GCRL_RELABEL_SAMPLE): a flush that stores an
// episode's T original rows once, each with a tail [ag (G) | remaining], and gathers that relabel a drawn row against a later row
// of its episode while the batch is assembled.  Layout, the contiguity invariant the gathers rest on and the relabel rule:
// her_ring.h.  The rule is restated in numpy in tests/her_relabel_ref.py, which is its definition.
//
// A translation unit of its own: the kernels of her_ring.hip (the default mode) keep their code, byte for byte.
#include "her_ring.h"
#include "ring_book.h"

#include <algorithm>

namespace {

constexpr int kMaxG = 8;
constexpr int kMaxEp = 8;           // episodes per flush launch (as her_ring.hip)
constexpr int kFlushRows = 16;      // rows per block of the flush
constexpr int kTailW = 12;          // floats of a record from o_r on that the gather keeps per row: r, d, ag (<= 8), remaining

// ---------------------------------------------------------------- flush: T staged records -> T ring records
struct FlushSampleArgs {
  float* ring;
  long long cap, tail, skip;      // rows whose running number is < skip fell off a too-small ring
  int nep, RG, RS, RW, G;
  const float* stage[kMaxEp];
  int T[kMaxEp];
};

// grid.x = ceil(longest episode / 16), grid.y = episode; a 16-lane group copies one staged record into its ring slot as full
// 16-byte stores: the leading RW floats and ag as staged, `remaining` = T - 1 - i behind them, zeros up to RS.  Same exclusive
// scan over the episodes' row counts, the same skip / tail / cap rules as her_flush_kernel.  No future pick is drawn.
__global__ __launch_bounds__(256) void her_flush_sample_kernel(FlushSampleArgs p) {
  __shared__ long long base_lds;
  const int e = blockIdx.y;
  const int T = p.T[e];
  const int n0 = blockIdx.x * kFlushRows;
  if (n0 >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 64) {
    long long rows = lane < p.nep ? (long long)p.T[lane] : 0;
    long long incl = rows;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      long long up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == e) base_lds = incl - rows;
  }
  __syncthreads();
  const int grp = tid >> 4, gl = tid & 15;
  const int i = n0 + grp;
  if (i >= T) return;
  const long long g = base_lds + i;
  if (g < p.skip) return;
  long long phys = p.tail + g;
  if (phys >= p.cap) phys -= p.cap;
  if (phys >= p.cap) phys %= p.cap;           // (a ring smaller than the flush)
  const float* rec = p.stage[e] + (long long)i * p.RG;
  float* out = p.ring + phys * p.RS;
  const int o_rem = p.RW + p.G;
  const float rem = (float)(T - 1 - i);
#pragma unroll
  for (int j = 0; j < 3; ++j) {               // RS <= 176 floats
    const int c4 = 64 * j + 4 * gl;
    if (c4 >= p.RS) continue;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < p.RG) v = *reinterpret_cast<const float4*>(rec + c4);
    float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c4 + u;
      x[u] = c == o_rem ? rem : (c > o_rem ? 0.f : x[u]);
    }
    *reinterpret_cast<float4*>(out + c4) = make_float4(x[0], x[1], x[2], x[3]);
  }
}

// ---------------------------------------------------------------- the relabel decision of one gathered row
struct RelabelRule {
  unsigned long long seed, ctr;   // ctr: rows gathered from this ring in this mode before the launch's row 0
  int k, rem_max;                 // rem_max = min(flush_len, cap) - 1: every address formed stays inside the ring whatever a tail holds
  int reward_kind;
  float thr;
};

// remaining (as stored) -> future offset f in [1, rem], or 0: the row stays as stored
__device__ inline int relabel_pick(const RelabelRule& q, long long row, float rem_f) {
  const int rem = (int)fminf(fmaxf(rem_f, 0.f), (float)q.rem_max);   // clamped to [0, rem_max] whatever the tail holds (NaN -> 0)
  if (rem <= 0) return 0;
  const unsigned long long c = q.ctr + (unsigned long long)row;
  if (gcrl::hash_below(q.seed, gcrl::kRelabelStream, 2ull * c, (uint32_t)(q.k + 1)) == 0) return 0;
  return 1 + (int)gcrl::hash_below(q.seed, gcrl::kRelabelStream, 2ull * c + 1ull, (uint32_t)rem);
}

// ---------------------------------------------------------------- gather (update engine)
struct GatherRelArgs {
  const float* ring;
  const uint32_t* idx;   // null: computed per row from `gen`
  gcrl::IdxGen gen;
  long long n, head, cap;
  int SA4, S4, RS, ldx;   // ldx == SA4
  float *sa, *nsa, *spa, *r, *d;
  const uint4* cp_src; uint4* cp_dst; int cp_n16;
  int S, G;
  RelabelRule rule;
};

typedef float gcrl_f4 __attribute__((ext_vector_type(4)));
__device__ inline void store4_nt(float* p, float4 v) {
  gcrl_f4 t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<gcrl_f4*>(p));
}

// her_gather_update_kernel's shape (her_ring.hip) with a patch stage.  One wave owns 16 consecutive batch rows:
//   (1) 16 indices in one coalesced load (or the keyed permutation per lane), ring wrap by compare-and-subtract;
//   (2) all 16 records in flight, 16 lanes x 16 B per record, now up to the quad that holds `remaining`; they land in the
//       wave-private LDS tile [sa 16 x SA4 | nsa 16 x SA4 | r 16 | d 16 | tail 16 x 12] (tail = the record from o_r on:
//       r, d, ag, remaining);
//   (3) lane l < 16 decides row l (counter hash of c = ctr + row), and the 16 future tails are ONE further round of loads, one
//       to three 16-byte loads per relabelled row; the future slot is phys + f brought back into the ring by compare-and-subtract
//       (f <= rem_max < cap);
//   (4) the lane patches its row in the tile — the goal slot of s and of ns, r by her_flush_kernel's arithmetic, d = 0 — and
//   (5) the tile leaves as contiguous 16-byte non-temporal stores.  The launch's last, partial wave takes the same path with its
//       stores guarded by row.
// The tile is private to the wave and a wave's LDS operations execute in order: no barrier between the stages, only the compiler
// is held back.  No waits between workgroups, no atomics, no per-thread scratch.
template <bool kHead>
__global__ __launch_bounds__(256) void her_gather_relabel_kernel(GatherRelArgs p) {
  extern __shared__ float gather_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane >> 4, v4 = lane & 15;
  if (kHead)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.cp_n16; i += gridDim.x * 256) p.cp_dst[i] = p.cp_src[i];
  const int SA4 = p.SA4, S4 = p.S4, o_r = SA4 + S4, G = p.G;
  const int o_last = o_r + ((2 + G) & ~3);                  // the quad that holds `remaining` (column o_r + 2 + G)
  const int nq = 4 * SA4;                                   // 16-byte quads of a [16][SA4] tile
  float* tile = gather_lds + (size_t)w * (8 * nq + 32 + 16 * kTailW);
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
      else *reinterpret_cast<float4*>(t_tail + rl * kTailW + (c0 - o_r)) = val[u];
    }
  }
  const int zq = (SA4 - S4) >> 2;          // quads of an nsa row beyond the record's ns group
  if (v4 < zq) {
#pragma unroll
    for (int u = 0; u < 4; ++u) *reinterpret_cast<float4*>(t_ns + (u * 4 + sub) * SA4 + S4 + v4 * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __builtin_amdgcn_wave_barrier();
  // ---- the patch stage: lane l < 16 owns row l
  if (lane < 16) {
    const float* tl = t_tail + lane * kTailW;
    float rew = tl[0], done = tl[1];
    const int f = r0 + lane < p.n ? relabel_pick(p.rule, r0 + lane, tl[2 + G]) : 0;
    if (f > 0) {
      unsigned long long fut = (unsigned long long)ph32 + (unsigned long long)f;
      if (fut >= (unsigned long long)p.cap) fut -= (unsigned long long)p.cap;
      const float* src = p.ring + (size_t)fut * p.RS + o_r;           // (16-byte aligned: o_r and RS are multiples of 4)
      float af[kTailW];
      const float4 q0 = *reinterpret_cast<const float4*>(src);
      float4 q1 = make_float4(0.f, 0.f, 0.f, 0.f), q2 = q1;
      if (G > 2) q1 = *reinterpret_cast<const float4*>(src + 4);       // o_r + 7 < RS
      if (G > 6) q2 = *reinterpret_cast<const float4*>(src + 8);       // o_r + 11 < RS
      af[0] = q0.x; af[1] = q0.y; af[2] = q0.z; af[3] = q0.w; af[4] = q1.x; af[5] = q1.y; af[6] = q1.z; af[7] = q1.w;
      af[8] = q2.x; af[9] = q2.y; af[10] = q2.z; af[11] = q2.w;
      float a_i[kMaxG];
#pragma unroll
      for (int q = 0; q < kMaxG; ++q) a_i[q] = q < G ? tl[2 + q] : 0.f;
      // compute_reward(ag_i, ag_f): d = ||ag_i - ag_f||_2 in fp32, one rounding per op (her_flush_kernel's arithmetic)
      float acc = 0.f;
#pragma unroll
      for (int q = 0; q < kMaxG; ++q)
        if (q < G) { const float df = __fsub_rn(a_i[q], af[2 + q]); acc = __fadd_rn(acc, __fmul_rn(df, df)); }
      const float dist = sqrtf(acc);
      rew = (p.rule.reward_kind == GCRL_REWARD_SPARSE) ? ((dist > p.rule.thr) ? -1.0f : -0.0f) : -dist;
      done = 0.f;
      float* gs = tile + lane * SA4 + (p.S - G);
      float* gn = t_ns + lane * SA4 + (p.S - G);
#pragma unroll
      for (int q = 0; q < kMaxG; ++q)
        if (q < G) { gs[q] = af[2 + q]; gn[q] = af[2 + q]; }
    }
    t_rd[lane] = rew;
    t_rd[16 + lane] = done;
  }
  __builtin_amdgcn_wave_barrier();
  // ---- stores
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
struct GatherRelPubArgs {
  const float* ring;
  const uint32_t* idx;
  gcrl::IdxGen gen;
  long long n, head, cap;
  int S, A, G, SA4, S4, RS;
  float *out_s, *out_a, *out_r, *out_ns, *out_d;
  int ld_s, ld_a, ld_ns;
  RelabelRule rule;
};

// a 16-lane group per row, 16 rows per block per pass; every lane of a group takes the row's decision itself (the same
// addresses: one fetch) and routes its columns to the outputs.  Not a hot path: any record width, no LDS.
__global__ __launch_bounds__(256) void her_gather_relabel_pub_kernel(GatherRelPubArgs p) {
  const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
  const int o_ns = p.SA4, o_r = p.SA4 + p.S4, RW = o_r + 2, G = p.G, S = p.S;
  for (long long row = (long long)blockIdx.x * 16 + grp; row < p.n; row += (long long)gridDim.x * 16) {
    unsigned long long phys = (unsigned long long)p.head + (p.idx ? p.idx[row] : gcrl::idxgen_at(p.gen, row));
    if (phys >= (unsigned long long)p.cap) phys %= (unsigned long long)p.cap;
    const float* rec = p.ring + (size_t)phys * p.RS;
    const int f = relabel_pick(p.rule, row, rec[RW + G]);
    unsigned long long fut = phys + (unsigned long long)f;
    if (fut >= (unsigned long long)p.cap) fut -= (unsigned long long)p.cap;
    const float* recf = p.ring + (size_t)fut * p.RS;
    float rew = rec[o_r], done = rec[o_r + 1];
    if (f > 0) {
      float acc = 0.f;
      for (int q = 0; q < G; ++q) { const float df = __fsub_rn(rec[RW + q], recf[RW + q]); acc = __fadd_rn(acc, __fmul_rn(df, df)); }
      const float dist = sqrtf(acc);
      rew = (p.rule.reward_kind == GCRL_REWARD_SPARSE) ? ((dist > p.rule.thr) ? -1.0f : -0.0f) : -dist;
      done = 0.f;
    }
    for (int c = gl; c < RW; c += 16) {
      float v = rec[c];
      if (c < S) {
        if (f > 0 && c >= S - G) v = recf[RW + (c - (S - G))];
        p.out_s[row * p.ld_s + c] = v;
      } else if (c < S + p.A) p.out_a[row * p.ld_a + (c - S)] = v;
      else if (c >= o_ns && c < o_ns + S) {
        const int cn = c - o_ns;
        if (f > 0 && cn >= S - G) v = recf[RW + (cn - (S - G))];
        p.out_ns[row * p.ld_ns + cn] = v;
      } else if (c == o_r) p.out_r[row] = rew;
      else if (c == o_r + 1) p.out_d[row] = done;
    }
  }
}

RelabelRule make_rule(const gcrl_her* h, uint64_t ctr) {
  RelabelRule q;
  q.seed = h->cfg.seed;
  q.ctr = ctr;
  q.k = h->cfg.k_future;
  q.rem_max = (int)std::min<int64_t>(h->cfg.flush_len, h->cfg.capacity) - 1;
  q.reward_kind = h->cfg.reward_kind;
  q.thr = h->cfg.reward_threshold;
  return q;
}

}  // namespace

namespace gcrl {

int her_relabel_flush(gcrl_her* h, int nep, const int* envs, const int* Ts, hipStream_t st, int64_t* rows_out) {
  if (h->goal_strategy == GCRL_GOAL_EPISODE) return her_goal_flush(h, nep, envs, Ts, st, rows_out);   // records with `elapsed` (her_strategy.hip)
  const gcrl_her_config& c = h->cfg;
  if (nep < 1 || nep > kMaxEp) return fail(GCRL_ERR_ARG, "flush: %d episodes in one launch (1..%d)", nep, kMaxEp);
  FlushSampleArgs fa;
  std::memset(&fa, 0, sizeof(fa));
  fa.ring = h->ring;
  fa.cap = c.capacity;
  RingBook book{c.capacity, h->head, h->len};
  fa.tail = book.tail();
  fa.nep = nep; fa.RG = h->RG; fa.RS = h->RS; fa.RW = h->RW; fa.G = h->G;
  int64_t total = 0;
  int maxT = 0;
  for (int e = 0; e < nep; ++e) {
    fa.stage[e] = h->stage + ((size_t)envs[e] * c.flush_len) * h->RG;
    fa.T[e] = Ts[e];
    total += Ts[e];
    maxT = std::max(maxT, Ts[e]);
  }
  fa.skip = book.append(total);
  dim3 grid((maxT + kFlushRows - 1) / kFlushRows, nep);
  hipLaunchKernelGGL(her_flush_sample_kernel, grid, dim3(256), 0, st, fa);
  GCRL_HIP(hipGetLastError());
  h->head = book.head;
  h->len = book.len;
  h->rows_pushed += (uint64_t)total;
  h->episodes_flushed += nep;
  h->mutation_epoch++;
  *rows_out = total;
  // a ring with an energy tree: the leaves of the rows just written, from the same staged records, in stream order behind the flush
  return her_prio_flush(h, nep, fa.stage, fa.T, fa.tail, fa.skip, total, st);
}

int her_relabel_gather_update(gcrl_her* h, const uint32_t* idx, uint64_t ctr, int64_t n, float* sa, float* nsa, float* spa, int ldx,
                              float* r, float* d, hipStream_t st, const void* cp_src, void* cp_dst, size_t cp_bytes) {
  if (h->goal_strategy != GCRL_GOAL_FUTURE)   // final / episode: her_strategy.hip
    return her_goal_gather_update(h, idx, ctr, 0.f, n, sa, nsa, spa, ldx, r, d, st, cp_src, cp_dst, cp_bytes);
  GatherRelArgs ga{h->ring, idx, h->last_gen, n, h->head, h->cfg.capacity, h->SA4, h->S4, h->RS, ldx, sa, nsa, spa, r, d,
                   (const uint4*)cp_src, (uint4*)cp_dst, (int)(cp_bytes / 16), h->S, h->G, make_rule(h, ctr)};
  const int blocks = (int)((n + 63) / 64);
  const size_t lds = 4 * ((size_t)32 * h->SA4 + 32 + 16 * kTailW) * sizeof(float);
  if (lds > 64 * 1024) return fail(GCRL_ERR_ARG, "her_gather_update: relabel: a batch row of %d floats does not fit the gather's tile", h->SA4);
  if (cp_bytes) hipLaunchKernelGGL(her_gather_relabel_kernel<true>, dim3(blocks), dim3(256), lds, st, ga);
  else hipLaunchKernelGGL(her_gather_relabel_kernel<false>, dim3(blocks), dim3(256), lds, st, ga);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int her_relabel_sample(gcrl_her* h, const uint32_t* idx_dev, uint64_t ctr, int64_t n, float* out_s, int ld_s, float* out_a, int ld_a,
                       float* out_r, float* out_ns, int ld_ns, float* out_d, hipStream_t st) {
  if (h->goal_strategy != GCRL_GOAL_FUTURE) return her_goal_sample(h, idx_dev, ctr, 0.f, n, out_s, ld_s, out_a, ld_a, out_r, out_ns, ld_ns, out_d, st);
  GatherRelPubArgs ga{h->ring, idx_dev, h->last_gen, (long long)n, h->head, h->cfg.capacity, h->S, h->A, h->G, h->SA4, h->S4, h->RS,
                      out_s, out_a, out_r, out_ns, out_d, ld_s, ld_a, ld_ns, make_rule(h, ctr)};
  const int blocks = (int)std::min<long long>((n + 15) / 16, 8192);
  hipLaunchKernelGGL(her_gather_relabel_pub_kernel, dim3(blocks), dim3(256), 0, st, ga);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl
