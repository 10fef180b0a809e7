// her_relabel.hip — the ring's sample-time relabelling mode (relabel = "sample", GCRL_RELABEL_SAMPLE), all of it: a flush that
// stores an episode's T original rows once, each with a tail [ag (G) | remaining] ([ag | remaining | elapsed] on an `episode`
// ring), and gathers that relabel a drawn row against another row of its episode while the batch is assembled — a later row
// (GCRL_GOAL_FUTURE), the last one (FINAL) or any other live one (EPISODE) — one-step or folding an n-step window (gcrl_her_set_nstep,
// n_step = N in 1..8) into its reward and its done flag.  Layout and the contiguity invariant the gathers rest on: her_ring.h.
// The rule is restated three times in numpy, each its definition: tests/her_relabel_ref.py (future, one-step), tests/her_nstep_ref.py
// (future, n-step) and tests/her_strategy_ref.py (all of it).  For the c-th gathered row, of logical index j, slot p:
//     rem  = clamp(remaining, 0, rem_max)      back = episode: min(clamp(elapsed, 0, rem_max), j); otherwise 0
//     n_c  = final: rem > 0 ? 1 : 0            future, episode: back + rem
//     relabel = n_c > 0 && hash_below(seed, K, 2c, k + 1) != 0
//     o    = final: rem                        future, episode: u = hash_below(seed, K, 2c + 1, n_c), u < back ? u - back : u - back + 1
//     goal slot g = p + o (mod cap), o signed            (future is episode with back = 0: o = 1 + u in [1, rem])
//     m = min(N, rem + 1)   last = p + m - 1   s, a <- record p   ns <- record last   (goal slots <- ag[g] when o != 0)
//     r_j (j < m) = o != 0 ? reward(ag[p + j], ag[g]) : r[p + j]          d_last = o != 0 ? 0 : d[last]
//     r <- r_0 + g (r_1 + g (.. r_{m-1}))     d <- m == 1 ? d_last : 1 - g^(m-1) (1 - d_last)       (fp32, one rounding per operation)
// Every TD site forms y = r + g (1 - d) q' with d read as a float, so the engine's kernels take the n-step target
// R + g^m (1 - d_last) q' from these two outputs unchanged.
#include "her_ring.h"
#include "ring_book.h"

#include <algorithm>

namespace {

constexpr int kMaxG = 8;
constexpr int kMaxN = 8;            // n_step <= 8: the (row, step) pairs of a wave's 16 rows are at most two per lane
constexpr int kMaxEp = 8;           // episodes per flush launch (as her_ring.hip)
constexpr int kFlushRows = 16;      // rows per block of the flush
constexpr int kTailW = 12;          // floats of a record from o_r on that the gathers keep per row: r, d, ag (<= 8), remaining, elapsed

// floats of a wave's LDS tile [sa 16 x SA4 | nsa 16 x SA4 | r 16 | d 16 | tails 16 x slots x 12]: slots = 1 (the row's own tail)
// for the one-step gather, N + 1 for the n-step gather
__host__ __device__ constexpr int tile_floats(int SA4, int slots) { return 32 * SA4 + 32 + 16 * slots * kTailW; }

// ---------------------------------------------------------------- flush: T staged records -> T ring records
struct FlushSampleArgs {
  float* ring;
  long long cap, tail, skip;      // rows whose running number is < skip fell off a too-small ring
  int nep, RG, RS, RW, G;
  int elapsed;                    // an `episode` ring: `elapsed` = i is stamped behind `remaining`
  const float* stage[kMaxEp];
  int T[kMaxEp];
};

// grid.x = ceil(longest episode / 16), grid.y = episode; a 16-lane group copies one staged record into its ring slot as full
// 16-byte stores: the leading RW floats and ag as staged, `remaining` = T - 1 - i behind them (and `elapsed` = i behind that on an
// `episode` ring), zeros up to RS.  Same exclusive scan over the episodes' row counts, the same skip / tail / cap rules as
// her_flush_kernel.  No future pick is drawn.
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
  const float rem = (float)(T - 1 - i), el = (float)i;
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
      x[u] = c == o_rem ? rem : (c == o_rem + 1 && p.elapsed ? el : (c > o_rem ? 0.f : x[u]));
    }
    *reinterpret_cast<float4*>(out + c4) = make_float4(x[0], x[1], x[2], x[3]);
  }
}

// ---------------------------------------------------------------- the relabel decision of one gathered row
struct RelabelRule {
  unsigned long long seed, ctr;   // ctr: rows gathered from this ring in sample mode before the launch's row 0
  int k, rem_max;                 // rem_max = min(flush_len, cap) - 1: every address formed stays inside the live ring whatever a tail holds
  int reward_kind;
  float thr;
  int strategy;                   // GCRL_GOAL_FUTURE, GCRL_GOAL_FINAL or GCRL_GOAL_EPISODE
  int N;                          // n_step
  float g32;                      // float32(gamma) (not read at N == 1)
};

__device__ inline int clamp_tail(const RelabelRule& q, float x) {
  return (int)fminf(fmaxf(x, 0.f), (float)q.rem_max);   // [0, rem_max] whatever the tail holds (NaN -> 0)
}

// live predecessors of the row's episode: elapsed clamped to [0, min(rem_max, j)], j the row's logical index (0 = the oldest live row)
__device__ inline int clamp_back(const RelabelRule& q, float el_f, uint32_t j) {
  if (q.strategy != GCRL_GOAL_EPISODE) return 0;        // (only an `episode` ring's records have such a word: it is not read)
  const int el = clamp_tail(q, el_f);
  return (uint32_t)el < j ? el : (int)j;
}

// clamped remaining and back -> signed offset o in [-back, rem] \ {0}, or 0: the row stays as stored.  `future` is `episode`
// with back = 0: key 2c against k + 1, then key 2c + 1 against rem, o = 1 + u.
__device__ inline int goal_pick(const RelabelRule& q, long long row, int rem, int back) {
  const int nc = q.strategy == GCRL_GOAL_FINAL ? (rem > 0 ? 1 : 0) : back + rem;
  if (nc <= 0) return 0;
  const unsigned long long c = q.ctr + (unsigned long long)row;
  if (gcrl::hash_below(q.seed, gcrl::kRelabelStream, 2ull * c, (uint32_t)(q.k + 1)) == 0) return 0;
  if (q.strategy == GCRL_GOAL_FINAL) return rem;        // key 2c + 1 is not evaluated
  const int u = (int)gcrl::hash_below(q.seed, gcrl::kRelabelStream, 2ull * c + 1ull, (uint32_t)nc);
  return u < back ? u - back : u - back + 1;
}

// slot < cap, |off| < cap, off signed: compare-and-subtract above, compare-and-add below
__device__ inline uint32_t wrap_slot(uint32_t slot, int off, long long cap) {
  long long x = (long long)slot + (long long)off;
  if (x >= cap) x -= cap;
  if (x < 0) x += cap;
  return (uint32_t)x;
}

// compute_reward(ag_i, ag_f): -||ag_i - ag_f||_2 or its threshold, fp32, one rounding per operation (her_flush_kernel's arithmetic)
__device__ inline float goal_reward(const RelabelRule& q, const float* ag_i, const float* ag_f, int G) {
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

// the quad of a record that holds the last tail word the strategy reads: `elapsed` (column o_r + 3 + G) on an `episode` ring,
// `remaining` (column o_r + 2 + G) otherwise — a `future` / `final` ring's records end with the quad of `remaining`
__device__ inline int last_quad(int o_r, int G, int strategy) {
  return o_r + (((strategy == GCRL_GOAL_EPISODE ? 3 : 2) + G) & ~3);
}

// [r, d, ag (G)] of the record whose column o_r is `src` (16-byte aligned: o_r and RS are multiples of 4): one to three 16-byte
// loads by G, zeros for the quads not loaded
__device__ inline void load_goal_tail(const float* src, int G, float4 (&q)[3]) {
  q[0] = *reinterpret_cast<const float4*>(src);
  q[1] = q[2] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (G > 2) q[1] = *reinterpret_cast<const float4*>(src + 4);        // o_r + 7 < RS
  if (G > 6) q[2] = *reinterpret_cast<const float4*>(src + 8);        // o_r + 11 < RS
}

// ---------------------------------------------------------------- gathers (update engine)
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

// stages (1) and (2) of both gathers: the wave's 16 indices (kept: j32, the logical index, beside ph32, the slot) and its 16
// records, up to the quad `o_last`, into the wave-private tile [sa 16 x SA4 | nsa 16 x SA4 | r 16 | d 16 | tails 16 x tw]
__device__ inline void load_rows(const GatherRelArgs& p, long long r0, int lane, int o_last, int tw, float* tile, float* t_ns, float* t_tail,
                                 uint32_t& ph32, uint32_t& j32) {
  const int sub = lane >> 4, v4 = lane & 15;
  const int SA4 = p.SA4, S4 = p.S4, o_r = SA4 + S4;
  ph32 = 0; j32 = 0;
  if (lane < 16 && r0 + lane < p.n) {
    j32 = p.idx ? p.idx[r0 + lane] : gcrl::idxgen_at(p.gen, r0 + lane);
    unsigned long long phys = (unsigned long long)p.head + j32;
    if (phys >= (unsigned long long)p.cap) phys -= (unsigned long long)p.cap;    // head, index < cap
    ph32 = (uint32_t)phys;
  }
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
}

// the last stage of both gathers: the tile leaves as contiguous 16-byte non-temporal stores, a partial wave's guarded by row
__device__ inline void store_rows(const GatherRelArgs& p, long long r0, int lane, const float* tile, const float* t_ns, const float* t_rd) {
  const int SA4 = p.SA4, S4 = p.S4, nq = 4 * SA4;
  const bool full = r0 + 16 <= p.n;
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

// her_gather_update_kernel's shape (her_ring.hip) with a patch stage.  One wave owns 16 consecutive batch rows:
//   (1) 16 indices in one coalesced load (or the keyed permutation per lane), ring wrap by compare-and-subtract; the deciding lane
//       keeps its row's logical index j beside the slot;
//   (2) all 16 records in flight, 16 lanes x 16 B per record, up to the quad that holds `elapsed` (episode) or `remaining`;
//       they land in the wave-private LDS tile [sa 16 x SA4 | nsa 16 x SA4 | r 16 | d 16 | tail 16 x 12];
//   (3) lane l < 16 decides row l (counter hash of c = ctr + row) and loads the goal row's tail, one to three 16-byte loads per
//       relabelled row; the goal slot is p + o, o signed, brought back into the ring by compare-and-subtract / compare-and-add
//       (|o| <= rem_max < cap; back <= j: the slot is a live row);
//   (4) the lane patches its row in the tile — the goal slot of s and of ns, r by her_flush_kernel's arithmetic, d = 0 — and
//   (5) the tile leaves as contiguous 16-byte non-temporal stores.  The launch's last, partial wave takes the same path with its
//       stores guarded by row.
// The tile is private to the wave and a wave's LDS operations execute in order: no barrier between the stages, only the compiler
// is held back.  No waits between workgroups, no atomics, no per-thread scratch.
template <bool kHead>
__global__ __launch_bounds__(256) void her_gather_relabel_kernel(GatherRelArgs p) {
  extern __shared__ float gather_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (kHead)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.cp_n16; i += gridDim.x * 256) p.cp_dst[i] = p.cp_src[i];
  const int SA4 = p.SA4, o_r = SA4 + p.S4, G = p.G;
  const int nq = 4 * SA4;                                   // 16-byte quads of a [16][SA4] tile
  float* tile = gather_lds + (size_t)w * tile_floats(SA4, 1);
  float* t_ns = tile + 4 * nq;
  float* t_rd = tile + 8 * nq;
  float* t_tail = t_rd + 32;
  const long long r0 = ((long long)blockIdx.x * 4 + w) * 16;
  if (r0 >= p.n) return;
  uint32_t ph32, j32;
  load_rows(p, r0, lane, last_quad(o_r, G, p.rule.strategy), kTailW, tile, t_ns, t_tail, ph32, j32);
  __builtin_amdgcn_wave_barrier();
  // ---- the patch stage: lane l < 16 owns row l
  if (lane < 16) {
    const float* tl = t_tail + lane * kTailW;
    float rew = tl[0], done = tl[1];
    int o = 0;
    if (r0 + lane < p.n) {
      const int rem = clamp_tail(p.rule, tl[2 + G]);
      o = goal_pick(p.rule, r0 + lane, rem, clamp_back(p.rule, tl[3 + G], j32));
    }
    if (o != 0) {
      float4 gq[3];
      load_goal_tail(p.ring + (size_t)wrap_slot(ph32, o, p.cap) * p.RS + o_r, G, gq);
      const float af[kMaxG] = {gq[0].z, gq[0].w, gq[1].x, gq[1].y, gq[1].z, gq[1].w, gq[2].x, gq[2].y};
      float a_i[kMaxG];
#pragma unroll
      for (int q = 0; q < kMaxG; ++q) a_i[q] = q < G ? tl[2 + q] : 0.f;
      rew = goal_reward(p.rule, a_i, af, G);
      done = 0.f;
      float* gs = tile + lane * SA4 + (p.S - G);
      float* gn = t_ns + lane * SA4 + (p.S - G);
#pragma unroll
      for (int q = 0; q < kMaxG; ++q)
        if (q < G) { gs[q] = af[q]; gn[q] = af[q]; }
    }
    t_rd[lane] = rew;
    t_rd[16 + lane] = done;
  }
  __builtin_amdgcn_wave_barrier();
  store_rows(p, r0, lane, tile, t_ns, t_rd);
}

// her_gather_relabel_kernel with a second round of loads, for a ring with n_step = N > 1.
//   (1), (2) as above, the tile's tails 16 x (N + 1) x 12: slot 0 of a row's tails is its own;
//   (3) lane l < 16 decides row l: o by the counter hash, m = min(N, rem + 1), last = p + m - 1; the wave reads them by __shfl;
//   (4) the second round, issued by all 64 lanes and in flight as a whole before anything of it is consumed: the ns group of record
//       `last` of every row with m > 1 and the tails [r, d, ag] of rows p + 1 .. p + m - 1 (slots 1 .. m - 1) and of the goal row
//       p + o (slot N), one to three 16-byte loads each, the (row, slot) pairs spread over the lanes: at most 8 + 6 loads per lane;
//   (5) lane l < 16 folds its row's rewards by Horner's rule from the last one, folds d, patches the goal slots in the tile, and
//   (6) the tile leaves as contiguous 16-byte non-temporal stores.
// Every slot formed is p + an offset in [-min(rem_max, j), rem_max], |offset| < cap, brought back into the ring.  No waits between
// workgroups, no atomics, no per-thread scratch (the per-step values live in the tile).
template <bool kHead>
__global__ __launch_bounds__(256) void her_gather_nstep_kernel(GatherRelArgs p) {
  extern __shared__ float nstep_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane >> 4, v4 = lane & 15;
  if (kHead)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < p.cp_n16; i += gridDim.x * 256) p.cp_dst[i] = p.cp_src[i];
  const int SA4 = p.SA4, o_r = SA4 + p.S4, G = p.G, N = p.rule.N;
  const int nq = 4 * SA4;                                   // 16-byte quads of a [16][SA4] tile
  const int tw = (N + 1) * kTailW;                          // floats of one row's tails
  float* tile = nstep_lds + (size_t)w * tile_floats(SA4, N + 1);
  float* t_ns = tile + 4 * nq;
  float* t_rd = tile + 8 * nq;
  float* t_tail = t_rd + 32;
  const long long r0 = ((long long)blockIdx.x * 4 + w) * 16;
  if (r0 >= p.n) return;
  uint32_t ph32, j32;
  load_rows(p, r0, lane, last_quad(o_r, G, p.rule.strategy), tw, tile, t_ns, t_tail, ph32, j32);
  __builtin_amdgcn_wave_barrier();
  // ---- (3) the decision: lane l < 16 owns row l (a row past the launch's end: o = 0, m = 1, nothing further is loaded for it)
  int o = 0, m = 1;
  uint32_t last32 = ph32, goal32 = ph32;
  if (lane < 16 && r0 + lane < p.n) {
    const int rem = clamp_tail(p.rule, t_tail[lane * tw + 2 + G]);
    o = goal_pick(p.rule, r0 + lane, rem, clamp_back(p.rule, t_tail[lane * tw + 3 + G], j32));
    m = min(N, rem + 1);
    last32 = wrap_slot(ph32, m - 1, p.cap);
    goal32 = wrap_slot(ph32, o, p.cap);
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
  const uint32_t ph_b = __shfl(ph32, v4, 64), goal_b = __shfl(goal32, v4, 64);   // this lane's tail pairs belong to row v4
  const int o_b = __shfl(o, v4, 64), m_b = __shfl(m, v4, 64);
  float4 tv[2][3];
  bool tuse[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int j = 1 + sub + 4 * t;          // tail slot 1 .. 8: j < N is row p + j, j == N the goal row
    tuse[t] = j < N ? j < m_b : (j == N && o_b != 0);
    const uint32_t slot = j < N ? wrap_slot(ph_b, tuse[t] ? j : 0, p.cap) : goal_b;
    const float* src = p.ring + (size_t)slot * p.RS + o_r;
    tv[t][0] = tv[t][1] = tv[t][2] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tuse[t]) load_goal_tail(src, G, tv[t]);
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
    const float* fa = tl + N * kTailW + 2;              // the goal row's achieved goal (read when o != 0 only)
    float acc = 0.f;
    for (int j = m - 1; j >= 0; --j) {
      const float* tj = tl + j * kTailW;
      const float rj = o != 0 ? goal_reward(p.rule, tj + 2, fa, G) : tj[0];
      acc = j == m - 1 ? rj : __fadd_rn(rj, __fmul_rn(p.rule.g32, acc));
    }
    const float d_last = o != 0 ? 0.f : tl[(m - 1) * kTailW + 1];
    if (o != 0) {
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
  store_rows(p, r0, lane, tile, t_ns, t_rd);
}

// ---------------------------------------------------------------- gathers (public sample): five dense outputs
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

// a 16-lane group per row, 16 rows per block per pass; every lane of a group takes the row's decision and folds its window
// itself (the same addresses: one fetch) and routes its columns to the outputs.  At N = 1 the window is the row: m = 1, last = p,
// r = r_0 and d = d_last.  Not a hot path: any record width, no LDS.
__global__ __launch_bounds__(256) void her_gather_relabel_pub_kernel(GatherRelPubArgs p) {
  const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
  const int o_ns = p.SA4, o_r = p.SA4 + p.S4, RW = o_r + 2, G = p.G, S = p.S;
  const bool epi = p.rule.strategy == GCRL_GOAL_EPISODE;
  for (long long row = (long long)blockIdx.x * 16 + grp; row < p.n; row += (long long)gridDim.x * 16) {
    const uint32_t j32 = p.idx ? p.idx[row] : gcrl::idxgen_at(p.gen, row);
    unsigned long long phys = (unsigned long long)p.head + j32;
    if (phys >= (unsigned long long)p.cap) phys %= (unsigned long long)p.cap;
    const uint32_t ph = (uint32_t)phys;
    const float* rec = p.ring + (size_t)ph * p.RS;
    const int rem = clamp_tail(p.rule, rec[RW + G]);
    const int o = goal_pick(p.rule, row, rem, clamp_back(p.rule, epi ? rec[RW + G + 1] : 0.f, j32));
    const int m = min(p.rule.N, rem + 1);
    const float* recl = p.ring + (size_t)wrap_slot(ph, m - 1, p.cap) * p.RS;
    const float* recf = p.ring + (size_t)wrap_slot(ph, o, p.cap) * p.RS;
    float acc = 0.f;
    for (int j = m - 1; j >= 0; --j) {
      const float* rj_rec = p.ring + (size_t)wrap_slot(ph, j, p.cap) * p.RS;
      float rj = rj_rec[o_r];
      if (o != 0) {       // goal_reward's arithmetic over the G live columns only: both rows are read from memory here
        float s2 = 0.f;
        for (int q = 0; q < G; ++q) { const float df = __fsub_rn(rj_rec[RW + q], recf[RW + q]); s2 = __fadd_rn(s2, __fmul_rn(df, df)); }
        const float dist = sqrtf(s2);
        rj = (p.rule.reward_kind == GCRL_REWARD_SPARSE) ? ((dist > p.rule.thr) ? -1.0f : -0.0f) : -dist;
      }
      acc = j == m - 1 ? rj : __fadd_rn(rj, __fmul_rn(p.rule.g32, acc));
    }
    const float done = fold_done(o != 0 ? 0.f : recl[o_r + 1], m, p.rule.g32);
    for (int c = gl; c < RW; c += 16) {
      if (c < S) {
        float v = rec[c];
        if (o != 0 && c >= S - G) v = recf[RW + (c - (S - G))];
        p.out_s[row * p.ld_s + c] = v;
      } else if (c < S + p.A) p.out_a[row * p.ld_a + (c - S)] = rec[c];
      else if (c >= o_ns && c < o_ns + S) {
        const int cn = c - o_ns;
        float v = recl[c];
        if (o != 0 && cn >= S - G) v = recf[RW + (cn - (S - G))];
        p.out_ns[row * p.ld_ns + cn] = v;
      } else if (c == o_r) p.out_r[row] = acc;
      else if (c == o_r + 1) p.out_d[row] = done;
    }
  }
}

RelabelRule make_rule(const gcrl_her* h, uint64_t ctr, float g32) {
  RelabelRule q;
  q.seed = h->cfg.seed;
  q.ctr = ctr;
  q.k = h->cfg.k_future;
  q.rem_max = (int)std::min<int64_t>(h->cfg.flush_len, h->cfg.capacity) - 1;
  q.reward_kind = h->cfg.reward_kind;
  q.thr = h->cfg.reward_threshold;
  q.strategy = h->goal_strategy;
  q.N = h->n_step;
  q.g32 = g32;
  return q;
}

int check_ring(const gcrl_her* h, const char* who) {
  if (h->goal_strategy != GCRL_GOAL_FUTURE && h->goal_strategy != GCRL_GOAL_FINAL && h->goal_strategy != GCRL_GOAL_EPISODE)
    return gcrl::fail(GCRL_ERR_STATE, "%s: goal_strategy: %d is not a strategy of the goal gathers", who, h->goal_strategy);
  if (h->n_step < 1 || h->n_step > kMaxN) return gcrl::fail(GCRL_ERR_STATE, "%s: n_step: %d outside 1..%d", who, h->n_step, kMaxN);
  return GCRL_OK;
}

}  // namespace

namespace gcrl {

int her_relabel_flush(gcrl_her* h, int nep, const int* envs, const int* Ts, hipStream_t st, int64_t* rows_out) {
  const gcrl_her_config& c = h->cfg;
  if (nep < 1 || nep > kMaxEp) return fail(GCRL_ERR_ARG, "flush: %d episodes in one launch (1..%d)", nep, kMaxEp);
  FlushSampleArgs fa;
  std::memset(&fa, 0, sizeof(fa));
  fa.ring = h->ring;
  fa.cap = c.capacity;
  RingBook book{c.capacity, h->head, h->len};
  fa.tail = book.tail();
  fa.nep = nep; fa.RG = h->RG; fa.RS = h->RS; fa.RW = h->RW; fa.G = h->G;
  fa.elapsed = h->goal_strategy == GCRL_GOAL_EPISODE;
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
  if (int rc = her_prio_flush(h, nep, fa.stage, fa.T, fa.tail, fa.skip, total, st)) return rc;
  return her_td_flush(h, total, st);   // a ring with a TD-error tree: the rows just written enter at p_max (her_td.hip)
}

int her_relabel_gather_update(gcrl_her* h, const uint32_t* idx, uint64_t ctr, float g32, int64_t n, float* sa, float* nsa, float* spa, int ldx,
                              float* r, float* d, hipStream_t st, const void* cp_src, void* cp_dst, size_t cp_bytes) {
  if (int rc = check_ring(h, "her_gather_update")) return rc;
  GatherRelArgs ga{h->ring, idx, h->last_gen, n, h->head, h->cfg.capacity, h->SA4, h->S4, h->RS, ldx, sa, nsa, spa, r, d,
                   (const uint4*)cp_src, (uint4*)cp_dst, (int)(cp_bytes / 16), h->S, h->G, make_rule(h, ctr, g32)};
  const int blocks = (int)((n + 63) / 64);
  const size_t lds = 4 * (size_t)tile_floats(h->SA4, h->n_step == 1 ? 1 : h->n_step + 1) * sizeof(float);   // 4 waves per block
  if (h->n_step == 1) {   // not the n-step kernel at N = 1: it holds 84 VGPRs against 57 and has a second round of loads
    if (lds > 64 * 1024) return fail(GCRL_ERR_ARG, "her_gather_update: relabel: a batch row of %d floats does not fit the gather's tile", h->SA4);
    if (cp_bytes) hipLaunchKernelGGL(her_gather_relabel_kernel<true>, dim3(blocks), dim3(256), lds, st, ga);
    else hipLaunchKernelGGL(her_gather_relabel_kernel<false>, dim3(blocks), dim3(256), lds, st, ga);
  } else {
    if (lds > 64 * 1024 || h->S4 > 128)
      return fail(GCRL_ERR_ARG, "her_gather_update: n_step: a batch row of %d floats with the tails of n_step = %d does not fit the gather's tile", h->SA4, h->n_step);
    if (cp_bytes) hipLaunchKernelGGL(her_gather_nstep_kernel<true>, dim3(blocks), dim3(256), lds, st, ga);
    else hipLaunchKernelGGL(her_gather_nstep_kernel<false>, dim3(blocks), dim3(256), lds, st, ga);
  }
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int her_relabel_sample(gcrl_her* h, const uint32_t* idx_dev, uint64_t ctr, float g32, int64_t n, float* out_s, int ld_s, float* out_a, int ld_a,
                       float* out_r, float* out_ns, int ld_ns, float* out_d, hipStream_t st) {
  if (int rc = check_ring(h, "gcrl_her_sample")) return rc;
  GatherRelPubArgs ga{h->ring, idx_dev, h->last_gen, (long long)n, h->head, h->cfg.capacity, h->S, h->A, h->G, h->SA4, h->S4, h->RS,
                      out_s, out_a, out_r, out_ns, out_d, ld_s, ld_a, ld_ns, make_rule(h, ctr, g32)};
  const int blocks = (int)std::min<long long>((n + 15) / 16, 8192);
  hipLaunchKernelGGL(her_gather_relabel_pub_kernel, dim3(blocks), dim3(256), 0, st, ga);
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
