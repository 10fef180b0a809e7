// her_prio.hip — energy-prioritised replay draw of a sample-mode HER ring (prioritise = "energy").
//
// The ring gets a priority tree of per_tree.hip's layout (per_host.h) whose leaves are written ONCE, by the flush: every row of a
// flushed episode gets (E_traj + eps)^alpha / T, E_traj the clipped energy gains of the episode's achieved-goal trajectory, read
// from the staged records the flush itself copied (`ag` at float RW of a staged record).  Nothing feeds back from the loss and
// there are no importance-sampling weights: the only thing that changes is which row indices a gather reads.  The rule is restated
// in numpy in tests/her_energy_ref.py, which is its definition.
//
// A translation unit of its own: the kernels of per_tree.hip and her_relabel.hip keep their code, byte for byte.  Neither kernel
// here waits for another workgroup, uses atomics, per-thread scratch or LDS.
#include "her_ring.h"
#include "per_tree.h"

#include <cmath>

namespace {

using gcrl::kPerFan;
using gcrl::kPerMaxLevels;

constexpr int kWaves = 4;             // waves per workgroup of the draw
constexpr int kOneWgThreads = 1024;   // the flush's single workgroup
constexpr int kMaxEp = 8;             // episodes per flush launch (as her_relabel.hip)
constexpr int kMaxT = 64;             // rows of an episode = lanes of the wave that reduces it

struct TreeView {
  float* tree;
  long long off[kPerMaxLevels];
  int levels;
};

__device__ inline float wave_sum64(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

__device__ inline void reduce_range(const TreeView& t, int k, long long p0, long long p1, int wave, int nwaves, int lane) {
  const float* child = t.tree + t.off[k - 1];
  float* parent = t.tree + t.off[k];
  for (long long node = p0 + wave; node < p1; node += nwaves) {
    const float s = wave_sum64(child[node * kPerFan + lane]);
    if (lane == 0) parent[node] = s;
  }
}

struct EnergyArgs {
  TreeView t;
  long long cap, tail, skip;          // the flush launch's own (her_flush_sample_kernel): rows whose running number is < skip were not written
  long long a0, a1, b0, b1;           // the slots the flush wrote, as at most two segments (per_pending_segments)
  int nep, RG, RW, G;
  const float* stage[kMaxEp];
  int T[kMaxEp];
  float potential, kinetic, clip, alpha, eps;
  int axis;
};

// ONE workgroup, behind the flush launch it describes.  Wave w takes episodes w, w + 16, ...: lane i < T forms E_i from ag_i and
// ag_{i-1}, takes E_{i-1} from its neighbour, e_i = fmin(fmax(E_i - E_{i-1}, 0), clip); the wave butterflies E_traj; lane i writes
// the leaf of the slot row i went to — the flush kernel's own running number / skip / tail / compare-and-subtract, so a skipped row
// writes nothing and every address stays inside the leaves.  Then the ancestors of the written segments, level by level, a barrier
// between the levels (per_refresh_kernel's second half).
__global__ __launch_bounds__(kOneWgThreads) void her_energy_kernel(EnergyArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (int e = wave; e < p.nep; e += nwaves) {
    const int T = p.T[e];
    long long base = 0;
    for (int q = 0; q < e; ++q) base += p.T[q];
    float E = 0.0f;
    if (lane < T) {
      const float* cur = p.stage[e] + (long long)lane * p.RG + p.RW;
      const float* prev = cur - (lane > 0 ? p.RG : 0);
      float acc = 0.0f;
      for (int c = 0; c < p.G; ++c) {
        const float df = __fsub_rn(cur[c], prev[c]);
        acc = __fadd_rn(acc, __fmul_rn(df, df));
      }
      const float kin = lane > 0 ? __fmul_rn(p.kinetic, acc) : 0.0f;
      const float pot = p.axis >= 0 ? __fmul_rn(p.potential, cur[p.axis]) : 0.0f;
      E = __fadd_rn(pot, kin);
    }
    const float Eprev = __shfl_up(E, 1, 64);
    float gain = 0.0f;
    if (lane > 0 && lane < T) gain = fminf(fmaxf(__fsub_rn(E, Eprev), 0.0f), p.clip);   // NaN -> 0, +inf -> clip
    const float x = __fadd_rn(wave_sum64(gain), p.eps);
    const float pe = p.alpha == 1.0f ? x : powf(x, p.alpha);
    const float leaf = __fdiv_rn(pe, (float)T);
    const long long g = base + lane;
    if (lane < T && g >= p.skip) {
      long long phys = p.tail + g;
      if (phys >= p.cap) phys -= p.cap;
      if (phys >= p.cap) phys %= p.cap;         // (a ring smaller than the flush)
      p.t.tree[phys] = leaf;
    }
  }
  long long a0 = p.a0, a1 = p.a1, b0 = p.b0, b1 = p.b1;
  for (int k = 1; k < p.t.levels; ++k) {
    __syncthreads();
    if (a1 > a0) { a0 = a0 / kPerFan; a1 = (a1 - 1) / kPerFan + 1; }
    if (b1 > b0) { b0 = b0 / kPerFan; b1 = (b1 - 1) / kPerFan + 1; }
    reduce_range(p.t, k, a0, a1, wave, nwaves, lane);
    reduce_range(p.t, k, b0, b1, wave, nwaves, lane);
  }
}

struct PrioDrawArgs {
  TreeView t;
  unsigned long long seed, c0;   // c0: rows drawn from this ring's tree before the launch's row 0
  long long rows, head, cap;
  uint32_t* idx;
};

// per_draw_kernel's descent (per_tree.hip), one wave per row; the uniform of row t at level k is keyed by ((c0 + t) << 3) + k —
// per_tree_ref.uniform24 with draw = c >> 20, b = c & 0xFFFFF.  Writes the logical index only.
__global__ __launch_bounds__(64 * kWaves) void her_prio_draw_kernel(PrioDrawArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const unsigned long long c = a.c0 + (unsigned long long)row;
  const unsigned long long key = gcrl::mix64(a.seed ^ gcrl::kPerKey);
  long long blk = 0;
  for (int k = a.t.levels - 1; k >= 0; --k) {
    const float v = a.t.tree[a.t.off[k] + blk * kPerFan + lane];
    float P = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float up = __shfl_up(P, off, 64);
      if (lane >= off) P = P + up;
    }
    const float total = __shfl(P, 63, 64);
    const unsigned long long h = gcrl::mix64(key + ((c << 3) + (unsigned long long)k));
    const float u = (float)(unsigned int)(h >> 40) * (1.0f / 16777216.0f);
    const float x = u * total;
    const bool pos = v > 0.0f;
    const unsigned long long hit = __ballot(pos && P > x);
    const unsigned long long any = __ballot(pos);
    const int child = hit ? __ffsll(hit) - 1 : (any ? 63 - __clzll(any) : 0);
    blk = blk * kPerFan + child;
  }
  if (lane == 0) {
    long long logical = blk - a.head;
    if (logical < 0) logical += a.cap;
    a.idx[row] = (uint32_t)logical;
  }
}

TreeView view_of(const gcrl_per_tree* t) {
  TreeView v;
  v.tree = t->tree;
  for (int k = 0; k < kPerMaxLevels; ++k) v.off[k] = t->L.off[k];
  v.levels = t->L.levels;
  return v;
}

}  // namespace

namespace gcrl {

int her_prio_flush(gcrl_her* h, int nep, const float* const* stage, const int* Ts, int64_t tail, int64_t skip, int64_t total, hipStream_t st) {
  gcrl_per_tree* t = h->per;
  if (!per_is_energy(t)) return GCRL_OK;
  if (nep < 1 || nep > kMaxEp) return fail(GCRL_ERR_ARG, "flush: prioritise: %d episodes in one launch (1..%d)", nep, kMaxEp);
  EnergyArgs ea;
  std::memset(&ea, 0, sizeof(ea));
  ea.t = view_of(t);
  ea.cap = h->cfg.capacity; ea.tail = tail; ea.skip = skip;
  // the ring's head / len are already those after the flush: its rows are the last min(total, cap) ones before the tail
  const PerSegs s = per_pending_segments(h->head, h->len, h->cfg.capacity, total);
  ea.a0 = s.a0; ea.a1 = s.a1; ea.b0 = s.b0; ea.b1 = s.b1;
  ea.nep = nep; ea.RG = h->RG; ea.RW = h->RW; ea.G = h->G;
  for (int e = 0; e < nep; ++e) {
    if (Ts[e] < 1 || Ts[e] > kMaxT) return fail(GCRL_ERR_ARG, "flush: prioritise: flush_len: an episode of %d rows (1..%d)", Ts[e], kMaxT);
    ea.stage[e] = stage[e];
    ea.T[e] = Ts[e];
  }
  const gcrl_energy_config& c = t->energy;
  ea.potential = c.potential; ea.kinetic = c.kinetic; ea.clip = c.clip; ea.alpha = c.alpha; ea.eps = c.eps; ea.axis = c.axis;
  hipLaunchKernelGGL(her_energy_kernel, dim3(1), dim3(kOneWgThreads), 0, st, ea);
  GCRL_HIP(hipGetLastError());
  t->launches++;
  t->synced_rows = h->rows_pushed;
  return GCRL_OK;
}

bool her_prio_on(const gcrl_her* h) { return h && per_is_energy(h->per); }

uint64_t her_prio_take(gcrl_her* h, int64_t rows) {
  const uint64_t c0 = h->per->prio_ctr;
  h->per->prio_ctr += (uint64_t)rows;
  return c0;
}

int her_prio_check(const gcrl_her* h, const char* who) {
  if (!h || !per_is_energy(h->per))
    return fail(GCRL_ERR_STATE, "%s: prioritise: no energy tree is attached to this ring (gcrl_her_prio_attach)", who);
  if (h->per->stale)
    return fail(GCRL_ERR_STATE, "%s: prioritise: the ring was reloaded after the tree was built: set its leaves first (gcrl_per_set_priorities)", who);
  return GCRL_OK;
}

int her_prio_draw_at(gcrl_her* h, uint64_t c0, int64_t rows, uint32_t* idx_dev, hipStream_t st) {
  if (int rc = her_prio_check(h, "her_prio_draw")) return rc;
  gcrl_per_tree* t = h->per;
  GCRL_CHECK_ARG(idx_dev && rows >= 1 && rows <= (1ll << 30), "her_prio_draw: %lld rows (1..2^30) / null index buffer", (long long)rows);
  if (h->len < 1) return fail(GCRL_ERR_NOT_ENOUGH, "[ERROR] Not enough in buffer to sample");
  PrioDrawArgs a;
  a.t = view_of(t);
  a.seed = h->cfg.seed; a.c0 = c0; a.rows = rows; a.head = h->head; a.cap = h->cfg.capacity; a.idx = idx_dev;
  hipLaunchKernelGGL(her_prio_draw_kernel, dim3((unsigned)((rows + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, st, a);
  GCRL_HIP(hipGetLastError());
  t->launches++;
  return GCRL_OK;
}

}  // namespace gcrl

extern "C" {

int gcrl_her_prio_attach(gcrl_her* h, const gcrl_energy_config* cfg) {
  GCRL_CHECK_ARG(h && cfg, "gcrl_her_prio_attach: null argument");
  if (h->per) return gcrl::fail(GCRL_ERR_STATE, "gcrl_her_prio_attach: prioritise: the ring already has a priority tree");
  if (h->relabel_mode != GCRL_RELABEL_SAMPLE)
    return gcrl::fail(GCRL_ERR_STATE, "gcrl_her_prio_attach: prioritise: the episode energy is read from the tails of a ring with sample-time "
                      "relabelling (GCRL_RELABEL_SAMPLE); this ring was created with GCRL_RELABEL_PUSH");
  GCRL_CHECK_ARG(h->cfg.flush_len <= kMaxT, "gcrl_her_prio_attach: flush_len %d: one wave reduces an episode (at most %d rows)", h->cfg.flush_len, kMaxT);
  GCRL_CHECK_ARG(std::isfinite(cfg->potential) && std::isfinite(cfg->kinetic), "gcrl_her_prio_attach: energy: potential %g / kinetic %g must be finite",
                 (double)cfg->potential, (double)cfg->kinetic);
  GCRL_CHECK_ARG(cfg->axis < h->G, "gcrl_her_prio_attach: energy: axis %d of a goal with %d components", cfg->axis, h->G);
  GCRL_CHECK_ARG(std::isfinite(cfg->clip) && cfg->clip > 0.0f, "gcrl_her_prio_attach: energy: clip %g (finite, > 0)", (double)cfg->clip);
  GCRL_CHECK_ARG(std::isfinite(cfg->eps) && cfg->eps > 0.0f, "gcrl_her_prio_attach: energy: eps %g (finite, > 0)", (double)cfg->eps);
  GCRL_CHECK_ARG(std::isfinite(cfg->alpha) && cfg->alpha >= 0.0f, "gcrl_her_prio_attach: energy: alpha %g (finite, >= 0)", (double)cfg->alpha);
  gcrl_per_tree* t = nullptr;
  if (int rc = gcrl::per_tree_alloc(h, "gcrl_her_prio_attach", &t)) return rc;
  t->source = gcrl::kPerSourceEnergy;
  t->energy = *cfg;
  if (t->energy.axis < 0) t->energy.axis = -1;
  t->alpha = cfg->alpha; t->eps = cfg->eps;
  t->synced_rows = h->rows_pushed;
  if (h->len > 0) {   // rows from before the tree: the floor leaf of a zero-energy episode of one row, then every node
    const float floor_leaf = cfg->alpha == 1.0f ? cfg->eps : std::pow(cfg->eps, cfg->alpha);
    std::vector<float> leaves((size_t)t->L.padded[0], 0.0f);
    for (int64_t j = 0; j < h->len; ++j) leaves[(size_t)gcrl::per_slot_of(j, h->head, h->cfg.capacity)] = floor_leaf;
    hipError_t e = hipMemcpy(t->tree, leaves.data(), leaves.size() * sizeof(float), hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? gcrl::per_rebuild(t, h->stream) : GCRL_OK;
    if (e == hipSuccess && rc == GCRL_OK) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || rc != GCRL_OK) {
      gcrl::per_tree_free(t);
      if (rc != GCRL_OK) return rc;
      GCRL_HIP(e);
    }
  }
  h->per = t;
  return GCRL_OK;
}

int gcrl_her_prio_mode(const gcrl_her* h) {
  if (h && gcrl::per_is_her_td(h->per)) return GCRL_PRIO_TD;
  return h && gcrl::per_is_energy(h->per) ? GCRL_PRIO_ENERGY : GCRL_PRIO_NONE;
}

int gcrl_her_prio_draw(gcrl_her* h, int64_t rows, uint32_t* idx_dev, void* stream) {
  GCRL_CHECK_ARG(h, "gcrl_her_prio_draw: null ring");
  if (int rc = gcrl::her_prio_draw_at(h, h->per ? h->per->prio_ctr : 0, rows, idx_dev, h->pick(stream))) return rc;
  h->per->prio_ctr += (uint64_t)rows;
  return GCRL_OK;
}

uint64_t gcrl_her_get_prio_counter(const gcrl_her* h) { return h && gcrl::per_is_energy(h->per) ? h->per->prio_ctr : 0; }

int gcrl_her_set_prio_counter(gcrl_her* h, uint64_t counter) {
  if (!h || !gcrl::per_is_energy(h->per))
    return gcrl::fail(GCRL_ERR_STATE, "gcrl_her_set_prio_counter: prioritise: no energy tree is attached to this ring (gcrl_her_prio_attach)");
  h->per->prio_ctr = counter;
  return GCRL_OK;
}

}  // extern "C"
