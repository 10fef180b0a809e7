// per_tree.hip — device-resident prioritised replay (the reference's PERBuffer, src/buffer.py:38-89, as device state):
// priorities, the proportional draw, the importance-sampling weights and the priority update as HIP kernels on a tree of
// fp32 sums in HBM.  NOT the reference's index stream (np.random.choice on numpy's global generator): a device mode beside
// the parity mode, defined by the restatement tests/per_tree_ref.py and held to it bit for bit.
//
// A node is ALWAYS the recomputed reduction of its 64 children in one fixed order (wave_sum64: the xor-butterfly 32, 16, 8,
// 4, 2, 1 across a wave), never an incremental add: the tree is a pure function of the leaves, whatever the update order.
// No kernel here waits for another workgroup, none uses atomics or per-thread scratch.
#include "per_tree.h"

#include <algorithm>
#include <cmath>

#include "her_ring.h"

namespace {

using gcrl::kPerFan;
using gcrl::kPerMaxLevels;

constexpr int kWaves = 4;               // waves per workgroup of the multi-workgroup kernels
constexpr int kOneWgThreads = 1024;     // the single-workgroup kernels (levels separated by barriers)
constexpr int64_t kPerRefreshOne = 65536;

#include "per_tree_dev.inc"   // TreeView, wave_sum64, reduce_range, view_of: shared with her_td.hip

// level k+1 <- the reduction of level k, one wave per node
__global__ __launch_bounds__(64 * kWaves) void per_level_kernel(const float* __restrict__ child, float* __restrict__ parent, long long nodes) {
  const int lane = threadIdx.x & 63;
  const long long node = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (node >= nodes) return;
  const float s = wave_sum64(child[node * kPerFan + lane]);
  if (lane == 0) parent[node] = s;
}

__global__ __launch_bounds__(256) void per_fill_kernel(float* __restrict__ leaves, long long a0, long long a1, long long b0, long long b1, float value) {
  const long long na = a1 - a0, n = na + (b1 - b0);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    leaves[i < na ? a0 + i : b0 + (i - na)] = value;
}

// pushes since the last refresh: leaves of two slot segments <- value, then their ancestors level by level (one workgroup,
// a barrier between the levels)
__global__ __launch_bounds__(kOneWgThreads) void per_refresh_kernel(TreeView t, long long a0, long long a1, long long b0, long long b1, float value) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (long long i = a0 + threadIdx.x; i < a1; i += blockDim.x) t.tree[i] = value;
  for (long long i = b0 + threadIdx.x; i < b1; i += blockDim.x) t.tree[i] = value;
  for (int k = 1; k < t.levels; ++k) {
    __syncthreads();
    if (a1 > a0) { a0 = a0 / kPerFan; a1 = (a1 - 1) / kPerFan + 1; }
    if (b1 > b0) { b0 = b0 / kPerFan; b1 = (b1 - 1) / kPerFan + 1; }
    reduce_range(t, k, a0, a1, wave, nwaves, lane);
    reduce_range(t, k, b0, b1, wave, nwaves, lane);   // (a node both segments cover is recomputed twice: the same value)
  }
}

struct DrawArgs {
  TreeView t;
  unsigned long long seed, draw;
  int B;
  long long head, cap;
  uint32_t* idx;
  float* p;
};

// One wave per batch element.  Top down, at every level: the block's 64 children in one load; the inclusive scan P by six
// shifted adds; a fresh 24-bit uniform u; x = u * P[63]; descend into the first child with P > x and value > 0, else the last
// child with value > 0 (the shifted-add scan is not monotone in fp32 and u * P[63] can round up to P[63]: a zero slot must
// never be drawn).  A block without a positive child (an empty tree) yields child 0: still inside the allocation.
__global__ __launch_bounds__(64 * kWaves) void per_draw_kernel(DrawArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= a.B) return;
  long long blk = 0;
  float leaf = 0.0f;
  for (int k = a.t.levels - 1; k >= 0; --k) {
    const float v = a.t.tree[a.t.off[k] + blk * kPerFan + lane];
    float P = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float up = __shfl_up(P, off, 64);
      if (lane >= off) P = P + up;
    }
    const float total = __shfl(P, 63, 64);
    const unsigned long long ctr = (((a.draw << 20) + (unsigned long long)b) << 3) + (unsigned long long)k;
    const unsigned long long h = gcrl::mix64(gcrl::mix64(a.seed ^ gcrl::kPerKey) + ctr);
    const float u = (float)(unsigned int)(h >> 40) * (1.0f / 16777216.0f);
    const float x = u * total;
    const bool pos = v > 0.0f;
    const unsigned long long hit = __ballot(pos && P > x);
    const unsigned long long any = __ballot(pos);
    const int child = hit ? __ffsll(hit) - 1 : (any ? 63 - __clzll(any) : 0);
    leaf = __shfl(v, child, 64);
    blk = blk * kPerFan + child;
  }
  if (lane == 0) {
    long long logical = blk - a.head;
    if (logical < 0) logical += a.cap;
    a.idx[b] = (uint32_t)logical;
    a.p[b] = leaf;
  }
}

// w_b = (N * (p_b / total))^(-beta) / max_b(...), total = the fixed-order reduction of the top block; one workgroup
__global__ __launch_bounds__(256) void per_weights_kernel(const float* __restrict__ top, const float* __restrict__ p, int B, float N, float neg_beta,
                                                          float* __restrict__ w) {
  __shared__ float smax[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float total = wave_sum64(top[lane]);
  float m = 0.0f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float x = powf(N * (p[b] / total), neg_beta);
    w[b] = x;
    m = fmaxf(m, x);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if (lane == 0) smax[wave] = m;
  __syncthreads();
  const float mx = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  for (int b = threadIdx.x; b < B; b += 256) w[b] = w[b] / mx;   // (each thread renormalises what it wrote itself)
}

struct UpdArgs {
  TreeView t;
  const uint32_t* idx;
  const float* td;
  int B;
  long long head, cap;
  float alpha, eps;
  float* hist;
};

// leaf of idx[b] <- (|td_b| + eps)^alpha where b is the LAST occurrence of its index (the reference's zip order,
// src/buffer.py:86-89), then the touched ancestors level by level, one wave per touched node, a barrier between the levels.
// Duplicate ancestors are recomputed redundantly: the value is the same.
__global__ __launch_bounds__(kOneWgThreads) void per_update_kernel(UpdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (int b = threadIdx.x; b < a.B; b += blockDim.x) {
    const uint32_t j = a.idx[b];
    const float td = a.td[b];
    if (a.hist) a.hist[b] = td;
    bool last = (long long)j < a.cap;
    for (int c = b + 1; last && c < a.B; ++c) last = a.idx[c] != j;
    if (last) {
      long long slot = a.head + (long long)j;
      if (slot >= a.cap) slot -= a.cap;
      a.t.tree[slot] = powf(fabsf(td) + a.eps, a.alpha);
    }
  }
  for (int k = 1; k < a.t.levels; ++k) {
    __syncthreads();
    const float* child = a.t.tree + a.t.off[k - 1];
    float* parent = a.t.tree + a.t.off[k];
    for (int b = wave; b < a.B; b += nwaves) {
      const uint32_t j = a.idx[b];
      if ((long long)j >= a.cap) continue;   // (wave-uniform)
      long long slot = a.head + (long long)j;
      if (slot >= a.cap) slot -= a.cap;
      const long long node = slot >> (6 * k);
      const float s = wave_sum64(child[node * kPerFan + lane]);
      if (lane == 0) parent[node] = s;
    }
  }
}

int rebuild(gcrl_per_tree* t, hipStream_t st) {
  for (int k = 1; k < t->L.levels; ++k) {
    const long long nodes = t->L.padded[k - 1] / kPerFan;
    hipLaunchKernelGGL(per_level_kernel, dim3((unsigned)((nodes + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, st, t->tree + t->L.off[k - 1],
                       t->tree + t->L.off[k], nodes);
    GCRL_HIP(hipGetLastError());
    t->launches++;
  }
  return GCRL_OK;
}

int need_tree(const gcrl_her* h, const char* who, bool fresh = true, bool td_only = false) {
  if (!h || !h->per) return gcrl::fail(GCRL_ERR_STATE, "%s: no priority tree is attached to this ring (gcrl_per_attach)", who);
  if (td_only && !gcrl::per_is_td(h->per))
    return gcrl::fail(GCRL_ERR_STATE, "%s: prioritise: the ring's tree holds episode energies (gcrl_her_prio_attach): it is drawn by gcrl_her_prio_draw, "
                      "takes no weights and no priority update", who);
  if (fresh && h->per->stale)
    return gcrl::fail(GCRL_ERR_STATE, "%s: the ring was reloaded after the tree was built: set its priorities first (gcrl_per_set_priorities)", who);
  return GCRL_OK;
}

}  // namespace

namespace gcrl {

void per_tree_free(gcrl_per_tree* t) {
  if (!t) return;
  if (t->tree) (void)hipFree(t->tree);
  if (t->p_drawn) (void)hipFree(t->p_drawn);
  if (t->p_max) (void)hipFree(t->p_max);
  delete t;
}

void per_release(gcrl_her* h) {
  gcrl_per_tree* t = h->per;
  h->per = nullptr;
  per_tree_free(t);
}

int per_tree_alloc(gcrl_her* h, const char* who, gcrl_per_tree** out) {
  PerLayout L;
  GCRL_CHECK_ARG(per_layout(h->cfg.capacity, &L), "%s: capacity %lld has no tree layout", who, (long long)h->cfg.capacity);
  GCRL_HIP(hipSetDevice(h->cfg.device));
  float* tree = nullptr;
  GCRL_HIP(hipMalloc((void**)&tree, (size_t)L.total * sizeof(float)));
  hipError_t e = hipMemset(tree, 0, (size_t)L.total * sizeof(float));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { (void)hipFree(tree); GCRL_HIP(e); }
  gcrl_per_tree* t = new gcrl_per_tree;
  t->L = L; t->tree = tree;
  *out = t;
  return GCRL_OK;
}

int per_rebuild(gcrl_per_tree* t, hipStream_t st) { return rebuild(t, st); }

void per_mark_stale(gcrl_her* h) {
  if (h->per) h->per->stale = true;
}

int per_refresh(gcrl_her* h, hipStream_t st) {
  gcrl_per_tree* t = h->per;
  // an energy tree's leaves are the flush's, and so are a HER ring's TD tree's (p_max, her_td.hip): never 1.0
  const int64_t pending = per_is_td(t) && !t->her_td ? (int64_t)(h->rows_pushed - t->synced_rows) : 0;
  t->synced_rows = h->rows_pushed;
  const PerSegs s = per_pending_segments(h->head, h->len, h->cfg.capacity, pending);
  const int64_t n = (s.a1 - s.a0) + (s.b1 - s.b0);
  if (n <= 0) return GCRL_OK;
  if (n <= kPerRefreshOne) {
    hipLaunchKernelGGL(per_refresh_kernel, dim3(1), dim3(kOneWgThreads), 0, st, view_of(t), (long long)s.a0, (long long)s.a1, (long long)s.b0,
                       (long long)s.b1, 1.0f);
    GCRL_HIP(hipGetLastError());
    t->launches++;
    return GCRL_OK;
  }
  hipLaunchKernelGGL(per_fill_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, t->tree, (long long)s.a0,
                     (long long)s.a1, (long long)s.b0, (long long)s.b1, 1.0f);
  GCRL_HIP(hipGetLastError());
  t->launches++;
  return rebuild(t, st);
}

int per_draw(gcrl_her* h, int B, float beta, uint32_t* idx_dev, float* w_dev, hipStream_t st) {
  if (int rc = need_tree(h, "per_draw", true, true)) return rc;
  gcrl_per_tree* t = h->per;
  GCRL_CHECK_ARG(idx_dev && B >= 1 && B <= (1 << 20), "per_draw: batch size %d (1..2^20) / null index buffer", B);
  // (a HER ring's TD tree draws with replacement from whatever rows there are; the callers that need B rows ask for them themselves)
  if (t->her_td ? h->len < 1 : h->len < B) return fail(GCRL_ERR_NOT_ENOUGH, "Not enough in buffer to sample");
  if (B > t->p_cap) {
    if (t->p_drawn) { GCRL_HIP(hipStreamSynchronize(st)); GCRL_HIP(hipFree(t->p_drawn)); t->p_drawn = nullptr; t->p_cap = 0; }
    GCRL_HIP(hipMalloc((void**)&t->p_drawn, (size_t)B * sizeof(float)));
    t->p_cap = B;
  }
  if (int rc = per_refresh(h, st)) return rc;
  DrawArgs a;
  a.t = view_of(t);
  a.seed = h->cfg.seed; a.draw = t->draws; a.B = B; a.head = h->head; a.cap = h->cfg.capacity; a.idx = idx_dev; a.p = t->p_drawn;
  hipLaunchKernelGGL(per_draw_kernel, dim3((unsigned)((B + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, st, a);
  GCRL_HIP(hipGetLastError());
  t->launches++;
  t->draws++;
  if (w_dev) {
    hipLaunchKernelGGL(per_weights_kernel, dim3(1), dim3(256), 0, st, t->tree + t->L.off[t->L.levels - 1], t->p_drawn, B, (float)h->len, -beta, w_dev);
    GCRL_HIP(hipGetLastError());
    t->launches++;
  }
  return GCRL_OK;
}

int per_update(gcrl_her* h, const uint32_t* idx_dev, const float* td_dev, int B, float* hist_dev, hipStream_t st) {
  if (int rc = need_tree(h, "per_update", true, true)) return rc;
  gcrl_per_tree* t = h->per;
  GCRL_CHECK_ARG(idx_dev && td_dev && B >= 1, "per_update: null buffer / batch size %d", B);
  if (t->her_td) return her_td_update(h, idx_dev, td_dev, B, hist_dev, st);   // a HER ring's TD tree: the update that also raises p_max (her_td.hip)
  if (int rc = per_refresh(h, st)) return rc;   // (rows pushed between the draw and this update: their 1.0 first, as in the reference's order)
  UpdArgs a;
  a.t = view_of(t);
  a.idx = idx_dev; a.td = td_dev; a.B = B; a.head = h->head; a.cap = h->cfg.capacity; a.alpha = t->alpha; a.eps = t->eps; a.hist = hist_dev;
  hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(kOneWgThreads), 0, st, a);
  GCRL_HIP(hipGetLastError());
  t->launches++;
  return GCRL_OK;
}

bool per_next_beta(gcrl_her* h, float* beta) {
  gcrl_per_tree* t = h->per;
  if (!per_is_td(t) || t->beta_pos >= t->betas.size()) return false;
  *beta = t->betas[t->beta_pos++];
  return true;
}

}  // namespace gcrl

extern "C" {

int gcrl_per_attach(gcrl_her* h, float alpha, float eps) {
  GCRL_CHECK_ARG(h, "gcrl_per_attach: null ring");
  if (h->relabel_mode == GCRL_RELABEL_SAMPLE)   // a property of the ring, not of this call's arguments (whether or not it has an energy tree)
    return gcrl::fail(GCRL_ERR_STATE, "gcrl_per_attach: relabel: a ring with sample-time relabelling (GCRL_RELABEL_SAMPLE) takes no priority tree");
  GCRL_CHECK_ARG(!h->per, "gcrl_per_attach: the ring already has a priority tree");
  GCRL_CHECK_ARG(std::isfinite(alpha) && alpha >= 0.0f && std::isfinite(eps) && eps > 0.0f, "gcrl_per_attach: alpha %g (>= 0) / eps %g (> 0)", (double)alpha, (double)eps);
  gcrl_per_tree* t = nullptr;
  if (int rc = gcrl::per_tree_alloc(h, "gcrl_per_attach", &t)) return rc;
  t->alpha = alpha; t->eps = eps;
  t->synced_rows = h->rows_pushed - (uint64_t)h->len;   // rows already in the ring: priority 1.0 at the first refresh
  h->per = t;
  return GCRL_OK;
}

int gcrl_per_attached(const gcrl_her* h) { return h && h->per ? 1 : 0; }

int gcrl_per_levels(const gcrl_her* h) { return h && h->per ? h->per->L.levels : 0; }

int64_t gcrl_per_level_size(const gcrl_her* h, int level) {
  return (h && h->per && level >= 0 && level < h->per->L.levels) ? h->per->L.padded[level] : -1;
}

int gcrl_per_draw(gcrl_her* h, int B, float beta, uint32_t* idx_dev, float* w_dev, void* stream) {
  GCRL_CHECK_ARG(h, "gcrl_per_draw: null ring");
  return gcrl::per_draw(h, B, beta, idx_dev, w_dev, h->pick(stream));
}

int gcrl_per_update(gcrl_her* h, const uint32_t* idx_dev, const float* td_dev, int B, void* stream) {
  GCRL_CHECK_ARG(h, "gcrl_per_update: null ring");
  return gcrl::per_update(h, idx_dev, td_dev, B, nullptr, h->pick(stream));
}

int gcrl_per_set_betas(gcrl_her* h, const float* betas_host, int n) {
  if (int rc = need_tree(h, "gcrl_per_set_betas", false, true)) return rc;
  GCRL_CHECK_ARG(n >= 0 && (betas_host || n == 0), "gcrl_per_set_betas: null array");
  h->per->betas.assign(betas_host, betas_host + n);
  h->per->beta_pos = 0;
  return GCRL_OK;
}

int gcrl_per_get_priorities(gcrl_her* h, float* out_host, int64_t n) {
  if (int rc = need_tree(h, "gcrl_per_get_priorities")) return rc;
  GCRL_CHECK_ARG(out_host && n == h->len, "gcrl_per_get_priorities: %lld values asked, the ring holds %lld rows", (long long)n, (long long)h->len);
  GCRL_HIP(hipDeviceSynchronize());   // pushes, draws and updates run on the caller's streams
  if (int rc = gcrl::per_refresh(h, h->stream)) return rc;
  GCRL_HIP(hipStreamSynchronize(h->stream));
  const int64_t cap = h->cfg.capacity;
  std::vector<float> leaves((size_t)cap);
  GCRL_HIP(hipMemcpy(leaves.data(), h->per->tree, (size_t)cap * sizeof(float), hipMemcpyDeviceToHost));
  for (int64_t j = 0; j < n; ++j) out_host[j] = leaves[(size_t)gcrl::per_slot_of(j, h->head, cap)];
  return GCRL_OK;
}

int gcrl_per_set_priorities(gcrl_her* h, const float* in_host, int64_t n) {
  if (int rc = need_tree(h, "gcrl_per_set_priorities", false)) return rc;
  GCRL_CHECK_ARG(in_host && n == h->len, "gcrl_per_set_priorities: %lld values given, the ring holds %lld rows", (long long)n, (long long)h->len);
  double sum = 0.0;
  for (int64_t j = 0; j < n; ++j) {
    GCRL_CHECK_ARG(std::isfinite(in_host[j]) && in_host[j] >= 0.0f, "gcrl_per_set_priorities: priority %lld is %g (finite, >= 0)", (long long)j, (double)in_host[j]);
    sum += in_host[j];
  }
  GCRL_CHECK_ARG(n == 0 || sum > 0.0, "gcrl_per_set_priorities: every priority is zero: nothing could be drawn");
  gcrl_per_tree* t = h->per;
  const int64_t cap = h->cfg.capacity;
  std::vector<float> leaves((size_t)t->L.padded[0], 0.0f);
  for (int64_t j = 0; j < n; ++j) leaves[(size_t)gcrl::per_slot_of(j, h->head, cap)] = in_host[j];
  GCRL_HIP(hipDeviceSynchronize());
  GCRL_HIP(hipMemcpy(t->tree, leaves.data(), leaves.size() * sizeof(float), hipMemcpyHostToDevice));
  if (int rc = rebuild(t, h->stream)) return rc;
  GCRL_HIP(hipStreamSynchronize(h->stream));
  t->synced_rows = h->rows_pushed;
  t->stale = false;
  return GCRL_OK;
}

int gcrl_per_read_level(gcrl_her* h, int level, float* out_host, int64_t n) {
  if (int rc = need_tree(h, "gcrl_per_read_level")) return rc;
  gcrl_per_tree* t = h->per;
  GCRL_CHECK_ARG(level >= 0 && level < t->L.levels, "gcrl_per_read_level: level %d of %d", level, t->L.levels);
  GCRL_CHECK_ARG(out_host && n == t->L.padded[level], "gcrl_per_read_level: level %d has %lld entries, %lld asked", level, (long long)t->L.padded[level], (long long)n);
  GCRL_HIP(hipDeviceSynchronize());
  if (int rc = gcrl::per_refresh(h, h->stream)) return rc;
  GCRL_HIP(hipStreamSynchronize(h->stream));
  GCRL_HIP(hipMemcpy(out_host, t->tree + t->L.off[level], (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return GCRL_OK;
}

int64_t gcrl_per_get_draw_counter(const gcrl_her* h) { return h && h->per ? (int64_t)h->per->draws : -1; }

int gcrl_per_set_draw_counter(gcrl_her* h, int64_t counter) {
  if (int rc = need_tree(h, "gcrl_per_set_draw_counter", false, true)) return rc;
  GCRL_CHECK_ARG(counter >= 0, "gcrl_per_set_draw_counter: counter %lld", (long long)counter);
  h->per->draws = (uint64_t)counter;
  return GCRL_OK;
}

int64_t gcrl_per_launches(const gcrl_her* h) { return h && h->per ? h->per->launches : -1; }

}  // extern "C"
