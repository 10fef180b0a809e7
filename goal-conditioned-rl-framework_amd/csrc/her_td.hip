// her_td.hip — TD-error prioritised replay of a sample-mode HER ring (prioritise = "td_error").
//
// The ring gets a priority tree of per_tree.hip's layout (per_host.h) whose leaves follow the loss: a drawn row's leaf becomes
// (|td| + eps)^alpha after the step that trained on it, as in §4h.  What differs from the PER buffer is the priority of a NEW row:
// not the constant 1.0 of the reference's PERBuffer.push but the largest priority seen so far, the PER paper's own rule, kept in one
// fp32 word `p_max` on the device (initially 1.0f).  A flush seeds the rows it wrote with that word as it stands in stream order; a
// priority update raises it.  Neither is ever read back in the loop.  The rule is restated in numpy in tests/her_td_ref.py, which is
// its definition.  The draw and the weights are per_tree.hip's launches, unchanged.
//
// A translation unit of its own: the kernels of per_tree.hip, her_prio.hip and her_relabel.hip keep their code, byte for byte.
// Neither kernel here waits for another workgroup, uses atomics or per-thread scratch; every store is a plain vector store.
#include "her_ring.h"
#include "per_tree.h"

#include <cmath>

namespace {

using gcrl::kPerFan;
using gcrl::kPerMaxLevels;

constexpr int kOneWgThreads = 1024;   // both kernels: one workgroup of 16 waves, the levels separated by barriers
constexpr int kOneWgWaves = kOneWgThreads / 64;
constexpr float kFltMax = 3.402823466e+38f;

#include "per_tree_dev.inc"   // TreeView, wave_sum64 (the tree's one reduction order), reduce_range, view_of: per_tree.hip's own

// ONE workgroup, behind the flush launch whose rows it seeds: p_max is loaded once, written to the (at most two) slot segments the
// flush wrote, then their ancestors level by level, a barrier between the levels — per_refresh_kernel's shape with the value read
// from memory.  The segments are the host's (per_pending_segments): inside [0, cap) by construction.
__global__ __launch_bounds__(kOneWgThreads) void her_td_seed_kernel(TreeView t, const float* __restrict__ p_max, long long a0, long long a1,
                                                                    long long b0, long long b1) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const float value = *p_max;
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

struct TdUpdArgs {
  TreeView t;
  const uint32_t* idx;
  const float* td;
  int B;
  long long head, cap;
  float alpha, eps;
  float* hist;
  float* p_max;
};

// ONE workgroup of 16 waves.  per_update_kernel's leaf stage — leaf of idx[b] <- (|td_b| + eps)^alpha where b is the LAST occurrence
// of its index; an index >= cap is skipped — and its ancestor stage, plus the reduction that raises p_max: m = the largest FINITE
// new value over all B rows with an index inside the ring (the overwritten occurrences of a duplicate included), in one order — per
// thread its rows in order, the wave's xor-butterfly 32 .. 1, then the waves' LDS words in wave order — and p_max <- fmaxf(p_max, m),
// written by thread 0 after the barrier that follows the leaf stage.  A NaN or infinite value is written to its leaf as §4h writes it
// and never reaches m; m starts at 0, so p_max never decreases.
__global__ __launch_bounds__(kOneWgThreads) void her_td_update_kernel(TdUpdArgs a) {
  __shared__ float smax[kOneWgWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  float m = 0.0f;
  for (int b = threadIdx.x; b < a.B; b += blockDim.x) {
    const uint32_t j = a.idx[b];
    const float td = a.td[b];
    if (a.hist) a.hist[b] = td;
    const bool inside = (long long)j < a.cap;
    const float x = __fadd_rn(fabsf(td), a.eps);
    const float v = a.alpha == 1.0f ? x : powf(x, a.alpha);
    if (inside && v <= kFltMax) m = fmaxf(m, v);   // (NaN and +inf fail the compare)
    bool last = inside;
    for (int c = b + 1; last && c < a.B; ++c) last = a.idx[c] != j;
    if (last) {
      long long slot = a.head + (long long)j;
      if (slot >= a.cap) slot -= a.cap;
      a.t.tree[slot] = v;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if (lane == 0) smax[wave] = m;
  for (int k = 1; k <= a.t.levels; ++k) {
    __syncthreads();
    if (k == 1 && threadIdx.x == 0) {
      float mx = smax[0];
      for (int w = 1; w < nwaves; ++w) mx = fmaxf(mx, smax[w]);
      *a.p_max = fmaxf(*a.p_max, mx);
    }
    if (k == a.t.levels) break;   // (a one-level tree: the barrier above still orders smax for thread 0)
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

int need_td(const gcrl_her* h, const char* who) {
  if (!h || !gcrl::per_is_her_td(h->per))
    return gcrl::fail(GCRL_ERR_STATE, "%s: prioritise: no TD-error tree is attached to this ring (gcrl_her_td_attach)", who);
  return GCRL_OK;
}

}  // namespace

namespace gcrl {

bool her_td_on(const gcrl_her* h) { return h && per_is_her_td(h->per); }

int her_td_flush(gcrl_her* h, int64_t total, hipStream_t st) {
  gcrl_per_tree* t = h->per;
  if (!per_is_her_td(t)) return GCRL_OK;
  // the ring's head / len are already those after the flush: its rows are the last min(total, cap) ones before the tail
  const PerSegs s = per_pending_segments(h->head, h->len, h->cfg.capacity, total);
  t->synced_rows = h->rows_pushed;   // (per_tree.hip's lazy 1.0-writing refresh never fires on such a tree)
  if ((s.a1 - s.a0) + (s.b1 - s.b0) <= 0) return GCRL_OK;
  hipLaunchKernelGGL(her_td_seed_kernel, dim3(1), dim3(kOneWgThreads), 0, st, view_of(t), (const float*)t->p_max, (long long)s.a0, (long long)s.a1,
                     (long long)s.b0, (long long)s.b1);
  GCRL_HIP(hipGetLastError());
  t->launches++;
  return GCRL_OK;
}

int her_td_update(gcrl_her* h, const uint32_t* idx_dev, const float* td_dev, int B, float* hist_dev, hipStream_t st) {
  gcrl_per_tree* t = h->per;
  TdUpdArgs a;
  a.t = view_of(t);
  a.idx = idx_dev; a.td = td_dev; a.B = B; a.head = h->head; a.cap = h->cfg.capacity; a.alpha = t->alpha; a.eps = t->eps; a.hist = hist_dev;
  a.p_max = t->p_max;
  hipLaunchKernelGGL(her_td_update_kernel, dim3(1), dim3(kOneWgThreads), 0, st, a);
  GCRL_HIP(hipGetLastError());
  t->launches++;
  return GCRL_OK;
}

}  // namespace gcrl

extern "C" {

int gcrl_her_td_attach(gcrl_her* h, float alpha, float eps) {
  GCRL_CHECK_ARG(h, "gcrl_her_td_attach: prioritise: null ring");
  if (h->relabel_mode != GCRL_RELABEL_SAMPLE)
    return gcrl::fail(GCRL_ERR_STATE, "gcrl_her_td_attach: prioritise: the TD-error tree of a HER ring has one leaf per stored transition and needs "
                      "sample-time relabelling (GCRL_RELABEL_SAMPLE); this ring was created with GCRL_RELABEL_PUSH");
  if (h->per) return gcrl::fail(GCRL_ERR_STATE, "gcrl_her_td_attach: prioritise: the ring already has a priority tree");
  if (!(std::isfinite(alpha) && alpha >= 0.0f && std::isfinite(eps) && eps > 0.0f))
    return gcrl::fail(GCRL_ERR_ARG, "gcrl_her_td_attach: prioritise: alpha %g (finite, >= 0) / eps %g (finite, > 0)", (double)alpha, (double)eps);
  gcrl_per_tree* t = nullptr;
  if (int rc = gcrl::per_tree_alloc(h, "gcrl_her_td_attach", &t)) return rc;
  t->source = gcrl::kPerSourceTd;
  t->her_td = true;
  t->alpha = alpha; t->eps = eps;
  t->synced_rows = h->rows_pushed;
  const float one = 1.0f;   // p_max's initial value
  hipError_t e = hipMalloc((void**)&t->p_max, 64);
  if (e == hipSuccess) e = hipMemcpy(t->p_max, &one, sizeof(one), hipMemcpyHostToDevice);
  int rc = GCRL_OK;
  if (e == hipSuccess && h->len > 0) {   // rows from before the tree: p_max's initial value, then every node
    std::vector<float> leaves((size_t)t->L.padded[0], 0.0f);
    for (int64_t j = 0; j < h->len; ++j) leaves[(size_t)gcrl::per_slot_of(j, h->head, h->cfg.capacity)] = one;
    e = hipMemcpy(t->tree, leaves.data(), leaves.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) rc = gcrl::per_rebuild(t, h->stream);
    if (e == hipSuccess && rc == GCRL_OK) e = hipStreamSynchronize(h->stream);
  }
  if (e != hipSuccess || rc != GCRL_OK) {
    gcrl::per_tree_free(t);
    if (rc != GCRL_OK) return rc;
    GCRL_HIP(e);
  }
  h->per = t;
  return GCRL_OK;
}

int gcrl_her_td_get_pmax(gcrl_her* h, float* out_host) {
  if (int rc = need_td(h, "gcrl_her_td_get_pmax")) return rc;
  GCRL_CHECK_ARG(out_host, "gcrl_her_td_get_pmax: null output");
  GCRL_HIP(hipDeviceSynchronize());   // flushes and updates run on the caller's streams
  GCRL_HIP(hipMemcpy(out_host, h->per->p_max, sizeof(float), hipMemcpyDeviceToHost));
  return GCRL_OK;
}

int gcrl_her_td_set_pmax(gcrl_her* h, float value) {
  if (int rc = need_td(h, "gcrl_her_td_set_pmax")) return rc;
  GCRL_CHECK_ARG(std::isfinite(value) && value > 0.0f, "gcrl_her_td_set_pmax: p_max %g (finite, > 0)", (double)value);
  GCRL_HIP(hipDeviceSynchronize());
  GCRL_HIP(hipMemcpy(h->per->p_max, &value, sizeof(float), hipMemcpyHostToDevice));
  return GCRL_OK;
}

}  // extern "C"
