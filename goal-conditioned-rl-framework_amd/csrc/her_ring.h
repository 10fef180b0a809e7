// her_ring.h — internal view of the HER replay ring (shared with the update engine).
//
// HBM layout.  One transition = one packed record of RS floats, 64-byte aligned:
//     [ s (S) | a (A) | pad ]  [ ns (S) | pad ]  [ r | d ]  zero pad
//       <-- SA4 = roundup(S+A,4) -->  <-- S4 = roundup(S,4) -->      RS = roundup(SA4+S4+2, 16)
// Records are contiguous in arrival order: ring[cap][RS].  A uniformly random row gather then
// touches ceil(4*RS/128) whole 128-B lines per row (PickAndPlace: 2 lines for 208 useful
// bytes) where five separate field arrays would touch 6-7.  Every field group starts on a
// 16-byte boundary, so the update engine's batch matrices ([s|a], [ns|..], [s|..], row stride
// SA4) are plain float4 copies of record slices, and [s|a] is already the critic's input row.  Logical index j (0 = oldest, what random.sample indexes in the reference's
// deque, src/buffer.py:124) lives at physical row (head + j) mod cap; head/len are host state.
//
// Staging: per env, up to flush_len records of RG = roundup(RW+G, 16) floats: the ring record's
// RW = SA4+S4+2 leading floats, then ag (G)          (the dg column is the goal slot of s itself)
//
// Sample-time relabelling (relabel_mode == GCRL_RELABEL_SAMPLE; kernels in her_relabel.hip).  The ring stores an episode's T
// ORIGINAL rows only; a record carries a tail behind its RW leading floats — ag (G floats, the staged achieved goal) and
// `remaining` (one float holding the integer T-1-i) — so RS = roundup(RW+G+1, 16).  The leading RW floats keep the layout above:
// whatever reads only them (read_rows, the clone kernels, save / load by whole records) is unchanged.
// INVARIANT the relabelling gathers rest on: an episode's rows are appended by ONE flush, contiguously and in step order, and
// eviction is FIFO.  So if row i of an episode is alive, rows i+1 .. T-1 of that episode are alive, at physical slots
// (phys_i + 1 .. phys_i + remaining) mod cap.  Eviction of an episode's OLDEST rows is therefore harmless, and so is load_state's
// re-laying of the rows at head 0 (it keeps the logical order).  Every address a gather forms stays inside the ring whatever a
// tail holds: `remaining` is clamped to [0, min(flush_len, cap) - 1] after the load and the future slot phys + f is brought back
// into range by compare-and-subtract.  A flush in this mode draws nothing: the MT stream is not consumed by it.
// The relabel rule, for the c-th row ever gathered from the ring in this mode (relabel_ctr, a 64-bit counter the host advances by
// n when it issues a launch of n rows; it travels as a kernel argument, as IdxGen does), K = kRelabelStream:
//     relabel = rem > 0 && hash_below(seed, K, 2c, k_future + 1) != 0        (share k/(k+1): the reference's 1 original : k copies)
//     f       = 1 + hash_below(seed, K, 2c + 1, rem);   fut = phys + f (mod cap)
// a relabelled row takes record fut's tail ag as the goal of s and of ns, its reward by her_flush_kernel's arithmetic from the two
// tails, done = 0.  Restated in tests/her_relabel_ref.py, which is the definition.
// Goal selection (goal_strategy; the same kernels, definition tests/her_strategy_ref.py).  The rule above is
// GCRL_GOAL_FUTURE.  A ring created with GCRL_GOAL_EPISODE carries a second tail word, [ag (G) | remaining | elapsed]: `elapsed`, one
// float holding the integer i, so RS = roundup(RW+G+2, 16); it sits at tail index 2 + G + 1 <= 11 of the record from o_r on, so
// the gathers' 12-float tails hold it for G <= 8.  A lone appended row has elapsed = 0.  Rings of the other strategies keep the
// records above.  The INVARIANT, extended backwards: logical index 0 is the oldest live row and eviction is FIFO, so of the i rows
// of its episode that precede a row of logical index j, exactly min(i, j) are alive, at physical slots
// (phys - 1 .. phys - min(i, j)) mod cap — after a wrap, after load_state's re-laying at head 0, on a ring smaller than a flush.
// The gathers clamp `elapsed` to [0, min(min(flush_len, cap) - 1, j)] before any address is formed and bring phys + o, o signed,
// back into the ring by compare-and-subtract (o > 0) or compare-and-add (o < 0): every address stays inside the live ring
// whatever a tail holds.  GCRL_GOAL_FINAL takes o = remaining; GCRL_GOAL_EPISODE draws o uniformly from [-back, rem] \ {0}.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"

namespace gcrl {

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// uniform integer in [0, n) from a 64-bit counter hash — the device-RNG ("fast") mode of the
// future-index pick and of the batch draw.  Restated bit-for-bit in oracle/her_oracle.py.
__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint32_t hash_below(uint64_t seed, uint64_t stream, uint64_t ctr,
                                                uint32_t n) {
  uint64_t h = mix64(mix64(seed ^ (stream * 0xd1342543de82ef95ull)) + ctr);
  return (uint32_t)(((h >> 32) * (uint64_t)n) >> 32);  // multiply-high range reduction
}

constexpr uint64_t kRelabelStream = 0x52454c4142454c21ull;   // stream id of the sample-time relabel draws ("RELABEL!")

// device-RNG batch draw: batch element t of draw d is pi_{seed,d}(t), pi a keyed permutation of [0, n)
// (a 4-round balanced Feistel network over the next even power of two, cycle-walked back into range).
// A permutation gives the batch its without-replacement property by construction — no rejection, no
// communication between the elements: every gather lane computes its own row index, so the device mode
// needs neither a host RNG nor an index upload.  Restated in oracle/her_oracle.py (HashRng.sample).
struct IdxGen {
  uint64_t seed, draw0;   // draw number of the launch's first batch
  uint32_t n;             // population (ring length)
  int B, half_bits;       // batch size; the Feistel halves are half_bits wide
};

__host__ __device__ inline int feistel_half_bits(uint32_t n) {
  int bits = 2;
  while (bits < 32 && (1ull << bits) < (uint64_t)n) ++bits;
  return (bits + 1) >> 1;
}

__host__ __device__ inline uint32_t feistel_index(uint64_t seed, uint64_t draw, uint32_t n, int hb, uint32_t t) {
  const uint32_t mask = hb >= 32 ? 0xffffffffu : ((1u << hb) - 1u);
  const uint64_t key = mix64(seed ^ (draw * 0xd1342543de82ef95ull) ^ 0x5bd1e995ull);
  uint64_t x = t;
  do {
    uint32_t L = (uint32_t)(x >> hb) & mask, R = (uint32_t)x & mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t f = (uint32_t)(mix64(key + (uint64_t)r * 0x9e3779b97f4a7c15ull + R) >> 32) & mask;
      const uint32_t nl = R;
      R = L ^ f;
      L = nl;
    }
    x = ((uint64_t)L << hb) | R;
  } while (x >= (uint64_t)n);
  return (uint32_t)x;
}

__host__ __device__ inline uint32_t idxgen_at(const IdxGen& g, long long row) {
  const long long m = row / g.B;
  return feistel_index(g.seed, g.draw0 + (uint64_t)m, g.n, g.half_bits, (uint32_t)(row - m * g.B));
}

}  // namespace gcrl

struct gcrl_per_tree;
struct gcrl_normalizer;

struct gcrl_her {
  gcrl_her_config cfg;
  int S, A, G, SA4, S4, RW, RS, RG;   // o_ns = SA4, o_r = SA4+S4, o_d = o_r+1, o_ag = RW
  int relabel_mode = 0;               // GCRL_RELABEL_*
  int goal_strategy = 0;              // GCRL_GOAL_*: fixed at creation (GCRL_GOAL_EPISODE widens the record's tail)
  uint64_t relabel_ctr = 0;           // sample mode: rows ever gathered from this ring (the relabel stream's counter)
  int n_step = 1;                     // sample mode: rows folded into a gathered row's reward and done flag (her_relabel.hip); configuration, not state
  double nstep_gamma = 0.0;           // the discount of the ring's own gathers (gcrl_her_sample, gcrl_her_gather_update); the update engine passes the agent's
  gcrl_mt* rng = nullptr;
  bool own_rng = false;
  hipStream_t stream = nullptr;

  float* ring = nullptr;   // [cap][RS]
  float* stage = nullptr;  // [nenvs][flush_len][RG]
  int64_t head = 0, len = 0;
  std::vector<int> staged;
  uint64_t episodes_flushed = 0;  // stream id of the device RNG
  uint64_t draws_done = 0;        // batch-draw counter of the device RNG
  gcrl::IdxGen last_gen{};        // device-RNG mode: what the next gather launch computes its indices from
  bool idx_on_device = true;      // false: no index array was uploaded (device-RNG mode)
  uint64_t mutation_epoch = 0;    // bumped by every flush
  uint64_t rows_pushed = 0;       // rows ever appended (>= len): what the priority tree measures its pending pushes against
  int normalize_mode = 0;         // GCRL_NORMALIZE_*: SAMPLE = the records are raw, the gathers' batches are normalised behind the gather (her_norm.hip)
  gcrl_normalizer* nz_obs = nullptr;   // borrowed: the observation normaliser of columns [0, norm_D) of a state (null: left raw)
  gcrl_normalizer* nz_dg = nullptr;    // borrowed: the goal normaliser of columns [norm_D, S) (null: left raw)
  int norm_D = 0;
  int norm_need = 0;              // bit 0 / 1: a gather needs nz_obs / nz_dg bound (gcrl_her_require_normalize)
  gcrl_per_tree* per = nullptr;   // the ring's priority tree (per_tree.h), or null: TD priorities (per_tree.hip) or episode energies (her_prio.hip), by its source tag

  // index upload: pinned host slots -> idx_dev
  static constexpr int kSlots = 8;
  uint32_t* idx_pinned[kSlots] = {};
  hipEvent_t slot_ev[kSlots] = {};
  size_t slot_rows = 0;
  int next_slot = 0;
  uint32_t* idx_dev = nullptr;
  size_t idx_dev_rows = 0;
  // pinned slots for whole-episode uploads
  float* epi_pinned[kSlots] = {};
  hipEvent_t epi_ev[kSlots] = {};
  int next_epi_slot = 0;
  // future indices of a flush launch when they exceed the inline kernel-argument space (k_future >= 42)
  uint8_t* fut_dev = nullptr;
  uint8_t* fut_pinned[kSlots] = {};
  hipEvent_t fut_ev[kSlots] = {};
  int next_fut_slot = 0;
  // GCRL_REWARD_HOST: the caller's compute_reward evaluates every relabel slot of a flush on the host (gcrl_her_set_reward_callback)
  gcrl_reward_fn reward_cb = nullptr;
  void* reward_cb_user = nullptr;
  std::vector<float> ag_mirror;          // [nenvs][flush_len][G]: host copy of the staged achieved goals
  std::vector<float> cb_ag, cb_goal;     // pair lists handed to the callback
  float* rew_dev = nullptr;
  float* rew_pinned[kSlots] = {};
  hipEvent_t rew_ev[kSlots] = {};
  int next_rew_slot = 0;
  // raw observation rows of a vector-env step and their normalised [obs | goal] state matrices (gcrl_her_process_step)
  float* ps_dev = nullptr;
  float* ps_pinned[kSlots] = {};
  size_t ps_floats = 0;
  int64_t flush_calls = 0;               // flush groups a vector-env step's bookkeeping has issued (gcrl_her_flush_calls)
  // per-env payload of a vector-env step (gcrl_her_push_batch)
  float* pay_dev = nullptr;
  float* pay_pinned[kSlots] = {};

  // gather-launch timing (gcrl_her_profile_*)
  bool prof = false;
  std::vector<hipEvent_t> prof_a, prof_b;
  std::vector<int64_t> prof_pair_rows;   // rows of each pending bracketed launch
  int64_t prof_class_rows = 0;           // statistics are kept for the LARGEST launch size seen (a cycle's main gather)
  size_t prof_used = 0;
  int64_t prof_launches = 0, prof_rows = 0;
  double prof_ms = 0.0;

  // NULL -> the handle's own stream; GCRL_STREAM_LEGACY -> HIP's legacy default stream
  hipStream_t pick(void* s) const {
    if (!s) return stream;
    if (s == GCRL_STREAM_LEGACY) return (hipStream_t) nullptr;
    return (hipStream_t)s;
  }
};

struct gcrl_normalizer;

namespace gcrl {

// the ring's priority tree (per_tree.hip): freed with the ring; marked stale when the rows are reloaded into other slots
void per_release(gcrl_her* h);
void per_mark_stale(gcrl_her* h);

// device RunningNormalizer (normalizer.hip): statistics update from device rows; out[:, col0:col0+D] = normalize(x)
// (z == null: plain copy)
void normalizer_view(const gcrl_normalizer* z, const double** mean, const double** var, double** count, double* clip, int* mode = nullptr);   // mode: norm_math.h bits
void normalizer_updated(gcrl_normalizer* z);   // call after enqueuing a launch that updates z
int normalizer_update_dev(gcrl_normalizer* z, const float* x_dev, int n, int ld, hipStream_t st);
int normalizer_apply_dev(const gcrl_normalizer* z, const float* x_dev, int n, int ld, int D, float* out_dev, int ld_out, int col0,
                         hipStream_t st);

// Draw M*B logical indices (random.sample semantics per batch) into a pinned slot and upload
// them to h->idx_dev on `st`.  idx_host != NULL: use those instead of drawing.  Returns the
// pinned host copy through *host_copy (valid until kSlots more uploads).
int her_upload_indices(gcrl_her* h, int B, int M, const uint32_t* idx_host, hipStream_t st,
                       const uint32_t** host_copy);

// Gather for the update engine: rows idx_dev[0..n) -> three GEMM-ready matrices with row
// stride ldx = roundup(S+A,4): sa = [s|a], nsa = [ns|0..], spa = [s|0..] (may be null: not written); r[n], d[n].
// `idx_dev` may point into pinned (device-mapped) host memory: the update engine's head launch of a call reads its 256
// indices straight from the upload block.  cp_*: the same launch also copies cp_bytes (a multiple of 16) from cp_src
// (pinned host) to cp_dst (device) — the call's control block travels with its first gather instead of as copies before it.
int her_gather_update(gcrl_her* h, const uint32_t* idx_dev, int64_t n, float* sa, float* nsa,
                      float* spa, int ldx, float* r, float* d, hipStream_t st, const void* cp_src = nullptr,
                      void* cp_dst = nullptr, size_t cp_bytes = 0, const uint64_t* relabel_ctr = nullptr, const double* gamma = nullptr);
// A ring in sample-time relabelling mode takes her_gather_relabel_kernel instead (her_relabel.hip).  relabel_ctr == null: the
// launch's first row is the ring's relabel_ctr, which advances by n; otherwise *relabel_ctr, and the ring's counter is left
// alone (the planner of the call advanced it: GatherCall::ctr).  With n_step > 1 such a ring takes her_gather_nstep_kernel, which
// discounts by float(*gamma) — the caller's, as its TD kernels cast it — or, gamma == null, by the ring's own.

// sample-time relabelling mode (her_relabel.hip): the flush of `nep` staged episodes (T rows each, bookkeeping included), the
// update engine's gather and the public sample's, each starting at relabel counter `ctr`; the indices are idx or, when null,
// h->last_gen's.  Every goal_strategy and every n_step of the ring: the gathers pick the one-step or the n-step kernel by
// h->n_step and discount by g32 (not read at n_step == 1).
int her_relabel_flush(gcrl_her* h, int nep, const int* envs, const int* Ts, hipStream_t st, int64_t* rows_out);
int her_relabel_gather_update(gcrl_her* h, const uint32_t* idx, uint64_t ctr, float g32, int64_t n, float* sa, float* nsa, float* spa, int ldx,
                              float* r, float* d, hipStream_t st, const void* cp_src, void* cp_dst, size_t cp_bytes);
int her_relabel_sample(gcrl_her* h, const uint32_t* idx_dev, uint64_t ctr, float g32, int64_t n, float* out_s, int ld_s, float* out_a, int ld_a,
                       float* out_r, float* out_ns, int ld_ns, float* out_d, hipStream_t st);
// energy-prioritised draw of such a ring (her_prio.hip; a no-op / refusal unless gcrl_her_prio_attach gave it an energy tree).
// her_prio_flush: ONE launch behind a flush launch — the leaves of the rows it wrote (stage / Ts / tail / skip: that launch's own
// arguments; `total` its rows; the ring's head / len already advanced) and their ancestors.  her_prio_check: GCRL_ERR_STATE without a
// fresh energy tree.  her_prio_draw_at: rows c0 .. c0 + rows - 1 of the ring's draw stream -> idx_dev (logical indices), one launch;
// the ring's counter is the caller's to advance (the planner of an update call does, as with GatherCall::ctr).
int her_prio_flush(gcrl_her* h, int nep, const float* const* stage, const int* Ts, int64_t tail, int64_t skip, int64_t total, hipStream_t st);
// her_prio_on: the ring has an energy tree.  her_prio_take: the counter as of now, advanced by `rows`.
bool her_prio_on(const gcrl_her* h);
uint64_t her_prio_take(gcrl_her* h, int64_t rows);
int her_prio_check(const gcrl_her* h, const char* who);
int her_prio_draw_at(gcrl_her* h, uint64_t c0, int64_t rows, uint32_t* idx_dev, hipStream_t st);
// TD-error tree of such a ring (her_td.hip; a no-op unless gcrl_her_td_attach gave it one).  her_td_flush: ONE launch behind a flush
// launch of `total` rows (the ring's head / len already advanced) — their leaves <- p_max as that device word stands in stream
// order, their ancestors recomputed.  her_td_on: the ring has such a tree.
int her_td_flush(gcrl_her* h, int64_t total, hipStream_t st);
bool her_td_on(const gcrl_her* h);
// sample-time normalisation (her_norm.hip).  her_norm_on: the ring is raw.  her_norm_check: GCRL_ERR_STATE naming `normalize` when a
// normaliser the ring's gathers need is not bound — callers ask before a ticket or a counter is consumed.  her_norm_rows: the
// in-place pass over one gather's sa / nsa / spa (spa may be null; n rows of stride ldx), one launch.  her_norm_dense: the same for
// the public sample()'s out_s / out_ns.  Both are no-ops on a ring in the default mode.
bool her_norm_on(const gcrl_her* h);
int her_norm_check(const gcrl_her* h, const char* who);
int her_norm_rows(const gcrl_her* h, int64_t n, float* sa, float* nsa, float* spa, int ldx, hipStream_t st);
int her_norm_dense(const gcrl_her* h, int64_t n, float* out_s, int ld_s, float* out_ns, int ld_ns, hipStream_t st);
// the raw-store form of the fused process_step launch (her_norm.hip): her_process_step_kernel's two statistics updates, then the
// step's rows and achieved goals staged as they came.  ProcRawArgs is her_ring.hip's ProcArgs, field for field.
struct ProcRawArgs {
  float* stage; const float* raw; const float* pay;
  double* mean; double* var; double* count; double clip;
  double* gmean; double* gvar; double* gcount; double gclip;
  int update, gupdate, n, env0, flush_len, D, S, A, G, SA4, S4, RG;
  int mode, gmode;
};
constexpr int kProcRawInlineFloats = 896;
// data != null: the rows and the payload travel inside the kernel arguments (floats <= kProcRawInlineFloats of them, the payload
// from data[raw_floats] on); otherwise p.raw / p.pay
int her_process_step_raw(const ProcRawArgs& p, const float* data, int raw_floats, int floats, hipStream_t st);
int her_process_step_raw_pop(const ProcRawArgs* tab_dev, const float* data_dev, int stride, int raw_floats, int members, hipStream_t st);

// One her_gather_update call stated before it is issued (the update engine's begin_call plans it, gcrl_pop_update_n issues the
// members' calls together).  `gen` is the ring's IdxGen as of the member's turn: members that share a ring each keep their own.
// `ctr` likewise is the ring's relabel counter as of the member's turn (sample-time relabelling mode), `gamma` the member's discount
// as of plan time (n-step returns: members that share a ring each gather with their own).
struct GatherCall {
  gcrl_her* h = nullptr;
  const uint32_t* idx = nullptr;
  IdxGen gen{};
  uint64_t ctr = 0;
  double gamma = 0.0;
  int64_t n = 0;
  float *sa = nullptr, *nsa = nullptr, *spa = nullptr;
  int ldx = 0;
  float *r = nullptr, *d = nullptr;
  const void* cp_src = nullptr; void* cp_dst = nullptr; size_t cp_bytes = 0;
};
constexpr int kGatherPopMax = 16;   // members of one population gather launch (their argument records travel by value)

// The gathers of P members as ONE her_gather_update_pop_kernel launch (grid (ceil(rows / 64), P), member = blockIdx.y; the head
// form when any member carries a side copy); given the same indices, bit for bit the members' own her_gather_update launches.
// *merged says whether that launch was issued: with P == 1, unequal record layouts, a ring with gather timing on or the
// development gather variants, the members' own launches run in member order instead.  So they do when any ring is in
// sample-time relabelling mode (no merged launch for that mode).
int her_gather_update_pop(const GatherCall* c, int P, hipStream_t st, bool* merged);

// gcrl_pop_process_step (her_ring.hip): one vector-env step of `members` rings as ONE her_process_step_pop_kernel launch (workgroup m =
// member m), then each ring's finish_vector_step in member order.  The members' raw rows and payloads travel in a pinned, mapped block
// the kernel reads directly (no staged copy): kSlots slots used in rotation, each guarded by an event recorded after its launch — nothing
// waits for this launch, so a slot is refilled only once the launch that read it is known to be over (as ps_pinned / epi_ev above).
// The mapping is coherent host memory, which the device does not cache, and the host's writes precede the launch.
struct PopProcStep {
  static constexpr int kSlots = 8;
  char* blk_host = nullptr; char* blk_dev = nullptr;
  size_t slot_floats = 0;
  hipEvent_t ev[kSlots] = {};
  int next = 0;
  void* tabs = nullptr;    // PopTabCache of the members' ProcArgs tables (pop.h)
  int64_t calls = 0, launches = 0;
};
int her_process_step_pop(PopProcStep* ps, int members, gcrl_her* const* rings, gcrl_normalizer* const* nz_obs, int update_stats,
                         gcrl_normalizer* const* nz_dg, int update_goal_stats, const float* obs_host, const float* next_obs_host, int obs_dim,
                         const float* dg_host, const float* next_dg_host, const float* ag_host, const float* next_ag_host,
                         const float* actions_host, const float* rewards_host, const uint8_t* dones_host, int env0, int n,
                         int64_t* rows_out, void* stream);
void her_process_step_pop_release(PopProcStep* ps);
// The device-block form (gcrl_pop_collect): the same one launch on CALLER-OWNED device memory data_dev [members][stride] floats, a
// member's slice raw (raw_floats, all six blocks) | pay [n][kPayW] (dev_env.h gcrl_env_group), then the same host bookkeeping in
// member order.  Nothing is uploaded besides the cached table and nothing is waited for.  The payloads' t words must be
// the rings' staged counts: the caller checks its host mirror of them against every ring BEFORE the first step is issued.
int her_process_step_pop_dev(PopProcStep* ps, int members, gcrl_her* const* rings, gcrl_normalizer* const* nz_obs, int update_stats,
                             gcrl_normalizer* const* nz_dg, int update_goal_stats, const float* data_dev, int stride, int raw_floats, int obs_dim,
                             int n, int64_t* rows_out, void* stream);

}  // namespace gcrl
