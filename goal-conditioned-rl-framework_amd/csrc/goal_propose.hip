// goal_propose.hip — practice goals for the device goal envs (goal_propose.h gcrl_goal_proposer): an archive of raw achieved goals and,
// at an episode boundary, a min-density pick among hashed candidates of it that becomes the new episode's goal.  The rule is restated
// in numpy in tests/goal_propose_ref.py, which is its definition; the result is that file's bit for bit (the counts are integers, so
// how the density sum is split among threads does not matter).
//
//   append   after every vector step the step's N next_ag rows (the last block of the env's raw buffer) go to logical positions
//            len .. len + N - 1 of the circular archive; when it is full the oldest entries go.
//   propose  in a step in which an env rolled over (its host t was max_steps - 1 before the step; a reset is not a roll-over): q is
//            read and incremented; with L = len >= min_fill, every rolled-over env i
//              takes a proposal iff float(hash_below(seed, kTakeStream, q N + i, 2^24)) * 2^-24 < share,
//              draws candidate k at logical index hash_below(seed, kCandStream, (q N + i) C + k, L),            k = 0 .. C - 1,
//              counts for each the archive entries m in [0, L) with ((dx dx + dy dy) + dz dz) < radius * radius (float32, no contraction),
//              and gets the candidate of the smallest count, ties to the smallest k, as floats 9..11 of its state record and as
//              columns D..D + 2 of its acting row: the two places that hold a new episode's goal.
//   kTakeStream = 0x5052414354414b45 ("PRACTAKE"), kCandStream = 0x5052414343414e44 ("PRACCAND").
//
// Kernel rules (dev_env.hip's): every address comes from the handle and from indices brought into range before use, whatever the
// archive holds; no atomics; no waits between workgroups; no per-thread scratch; plain vector stores only; built with
// -ffp-contract=off.
#include <algorithm>
#include <cmath>

#include "goal_propose.h"
#include "her_ring.h"   // hash_below

namespace {

constexpr unsigned long long kTakeStream = 0x5052414354414b45ull;   // "PRACTAKE"
constexpr unsigned long long kCandStream = 0x5052414343414e44ull;   // "PRACCAND"
constexpr int kThreads = 256;
constexpr int kTileF4 = kGoalTile * 3 / 4;      // 16-byte words of a tile
constexpr int kTileGroups = kGoalTile / 4;      // groups of 4 entries = 3 whole 16-byte words
static_assert(kGoalTile % 4 == 0 && kTileGroups % kThreads == 0, "a tile is whole groups, a whole number of them per thread stripe");

// ---------------------------------------------------------------- append: one thread per float of the N rows
struct AppendArgs { const float* src; float* archive; int N, cap, tail; };
__global__ __launch_bounds__(kThreads) void goal_archive_append_kernel(AppendArgs a) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= 3 * a.N) return;
  const int i = f / 3, c = f - 3 * i;
  int slot = a.tail + i;                        // tail < cap and i < N <= cap: one compare brings it back
  if (slot >= a.cap) slot -= a.cap;
  a.archive[(size_t)3 * slot + c] = a.src[f];
}

// ---------------------------------------------------------------- propose: one workgroup per rolled-over env
struct ProposeArgs {
  const float* archive; float* state; float* rows;
  int cap, head, L, C, log2cp;                  // log2cp: log2 of C rounded up to a power of two
  int N, SW, D;
  float rho2, share;
  unsigned long long seed, qN;                  // qN = q * N
  uint32_t bits[kEnvMaxN / 32];                 // the rolled-over envs
};
static_assert(sizeof(ProposeArgs) <= 4096, "kernel arguments are limited to 4 KB");

__device__ inline int below_rho(float ex, float ey, float ez, float cx, float cy, float cz, float rho2) {
  const float dx = ex - cx, dy = ey - cy, dz = ez - cz;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  return d2 < rho2 ? 1 : 0;                     // a NaN entry counts for nobody
}

__global__ __launch_bounds__(kThreads) void goal_propose_kernel(ProposeArgs a) {
  __shared__ float4 tile[kTileF4];
  __shared__ float cand[kGoalMaxCand * 3];
  __shared__ int part[kThreads / 64][kGoalMaxCand];
  const int tid = threadIdx.x;
  // the env of this workgroup: the blockIdx.x-th set bit
  int want = blockIdx.x, env = -1;
#pragma unroll
  for (int w = 0; w < kEnvMaxN / 32; ++w) {
    uint32_t b = a.bits[w];
    const int pc = __popc(b);
    if (env < 0) {
      if (want < pc) {
        for (int j = 0; j < want; ++j) b &= b - 1;
        env = w * 32 + __ffs(b) - 1;
      } else {
        want -= pc;
      }
    }
  }
  if (env < 0 || env >= a.N) return;
  const unsigned long long ctr = a.qN + (unsigned long long)env;
  const float u = (float)gcrl::hash_below(a.seed, kTakeStream, ctr, 1u << 24) * (1.0f / 16777216.0f);
  if (!(u < a.share)) return;                   // the env keeps its task goal (the whole workgroup leaves)
  if (tid < a.C) {
    int slot = a.head + (int)gcrl::hash_below(a.seed, kCandStream, ctr * (unsigned long long)a.C + (unsigned long long)tid, (uint32_t)a.L);
    if (slot >= a.cap) slot -= a.cap;           // head < cap and the index < L <= cap
    const float* e = a.archive + (size_t)3 * slot;
    cand[3 * tid] = e[0]; cand[3 * tid + 1] = e[1]; cand[3 * tid + 2] = e[2];
  }
  __syncthreads();
  // thread = (candidate k, stripe): the threads of a stripe read the same entries (LDS broadcast)
  const int cp = 1 << a.log2cp, k = tid & (cp - 1), stripe = tid >> a.log2cp, stripes = kThreads >> a.log2cp;
  const int kc = k < a.C ? k : a.C - 1;         // (a lane past C counts for nobody: its sum is never read)
  const float cx = cand[3 * kc], cy = cand[3 * kc + 1], cz = cand[3 * kc + 2];
  // the live slots are [head, head + L) mod cap: one range, or after a wrap two that the tiles of [0, cap) cover
  const bool wraps = a.head + a.L > a.cap;
  const int lo = wraps ? 0 : a.head, hi = wraps ? a.cap : a.head + a.L;
  const int total_f4 = (a.cap * 3 + 3) / 4;     // the allocation holds these 16-byte words (and one more)
  const float4* arch4 = reinterpret_cast<const float4*>(a.archive);
  const float nan = __int_as_float(0x7fc00000);
  int cnt = 0;
  for (int t = lo / kGoalTile; t * kGoalTile < hi; ++t) {
    // stage: 16-byte loads; a float whose slot is not live becomes a NaN, which no comparison counts
#pragma unroll
    for (int v = tid; v < kTileF4; v += kThreads) {
      const int g4 = t * kTileF4 + v;
      float4 x = g4 < total_f4 ? arch4[g4] : make_float4(nan, nan, nan, nan);
      float w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int slot = (4 * g4 + c) / 3;
        int rel = slot - a.head;
        if (rel < 0) rel += a.cap;
        if (slot >= a.cap || rel >= a.L) w[c] = nan;
      }
      tile[v] = make_float4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
    for (int g = stripe; g < kTileGroups; g += stripes) {
      const float4 p0 = tile[3 * g], p1 = tile[3 * g + 1], p2 = tile[3 * g + 2];
      cnt += below_rho(p0.x, p0.y, p0.z, cx, cy, cz, a.rho2);
      cnt += below_rho(p0.w, p1.x, p1.y, cx, cy, cz, a.rho2);
      cnt += below_rho(p1.z, p1.w, p2.x, cx, cy, cz, a.rho2);
      cnt += below_rho(p2.y, p2.z, p2.w, cx, cy, cz, a.rho2);
    }
    __syncthreads();
  }
  // the lanes of a wave that share a candidate, then the waves through LDS
  for (int off = 32; off >= cp; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane < cp) part[wave][lane] = cnt;        // (cp == 64: a wave is one stripe and nothing was shuffled)
  __syncthreads();
  if (tid != 0) return;
  int best = 0, best_cnt = 0x7fffffff;
  for (int c = 0; c < a.C; ++c) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += part[w][c];
    if (s < best_cnt) { best_cnt = s; best = c; }   // strict: a tie stays with the smaller k
  }
  float* st = a.state + (size_t)env * a.SW + 9;
  float* row = a.rows + (size_t)env * (a.D + kEnvG) + a.D;
#pragma unroll
  for (int c = 0; c < 3; ++c) { const float v = cand[3 * best + c]; st[c] = v; row[c] = v; }
}

// ---------------------------------------------------------------- host side
constexpr uint32_t kGoalMagic = 0x4c414f47u;    // "GOAL"
struct GoalHeader {
  uint32_t magic; int32_t cap, C, min_fill; float radius, share; uint64_t seed;
  int32_t N, head, len, pad; uint64_t q; int64_t appended, roll_steps, patched;
};
static_assert(sizeof(GoalHeader) == 80, "the blob's header is 80 bytes");

size_t archive_bytes(const gcrl_goal_proposer* p) { return (size_t)p->cap * 3 * sizeof(float); }
size_t blob_bytes(const gcrl_goal_proposer* p) { return sizeof(GoalHeader) + archive_bytes(p); }
hipStream_t pick_stream(void* s) { return s == GCRL_STREAM_LEGACY ? (hipStream_t) nullptr : (hipStream_t)s; }

int settings_check(const char* who, int capacity, int candidates, float radius, float share, int min_fill) {
  GCRL_CHECK_ARG(capacity >= 1 && capacity <= kGoalMaxCap, "%s: capacity: %d (1..65536 required)", who, capacity);
  GCRL_CHECK_ARG(candidates >= 1 && candidates <= kGoalMaxCand, "%s: candidates: %d (1..64 required)", who, candidates);
  GCRL_CHECK_ARG(std::isfinite(radius) && radius > 0.f, "%s: radius: %g (finite and > 0 required)", who, (double)radius);
  GCRL_CHECK_ARG(share > 0.f && share <= 1.f, "%s: share: %g (must lie in (0, 1])", who, (double)share);
  GCRL_CHECK_ARG(min_fill >= 1 && min_fill <= capacity, "%s: min_fill: %d (1..capacity = %d required)", who, min_fill, capacity);
  return GCRL_OK;
}

// the binding rules on plain numbers, shared by goal_proposer_check and gcrl_goal_proposer_bind_check
int bind_check(const char* who, int capacity, int bound_n, int same_env, int device, int env_members, int env_n, int env_device) {
  GCRL_CHECK_ARG(env_members == 1, "%s: members: a group of %d members (practice goals are built for a standalone env)", who, env_members);
  GCRL_CHECK_ARG(env_device == device, "%s: device: the env lives on device %d, the proposer on device %d", who, env_device, device);
  GCRL_CHECK_ARG(bound_n == 0 || (same_env && bound_n == env_n), "%s: env: the proposer is bound to %s env of %d envs, this one has %d", who,
                 same_env ? "an" : "another", bound_n, env_n);
  GCRL_CHECK_ARG(capacity >= env_n, "%s: capacity: %d entries cannot take a step of %d envs", who, capacity, env_n);
  return GCRL_OK;
}

}  // namespace

namespace gcrl {

int goal_proposer_bind_check(const gcrl_goal_proposer* p, const gcrl_env_group* env, const char* who) {
  GCRL_CHECK_ARG(p && env, "%s: null proposer or env handle", who);
  const int same = !p->env_token || p->env_token == env->token;
  return bind_check(who, p->cap, p->N, same, p->device, env->P, env->N, env->device);
}

int goal_proposer_check(const gcrl_goal_proposer* p, const gcrl_env_group* env, const char* who) {
  if (int rc = goal_proposer_bind_check(p, env, who)) return rc;
  if (env->vsteps == 0 || env->vsteps == p->seen_vsteps)
    return fail(GCRL_ERR_STATE, "%s: env: no env step since %s: a step is taken in once, behind gcrl_env_step", who,
                env->vsteps == 0 ? "the env was created" : "the proposer's last step");
  return GCRL_OK;
}

int goal_proposer_step_launch(gcrl_goal_proposer* p, gcrl_env_group* env, hipStream_t st, long long* launches) {
  const int N = env->N, cap = p->cap;
  AppendArgs ap{env->raw() + (size_t)N * (2 * env->D + 3 * kEnvG), p->archive, N, cap, (p->head + p->len) % cap};
  hipLaunchKernelGGL(goal_archive_append_kernel, dim3((3 * N + kThreads - 1) / kThreads), dim3(kThreads), 0, st, ap);
  GCRL_HIP(hipGetLastError());
  *launches += 1;
  const int over = p->len + N - cap;
  if (over > 0) { p->head = (p->head + over) % cap; p->len = cap; } else { p->len += N; }
  p->appended += N;
  p->env_token = env->token; p->N = N; p->seen_vsteps = env->vsteps;
  ProposeArgs pa;
  std::memset(&pa, 0, sizeof(pa));
  int rolled = 0, takers = 0;
  const unsigned long long qN = (unsigned long long)p->q * (unsigned long long)N;
  for (int i = 0; i < N; ++i) {
    if (!env->rolled[i]) continue;
    pa.bits[i >> 5] |= 1u << (i & 31);
    rolled += 1;
    if ((float)hash_below(p->seed, kTakeStream, qN + (unsigned long long)i, 1u << 24) * (1.0f / 16777216.0f) < p->share) takers += 1;
  }
  if (!rolled) return GCRL_OK;
  p->q += 1;
  p->roll_steps += 1;
  if (p->len < p->min_fill) return GCRL_OK;
  pa.archive = p->archive; pa.state = env->state; pa.rows = env->rows;
  pa.cap = cap; pa.head = p->head; pa.L = p->len; pa.C = p->C;
  while ((1 << pa.log2cp) < p->C) pa.log2cp += 1;
  pa.N = N; pa.SW = env->SW; pa.D = env->D;
  pa.rho2 = p->radius * p->radius; pa.share = p->share;
  pa.seed = p->seed; pa.qN = qN;
  hipLaunchKernelGGL(goal_propose_kernel, dim3(rolled), dim3(kThreads), 0, st, pa);
  GCRL_HIP(hipGetLastError());
  *launches += 1;
  p->patched += takers;
  return GCRL_OK;
}

}  // namespace gcrl

extern "C" {

gcrl_goal_proposer* gcrl_goal_proposer_create(int capacity, int candidates, float radius, float share, int min_fill, uint64_t seed, int device) {
  const char* who = "gcrl_goal_proposer_create";
  if (settings_check(who, capacity, candidates, radius, share, min_fill)) return nullptr;
  const int ndev = gcrl_device_count();
  if (ndev <= 0 || device < 0 || device >= ndev) {
    gcrl::fail(GCRL_ERR_HIP, "%s: no usable HIP device (count=%d, requested %d); there is no CPU fallback", who, ndev, device);
    return nullptr;
  }
  gcrl_goal_proposer* p = new gcrl_goal_proposer;
  p->cap = capacity; p->C = candidates; p->radius = radius; p->share = share; p->min_fill = min_fill; p->seed = seed; p->device = device;
  const size_t bytes = (archive_bytes(p) + 15) / 16 * 16 + 16;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc((void**)&p->archive, bytes);
  if (e == hipSuccess) e = hipMemset(p->archive, 0, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    gcrl::fail(GCRL_ERR_HIP, "%s: archive allocation failed: %s", who, hipGetErrorString(e));
    gcrl_goal_proposer_destroy(p);
    return nullptr;
  }
  return p;
}

void gcrl_goal_proposer_destroy(gcrl_goal_proposer* p) {
  if (!p) return;
  if (p->archive) { (void)hipDeviceSynchronize(); (void)hipFree(p->archive); }
  delete p;
}

int gcrl_goal_proposer_bind_check(int capacity, int bound_num_envs, int same_env, int device, int env_members, int env_num_envs, int env_device) {
  return bind_check("gcrl_goal_proposer_bind_check", capacity, bound_num_envs, same_env, device, env_members, env_num_envs, env_device);
}

int gcrl_goal_proposer_step(gcrl_goal_proposer* p, gcrl_env* env, void* stream) {
  if (int rc = gcrl::goal_proposer_check(p, env, "gcrl_goal_proposer_step")) return rc;
  long long launches = 0;
  return gcrl::goal_proposer_step_launch(p, env, env->pick(stream), &launches);
}

int gcrl_goal_proposer_stats(const gcrl_goal_proposer* p, int64_t* appended, int64_t* roll_steps, int64_t* patched) {
  GCRL_CHECK_ARG(p, "gcrl_goal_proposer_stats: null handle");
  if (appended) *appended = p->appended;
  if (roll_steps) *roll_steps = p->roll_steps;
  if (patched) *patched = p->patched;
  return GCRL_OK;
}

int gcrl_goal_proposer_get(const gcrl_goal_proposer* p, int* capacity, int* candidates, float* radius, float* share, int* min_fill, uint64_t* seed,
                           int* device, int* num_envs, int* head, int* len, uint64_t* counter, int* tile) {
  GCRL_CHECK_ARG(p, "gcrl_goal_proposer_get: null handle");
  if (capacity) *capacity = p->cap;
  if (candidates) *candidates = p->C;
  if (radius) *radius = p->radius;
  if (share) *share = p->share;
  if (min_fill) *min_fill = p->min_fill;
  if (seed) *seed = p->seed;
  if (device) *device = p->device;
  if (num_envs) *num_envs = p->N;
  if (head) *head = p->head;
  if (len) *len = p->len;
  if (counter) *counter = p->q;
  if (tile) *tile = kGoalTile;
  return GCRL_OK;
}

int gcrl_goal_proposer_read(gcrl_goal_proposer* p, float* dst_host, void* stream) {
  GCRL_CHECK_ARG(p && dst_host, "gcrl_goal_proposer_read: null argument");
  hipStream_t st = pick_stream(stream);
  const int first = std::min(p->len, p->cap - p->head);   // entries from head to the end of the allocation
  if (first > 0) GCRL_HIP(hipMemcpyAsync(dst_host, p->archive + (size_t)3 * p->head, (size_t)first * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  if (p->len > first) GCRL_HIP(hipMemcpyAsync(dst_host + (size_t)3 * first, p->archive, (size_t)(p->len - first) * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  GCRL_HIP(hipStreamSynchronize(st));
  return GCRL_OK;
}

int64_t gcrl_goal_proposer_state_bytes(const gcrl_goal_proposer* p) { return p ? (int64_t)blob_bytes(p) : 0; }

// blob: GoalHeader | the archive's cap * 3 floats at their physical slots
int gcrl_goal_proposer_save_state(gcrl_goal_proposer* p, void* dst_host, int64_t n, void* stream) {
  GCRL_CHECK_ARG(p && dst_host && n == (int64_t)blob_bytes(p), "gcrl_goal_proposer_save_state: the blob is %lld bytes", p ? (long long)blob_bytes(p) : 0ll);
  const GoalHeader hd{kGoalMagic, p->cap, p->C, p->min_fill, p->radius, p->share, p->seed, p->N, p->head, p->len, 0, p->q, p->appended, p->roll_steps, p->patched};
  std::memcpy(dst_host, &hd, sizeof(hd));
  hipStream_t st = pick_stream(stream);
  GCRL_HIP(hipMemcpyAsync(static_cast<char*>(dst_host) + sizeof(hd), p->archive, archive_bytes(p), hipMemcpyDeviceToHost, st));
  GCRL_HIP(hipStreamSynchronize(st));
  return GCRL_OK;
}

int gcrl_goal_proposer_load_state(gcrl_goal_proposer* p, const void* src_host, int64_t n, void* stream) {
  const char* who = "gcrl_goal_proposer_load_state";
  GCRL_CHECK_ARG(p && src_host && n >= (int64_t)sizeof(GoalHeader), "%s: null argument or a blob shorter than its header", who);
  GoalHeader hd;
  std::memcpy(&hd, src_host, sizeof(hd));
  GCRL_CHECK_ARG(hd.magic == kGoalMagic, "%s: not a goal proposer state blob", who);
  GCRL_CHECK_ARG(hd.cap == p->cap, "%s: capacity: the blob holds %d, the handle %d", who, hd.cap, p->cap);
  GCRL_CHECK_ARG(hd.C == p->C, "%s: candidates: the blob holds %d, the handle %d", who, hd.C, p->C);
  GCRL_CHECK_ARG(std::memcmp(&hd.radius, &p->radius, sizeof(float)) == 0, "%s: radius: the blob holds %g, the handle %g", who, (double)hd.radius, (double)p->radius);
  GCRL_CHECK_ARG(std::memcmp(&hd.share, &p->share, sizeof(float)) == 0, "%s: share: the blob holds %g, the handle %g", who, (double)hd.share, (double)p->share);
  GCRL_CHECK_ARG(hd.min_fill == p->min_fill, "%s: min_fill: the blob holds %d, the handle %d", who, hd.min_fill, p->min_fill);
  GCRL_CHECK_ARG(hd.seed == p->seed, "%s: seed: the blob holds %llu, the handle %llu", who, (unsigned long long)hd.seed, (unsigned long long)p->seed);
  GCRL_CHECK_ARG(hd.N >= 0 && hd.N <= kEnvMaxN && (hd.N == 0 || p->N == 0 || hd.N == p->N), "%s: num_envs: the blob was written for %d envs, the handle is bound to %d", who,
                 hd.N, p->N);
  GCRL_CHECK_ARG(hd.head >= 0 && hd.head < p->cap, "%s: head: %d outside [0, capacity)", who, hd.head);
  GCRL_CHECK_ARG(hd.len >= 0 && hd.len <= p->cap, "%s: len: %d outside [0, capacity]", who, hd.len);
  GCRL_CHECK_ARG(n == (int64_t)blob_bytes(p), "%s: the blob is %lld bytes, expected %lld", who, (long long)n, (long long)blob_bytes(p));
  hipStream_t st = pick_stream(stream);
  GCRL_HIP(hipMemcpyAsync(p->archive, static_cast<const char*>(src_host) + sizeof(hd), archive_bytes(p), hipMemcpyHostToDevice, st));
  GCRL_HIP(hipStreamSynchronize(st));   // (the source is the caller's pageable memory)
  if (hd.N) p->N = hd.N;
  p->head = hd.head; p->len = hd.len; p->q = hd.q;
  p->appended = hd.appended; p->roll_steps = hd.roll_steps; p->patched = hd.patched;
  return GCRL_OK;
}

}  // extern "C"
