// dev_env.hip — three built-in goal environments that live on the device (dev_env.h), and the small launches the device-row acting
// entries and the collect loop of agent.hip need around them.
//
//   reach (D = 7, A = 3)    a point mass in a box: obs = [pos, vel, t / T], achieved goal = pos
//   push  (D = 13, A = 3)   a pusher and a puck on the plane z = 0: obs = [p, q, q - p, vel_p, t / T], achieved goal = q; the puck moves by
//                           the pusher's planar displacement while the pusher's new position is inside the contact radius
//   pick  (D = 20, A = 4)   a gripper with a finger opening w and an object that rests on the table: obs = [p, q, q - p, vel_p, vel_q, w,
//                           vel_w, held, near, t / T], achieved goal = q; the object is grasped when the fingers close around it, moves
//                           with the gripper while they stay closed and falls when released; half the goals lie in the air
//
// G = 3, fixed horizon T, sparse reward -(dist > thr) formed as the replay ring's relabelling kernels form it, no termination.
// All arithmetic is float32, one rounding per operation (the unit is built with -ffp-contract=off): + - * /, comparisons,
// fminf / fmaxf and the correctly rounded square root of the reward's distance.  The rule — constants, operation order, what a NaN
// action counts as, the random-number keys — is restated in numpy in tests/dev_env_ref.py (reach, push) and
// tests/dev_env_pick_ref.py (pick), which are its definition.
//
// Random numbers: u(env, episode, component) = hash_below(seed, kEnvStream + env, 8 * episode + component, 2^24) * 2^-24.  No state
// besides the counters, so an env's episode j is the same whatever N is and whenever it is reached.
//
// What an env's thread does on a reset and on a step lives in dev_env_body.h (env_reset_body, env_step_body): the kernels here and the
// population kernels of dev_env_group.hip (gcrl_env_group: P x N envs in single allocations) call the same text, each on the EnvArgs of
// one standalone env — so member m of a group IS a gcrl_env of seeds[m].
//
// Kernel rules: every address comes from the handle or the group's member table (or, for the pack and fill launches, from the
// caller's checked arguments); an env index >= N — for a group: a member index >= P — does nothing; no atomics; no waits between
// workgroups; no per-thread scratch (every loop is over a small constant and unrolled); plain vector stores only.
#include "dev_env.h"

#include <vector>

#include "dev_env_body.h"   // EnvArgs, env_reset_body, env_step_body

namespace {

// the selection travels inside the kernel arguments (N <= 1024): one byte per env, ignored on a restart
struct ResetArgs { EnvArgs a; unsigned char mask[kEnvMaxN]; };
static_assert(sizeof(ResetArgs) <= 4096, "kernel arguments are limited to 4 KB");
__global__ __launch_bounds__(64) void env_reset_kernel(ResetArgs q) {
  const EnvArgs& a = q.a;
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.N) return;
  if (!a.restart && !q.mask[i]) return;
  env_reset_body(a, i);
}

__global__ __launch_bounds__(64) void env_step_kernel(EnvArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.N) return;
  env_step_body(a, i);
}

__global__ __launch_bounds__(256) void proc_pack_kernel(gcrl::ProcPack p) {
  const int n = p.n, D = p.D, G = p.G, A = p.A;
  const int per = 2 * D + 4 * G + 3 + A + G;      // elements written per env
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)n * per) return;
  const int i = (int)(e / per); int c = (int)(e - (long long)i * per);
  float* raw = p.raw; float* pw = p.pay + (size_t)i * kEnvPayW;
  if (c < D) { raw[(size_t)i * D + c] = p.obs[(size_t)i * D + c]; return; }
  c -= D;
  if (c < D) { raw[(size_t)n * D + (size_t)i * D + c] = p.nobs[(size_t)i * D + c]; return; }
  c -= D;
  float* g0 = raw + (size_t)2 * n * D;
  if (c < 4 * G) {
    const int b = c / G, k = c - b * G;
    const float* src = b == 0 ? p.dg : b == 1 ? p.ndg : b == 2 ? p.ag : p.nag;
    if (b >= 2 && !p.ag) return;
    g0[(size_t)b * n * G + (size_t)i * G + k] = src[(size_t)i * G + k];
    return;
  }
  c -= 4 * G;
  if (c == 0) pw[0] = __int_as_float(p.t ? p.t[i] : p.t0);
  else if (c == 1) pw[1] = p.rew[i];
  else if (c == 2) pw[2] = 0.f;
  else if (c < 3 + A) pw[c] = p.act[(size_t)i * A + (c - 3)];
  else pw[c] = p.nag[(size_t)i * G + (c - 3 - A)];
}

__global__ __launch_bounds__(256) void clipped_normal_fill_kernel(float* out, int n, unsigned long long seed, unsigned long long ctr0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = fminf(fmaxf(gcrl::hash_normal(seed, ctr0 + (unsigned long long)i), -1.0f), 1.0f);
}
__global__ __launch_bounds__(256) void normal_fill_kernel(void* out, int f64, int n, unsigned long long seed, unsigned long long ctr0, double scale) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = (double)gcrl::hash_normal(seed, ctr0 + (unsigned long long)i) * scale;
  if (f64) static_cast<double*>(out)[i] = v;
  else static_cast<float*>(out)[i] = (float)v;
}
__global__ __launch_bounds__(256) void round_to_f32_kernel(const double* in64, float* out32, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out32[i] = (float)in64[i];
}

EnvArgs base_args(gcrl_env* e) {
  EnvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.state = e->state; a.t = e->t; a.cnt = e->cnt; a.rsum = e->rsum;
  a.rows = e->rows; a.raw = e->raw; a.pay = e->pay;
  a.kind = e->kind; a.N = e->N; a.T = e->T; a.D = e->D; a.thr = e->thr; a.seed = e->seed;
  return a;
}

bool known_kind(int kind) { return kind == GCRL_ENV_REACH || kind == GCRL_ENV_PUSH || kind == GCRL_ENV_PICK; }

size_t state_bytes(const gcrl_env* e) {
  return sizeof(EnvHeader) + (size_t)e->N * (e->SW * sizeof(float) + sizeof(int) + 3 * sizeof(unsigned long long) + sizeof(double)) +
         (size_t)e->N * (e->D + kEnvG) * sizeof(float);
}

}  // namespace

namespace gcrl {

int env_step_launch(gcrl_env* e, const void* actions_dev, int f64, hipStream_t st) { return env_step_launch_noise(e, actions_dev, f64, nullptr, 0, 0, 0, 0.0, st); }

int env_step_launch_noise(gcrl_env* e, const void* actions_dev, int f64, void* noise, int noise_f64, unsigned long long noise_seed,
                          unsigned long long noise_ctr0, double noise_scale, hipStream_t st) {
  EnvArgs a = base_args(e);
  a.act = actions_dev; a.act_f64 = f64 ? 1 : 0;
  a.noise = noise; a.noise_f64 = noise_f64; a.noise_seed = noise_seed; a.noise_ctr0 = noise_ctr0; a.noise_scale = noise_scale;
  hipLaunchKernelGGL(env_step_kernel, dim3((e->N + 63) / 64), dim3(64), 0, st, a);
  GCRL_HIP(hipGetLastError());
  e->steps += 1; e->launches += 1;
  for (int32_t& t : e->t_host) t = t + 1 == e->T ? 0 : t + 1;   // the kernel's rule for t
  return GCRL_OK;
}

int proc_pack_launch(const ProcPack& p, hipStream_t st) {
  const long long total = (long long)p.n * (2 * p.D + 4 * p.G + 3 + p.A + p.G);
  hipLaunchKernelGGL(proc_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int clipped_normal_fill(float* out, int n, unsigned long long seed, unsigned long long ctr0, hipStream_t st) {
  hipLaunchKernelGGL(clipped_normal_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, out, n, seed, ctr0);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}
int normal_fill(void* out, int f64, int n, unsigned long long seed, unsigned long long ctr0, double scale, hipStream_t st) {
  hipLaunchKernelGGL(normal_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, out, f64, n, seed, ctr0, scale);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}
int round_to_f32(const double* in64, float* out32, int n, hipStream_t st) {
  hipLaunchKernelGGL(round_to_f32_kernel, dim3((n + 255) / 256), dim3(256), 0, st, in64, out32, n);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl

extern "C" {

gcrl_env* gcrl_env_create(int kind, int num_envs, uint64_t seed, int max_steps, float threshold, int device) {
  auto bad = [](const char* m) -> gcrl_env* { gcrl::fail(GCRL_ERR_ARG, "gcrl_env_create: %s", m); return nullptr; };
  if (!known_kind(kind)) return bad("kind: GCRL_ENV_REACH, GCRL_ENV_PUSH or GCRL_ENV_PICK required");
  if (num_envs < 1 || num_envs > kEnvMaxN) return bad("num_envs: 1..1024 required");
  if (max_steps < 1 || max_steps > 64) return bad("max_steps: 1..64 required (the replay ring's flush length limit)");
  if (!(threshold > 0.f) || !(threshold < kBox)) return bad("threshold: must lie in (0, 0.3)");
  if (kind != GCRL_ENV_REACH && !(2.0f * threshold <= kSpawn)) return bad("threshold: push and pick place the goal at least 2 * threshold from the puck and need 2 * threshold <= 0.15");
  int ndev = gcrl_device_count();
  if (ndev <= 0 || device < 0 || device >= ndev) {
    gcrl::fail(GCRL_ERR_HIP, "gcrl_env_create: no usable HIP device (count=%d, requested %d); there is no CPU fallback", ndev, device);
    return nullptr;
  }
  gcrl_env* e = new gcrl_env;
  e->kind = kind; e->N = num_envs; e->T = max_steps; e->thr = threshold; e->seed = seed; e->device = device;
  e->D = env_obs_dim(kind); e->A = env_action_dim(kind); e->SW = env_state_w(kind);
  const size_t N = (size_t)num_envs, raw_floats = N * (2 * e->D + 4 * kEnvG);
  auto ok = [&](hipError_t r, const char* what) {
    if (r == hipSuccess) return true;
    gcrl::fail(GCRL_ERR_HIP, "gcrl_env_create: %s failed: %s", what, hipGetErrorString(r));
    return false;
  };
  bool good = ok(hipSetDevice(device), "hipSetDevice") && ok(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking), "hipStreamCreate") &&
              ok(hipMalloc((void**)&e->state, N * e->SW * sizeof(float)), "hipMalloc") && ok(hipMalloc((void**)&e->t, N * sizeof(int)), "hipMalloc") &&
              ok(hipMalloc((void**)&e->cnt, N * 3 * sizeof(unsigned long long)), "hipMalloc") && ok(hipMalloc((void**)&e->rsum, N * sizeof(double)), "hipMalloc") &&
              ok(hipMalloc((void**)&e->rows, N * (e->D + kEnvG) * sizeof(float)), "hipMalloc") && ok(hipMalloc((void**)&e->raw, raw_floats * sizeof(float)), "hipMalloc") &&
              ok(hipMalloc((void**)&e->pay, N * kEnvPayW * sizeof(float)), "hipMalloc");
  if (good) good = ok(hipMemset(e->state, 0, N * e->SW * sizeof(float)), "hipMemset") && ok(hipMemset(e->t, 0, N * sizeof(int)), "hipMemset") &&
                   ok(hipMemset(e->cnt, 0, N * 3 * sizeof(unsigned long long)), "hipMemset") && ok(hipMemset(e->rsum, 0, N * sizeof(double)), "hipMemset") &&
                   ok(hipMemset(e->raw, 0, raw_floats * sizeof(float)), "hipMemset") && ok(hipMemset(e->pay, 0, N * kEnvPayW * sizeof(float)), "hipMemset");
  if (good) {
    ResetArgs q;
    std::memset(&q, 0, sizeof(q));
    q.a = base_args(e);
    q.a.restart = 1;
    e->t_host.assign(N, 0);
    hipLaunchKernelGGL(env_reset_kernel, dim3((e->N + 63) / 64), dim3(64), 0, (hipStream_t) nullptr, q);
    good = ok(hipGetLastError(), "env_reset_kernel") && ok(hipDeviceSynchronize(), "hipDeviceSynchronize");   // the first step runs on the CALLER's stream
    e->launches += 1;
  }
  if (!good) { gcrl_env_destroy(e); return nullptr; }
  return e;
}

void gcrl_env_destroy(gcrl_env* e) {
  if (!e) return;
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (void* p : {(void*)e->state, (void*)e->t, (void*)e->cnt, (void*)e->rsum, (void*)e->rows, (void*)e->raw, (void*)e->pay, (void*)e->script_act})
    if (p) (void)hipFree(p);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

int gcrl_env_dims(const gcrl_env* e, int* kind, int* num_envs, int* obs_dim, int* goal_dim, int* ac_dim, int* max_steps, float* threshold, uint64_t* seed) {
  GCRL_CHECK_ARG(e, "gcrl_env_dims: null handle");
  if (kind) *kind = e->kind;
  if (num_envs) *num_envs = e->N;
  if (obs_dim) *obs_dim = e->D;
  if (goal_dim) *goal_dim = kEnvG;
  if (ac_dim) *ac_dim = e->A;
  if (max_steps) *max_steps = e->T;
  if (threshold) *threshold = e->thr;
  if (seed) *seed = e->seed;
  return GCRL_OK;
}

int gcrl_env_buffers(gcrl_env* e, float** rows, float** raw, float** pay) {
  GCRL_CHECK_ARG(e, "gcrl_env_buffers: null handle");
  if (rows) *rows = e->rows;
  if (raw) *raw = e->raw;
  if (pay) *pay = e->pay;
  return GCRL_OK;
}

int gcrl_env_reset(gcrl_env* e, const uint8_t* mask_host, void* stream) {
  GCRL_CHECK_ARG(e, "gcrl_env_reset: null handle");
  ResetArgs q;
  std::memset(&q, 0, sizeof(q));
  q.a = base_args(e);
  q.a.restart = mask_host ? 0 : 1;
  if (mask_host) std::memcpy(q.mask, mask_host, (size_t)e->N);
  hipLaunchKernelGGL(env_reset_kernel, dim3((e->N + 63) / 64), dim3(64), 0, e->pick(stream), q);
  GCRL_HIP(hipGetLastError());
  e->launches += 1;
  for (int i = 0; i < e->N; ++i) if (!mask_host || mask_host[i]) e->t_host[i] = 0;
  if (!mask_host) e->steps = 0;
  return GCRL_OK;
}

int gcrl_env_step(gcrl_env* e, const void* actions_dev, int actions_f64, void* stream) {
  GCRL_CHECK_ARG(e && actions_dev, "gcrl_env_step: null argument");
  return gcrl::env_step_launch(e, actions_dev, actions_f64, e->pick(stream));
}

int gcrl_env_stats(gcrl_env* e, int64_t* episodes, int64_t* successes, double* reward_sum, void* stream) {
  GCRL_CHECK_ARG(e, "gcrl_env_stats: null handle");
  std::vector<unsigned long long> cn((size_t)e->N * 3);
  std::vector<double> rs((size_t)e->N);
  hipStream_t st = e->pick(stream);
  GCRL_HIP(hipMemcpyAsync(cn.data(), e->cnt, cn.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  GCRL_HIP(hipMemcpyAsync(rs.data(), e->rsum, rs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  GCRL_HIP(hipStreamSynchronize(st));
  int64_t ep = 0, su = 0; double r = 0.0;
  for (int i = 0; i < e->N; ++i) { ep += (int64_t)cn[(size_t)i * 3 + 1]; su += (int64_t)cn[(size_t)i * 3 + 2]; r += rs[i]; }
  if (episodes) *episodes = ep;
  if (successes) *successes = su;
  if (reward_sum) *reward_sum = r;
  return GCRL_OK;
}

int64_t gcrl_env_state_bytes(const gcrl_env* e) { return e ? (int64_t)state_bytes(e) : 0; }

// blob: header | state [N][12] f32 (pick: [N][18]) | t [N] i32 | counters [N][3] u64 | reward sums [N] f64 | acting rows [N][D + G] f32
int gcrl_env_save_state(gcrl_env* e, void* dst_host, int64_t n, void* stream) {
  GCRL_CHECK_ARG(e && dst_host && n == (int64_t)state_bytes(e), "gcrl_env_save_state: the blob is %lld bytes", e ? (long long)state_bytes(e) : 0ll);
  hipStream_t st = e->pick(stream);
  EnvHeader hd{kEnvMagic, e->kind, e->N, e->T, e->thr, 0u, e->seed, e->steps};
  char* o = static_cast<char*>(dst_host);
  std::memcpy(o, &hd, sizeof(hd)); o += sizeof(hd);
  const size_t N = (size_t)e->N;
  const void* src[5] = {e->state, e->t, e->cnt, e->rsum, e->rows};
  const size_t len[5] = {N * e->SW * sizeof(float), N * sizeof(int), N * 3 * sizeof(unsigned long long), N * sizeof(double), N * (e->D + kEnvG) * sizeof(float)};
  for (int k = 0; k < 5; ++k) { GCRL_HIP(hipMemcpyAsync(o, src[k], len[k], hipMemcpyDeviceToHost, st)); o += len[k]; }
  GCRL_HIP(hipStreamSynchronize(st));
  return GCRL_OK;
}

int gcrl_env_load_state(gcrl_env* e, const void* src_host, int64_t n, void* stream) {
  GCRL_CHECK_ARG(e && src_host && n >= (int64_t)sizeof(EnvHeader), "gcrl_env_load_state: null argument or a blob shorter than its header");
  EnvHeader hd;
  std::memcpy(&hd, src_host, sizeof(hd));
  GCRL_CHECK_ARG(hd.magic == kEnvMagic, "gcrl_env_load_state: not an environment state blob");
  GCRL_CHECK_ARG(hd.kind == e->kind, "gcrl_env_load_state: kind: the blob holds kind %d, the handle %d", hd.kind, e->kind);
  GCRL_CHECK_ARG(hd.N == e->N, "gcrl_env_load_state: num_envs: the blob holds %d envs, the handle %d", hd.N, e->N);
  GCRL_CHECK_ARG(hd.T == e->T, "gcrl_env_load_state: max_steps: the blob holds %d, the handle %d", hd.T, e->T);
  GCRL_CHECK_ARG(std::memcmp(&hd.thr, &e->thr, sizeof(float)) == 0, "gcrl_env_load_state: threshold: the blob holds %g, the handle %g", hd.thr, e->thr);
  GCRL_CHECK_ARG(n == (int64_t)state_bytes(e), "gcrl_env_load_state: the blob is %lld bytes, expected %lld", (long long)n, (long long)state_bytes(e));
  hipStream_t st = e->pick(stream);
  const char* o = static_cast<const char*>(src_host) + sizeof(hd);
  const size_t N = (size_t)e->N;
  void* dst[5] = {e->state, e->t, e->cnt, e->rsum, e->rows};
  const size_t len[5] = {N * e->SW * sizeof(float), N * sizeof(int), N * 3 * sizeof(unsigned long long), N * sizeof(double), N * (e->D + kEnvG) * sizeof(float)};
  for (int k = 0; k < 5; ++k) { GCRL_HIP(hipMemcpyAsync(dst[k], o, len[k], hipMemcpyHostToDevice, st)); o += len[k]; }
  GCRL_HIP(hipStreamSynchronize(st));   // (the source is the caller's pageable memory)
  e->seed = hd.seed; e->steps = hd.steps;
  std::memcpy(e->t_host.data(), static_cast<const char*>(src_host) + sizeof(hd) + len[0], len[1]);
  return GCRL_OK;
}

// raw | pay of one vector step from separate contiguous float32 device tensors (for callers that hold the pieces separately)
int gcrl_proc_pack(const float* obs, const float* next_obs, const float* dg, const float* next_dg, const float* ag, const float* next_ag,
                   const float* actions, const float* rewards, const int32_t* t_dev, int t0, int n, int obs_dim, int goal_dim, int action_dim, float* raw_out,
                   float* pay_out, void* stream) {
  GCRL_CHECK_ARG(obs && next_obs && dg && next_dg && next_ag && actions && rewards && raw_out && pay_out, "gcrl_proc_pack: null argument");
  GCRL_CHECK_ARG(n >= 1 && obs_dim >= 1 && goal_dim >= 1 && action_dim >= 1 && 3 + action_dim + goal_dim <= kEnvPayW && t0 >= 0,
                 "gcrl_proc_pack: n, dimensions and t0 must be positive and action_dim + goal_dim fit the payload");
  gcrl::ProcPack p{obs, next_obs, dg, next_dg, ag, next_ag, actions, rewards, t_dev, raw_out, pay_out, n, obs_dim, goal_dim, action_dim, t0};
  hipStream_t st = stream == GCRL_STREAM_LEGACY ? (hipStream_t) nullptr : (hipStream_t)stream;
  return gcrl::proc_pack_launch(p, st);
}

}  // extern "C"
