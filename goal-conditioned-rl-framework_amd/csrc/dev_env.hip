// dev_env.hip — four built-in goal environments that live on the device (dev_env.h), and the small launches the device-row acting
// entries and the collect loop of agent.hip need around them.
//
//   reach (D = 7, A = 3)    a point mass in a box: obs = [pos, vel, t / T], achieved goal = pos
//   push  (D = 13, A = 3)   a pusher and a puck on the plane z = 0: obs = [p, q, q - p, vel_p, t / T], achieved goal = q; the puck moves by
//                           the pusher's planar displacement while the pusher's new position is inside the contact radius
//   pick  (D = 20, A = 4)   a gripper with a finger opening w and an object that rests on the table: obs = [p, q, q - p, vel_p, vel_q, w,
//                           vel_w, held, near, t / T], achieved goal = q; the object is grasped when the fingers close around it, moves
//                           with the gripper while they stay closed and falls when released; half the goals lie in the air
//   glide (D = 16, A = 3)   a pusher and a puck that keeps moving: obs = [p, q, q - p, vel_p, vel_q, t / T], achieved goal = q; a touched
//                           puck takes the pusher's displacement, a free one keeps 0.9 of its last displacement per step, a wall stops
//                           the component that meets it; the goals lie beyond the pusher's box, so the puck has to be struck and let go
//
// G = 3, fixed horizon T, sparse reward -(dist > thr) formed as the replay ring's relabelling kernels form it, no termination.
// All arithmetic is float32, one rounding per operation (the unit is built with -ffp-contract=off): + - * /, comparisons,
// fminf / fmaxf and the correctly rounded square root of the reward's distance.  The rule — constants, operation order, what a NaN
// action counts as, the random-number keys — is restated in numpy in tests/dev_env_ref.py (reach, push) and
// tests/dev_env_pick_ref.py (pick) and tests/dev_env_glide_ref.py (glide), which are its definition.
//
// Random numbers: u(env, episode, component) = hash_below(seed, kEnvStream + env, 8 * episode + component, 2^24) * 2^-24.  No state
// besides the counters, so an env's episode j is the same whatever N is and whenever it is reached.
//
// What an env's thread does on a reset and on a step lives in dev_env_body.h (env_reset_body, env_step_body).  This unit holds the
// by-value kernels — one member's EnvArgs in the launch, no table — which every one-member group launches, a standalone gcrl_env
// among them; dev_env_group.hip holds the member-table kernels of a group of several, which call the same text, and all host code of
// the handle (gcrl_env_group, dev_env.h), the gcrl_env_* entries included.
//
// Kernel rules: every address comes from the handle or the group's member table (or, for the pack and fill launches, from the
// caller's checked arguments); an env index >= N — for a group: a member index >= P — does nothing; no atomics; no waits between
// workgroups; no per-thread scratch (every loop is over a small constant and unrolled); plain vector stores only.
#include "dev_env_body.h"   // dev_env.h, EnvArgs, env_reset_body, env_step_body

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

}  // namespace

namespace gcrl {

int env_step_args_launch(const EnvArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(env_step_kernel, dim3((a.N + 63) / 64), dim3(64), 0, st, a);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

int env_reset_args_launch(const EnvArgs& a, const uint8_t* mask_host, hipStream_t st) {
  ResetArgs q;
  std::memset(&q, 0, sizeof(q));
  q.a = a;
  if (!a.restart) std::memcpy(q.mask, mask_host, (size_t)a.N);
  hipLaunchKernelGGL(env_reset_kernel, dim3((a.N + 63) / 64), dim3(64), 0, st, q);
  GCRL_HIP(hipGetLastError());
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
