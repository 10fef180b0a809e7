// dev_env_group.hip — the handle of the device-resident goal environments (dev_env.h gcrl_env_group): P x N envs of one built-in kind in
// single allocations, laid out at the strides the population kernels read.  All host code of the handle lives here, once, for the
// gcrl_env_group_* entries and for the gcrl_env_* entries at the end (a gcrl_env is a one-member group): creation, a member's
// slices, its saved record, stats, and the launch rule — a one-member group launches dev_env.hip's by-value kernels on the EnvArgs of
// member 0, built on the host; a group of several launches the kernels here, which build each member's EnvArgs per thread from a
// device table.  Both forms call dev_env_body.h's env_step_body / env_reset_body.
//
// Kernel rules (dev_env.hip's): every address comes from the handle or the member table; a member index >= P does nothing (the env
// index is below N by construction); no atomics; no waits between workgroups; no per-thread scratch; plain vector stores only; the
// unit is built with -ffp-contract=off.
#include <atomic>
#include <vector>

#include "dev_env_body.h"
#include "pop.h"        // PopTabCache

namespace {

// ---------------------------------------------------------------- the group's kernels: one thread per env of P x N, member = e / N
// What belongs to the member travels in a device table (cached by content: it is the same call after call); what changes from step to
// step — where the actions come from and the counters of the two hash streams — travels in the kernel arguments.
struct EnvPopTab { unsigned long long seed, eps_seed, noise_seed; double noise_scale; };
struct EnvPopArgs {
  float* state; int* t; unsigned long long* cnt; double* rsum; float* rows; float* data; double* noise64;
  const EnvPopTab* tab;
  int kind, P, N, T, D, stride_n, stride, raw_floats, restart;
  float thr;
  const void* act[kEnvGroupMaxP];
  unsigned long long eps_ctr0[kEnvGroupMaxP], noise_ctr0[kEnvGroupMaxP];
  unsigned char src[kEnvGroupMaxP], noise_on[kEnvGroupMaxP];
};
// member m's view of the group, on the device and (member_env_args) on the host: its slices and the group's dimensions
__host__ __device__ inline void member_slices(const EnvPopArgs& q, int m, EnvArgs& a) {
  const size_t o = (size_t)m * q.N;
  a.state = q.state + o * env_state_w(q.kind); a.t = q.t + o; a.cnt = q.cnt + o * 3; a.rsum = q.rsum + o;
  a.rows = q.rows + (size_t)m * q.stride_n * (q.D + kEnvG);
  a.raw = q.data + (size_t)m * q.stride; a.pay = a.raw + q.raw_floats;
  a.kind = q.kind; a.N = q.N; a.T = q.T; a.D = q.D; a.thr = q.thr; a.restart = q.restart;
}
__device__ inline void member_args(const EnvPopArgs& q, int m, EnvArgs& a) {
  member_slices(q, m, a);
  a.seed = q.tab[m].seed;
}
__global__ __launch_bounds__(64) void env_step_pop_kernel(EnvPopArgs q) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  const int m = e / q.N, i = e - m * q.N;
  if (m >= q.P) return;
  EnvArgs a;
  member_args(q, m, a);
  const int src = q.src[m];
  a.act = q.act[m]; a.act_f64 = src == gcrl::kEnvActF64 ? 1 : 0;
  a.act_eps = src == gcrl::kEnvActEps ? 1 : 0; a.eps_seed = q.tab[m].eps_seed; a.eps_ctr0 = q.eps_ctr0[m];
  a.noise = q.noise_on[m] ? (void*)(q.noise64 + (size_t)m * q.stride_n * env_action_dim(q.kind)) : nullptr; a.noise_f64 = 1;
  a.noise_seed = q.tab[m].noise_seed; a.noise_ctr0 = q.noise_ctr0[m]; a.noise_scale = q.tab[m].noise_scale;
  env_step_body(a, i);
}
// the selection as one bit per env of P x N inside the kernel arguments (16 x 1024 bits = 2 KB), ignored on a restart
struct ResetPopArgs { EnvPopArgs q; uint32_t bits[kEnvGroupMaxP * kEnvMaxN / 32]; };
static_assert(sizeof(ResetPopArgs) <= 4096, "kernel arguments are limited to 4 KB");
__global__ __launch_bounds__(64) void env_reset_pop_kernel(ResetPopArgs r) {
  const EnvPopArgs& q = r.q;
  const int e = blockIdx.x * 64 + threadIdx.x;
  const int m = e / q.N, i = e - m * q.N;
  if (m >= q.P) return;
  if (!q.restart && !((r.bits[e >> 5] >> (e & 31)) & 1u)) return;
  EnvArgs a;
  member_args(q, m, a);
  env_reset_body(a, i);
}

}  // namespace

// ---------------------------------------------------------------- the handle's host side
namespace {

constexpr uint32_t kEnvMagic = 0x564e4547u;     // "GENV"
constexpr uint32_t kGroupMagic = 0x50524747u;   // "GGRP"
// A member's record starts with an EnvHeader; a standalone env's blob is its one member's record, a group's blob a GroupHeader and P records
struct EnvHeader { uint32_t magic; int32_t kind, N, T; float thr; uint32_t pad; uint64_t seed; int64_t steps; };
struct GroupHeader { uint32_t magic; int32_t kind, P, N, T; float thr; };

EnvPopArgs group_args(const gcrl_env_group* g) {
  EnvPopArgs q;
  std::memset(&q, 0, sizeof(q));
  q.state = g->state; q.t = g->t; q.cnt = g->cnt; q.rsum = g->rsum; q.rows = g->rows; q.data = g->data; q.noise64 = g->noise64;
  q.kind = g->kind; q.P = g->P; q.N = g->N; q.T = g->T; q.D = g->D; q.stride_n = g->stride_n; q.stride = g->stride; q.raw_floats = g->raw_floats;
  q.thr = g->thr;
  return q;
}
// member k as one env: what the by-value kernels take (actions, rider and restart flag left at zero)
EnvArgs member_env_args(const gcrl_env_group* g, int k) {
  EnvArgs a;
  std::memset(&a, 0, sizeof(a));
  member_slices(group_args(g), k, a);
  a.seed = g->seeds[k];
  return a;
}
// the five blocks of member k's record, in the record's order: state [N][SW] f32 | t [N] i32 | counters [N][3] u64 | reward sums [N] f64 |
// acting rows [N][D + G] f32
struct MemberBlocks { void* p[5]; size_t len[5]; };
MemberBlocks member_blocks(const gcrl_env_group* g, int k) {
  const EnvArgs a = member_env_args(g, k);
  const size_t N = (size_t)g->N;
  return {{a.state, a.t, a.cnt, a.rsum, a.rows},
          {N * g->SW * sizeof(float), N * sizeof(int), N * 3 * sizeof(unsigned long long), N * sizeof(double), N * (g->D + kEnvG) * sizeof(float)}};
}
// whether a record of these dimensions fits the handle, naming the field that does not
int header_check(const gcrl_env_group* g, const char* who, const EnvHeader& hd) {
  GCRL_CHECK_ARG(hd.magic == kEnvMagic, "%s: not an environment state blob", who);
  GCRL_CHECK_ARG(hd.kind == g->kind, "%s: kind: the blob holds kind %d, the handle %d", who, hd.kind, g->kind);
  GCRL_CHECK_ARG(hd.N == g->N, "%s: num_envs: the blob holds %d envs, the handle %d", who, hd.N, g->N);
  GCRL_CHECK_ARG(hd.T == g->T, "%s: max_steps: the blob holds %d, the handle %d", who, hd.T, g->T);
  GCRL_CHECK_ARG(std::memcmp(&hd.thr, &g->thr, sizeof(float)) == 0, "%s: threshold: the blob holds %g, the handle %g", who, hd.thr, g->thr);
  return GCRL_OK;
}

// the members' table of a launch of a group of several (null rider arguments: the seeds alone)
int group_table(gcrl_env_group* g, const gcrl::EnvPopMember* m, hipStream_t st, const EnvPopTab** out) {
  EnvPopTab tab[kEnvGroupMaxP];
  std::memset(tab, 0, sizeof(tab));
  for (int k = 0; k < g->P; ++k) {
    tab[k].seed = g->seeds[k];
    if (m) { tab[k].eps_seed = m[k].eps_seed; tab[k].noise_seed = m[k].noise_seed; tab[k].noise_scale = m[k].noise_scale; }
  }
  void* dev = nullptr;
  if (static_cast<gcrl::PopTabCache*>(g->tabs)->get(tab, sizeof(EnvPopTab) * g->P, st, &dev)) return gcrl::fail(GCRL_ERR_HIP, "gcrl_env_group: member table upload failed");
  *out = static_cast<const EnvPopTab*>(dev);
  return GCRL_OK;
}
// what a step launch of either form leaves on the host
int stepped(gcrl_env_group* g) {
  g->launches += 1;
  for (int k = 0; k < g->P; ++k) g->steps[k] += 1;
  g->vsteps += 1;
  g->rolled.resize(g->t_host.size());
  for (size_t e = 0; e < g->t_host.size(); ++e) {   // the kernel's rule for t
    int32_t& t = g->t_host[e];
    g->rolled[e] = t + 1 == g->T ? 1 : 0;
    t = g->rolled[e] ? 0 : t + 1;
  }
  return GCRL_OK;
}

// A one-member group's step: env_step_kernel on the EnvArgs env_step_pop_kernel would build for member 0, built here; the rider
// writes to `noise` (float64 or float32)
int step_one(gcrl_env_group* g, const gcrl::EnvPopMember& m, void* noise, int noise_f64, hipStream_t st) {
  EnvArgs a = member_env_args(g, 0);
  a.act = m.act; a.act_f64 = m.src == gcrl::kEnvActF64 ? 1 : 0;
  a.act_eps = m.src == gcrl::kEnvActEps ? 1 : 0; a.eps_seed = m.eps_seed; a.eps_ctr0 = m.eps_ctr0;
  a.noise = m.noise_on ? noise : nullptr; a.noise_f64 = noise_f64;
  a.noise_seed = m.noise_seed; a.noise_ctr0 = m.noise_ctr0; a.noise_scale = m.noise_scale;
  if (int rc = gcrl::env_step_args_launch(a, st)) return rc;
  return stepped(g);
}
// mask_host [P][N] bytes: those envs go on to their next episode; null: every env back to episode 0, counters to zero
int env_group_reset(gcrl_env_group* g, const uint8_t* mask_host, hipStream_t st) {
  const int total = g->P * g->N;
  if (g->P == 1) {
    EnvArgs a = member_env_args(g, 0);
    a.restart = mask_host ? 0 : 1;
    if (int rc = gcrl::env_reset_args_launch(a, mask_host, st)) return rc;
  } else {
    ResetPopArgs r;
    std::memset(&r, 0, sizeof(r));
    r.q = group_args(g);
    r.q.restart = mask_host ? 0 : 1;
    if (int rc = group_table(g, nullptr, st, &r.q.tab)) return rc;
    if (mask_host)
      for (int e = 0; e < total; ++e) if (mask_host[e]) r.bits[e >> 5] |= 1u << (e & 31);
    hipLaunchKernelGGL(env_reset_pop_kernel, dim3((total + 63) / 64), dim3(64), 0, st, r);
    GCRL_HIP(hipGetLastError());
  }
  g->launches += 1;
  for (int e = 0; e < total; ++e) if (!mask_host || mask_host[e]) g->t_host[e] = 0;
  if (!mask_host) for (int k = 0; k < g->P; ++k) g->steps[k] = 0;
  return GCRL_OK;
}

int env_group_init(gcrl_env_group* g, const char* who, int kind, int members, int num_envs, const uint64_t* seeds, int max_steps, float threshold,
                   int device) {
  GCRL_CHECK_ARG(kind == GCRL_ENV_REACH || kind == GCRL_ENV_PUSH || kind == GCRL_ENV_PICK || kind == GCRL_ENV_GLIDE,
                 "%s: kind: GCRL_ENV_REACH, GCRL_ENV_PUSH, GCRL_ENV_PICK or GCRL_ENV_GLIDE required", who);
  GCRL_CHECK_ARG(members >= 1 && members <= kEnvGroupMaxP, "%s: members: 1..16 required", who);
  GCRL_CHECK_ARG(seeds, "%s: seeds: null array", who);
  GCRL_CHECK_ARG(num_envs >= 1 && num_envs <= kEnvMaxN, "%s: num_envs: 1..1024 required", who);
  GCRL_CHECK_ARG(max_steps >= 1 && max_steps <= 64, "%s: max_steps: 1..64 required (the replay ring's flush length limit)", who);
  GCRL_CHECK_ARG(threshold > 0.f && threshold < kBox, "%s: threshold: must lie in (0, 0.3)", who);
  GCRL_CHECK_ARG(kind == GCRL_ENV_REACH || 2.0f * threshold <= kSpawn,
                 "%s: threshold: push and pick place the goal at least 2 * threshold from the puck and need 2 * threshold <= 0.15; glide keeps the limit", who);
  const int ndev = gcrl_device_count();
  if (ndev <= 0 || device < 0 || device >= ndev)
    return gcrl::fail(GCRL_ERR_HIP, "%s: no usable HIP device (count=%d, requested %d); there is no CPU fallback", who, ndev, device);
  g->kind = kind; g->P = members; g->N = num_envs; g->T = max_steps; g->thr = threshold; g->device = device;
  g->D = env_obs_dim(kind); g->A = env_action_dim(kind); g->SW = env_state_w(kind);
  for (int k = 0; k < members; ++k) g->seeds[k] = seeds[k];
  g->stride_n = (num_envs + 3) / 4 * 4 + 4;   // at least four rows past N in every member's slice: never read, never written
  g->raw_floats = num_envs * (2 * g->D + 4 * kEnvG);
  g->stride = (g->raw_floats + num_envs * kEnvPayW + 3) / 4 * 4 + 4;
  static std::atomic<uintptr_t> serial{0};
  g->token = reinterpret_cast<const void*>(++serial);
  if (members > 1) g->tabs = new gcrl::PopTabCache;
  const size_t PN = (size_t)members * num_envs, PS = (size_t)members * g->stride_n;
  int rc = GCRL_OK;
  auto ok = [&](hipError_t r, const char* what) {
    if (r != hipSuccess) rc = gcrl::fail(GCRL_ERR_HIP, "%s: %s failed: %s", who, what, hipGetErrorString(r));
    return r == hipSuccess;
  };
  struct Blk { void** p; size_t bytes; };
  const Blk blks[8] = {{(void**)&g->state, PN * g->SW * sizeof(float)}, {(void**)&g->t, PN * sizeof(int)},
                       {(void**)&g->cnt, PN * 3 * sizeof(unsigned long long)}, {(void**)&g->rsum, PN * sizeof(double)},
                       {(void**)&g->rows, PS * (g->D + kEnvG) * sizeof(float)}, {(void**)&g->data, (size_t)members * g->stride * sizeof(float)},
                       {(void**)&g->noise64, PS * g->A * sizeof(double)}, {(void**)&g->act64, PS * g->A * sizeof(double)}};
  bool good = ok(hipSetDevice(device), "hipSetDevice") && ok(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking), "hipStreamCreate");
  for (const Blk& b : blks) good = good && ok(hipMalloc(b.p, b.bytes), "hipMalloc") && ok(hipMemset(*b.p, 0, b.bytes), "hipMemset");
  if (!good) return rc;
  g->t_host.assign(PN, 0);
  if ((rc = env_group_reset(g, nullptr, (hipStream_t) nullptr))) return rc;
  ok(hipDeviceSynchronize(), "hipDeviceSynchronize");   // the first step runs on the CALLER's stream
  return rc;
}

void env_group_release(gcrl_env_group* g) {
  if (g->stream) (void)hipDeviceSynchronize();   // (a launch on any stream may still read the blocks or a table)
  for (void* p : {(void*)g->state, (void*)g->t, (void*)g->cnt, (void*)g->rsum, (void*)g->rows, (void*)g->data, (void*)g->noise64, (void*)g->act64,
                  (void*)g->script_act})
    if (p) (void)hipFree(p);
  if (g->tabs) { static_cast<gcrl::PopTabCache*>(g->tabs)->release(); delete static_cast<gcrl::PopTabCache*>(g->tabs); }
  if (g->stream) (void)hipStreamDestroy(g->stream);
}

}  // namespace

namespace gcrl {

int env_group_step_launch(gcrl_env_group* g, const EnvPopMember* m, hipStream_t st) {
  if (g->P == 1) return step_one(g, m[0], g->noise64, 1, st);
  EnvPopArgs q = group_args(g);
  if (int rc = group_table(g, m, st, &q.tab)) return rc;
  for (int k = 0; k < g->P; ++k) {
    q.act[k] = m[k].act; q.src[k] = (unsigned char)m[k].src; q.eps_ctr0[k] = m[k].eps_ctr0;
    q.noise_on[k] = m[k].noise_on ? 1 : 0; q.noise_ctr0[k] = m[k].noise_ctr0;
  }
  const int total = g->P * g->N;
  hipLaunchKernelGGL(env_step_pop_kernel, dim3((total + 63) / 64), dim3(64), 0, st, q);
  GCRL_HIP(hipGetLastError());
  return stepped(g);
}

int env_step_launch(gcrl_env_group* g, const void* actions_dev, int f64, hipStream_t st) { return env_step_launch_noise(g, actions_dev, f64, nullptr, 0, 0, 0, 0.0, st); }

int env_step_launch_noise(gcrl_env_group* g, const void* actions_dev, int f64, void* noise, int noise_f64, unsigned long long noise_seed,
                          unsigned long long noise_ctr0, double noise_scale, hipStream_t st) {
  const EnvPopMember m{actions_dev, f64 ? kEnvActF64 : kEnvActF32, 0, 0, noise ? 1 : 0, noise_seed, noise_ctr0, noise_scale};
  return step_one(g, m, noise, noise_f64, st);
}

}  // namespace gcrl

namespace {

int env_group_stats(gcrl_env_group* g, int64_t* episodes, int64_t* successes, double* reward_sum, hipStream_t st) {
  const size_t PN = (size_t)g->P * g->N;
  std::vector<unsigned long long> cn(PN * 3);
  std::vector<double> rs(PN);
  GCRL_HIP(hipMemcpyAsync(cn.data(), g->cnt, cn.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  GCRL_HIP(hipMemcpyAsync(rs.data(), g->rsum, rs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  GCRL_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < g->P; ++k) {
    int64_t ep = 0, su = 0; double r = 0.0;
    for (int i = 0; i < g->N; ++i) {
      const size_t e = (size_t)k * g->N + i;
      ep += (int64_t)cn[e * 3 + 1]; su += (int64_t)cn[e * 3 + 2]; r += rs[e];
    }
    if (episodes) episodes[k] = ep;
    if (successes) successes[k] = su;
    if (reward_sum) reward_sum[k] = r;
  }
  return GCRL_OK;
}

size_t env_member_bytes(const gcrl_env_group* g) {
  const MemberBlocks b = member_blocks(g, 0);
  size_t n = sizeof(EnvHeader);
  for (size_t len : b.len) n += len;
  return n;
}
size_t group_bytes(const gcrl_env_group* g) { return sizeof(GroupHeader) + (size_t)g->P * env_member_bytes(g); }

int env_member_save(gcrl_env_group* g, int k, void* dst_host, hipStream_t st) {
  const EnvHeader hd{kEnvMagic, g->kind, g->N, g->T, g->thr, 0u, g->seeds[k], g->steps[k]};
  char* o = static_cast<char*>(dst_host);
  std::memcpy(o, &hd, sizeof(hd)); o += sizeof(hd);
  const MemberBlocks b = member_blocks(g, k);
  for (int i = 0; i < 5; ++i) { GCRL_HIP(hipMemcpyAsync(o, b.p[i], b.len[i], hipMemcpyDeviceToHost, st)); o += b.len[i]; }
  return GCRL_OK;
}

int env_member_check(const gcrl_env_group* g, const char* who, const void* rec_host, int64_t n) {
  GCRL_CHECK_ARG(g && rec_host && n >= (int64_t)sizeof(EnvHeader), "%s: null argument or a blob shorter than its header", who);
  EnvHeader hd;
  std::memcpy(&hd, rec_host, sizeof(hd));
  if (int rc = header_check(g, who, hd)) return rc;
  GCRL_CHECK_ARG(n == (int64_t)env_member_bytes(g), "%s: the blob is %lld bytes, expected %lld", who, (long long)n, (long long)env_member_bytes(g));
  return GCRL_OK;
}

int env_member_load(gcrl_env_group* g, int k, const void* rec_host, hipStream_t st) {
  EnvHeader hd;
  const char* o = static_cast<const char*>(rec_host);
  std::memcpy(&hd, o, sizeof(hd)); o += sizeof(hd);
  const MemberBlocks b = member_blocks(g, k);
  std::memcpy(g->t_host.data() + (size_t)k * g->N, o + b.len[0], b.len[1]);
  for (int i = 0; i < 5; ++i) { GCRL_HIP(hipMemcpyAsync(b.p[i], o, b.len[i], hipMemcpyHostToDevice, st)); o += b.len[i]; }
  g->seeds[k] = hd.seed; g->steps[k] = hd.steps;
  return GCRL_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- gcrl_env_group (include/gcrl.h)
gcrl_env_group* gcrl_env_group_create(int kind, int members, int num_envs, const uint64_t* seeds, int max_steps, float threshold, int device) {
  gcrl_env_group* g = new gcrl_env_group;
  if (env_group_init(g, "gcrl_env_group_create", kind, members, num_envs, seeds, max_steps, threshold, device)) { gcrl_env_group_destroy(g); return nullptr; }
  return g;
}

void gcrl_env_group_destroy(gcrl_env_group* g) {
  if (!g) return;
  env_group_release(g);
  delete g;
}

int gcrl_env_group_dims(const gcrl_env_group* g, int* kind, int* members, int* num_envs, int* obs_dim, int* goal_dim, int* ac_dim, int* max_steps,
                        float* threshold, uint64_t* seeds_out, int* stride_n, int* stride, int* raw_floats) {
  GCRL_CHECK_ARG(g, "gcrl_env_group_dims: null handle");
  if (kind) *kind = g->kind;
  if (members) *members = g->P;
  if (num_envs) *num_envs = g->N;
  if (obs_dim) *obs_dim = g->D;
  if (goal_dim) *goal_dim = kEnvG;
  if (ac_dim) *ac_dim = g->A;
  if (max_steps) *max_steps = g->T;
  if (threshold) *threshold = g->thr;
  if (seeds_out) for (int k = 0; k < g->P; ++k) seeds_out[k] = g->seeds[k];
  if (stride_n) *stride_n = g->stride_n;
  if (stride) *stride = g->stride;
  if (raw_floats) *raw_floats = g->raw_floats;
  return GCRL_OK;
}

int gcrl_env_group_buffers(gcrl_env_group* g, float** rows, float** data, double** noise64, double** act64) {
  GCRL_CHECK_ARG(g, "gcrl_env_group_buffers: null handle");
  if (rows) *rows = g->rows;
  if (data) *data = g->data;
  if (noise64) *noise64 = g->noise64;
  if (act64) *act64 = g->act64;
  return GCRL_OK;
}

int gcrl_env_group_reset(gcrl_env_group* g, const uint8_t* mask_host, void* stream) {
  GCRL_CHECK_ARG(g, "gcrl_env_group_reset: null handle");
  return env_group_reset(g, mask_host, g->pick(stream));
}

int gcrl_env_group_step(gcrl_env_group* g, const void* actions_dev, int actions_f64, const uint8_t* eps_members, const uint64_t* eps_seeds,
                        const uint64_t* eps_ctr0, void* stream) {
  GCRL_CHECK_ARG(g, "gcrl_env_group_step: null handle");
  GCRL_CHECK_ARG(!eps_members || (eps_seeds && eps_ctr0), "gcrl_env_group_step: eps_seeds / eps_ctr0: null array with eps_members given");
  gcrl::EnvPopMember m[kEnvGroupMaxP];
  std::memset(m, 0, sizeof(m));
  bool need_act = false;
  for (int k = 0; k < g->P; ++k) need_act = need_act || !(eps_members && eps_members[k]);
  GCRL_CHECK_ARG(actions_dev || !need_act, "gcrl_env_group_step: actions_dev: null array");
  const size_t per = (size_t)g->N * g->A * (actions_f64 ? sizeof(double) : sizeof(float));
  for (int k = 0; k < g->P; ++k) {
    if (eps_members && eps_members[k]) { m[k].src = gcrl::kEnvActEps; m[k].eps_seed = eps_seeds[k]; m[k].eps_ctr0 = eps_ctr0[k]; }
    else { m[k].src = actions_f64 ? gcrl::kEnvActF64 : gcrl::kEnvActF32; m[k].act = static_cast<const char*>(actions_dev) + (size_t)k * per; }
  }
  return gcrl::env_group_step_launch(g, m, g->pick(stream));
}

int gcrl_env_group_stats(gcrl_env_group* g, int64_t* episodes, int64_t* successes, double* reward_sum, void* stream) {
  GCRL_CHECK_ARG(g, "gcrl_env_group_stats: null handle");
  return env_group_stats(g, episodes, successes, reward_sum, g->pick(stream));
}

int64_t gcrl_env_group_state_bytes(const gcrl_env_group* g) { return g ? (int64_t)group_bytes(g) : 0; }

// blob: group header | P member records
int gcrl_env_group_save_state(gcrl_env_group* g, void* dst_host, int64_t n, void* stream) {
  GCRL_CHECK_ARG(g && dst_host && n == (int64_t)group_bytes(g), "gcrl_env_group_save_state: the blob is %lld bytes", g ? (long long)group_bytes(g) : 0ll);
  hipStream_t st = g->pick(stream);
  const GroupHeader gh{kGroupMagic, g->kind, g->P, g->N, g->T, g->thr};
  char* o = static_cast<char*>(dst_host);
  std::memcpy(o, &gh, sizeof(gh)); o += sizeof(gh);
  for (int k = 0; k < g->P; ++k, o += env_member_bytes(g))
    if (int rc = env_member_save(g, k, o, st)) return rc;
  GCRL_HIP(hipStreamSynchronize(st));
  return GCRL_OK;
}

int gcrl_env_group_load_state(gcrl_env_group* g, const void* src_host, int64_t n, void* stream) {
  const char* who = "gcrl_env_group_load_state";
  GCRL_CHECK_ARG(g && src_host && n >= (int64_t)sizeof(GroupHeader), "%s: null argument or a blob shorter than its header", who);
  GroupHeader gh;
  std::memcpy(&gh, src_host, sizeof(gh));
  GCRL_CHECK_ARG(gh.magic == kGroupMagic, "%s: not an environment group state blob", who);
  GCRL_CHECK_ARG(gh.P == g->P, "%s: members: the blob holds %d members, the handle %d", who, gh.P, g->P);
  if (int rc = header_check(g, who, EnvHeader{kEnvMagic, gh.kind, gh.N, gh.T, gh.thr, 0u, 0u, 0})) return rc;
  GCRL_CHECK_ARG(n == (int64_t)group_bytes(g), "%s: the blob is %lld bytes, expected %lld", who, (long long)n, (long long)group_bytes(g));
  const size_t mb = env_member_bytes(g);
  const char* base = static_cast<const char*>(src_host) + sizeof(gh);
  for (int k = 0; k < g->P; ++k)   // every member's header before anything is overwritten
    if (env_member_check(g, who, base + k * mb, (int64_t)mb))
      return gcrl::fail(GCRL_ERR_ARG, "%s: members: member %d's record does not match the group header", who, k);
  hipStream_t st = g->pick(stream);
  for (int k = 0; k < g->P; ++k)
    if (int rc = env_member_load(g, k, base + k * mb, st)) return rc;
  GCRL_HIP(hipStreamSynchronize(st));   // (the source is the caller's pageable memory)
  return GCRL_OK;
}

// ---------------------------------------------------------------- gcrl_env (include/gcrl.h): a one-member group, entry by entry
gcrl_env* gcrl_env_create(int kind, int num_envs, uint64_t seed, int max_steps, float threshold, int device) {
  gcrl_env* e = new gcrl_env;
  if (env_group_init(e, "gcrl_env_create", kind, 1, num_envs, &seed, max_steps, threshold, device)) { gcrl_env_destroy(e); return nullptr; }
  return e;
}

void gcrl_env_destroy(gcrl_env* e) {
  if (!e) return;
  env_group_release(e);
  delete e;
}

int gcrl_env_dims(const gcrl_env* e, int* kind, int* num_envs, int* obs_dim, int* goal_dim, int* ac_dim, int* max_steps, float* threshold, uint64_t* seed) {
  GCRL_CHECK_ARG(e, "gcrl_env_dims: null handle");
  return gcrl_env_group_dims(e, kind, nullptr, num_envs, obs_dim, goal_dim, ac_dim, max_steps, threshold, seed, nullptr, nullptr, nullptr);
}

int gcrl_env_buffers(gcrl_env* e, float** rows, float** raw, float** pay) {
  GCRL_CHECK_ARG(e, "gcrl_env_buffers: null handle");
  if (rows) *rows = e->rows;
  if (raw) *raw = e->raw();
  if (pay) *pay = e->pay();
  return GCRL_OK;
}

int gcrl_env_reset(gcrl_env* e, const uint8_t* mask_host, void* stream) {
  GCRL_CHECK_ARG(e, "gcrl_env_reset: null handle");
  return env_group_reset(e, mask_host, e->pick(stream));
}

int gcrl_env_step(gcrl_env* e, const void* actions_dev, int actions_f64, void* stream) {
  GCRL_CHECK_ARG(e && actions_dev, "gcrl_env_step: null argument");
  return gcrl::env_step_launch(e, actions_dev, actions_f64, e->pick(stream));
}

int gcrl_env_stats(gcrl_env* e, int64_t* episodes, int64_t* successes, double* reward_sum, void* stream) {
  GCRL_CHECK_ARG(e, "gcrl_env_stats: null handle");
  return env_group_stats(e, episodes, successes, reward_sum, e->pick(stream));
}

int64_t gcrl_env_state_bytes(const gcrl_env* e) { return e ? (int64_t)env_member_bytes(e) : 0; }

// blob: the one member's record (dev_env.h env_member_save)
int gcrl_env_save_state(gcrl_env* e, void* dst_host, int64_t n, void* stream) {
  GCRL_CHECK_ARG(e && dst_host && n == (int64_t)env_member_bytes(e), "gcrl_env_save_state: the blob is %lld bytes", e ? (long long)env_member_bytes(e) : 0ll);
  hipStream_t st = e->pick(stream);
  if (int rc = env_member_save(e, 0, dst_host, st)) return rc;
  GCRL_HIP(hipStreamSynchronize(st));
  return GCRL_OK;
}

int gcrl_env_load_state(gcrl_env* e, const void* src_host, int64_t n, void* stream) {
  const char* who = "gcrl_env_load_state";
  if (int rc = env_member_check(e, who, src_host, n)) return rc;
  hipStream_t st = e->pick(stream);
  if (int rc = env_member_load(e, 0, src_host, st)) return rc;
  GCRL_HIP(hipStreamSynchronize(st));   // (the source is the caller's pageable memory)
  return GCRL_OK;
}

}  // extern "C"
