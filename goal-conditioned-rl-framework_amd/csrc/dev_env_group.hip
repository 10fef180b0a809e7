// dev_env_group.hip — groups of device-resident goal environments (dev_env.h gcrl_env_group; include/gcrl.h gcrl_env_group_*): P x N envs of
// one built-in kind in single allocations, laid out at the strides the population kernels read, for gcrl_pop_collect and
// gcrl_pop_evaluate (agent_pop.inc).  Member m IS a gcrl_env of seeds[m]: the kernels here build, per thread, the EnvArgs a standalone
// env of that seed would pass, pointed at the member's slices, and call dev_env_body.h's env_step_body / env_reset_body — the text
// env_step_kernel and env_reset_kernel call.
//
// Kernel rules (dev_env.hip's): every address comes from the handle or the member table; a member index >= P does nothing (the env
// index is below N by construction); no atomics; no waits between workgroups; no per-thread scratch; plain vector stores only; the
// unit is built with -ffp-contract=off.
#include <algorithm>
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
// member m's view of the group: the EnvArgs a standalone env of its seed would pass, on its slices
__device__ inline void member_args(const EnvPopArgs& q, int m, EnvArgs& a) {
  const size_t o = (size_t)m * q.N;
  a.state = q.state + o * env_state_w(q.kind); a.t = q.t + o; a.cnt = q.cnt + o * 3; a.rsum = q.rsum + o;
  a.rows = q.rows + (size_t)m * q.stride_n * (q.D + kEnvG);
  a.raw = q.data + (size_t)m * q.stride; a.pay = a.raw + q.raw_floats;
  a.kind = q.kind; a.N = q.N; a.T = q.T; a.D = q.D; a.thr = q.thr; a.restart = q.restart;
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

// ---------------------------------------------------------------- the group's host side
namespace {

constexpr uint32_t kGroupMagic = 0x50524747u;   // "GGRP"
struct GroupHeader { uint32_t magic; int32_t kind, P, N, T; float thr; };

EnvPopArgs group_args(gcrl_env_group* g) {
  EnvPopArgs q;
  std::memset(&q, 0, sizeof(q));
  q.state = g->state; q.t = g->t; q.cnt = g->cnt; q.rsum = g->rsum; q.rows = g->rows; q.data = g->data; q.noise64 = g->noise64;
  q.kind = g->kind; q.P = g->P; q.N = g->N; q.T = g->T; q.D = g->D; q.stride_n = g->stride_n; q.stride = g->stride; q.raw_floats = g->raw_floats;
  q.thr = g->thr;
  return q;
}
// the members' table of a launch (null rider arguments: the seeds alone)
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
size_t member_bytes(const gcrl_env_group* g) {
  return sizeof(EnvHeader) + (size_t)g->N * (g->SW * sizeof(float) + sizeof(int) + 3 * sizeof(unsigned long long) + sizeof(double)) +
         (size_t)g->N * (g->D + kEnvG) * sizeof(float);
}
size_t group_bytes(const gcrl_env_group* g) { return sizeof(GroupHeader) + (size_t)g->P * member_bytes(g); }
int group_reset_launch(gcrl_env_group* g, const uint8_t* mask_host, hipStream_t st) {
  ResetPopArgs r;
  std::memset(&r, 0, sizeof(r));
  r.q = group_args(g);
  r.q.restart = mask_host ? 0 : 1;
  if (int rc = group_table(g, nullptr, st, &r.q.tab)) return rc;
  const int total = g->P * g->N;
  if (mask_host)
    for (int e = 0; e < total; ++e) if (mask_host[e]) r.bits[e >> 5] |= 1u << (e & 31);
  hipLaunchKernelGGL(env_reset_pop_kernel, dim3((total + 63) / 64), dim3(64), 0, st, r);
  GCRL_HIP(hipGetLastError());
  g->launches += 1;
  for (int e = 0; e < total; ++e) if (!mask_host || mask_host[e]) g->t_host[e] = 0;
  if (!mask_host) for (int k = 0; k < g->P; ++k) g->steps[k] = 0;
  return GCRL_OK;
}

}  // namespace

namespace gcrl {

int env_group_step_launch(gcrl_env_group* g, const EnvPopMember* m, hipStream_t st) {
  EnvPopArgs q = group_args(g);
  if (int rc = group_table(g, m, st, &q.tab)) return rc;
  for (int k = 0; k < g->P; ++k) {
    q.act[k] = m[k].act; q.src[k] = (unsigned char)m[k].src; q.eps_ctr0[k] = m[k].eps_ctr0;
    q.noise_on[k] = m[k].noise_on ? 1 : 0; q.noise_ctr0[k] = m[k].noise_ctr0;
  }
  const int total = g->P * g->N;
  hipLaunchKernelGGL(env_step_pop_kernel, dim3((total + 63) / 64), dim3(64), 0, st, q);
  GCRL_HIP(hipGetLastError());
  g->launches += 1;
  for (int k = 0; k < g->P; ++k) g->steps[k] += 1;
  for (int32_t& t : g->t_host) t = t + 1 == g->T ? 0 : t + 1;   // the kernel's rule for t
  return GCRL_OK;
}

gcrl_env* env_group_view(gcrl_env_group* g) {
  if (!g->view) g->view = new gcrl_env;
  gcrl_env* e = g->view;
  e->kind = g->kind; e->N = g->N; e->T = g->T; e->D = g->D; e->A = g->A; e->SW = g->SW; e->device = g->device; e->thr = g->thr; e->seed = g->seeds[0]; e->stream = g->stream;
  e->state = g->state; e->t = g->t; e->cnt = g->cnt; e->rsum = g->rsum; e->rows = g->rows; e->raw = g->data; e->pay = g->data + g->raw_floats;
  e->steps = g->steps[0]; e->launches = g->launches;
  e->t_host.assign(g->t_host.begin(), g->t_host.begin() + g->N);
  return e;
}
void env_group_view_done(gcrl_env_group* g) {
  gcrl_env* e = g->view;
  g->steps[0] = e->steps; g->launches = e->launches;
  std::copy(e->t_host.begin(), e->t_host.end(), g->t_host.begin());
}

}  // namespace gcrl

extern "C" {

// ---------------------------------------------------------------- gcrl_env_group (include/gcrl.h)
gcrl_env_group* gcrl_env_group_create(int kind, int members, int num_envs, const uint64_t* seeds, int max_steps, float threshold, int device) {
  auto bad = [](const char* m) -> gcrl_env_group* { gcrl::fail(GCRL_ERR_ARG, "gcrl_env_group_create: %s", m); return nullptr; };
  if (kind != GCRL_ENV_REACH && kind != GCRL_ENV_PUSH && kind != GCRL_ENV_PICK) return bad("kind: GCRL_ENV_REACH, GCRL_ENV_PUSH or GCRL_ENV_PICK required");
  if (members < 1 || members > kEnvGroupMaxP) return bad("members: 1..16 required");
  if (!seeds) return bad("seeds: null array");
  if (num_envs < 1 || num_envs > kEnvMaxN) return bad("num_envs: 1..1024 required");
  if (max_steps < 1 || max_steps > 64) return bad("max_steps: 1..64 required (the replay ring's flush length limit)");
  if (!(threshold > 0.f) || !(threshold < kBox)) return bad("threshold: must lie in (0, 0.3)");
  if (kind != GCRL_ENV_REACH && !(2.0f * threshold <= kSpawn)) return bad("threshold: push and pick place the goal at least 2 * threshold from the puck and need 2 * threshold <= 0.15");
  int ndev = gcrl_device_count();
  if (ndev <= 0 || device < 0 || device >= ndev) {
    gcrl::fail(GCRL_ERR_HIP, "gcrl_env_group_create: no usable HIP device (count=%d, requested %d); there is no CPU fallback", ndev, device);
    return nullptr;
  }
  gcrl_env_group* g = new gcrl_env_group;
  g->kind = kind; g->P = members; g->N = num_envs; g->T = max_steps; g->thr = threshold; g->device = device;
  g->D = env_obs_dim(kind); g->A = env_action_dim(kind); g->SW = env_state_w(kind);
  for (int k = 0; k < members; ++k) g->seeds[k] = seeds[k];
  g->stride_n = (num_envs + 3) / 4 * 4 + 4;   // at least four rows past N in every member's slice: never read, never written
  g->raw_floats = num_envs * (2 * g->D + 4 * kEnvG);
  g->stride = (g->raw_floats + num_envs * kEnvPayW + 3) / 4 * 4 + 4;
  static std::atomic<uintptr_t> serial{0};
  g->token = reinterpret_cast<const void*>(++serial);
  g->tabs = new gcrl::PopTabCache;
  const size_t PN = (size_t)members * num_envs, PS = (size_t)members * g->stride_n;
  auto ok = [&](hipError_t r, const char* what) {
    if (r == hipSuccess) return true;
    gcrl::fail(GCRL_ERR_HIP, "gcrl_env_group_create: %s failed: %s", what, hipGetErrorString(r));
    return false;
  };
  struct Blk { void** p; size_t bytes; };
  const Blk blks[8] = {{(void**)&g->state, PN * g->SW * sizeof(float)}, {(void**)&g->t, PN * sizeof(int)},
                       {(void**)&g->cnt, PN * 3 * sizeof(unsigned long long)}, {(void**)&g->rsum, PN * sizeof(double)},
                       {(void**)&g->rows, PS * (g->D + kEnvG) * sizeof(float)}, {(void**)&g->data, (size_t)members * g->stride * sizeof(float)},
                       {(void**)&g->noise64, PS * g->A * sizeof(double)}, {(void**)&g->act64, PS * g->A * sizeof(double)}};
  bool good = ok(hipSetDevice(device), "hipSetDevice") && ok(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking), "hipStreamCreate");
  for (const Blk& b : blks) good = good && ok(hipMalloc(b.p, b.bytes), "hipMalloc") && ok(hipMemset(*b.p, 0, b.bytes), "hipMemset");
  if (good) {
    g->t_host.assign(PN, 0);
    good = group_reset_launch(g, nullptr, (hipStream_t) nullptr) == GCRL_OK && ok(hipDeviceSynchronize(), "hipDeviceSynchronize");   // the first step runs on the CALLER's stream
  }
  if (!good) { gcrl_env_group_destroy(g); return nullptr; }
  return g;
}

void gcrl_env_group_destroy(gcrl_env_group* g) {
  if (!g) return;
  (void)hipDeviceSynchronize();   // (a launch on any stream may still read the blocks or a table)
  for (void* p : {(void*)g->state, (void*)g->t, (void*)g->cnt, (void*)g->rsum, (void*)g->rows, (void*)g->data, (void*)g->noise64, (void*)g->act64})
    if (p) (void)hipFree(p);
  if (g->tabs) { static_cast<gcrl::PopTabCache*>(g->tabs)->release(); delete static_cast<gcrl::PopTabCache*>(g->tabs); }
  if (g->stream) (void)hipStreamDestroy(g->stream);
  delete g->view;   // (it owns none of its pointers)
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
  return group_reset_launch(g, mask_host, g->pick(stream));
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
  const size_t PN = (size_t)g->P * g->N;
  std::vector<unsigned long long> cn(PN * 3);
  std::vector<double> rs(PN);
  hipStream_t st = g->pick(stream);
  GCRL_HIP(hipMemcpyAsync(cn.data(), g->cnt, cn.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  GCRL_HIP(hipMemcpyAsync(rs.data(), g->rsum, rs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  GCRL_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < g->P; ++k) {
    int64_t ep = 0, su = 0; double r = 0.0;
    for (int i = 0; i < g->N; ++i) {   // (gcrl_env_stats' order of summation)
      const size_t e = (size_t)k * g->N + i;
      ep += (int64_t)cn[e * 3 + 1]; su += (int64_t)cn[e * 3 + 2]; r += rs[e];
    }
    if (episodes) episodes[k] = ep;
    if (successes) successes[k] = su;
    if (reward_sum) reward_sum[k] = r;
  }
  return GCRL_OK;
}

int64_t gcrl_env_group_state_bytes(const gcrl_env_group* g) { return g ? (int64_t)group_bytes(g) : 0; }

// blob: group header | P member blobs, each what gcrl_env_save_state writes for a standalone env in the member's state
int gcrl_env_group_save_state(gcrl_env_group* g, void* dst_host, int64_t n, void* stream) {
  GCRL_CHECK_ARG(g && dst_host && n == (int64_t)group_bytes(g), "gcrl_env_group_save_state: the blob is %lld bytes", g ? (long long)group_bytes(g) : 0ll);
  hipStream_t st = g->pick(stream);
  GroupHeader gh{kGroupMagic, g->kind, g->P, g->N, g->T, g->thr};
  char* o = static_cast<char*>(dst_host);
  std::memcpy(o, &gh, sizeof(gh)); o += sizeof(gh);
  const size_t N = (size_t)g->N, W = (size_t)g->D + kEnvG;
  for (int k = 0; k < g->P; ++k) {
    EnvHeader hd{kEnvMagic, g->kind, g->N, g->T, g->thr, 0u, g->seeds[k], g->steps[k]};
    std::memcpy(o, &hd, sizeof(hd)); o += sizeof(hd);
    const void* src[5] = {g->state + k * N * g->SW, g->t + k * N, g->cnt + k * N * 3, g->rsum + k * N, g->rows + (size_t)k * g->stride_n * W};
    const size_t len[5] = {N * g->SW * sizeof(float), N * sizeof(int), N * 3 * sizeof(unsigned long long), N * sizeof(double), N * W * sizeof(float)};
    for (int b = 0; b < 5; ++b) { GCRL_HIP(hipMemcpyAsync(o, src[b], len[b], hipMemcpyDeviceToHost, st)); o += len[b]; }
  }
  GCRL_HIP(hipStreamSynchronize(st));
  return GCRL_OK;
}

int gcrl_env_group_load_state(gcrl_env_group* g, const void* src_host, int64_t n, void* stream) {
  GCRL_CHECK_ARG(g && src_host && n >= (int64_t)sizeof(GroupHeader), "gcrl_env_group_load_state: null argument or a blob shorter than its header");
  GroupHeader gh;
  std::memcpy(&gh, src_host, sizeof(gh));
  GCRL_CHECK_ARG(gh.magic == kGroupMagic, "gcrl_env_group_load_state: not an environment group state blob");
  GCRL_CHECK_ARG(gh.kind == g->kind, "gcrl_env_group_load_state: kind: the blob holds kind %d, the handle %d", gh.kind, g->kind);
  GCRL_CHECK_ARG(gh.P == g->P, "gcrl_env_group_load_state: members: the blob holds %d members, the handle %d", gh.P, g->P);
  GCRL_CHECK_ARG(gh.N == g->N, "gcrl_env_group_load_state: num_envs: the blob holds %d envs per member, the handle %d", gh.N, g->N);
  GCRL_CHECK_ARG(gh.T == g->T, "gcrl_env_group_load_state: max_steps: the blob holds %d, the handle %d", gh.T, g->T);
  GCRL_CHECK_ARG(std::memcmp(&gh.thr, &g->thr, sizeof(float)) == 0, "gcrl_env_group_load_state: threshold: the blob holds %g, the handle %g", gh.thr, g->thr);
  GCRL_CHECK_ARG(n == (int64_t)group_bytes(g), "gcrl_env_group_load_state: the blob is %lld bytes, expected %lld", (long long)n, (long long)group_bytes(g));
  const size_t N = (size_t)g->N, W = (size_t)g->D + kEnvG, mb = member_bytes(g);
  const char* base = static_cast<const char*>(src_host) + sizeof(gh);
  for (int k = 0; k < g->P; ++k) {   // every member's header before anything is overwritten
    EnvHeader hd;
    std::memcpy(&hd, base + k * mb, sizeof(hd));
    GCRL_CHECK_ARG(hd.magic == kEnvMagic && hd.kind == g->kind && hd.N == g->N && hd.T == g->T && std::memcmp(&hd.thr, &g->thr, sizeof(float)) == 0,
                   "gcrl_env_group_load_state: members: member %d's record does not match the group header", k);
  }
  hipStream_t st = g->pick(stream);
  for (int k = 0; k < g->P; ++k) {
    EnvHeader hd;
    const char* o = base + k * mb;
    std::memcpy(&hd, o, sizeof(hd)); o += sizeof(hd);
    void* dst[5] = {g->state + k * N * g->SW, g->t + k * N, g->cnt + k * N * 3, g->rsum + k * N, g->rows + (size_t)k * g->stride_n * W};
    const size_t len[5] = {N * g->SW * sizeof(float), N * sizeof(int), N * 3 * sizeof(unsigned long long), N * sizeof(double), N * W * sizeof(float)};
    std::memcpy(g->t_host.data() + k * N, o + len[0], len[1]);
    for (int b = 0; b < 5; ++b) { GCRL_HIP(hipMemcpyAsync(dst[b], o, len[b], hipMemcpyHostToDevice, st)); o += len[b]; }
    g->seeds[k] = hd.seed; g->steps[k] = hd.steps;
  }
  GCRL_HIP(hipStreamSynchronize(st));   // (the source is the caller's pageable memory)
  return GCRL_OK;
}

}  // extern "C"
