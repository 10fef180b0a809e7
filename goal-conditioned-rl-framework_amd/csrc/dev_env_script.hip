// dev_env_script.hip — the pick kind's scripted controller as a device kernel, and the native loop that fills a HER ring from it
// (include/gcrl.h gcrl_env_scripted_act, gcrl_her_collect_scripted).  The controller is defined by scripted_action in
// tests/dev_env_pick_ref.py, in float32 with one rounding per operation:
//
//   held:  a[c] = clamp((goal[c] - q[c]) / STEP, -1, 1);  a[3] = -1                      carry the object to the goal, fingers closed
//   else:  d = q - p;  s = sum_c d[c]^2
//          s < 0.01 * 0.01 ?  a = (0, 0, 0, -1)                                           over the object: close the fingers
//                          :  a[c] = clamp(d[c] / STEP, -1, 1), a[3] = +1                 go to the object, fingers open
//
// Optional noise, float(double(hash_normal(seed, ctr0 + i * 4 + c)) * noise_std), is added before a final clamp to [-1, 1].
//
// Kernel rules (dev_env.hip's): every address comes from the handle or the caller's checked arguments; an env index >= N does
// nothing; no atomics; no waits; no per-thread scratch; plain vector stores only; the unit is built with -ffp-contract=off.
#include "dev_env_body.h"   // EnvArgs, load_state, the rule's constants

namespace {

constexpr float kReached = 0.01f * 0.01f;

struct ScriptArgs {
  EnvArgs a;              // state, kind and N alone are read
  float* out;             // [N][4]
  int noisy; double noise_std; unsigned long long seed, ctr0;
};

__device__ inline float unit(float x) { return fminf(fmaxf(x, -1.0f), 1.0f); }

__global__ __launch_bounds__(64) void env_scripted_kernel(ScriptArgs q) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= q.a.N) return;
  EnvState s;
  load_state(q.a, i, s);
  float act[4];
  if (s.held != 0.f) {
#pragma unroll
    for (int c = 0; c < 3; ++c) act[c] = unit((s.goal[c] - s.q[c]) / kStep);
    act[3] = -1.0f;
  } else {
    float d[3], sum = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) { d[c] = s.q[c] - s.p[c]; sum = sum + d[c] * d[c]; }
    const bool over = sum < kReached;
#pragma unroll
    for (int c = 0; c < 3; ++c) act[c] = over ? 0.0f : unit(d[c] / kStep);
    act[3] = over ? -1.0f : 1.0f;
  }
  float* o = q.out + (size_t)i * 4;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float x = act[c];
    if (q.noisy) x = unit(x + (float)((double)gcrl::hash_normal(q.seed, q.ctr0 + (unsigned long long)i * 4 + c) * q.noise_std));
    o[c] = x;
  }
}

}  // namespace

namespace gcrl {

int env_scripted_launch(gcrl_env_group* e, float* out, double noise_std, unsigned long long seed, unsigned long long ctr0, hipStream_t st) {
  ScriptArgs q;
  std::memset(&q, 0, sizeof(q));
  q.a.state = e->state; q.a.kind = e->kind; q.a.N = e->N;
  q.out = out; q.noisy = noise_std > 0.0 ? 1 : 0; q.noise_std = noise_std; q.seed = seed; q.ctr0 = ctr0;
  hipLaunchKernelGGL(env_scripted_kernel, dim3((e->N + 63) / 64), dim3(64), 0, st, q);
  GCRL_HIP(hipGetLastError());
  e->launches += 1;
  return GCRL_OK;
}

}  // namespace gcrl

extern "C" {

int gcrl_env_scripted_act(gcrl_env* env, float* out_dev, double noise_std, uint64_t seed, uint64_t counter, void* stream) {
  const char* who = "gcrl_env_scripted_act";
  GCRL_CHECK_ARG(env && out_dev, "%s: null argument", who);
  GCRL_CHECK_ARG(env->kind == GCRL_ENV_PICK, "%s: kind: the scripted controller is the pick kind's; this env has kind %d", who, env->kind);
  GCRL_CHECK_ARG(noise_std >= 0.0 && noise_std <= 1e30, "%s: noise_std: a finite value >= 0 required", who);
  return gcrl::env_scripted_launch(env, out_dev, noise_std, seed, counter * (unsigned long long)env->N * env->A, env->pick(stream));
}

int64_t gcrl_her_collect_scripted(gcrl_her* ring, gcrl_env* env, gcrl_normalizer* nz_obs, gcrl_normalizer* nz_dg, int steps, double noise_std,
                                  uint64_t seed, uint64_t counter0, void* stream) {
  const char* who = "gcrl_her_collect_scripted";
  GCRL_CHECK_ARG(ring && env, "%s: null argument", who);
  // every refusal comes before a ring slot or a step of the env is consumed
  GCRL_CHECK_ARG(steps >= 1, "%s: steps: %d (>= 1 required)", who, steps);
  GCRL_CHECK_ARG(env->kind == GCRL_ENV_PICK, "%s: kind: the scripted controller is the pick kind's; this env has kind %d", who, env->kind);
  GCRL_CHECK_ARG(noise_std >= 0.0 && noise_std <= 1e30, "%s: noise_std: a finite value >= 0 required", who);
  GCRL_CHECK_ARG(env->device == ring->cfg.device, "%s: env: it lives on device %d, the ring on device %d", who, env->device, ring->cfg.device);
  GCRL_CHECK_ARG(env->N <= ring->cfg.nenvs, "%s: env: %d envs for a ring of %d episode slots", who, env->N, ring->cfg.nenvs);
  GCRL_CHECK_ARG(env->D + kEnvG == ring->S && env->A == ring->A && kEnvG == ring->G, "%s: env: obs_dim %d + goal_dim %d / action_dim %d, the ring has state_dim %d / action_dim %d / goal_dim %d",
                 who, env->D, kEnvG, env->A, ring->S, ring->A, ring->G);
  GCRL_CHECK_ARG(env->T == ring->cfg.flush_len, "%s: max_steps: the env's horizon %d differs from the ring's flush length %d", who, env->T, ring->cfg.flush_len);
  GCRL_CHECK_ARG(ring->cfg.reward_kind == GCRL_REWARD_SPARSE, "%s: compute_reward: the ring's reward kind is %s; the env's reward is the built-in sparse kind", who,
                 ring->cfg.reward_kind == GCRL_REWARD_HOST ? "a host callback" : "dense");
  GCRL_CHECK_ARG(std::memcmp(&env->thr, &ring->cfg.reward_threshold, sizeof(float)) == 0, "%s: threshold: the env's %g differs from the ring's %g", who, env->thr,
                 ring->cfg.reward_threshold);
  GCRL_CHECK_ARG(!nz_obs || gcrl_normalizer_size(nz_obs) == env->D, "%s: nz_obs: the observation normaliser has size %d for obs_dim %d", who,
                 nz_obs ? gcrl_normalizer_size(nz_obs) : 0, env->D);
  GCRL_CHECK_ARG(!nz_dg || gcrl_normalizer_size(nz_dg) == kEnvG, "%s: nz_dg: the goal normaliser has size %d for goal_dim %d", who,
                 nz_dg ? gcrl_normalizer_size(nz_dg) : 0, kEnvG);
  const int N = env->N;
  for (int i = 0; i < N; ++i)
    if (env->t_host[i] != ring->staged[i])
      return gcrl::fail(GCRL_ERR_STATE, "%s: t: env %d is at step %d of its episode, the ring has %d transitions staged for it", who, i, env->t_host[i], ring->staged[i]);
  hipStream_t st = ring->pick(stream);
  void* sarg = stream ? stream : (void*)ring->stream;   // one stream for both handles: the loop is stream-ordered
  // the controller's actions have a block of their own, kept by the env for as long as it lives
  if (!env->script_act) GCRL_HIP(hipMalloc((void**)&env->script_act, (size_t)N * env->A * sizeof(float)));
  const unsigned long long per_step = (unsigned long long)N * env->A;
  std::vector<int32_t> t_before;
  int64_t total = 0;
  for (int s = 0; s < steps; ++s) {
    if (int rc = gcrl::env_scripted_launch(env, env->script_act, noise_std, seed, (counter0 + (unsigned long long)s) * per_step, st)) return rc;
    t_before.assign(env->t_host.begin(), env->t_host.end());   // the payload's t words: the envs' step counts BEFORE the step
    if (int rc = gcrl::env_step_launch(env, env->script_act, 0, st)) return rc;
    const int64_t r = gcrl_her_process_step_dev(ring, nz_obs, nz_obs ? 1 : 0, nz_dg, nz_dg ? 1 : 0, env->raw(), env->pay(), env->D, t_before.data(), nullptr, 0, N, sarg);
    if (r < 0) return r;
    total += r;
  }
  return total;
}

}  // extern "C"
