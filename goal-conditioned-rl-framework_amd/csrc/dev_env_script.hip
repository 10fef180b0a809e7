// dev_env_script.hip — the pick and glide kinds' scripted controllers as one device kernel, and the native loop that fills a HER ring
// from it (include/gcrl.h gcrl_env_scripted_act, gcrl_her_collect_scripted).  Both are stateless functions of the env's state record,
// in float32 with one rounding per operation.  pick, defined by scripted_action in tests/dev_env_pick_ref.py:
//
//   held:  a[c] = clamp((goal[c] - q[c]) / STEP, -1, 1);  a[3] = -1                      carry the object to the goal, fingers closed
//   else:  d = q - p;  s = sum_c d[c]^2
//          s < 0.01 * 0.01 ?  a = (0, 0, 0, -1)                                           over the object: close the fingers
//                          :  a[c] = clamp(d[c] / STEP, -1, 1), a[3] = +1                 go to the object, fingers open
//
// glide, defined by scripted_action in tests/dev_env_glide_ref.py — strike the puck so that its glide ends on the goal, then let go:
//
//   d = goal.xy - q.xy;  L = sqrt(d.x^2 + d.y^2);  L < 1e-6 ?  a = 0
//   u = d / L;  rest = (sqrt(vq.x^2 + vq.y^2) * FRICTION) / (1 - FRICTION)              the way the puck still glides by itself
//   rest >= L - 0.5 * thr ?  a = (unit(-u.x), unit(-u.y), 0)                             hands off: it will arrive
//   e = (q.xy - 0.03 * u) - p.xy;  off = e.x^2 + e.y^2                                   the striking position behind the puck
//   off > 0.005^2:  p.z < LIFT - 0.005 and off > 0.02^2 ?  a = (0, 0, unit((LIFT - p.z) / STEP))        rise before travelling
//                   else a.xy = unit(e / STEP), a.z = unit(((off > 0.02^2 ? LIFT : 0) - p.z) / STEP)
//   p.z > 0.005:    a.xy = unit(e / STEP), a.z = unit((0 - p.z) / STEP)                  descend behind the puck
//   else            v = L > 0.9 * (STEP / (1 - FRICTION)) ? STEP : L * (1 - FRICTION);  a.xy = unit(u * v / STEP), a.z = 0
//
// Optional noise, float(double(hash_normal(seed, ctr0 + i * A + c)) * noise_std), is added before a final clamp to [-1, 1].
//
// Kernel rules (dev_env.hip's): every address comes from the handle or the caller's checked arguments; an env index >= N does
// nothing; no atomics; no waits; no per-thread scratch; plain vector stores only; the unit is built with -ffp-contract=off.
#include "dev_env_body.h"   // EnvArgs, load_state, the rule's constants

namespace {

constexpr float kReached = 0.01f * 0.01f;
// glide: 1 - FRICTION, the striking position's distance behind the puck, "in place" and "travel at LIFT" squared distances, the
// slack in z, and the distance beyond which one strike cannot reach the goal
constexpr float kOneMinusF = 1.0f - kFriction, kBehind = 0.03f, kNear2 = 0.005f * 0.005f, kAway2 = 0.02f * 0.02f, kSlack = 0.005f;
constexpr float kCarry = 0.9f * (kStep / kOneMinusF);

struct ScriptArgs {
  EnvArgs a;              // state, kind, N and thr alone are read
  float* out;             // [N][A]
  int noisy; double noise_std; unsigned long long seed, ctr0;
};

__device__ inline float unit(float x) { return fminf(fmaxf(x, -1.0f), 1.0f); }

__global__ __launch_bounds__(64) void env_scripted_kernel(ScriptArgs q) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= q.a.N) return;
  EnvState s;
  load_state(q.a, i, s);
  const int A = env_action_dim(q.a.kind);
  float act[4];
  if (q.a.kind == GCRL_ENV_GLIDE) {
    act[0] = 0.f; act[1] = 0.f; act[2] = 0.f; act[3] = 0.f;
    const float dx = s.goal[0] - s.q[0], dy = s.goal[1] - s.q[1];
    const float L = sqrtf(dx * dx + dy * dy);
    if (!(L < 1e-6f)) {
      const float ux = dx / L, uy = dy / L;
      const float rest = (sqrtf(s.vq[0] * s.vq[0] + s.vq[1] * s.vq[1]) * kFriction) / kOneMinusF;
      const float ex = (s.q[0] - kBehind * ux) - s.p[0], ey = (s.q[1] - kBehind * uy) - s.p[1];
      const float off = ex * ex + ey * ey;
      if (rest >= L - 0.5f * q.a.thr) {
        act[0] = unit(-ux); act[1] = unit(-uy);
      } else if (off > kNear2) {
        const bool away = off > kAway2;
        if (s.p[2] < kLift - kSlack && away) {
          act[2] = unit((kLift - s.p[2]) / kStep);
        } else {
          act[0] = unit(ex / kStep); act[1] = unit(ey / kStep);
          act[2] = unit(((away ? kLift : 0.0f) - s.p[2]) / kStep);
        }
      } else if (s.p[2] > kSlack) {
        act[0] = unit(ex / kStep); act[1] = unit(ey / kStep);
        act[2] = unit((0.0f - s.p[2]) / kStep);
      } else {
        const float v = L > kCarry ? kStep : L * kOneMinusF;
        act[0] = unit((ux * v) / kStep); act[1] = unit((uy * v) / kStep);
      }
    }
  } else if (s.held != 0.f) {
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
  float* o = q.out + (size_t)i * A;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c < A) {
      float x = act[c];
      if (q.noisy) x = unit(x + (float)((double)gcrl::hash_normal(q.seed, q.ctr0 + (unsigned long long)i * A + c) * q.noise_std));
      o[c] = x;
    }
  }
}

}  // namespace

namespace gcrl {

int env_scripted_launch(gcrl_env_group* e, float* out, double noise_std, unsigned long long seed, unsigned long long ctr0, hipStream_t st) {
  ScriptArgs q;
  std::memset(&q, 0, sizeof(q));
  q.a.state = e->state; q.a.kind = e->kind; q.a.N = e->N; q.a.thr = e->thr;
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
  GCRL_CHECK_ARG(env->kind == GCRL_ENV_PICK || env->kind == GCRL_ENV_GLIDE, "%s: kind: the pick and glide kinds alone have a scripted controller; this env has kind %d", who,
                 env->kind);
  GCRL_CHECK_ARG(noise_std >= 0.0 && noise_std <= 1e30, "%s: noise_std: a finite value >= 0 required", who);
  return gcrl::env_scripted_launch(env, out_dev, noise_std, seed, counter * (unsigned long long)env->N * env->A, env->pick(stream));
}

int64_t gcrl_her_collect_scripted(gcrl_her* ring, gcrl_env* env, gcrl_normalizer* nz_obs, gcrl_normalizer* nz_dg, int steps, double noise_std,
                                  uint64_t seed, uint64_t counter0, void* stream) {
  const char* who = "gcrl_her_collect_scripted";
  GCRL_CHECK_ARG(ring && env, "%s: null argument", who);
  // every refusal comes before a ring slot or a step of the env is consumed
  GCRL_CHECK_ARG(steps >= 1, "%s: steps: %d (>= 1 required)", who, steps);
  GCRL_CHECK_ARG(env->kind == GCRL_ENV_PICK || env->kind == GCRL_ENV_GLIDE, "%s: kind: the pick and glide kinds alone have a scripted controller; this env has kind %d", who,
                 env->kind);
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
