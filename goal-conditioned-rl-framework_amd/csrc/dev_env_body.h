// dev_env_body.h — what the environment units share: EnvArgs, the arguments of ONE member of a gcrl_env_group (a standalone gcrl_env is a
// one-member group), and the device text of what an env's thread does with them on a reset and on a step.  dev_env.hip's
// env_reset_kernel / env_step_kernel take an EnvArgs by value: the form every one-member group launches, with the arguments built on
// the host from member 0's slices.  dev_env_group.hip's population kernels build the same EnvArgs per thread from the member table of
// a group of several — so a member's arithmetic is the same text whichever form runs it.  The rule is restated in numpy in
// tests/dev_env_ref.py (reach, push), tests/dev_env_pick_ref.py (pick) and tests/dev_env_glide_ref.py (glide), which are its
// definition.  Units that include this are built with -ffp-contract=off.
//
// The action width and the state record's width follow the kind (dev_env.h env_action_dim, env_state_w).  Every small array is
// indexed by the constants of a fully unrolled loop, a fourth action component behind `c < A`: nothing lives in per-thread scratch.
#pragma once
#include "dev_env.h"
#include "her_ring.h"   // hash_below
#include "ops.h"        // hash_normal

struct EnvArgs {
  float* state; int* t; unsigned long long* cnt; double* rsum;
  float* rows; float* raw; float* pay;
  const void* act; int act_f64;
  // act_eps: the env's thread forms its own action, clamp(hash_normal(eps_seed, eps_ctr0 + i * A + c), -1, 1) — what clipped_normal_fill writes
  int act_eps; unsigned long long eps_seed, eps_ctr0;
  int restart;
  int kind, N, T, D;
  float thr;
  unsigned long long seed;
  // rider of the collect loop: the exploration noise of the NEXT vector step, A elements per env, written by the env's thread
  void* noise; int noise_f64; unsigned long long noise_seed, noise_ctr0; double noise_scale;
};

namespace gcrl {
// dev_env.hip, for the group's host code: the by-value kernels on `st`.  mask_host (a.N bytes) selects the envs that go on to their
// next episode; it is ignored when a.restart is set
int env_step_args_launch(const EnvArgs& a, hipStream_t st);
int env_reset_args_launch(const EnvArgs& a, const uint8_t* mask_host, hipStream_t st);
}  // namespace gcrl

namespace {

constexpr unsigned long long kEnvStream = 0x4445562d454e5621ull;   // "DEV-ENV!"
constexpr float kStep = 0.04f, kBox = 0.3f, kSpawn = 0.15f, kContact = 0.05f, kLift = 0.1f;
constexpr float kFinger = 0.02f, kOpen = 0.08f, kClose = 0.04f, kFall = 0.04f;   // pick: finger travel per step, opening, grasp width, fall per step
constexpr float kFriction = 0.9f, kFar = 0.9f;                                   // glide: share of its displacement a free puck keeps, the far wall in x

__device__ inline float u01(unsigned long long seed, int env, unsigned long long ep, int comp) {
  return (float)gcrl::hash_below(seed, kEnvStream + (unsigned long long)env, 8ull * ep + (unsigned long long)comp, 1u << 24) * (1.0f / 16777216.0f);
}
__device__ inline float spawn(float u) { return (u * 2.0f - 1.0f) * kSpawn; }
__device__ inline float clamp_box(float x) { return fminf(fmaxf(x, -kBox), kBox); }
__device__ inline float clamp_z(float x) { return fminf(fmaxf(x, 0.0f), kBox); }

// pick alone uses w (finger opening), held (0 / 1) and vw (the fingers' displacement of the last step); pick and glide use vq (the object's)
struct EnvState { float p[3], q[3], vel[3], goal[3]; float w, held, vq[3], vw; };

__device__ inline void seed_env(const EnvArgs& a, int i, unsigned long long ep, EnvState& s) {
#pragma unroll
  for (int c = 0; c < 3; ++c) { s.vel[c] = 0.f; s.vq[c] = 0.f; }
  s.w = kOpen; s.held = 0.f; s.vw = 0.f;
  if (a.kind == GCRL_ENV_REACH) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { s.p[c] = spawn(u01(a.seed, i, ep, c)); s.q[c] = 0.f; s.goal[c] = spawn(u01(a.seed, i, ep, 3 + c)); }
  } else if (a.kind == GCRL_ENV_GLIDE) {
    s.q[0] = spawn(u01(a.seed, i, ep, 0)); s.q[1] = spawn(u01(a.seed, i, ep, 1)); s.q[2] = 0.f;
    s.p[0] = spawn(u01(a.seed, i, ep, 2)); s.p[1] = spawn(u01(a.seed, i, ep, 3)); s.p[2] = kLift;
    s.goal[0] = 0.45f + u01(a.seed, i, ep, 4) * 0.2f;          // beyond the pusher's box
    s.goal[1] = spawn(u01(a.seed, i, ep, 5));
    s.goal[2] = 0.f;
  } else {
    s.q[0] = spawn(u01(a.seed, i, ep, 0)); s.q[1] = spawn(u01(a.seed, i, ep, 1)); s.q[2] = 0.f;
    s.p[0] = spawn(u01(a.seed, i, ep, 2)); s.p[1] = spawn(u01(a.seed, i, ep, 3)); s.p[2] = kLift;
    const float two = 2.0f * a.thr;
    const float m = two + u01(a.seed, i, ep, 4) * (kSpawn - two);
    s.goal[0] = u01(a.seed, i, ep, 5) < 0.5f ? s.q[0] - m : s.q[0] + m;
    s.goal[1] = spawn(u01(a.seed, i, ep, 6));
    s.goal[2] = a.kind == GCRL_ENV_PICK ? fmaxf(spawn(u01(a.seed, i, ep, 7)), 0.0f) : 0.f;
  }
}

__device__ inline void load_state(const EnvArgs& a, int i, EnvState& s) {
  const float* w = a.state + (size_t)i * env_state_w(a.kind);
#pragma unroll
  for (int c = 0; c < 3; ++c) { s.p[c] = w[c]; s.q[c] = w[3 + c]; s.vel[c] = w[6 + c]; s.goal[c] = w[9 + c]; s.vq[c] = 0.f; }
  s.w = kOpen; s.held = 0.f; s.vw = 0.f;
  if (a.kind == GCRL_ENV_PICK) {
    s.w = w[12]; s.held = w[13]; s.vw = w[17];
#pragma unroll
    for (int c = 0; c < 3; ++c) s.vq[c] = w[14 + c];
  } else if (a.kind == GCRL_ENV_GLIDE) {
#pragma unroll
    for (int c = 0; c < 3; ++c) s.vq[c] = w[12 + c];
  }
}
__device__ inline void store_state(const EnvArgs& a, int i, const EnvState& s) {
  float* w = a.state + (size_t)i * env_state_w(a.kind);
#pragma unroll
  for (int c = 0; c < 3; ++c) { w[c] = s.p[c]; w[3 + c] = s.q[c]; w[6 + c] = s.vel[c]; w[9 + c] = s.goal[c]; }
  if (a.kind == GCRL_ENV_PICK) {
    w[12] = s.w; w[13] = s.held; w[17] = s.vw;
#pragma unroll
    for (int c = 0; c < 3; ++c) w[14 + c] = s.vq[c];
  } else if (a.kind == GCRL_ENV_GLIDE) {
#pragma unroll
    for (int c = 0; c < 3; ++c) w[12 + c] = s.vq[c];
  }
}
// squared distance of x and y, the squares summed in component order
__device__ inline float dist2(const float* x, const float* y) {
  float d2 = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) { const float df = x[c] - y[c]; d2 = d2 + df * df; }
  return d2;
}
// obs of state s at step count t -> o[0 .. D)
__device__ inline void write_obs(const EnvArgs& a, const EnvState& s, int t, float* o) {
  const float tt = (float)t / (float)a.T;
  if (a.kind == GCRL_ENV_REACH) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = s.p[c]; o[3 + c] = s.vel[c]; }
    o[6] = tt;
  } else if (a.kind == GCRL_ENV_PUSH) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = s.p[c]; o[3 + c] = s.q[c]; o[6 + c] = s.q[c] - s.p[c]; o[9 + c] = s.vel[c]; }
    o[12] = tt;
  } else if (a.kind == GCRL_ENV_GLIDE) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = s.p[c]; o[3 + c] = s.q[c]; o[6 + c] = s.q[c] - s.p[c]; o[9 + c] = s.vel[c]; o[12 + c] = s.vq[c]; }
    o[15] = tt;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = s.p[c]; o[3 + c] = s.q[c]; o[6 + c] = s.q[c] - s.p[c]; o[9 + c] = s.vel[c]; o[12 + c] = s.vq[c]; }
    o[15] = s.w; o[16] = s.vw; o[17] = s.held;
    o[18] = dist2(s.p, s.q) < kContact * kContact ? 1.0f : 0.0f;
    o[19] = tt;
  }
}
__device__ inline void write_row(const EnvArgs& a, int i, const EnvState& s, int t) {
  float* row = a.rows + (size_t)i * (a.D + kEnvG);
  write_obs(a, s, t, row);
#pragma unroll
  for (int c = 0; c < 3; ++c) row[a.D + c] = s.goal[c];
}

// env i of `a`: back to episode 0 with the counters at zero (a.restart), or on to its next episode
__device__ inline void env_reset_body(const EnvArgs& a, int i) {
  unsigned long long* cn = a.cnt + (size_t)i * 3;
  unsigned long long ep;
  if (a.restart) {
    ep = 0; cn[1] = 0; cn[2] = 0; a.rsum[i] = 0.0;
  } else {
    ep = cn[0] + 1;
  }
  cn[0] = ep;
  EnvState s;
  seed_env(a, i, ep, s);
  store_state(a, i, s);
  a.t[i] = 0;
  write_row(a, i, s, 0);
}

// an action component as the rule takes it: a NaN counts as 0, then clamped to [-1, 1]
__device__ inline float clean_action(float x) {
  x = (x == x) ? x : 0.0f;
  return fminf(fmaxf(x, -1.0f), 1.0f);
}

// one step of env i of `a`: the body env_step_kernel and env_step_pop_kernel share, so a member's step is the same in a group of one and of many
__device__ inline void env_step_body(const EnvArgs& a, int i) {
  const int N = a.N, D = a.D, A = env_action_dim(a.kind);
  EnvState s;
  load_state(a, i, s);
  int t = a.t[i];
  float* obs = a.raw + (size_t)i * D;
  float* nobs = a.raw + (size_t)N * D + (size_t)i * D;
  float* dg = a.raw + (size_t)2 * N * D + (size_t)i * kEnvG;
  float* ndg = dg + (size_t)N * kEnvG;
  float* ag = ndg + (size_t)N * kEnvG;
  float* nag = ag + (size_t)N * kEnvG;
  float* pw = a.pay + (size_t)i * kEnvPayW;
  write_obs(a, s, t, obs);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    dg[c] = s.goal[c]; ndg[c] = s.goal[c];
    ag[c] = a.kind == GCRL_ENV_REACH ? s.p[c] : s.q[c];
  }
  float act[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    act[c] = 0.f;
    if (c < A) {
      if (a.act_eps) act[c] = fminf(fmaxf(gcrl::hash_normal(a.eps_seed, a.eps_ctr0 + (unsigned long long)i * A + c), -1.0f), 1.0f);
      else act[c] = a.act_f64 ? (float)static_cast<const double*>(a.act)[(size_t)i * A + c] : static_cast<const float*>(a.act)[(size_t)i * A + c];
    }
  }
  float pn[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    s.vel[c] = kStep * clean_action(act[c]);
    pn[c] = clamp_box(s.p[c] + s.vel[c]);
  }
  if (a.kind == GCRL_ENV_PUSH) {
    if (dist2(pn, s.q) < kContact * kContact) {
      s.q[0] = clamp_box(s.q[0] + (pn[0] - s.p[0]));
      s.q[1] = clamp_box(s.q[1] + (pn[1] - s.p[1]));
    }
  } else if (a.kind == GCRL_ENV_PICK) {
    pn[2] = clamp_z(s.p[2] + s.vel[2]);                       // the gripper stays above the table
    const float wn = fminf(fmaxf(s.w + kFinger * clean_action(act[3]), 0.0f), kOpen);
    const bool near = dist2(pn, s.q) < kContact * kContact, closed = wn < kClose;
    // a grasp: the fingers close while around the object; it lasts while they stay closed
    const bool held = s.held != 0.f ? closed : (near && closed && s.w >= kClose);
    float qn[3];
    if (held) {
      qn[0] = clamp_box(s.q[0] + (pn[0] - s.p[0]));
      qn[1] = clamp_box(s.q[1] + (pn[1] - s.p[1]));
      qn[2] = clamp_z(s.q[2] + (pn[2] - s.p[2]));
    } else {
      const bool shove = near && closed;                      // a closed fist pushes, as `push`
      qn[0] = shove ? clamp_box(s.q[0] + (pn[0] - s.p[0])) : s.q[0];
      qn[1] = shove ? clamp_box(s.q[1] + (pn[1] - s.p[1])) : s.q[1];
      qn[2] = fmaxf(s.q[2] - kFall, 0.0f);                    // a released object falls
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { s.vq[c] = qn[c] - s.q[c]; s.q[c] = qn[c]; }
    s.vw = wn - s.w; s.w = wn; s.held = held ? 1.0f : 0.0f;
  } else if (a.kind == GCRL_ENV_GLIDE) {
    // a touched puck takes the pusher's displacement, a free one keeps kFriction of its own; a wall stops that component
    const bool contact = dist2(pn, s.q) < kContact * kContact;
    const float dx = contact ? pn[0] - s.p[0] : kFriction * s.vq[0];
    const float dy = contact ? pn[1] - s.p[1] : kFriction * s.vq[1];
    const float qx = fminf(fmaxf(s.q[0] + dx, -kBox), kFar), qy = clamp_box(s.q[1] + dy);
    s.vq[0] = qx - s.q[0]; s.vq[1] = qy - s.q[1]; s.vq[2] = 0.0f - s.q[2];
    s.q[0] = qx; s.q[1] = qy; s.q[2] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) s.p[c] = pn[c];
  pw[0] = __int_as_float(t);
  t += 1;
  write_obs(a, s, t, nobs);
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c < A) pw[3 + c] = act[c];
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float g = a.kind == GCRL_ENV_REACH ? s.p[c] : s.q[c];
    nag[c] = g;
    pw[3 + A + c] = g;
    const float df = g - s.goal[c];
    acc = acc + df * df;
  }
  const float dist = sqrtf(acc);
  const float r = dist > a.thr ? -1.0f : -0.0f;
  pw[1] = r; pw[2] = 0.f;
  a.rsum[i] = a.rsum[i] + (double)r;
  if (t == a.T) {
    unsigned long long* cn = a.cnt + (size_t)i * 3;
    cn[1] = cn[1] + 1;
    if (dist < a.thr) cn[2] = cn[2] + 1;
    const unsigned long long ep = cn[0] + 1;
    cn[0] = ep;
    seed_env(a, i, ep, s);
    t = 0;
  }
  store_state(a, i, s);
  a.t[i] = t;
  write_row(a, i, s, t);
  if (a.noise) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < A) {
        const float z = gcrl::hash_normal(a.noise_seed, a.noise_ctr0 + (unsigned long long)i * A + c);
        if (a.noise_f64) static_cast<double*>(a.noise)[(size_t)i * A + c] = (double)z * a.noise_scale;
        else static_cast<float*>(a.noise)[(size_t)i * A + c] = (float)((double)z * a.noise_scale);
      }
    }
  }
}

}  // namespace
