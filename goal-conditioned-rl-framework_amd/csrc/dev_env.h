// dev_env.h — device-resident goal environments: P x N independent envs of one built-in kind whose state, counters and the blocks of a
// vector step live in device memory, behind ONE handle type, gcrl_env_group.  The ABI's gcrl_env is a group of one member and nothing
// more.  One step launch writes every member's `raw` and `pay` blocks in the layout her_ring.hip's her_process_step_body reads and the
// next step's acting rows [obs | goal] in the layout the acting kernels read, so a collect loop (agent.hip, agent_pop.inc) is
// act -> step -> process-step with nothing crossing to the host.
// The rule is restated in numpy in tests/dev_env_ref.py (reach, push), tests/dev_env_pick_ref.py (pick) and tests/dev_env_glide_ref.py
// (glide), which are its definition.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"

constexpr int kEnvG = 3;                 // goal width of every kind
constexpr int kEnvPayW = 32;             // floats per env of the payload block (her_ring.hip kPayW)
constexpr int kEnvMaxN = 1024;
// per kind: action width, observation width, and floats per env of the state record —
// p(3) q(3) vel_p(3) goal(3), for pick | w held vel_q(3) vel_w, for glide | vel_q(3)
__host__ __device__ constexpr int env_action_dim(int kind) { return kind == GCRL_ENV_PICK ? 4 : 3; }
__host__ __device__ constexpr int env_obs_dim(int kind) {
  return kind == GCRL_ENV_REACH ? 7 : kind == GCRL_ENV_PUSH ? 13 : kind == GCRL_ENV_GLIDE ? 16 : 20;
}
__host__ __device__ constexpr int env_state_w(int kind) { return kind == GCRL_ENV_PICK ? 18 : kind == GCRL_ENV_GLIDE ? 15 : 12; }

// P x N envs in single allocations: the only struct that owns env memory.  Member m has its own seed, state, counters and
// random-number keys; its blocks are slices at the strides the population kernels take (rowchain.h RowActPop, act_bn.h ActBnPop,
// her_ring.hip her_process_step_pop_kernel).  The slices of member 0 of a one-member group are the contiguous blocks the single-agent
// kernels take: no kernel reads the padding past N.
constexpr int kEnvGroupMaxP = 16;        // a population's member limit
struct gcrl_env_group {
  int kind = 0, P = 0, N = 0, T = 0, D = 0, device = 0;
  int A = 3, SW = 12;                    // env_action_dim(kind), env_state_w(kind)
  int stride_n = 0;                      // rows per member of rows / noise64 / act64 (> N: the rows past N are never touched)
  int stride = 0, raw_floats = 0;        // floats per member of `data`; a member's slice is raw (raw_floats) | pay [N][kEnvPayW]
  float thr = 0.f;
  uint64_t seeds[kEnvGroupMaxP] = {};
  hipStream_t stream = nullptr;
  // device state: everything a resume needs
  float* state = nullptr;                // [P][N][SW]
  int* t = nullptr;                      // [P][N] steps taken in the running episode
  unsigned long long* cnt = nullptr;     // [P][N][3]: episode index (the RNG key), episodes finished, successes
  double* rsum = nullptr;                // [P][N] reward sum
  // blocks of a step
  float* rows = nullptr;                 // [P][stride_n][D + G] acting rows of the NEXT step
  float* data = nullptr;                 // [P][stride]: raw = [obs N*D | next_obs N*D | dg N*G | next_dg N*G | ag N*G | next_ag N*G], then
                                         // pay [N][kEnvPayW] = t | r | done = 0 | action(A) | next_ag(G)
  double* noise64 = nullptr;             // [P][stride_n][A]: the exploration noise / eps of the next vector step (the population collect loop's)
  double* act64 = nullptr;               // [P][stride_n][A]: the acting launch's float64 actions (the population collect and evaluate loops')
  float* script_act = nullptr;           // [N][A] the scripted controller's actions (gcrl_her_collect_scripted; allocated on first use)
  void* tabs = nullptr;                  // P > 1: PopTabCache (pop.h) of the launches' member tables
  int64_t steps[kEnvGroupMaxP] = {}, launches = 0;   // vector steps taken per member / kernel launches issued since creation
  std::vector<int32_t> t_host;           // [P][N] host mirror of t: the step kernel's rule (t + 1, 0 at the horizon) needs no read-back
  std::vector<uint8_t> rolled;           // [P][N] whether the LAST step launch took the env over its horizon (a reset is not a roll-over)
  int64_t vsteps = 0;                    // step launches since creation, never reset: names "the last step" for goal_propose.hip
  const void* token = nullptr;           // unique per handle ever created (a small serial, never an address): names the handle in an agent's
                                         // record of whose noise its stream last wrote, so a later handle at a reused address is not mistaken for it

  float* raw(int m = 0) const { return data + (size_t)m * stride; }
  float* pay(int m = 0) const { return raw(m) + raw_floats; }
  hipStream_t pick(void* s) const {
    if (!s) return stream;
    if (s == GCRL_STREAM_LEGACY) return (hipStream_t) nullptr;
    return (hipStream_t)s;
  }
};
struct gcrl_env : gcrl_env_group {};     // the ABI's name of a one-member group

namespace gcrl {

// ---- the handle's step launches (dev_env_group.hip, with all other host code of the handle)
// What a step needs of member m.  src: where its actions come from.
enum { kEnvActF32 = 0, kEnvActF64 = 1, kEnvActEps = 2 };
struct EnvPopMember {
  const void* act;                       // [N][A] float32 (kEnvActF32) or float64 (kEnvActF64); ignored for kEnvActEps
  int src;
  // kEnvActEps: action (i, j) = clamp(hash_normal(eps_seed, eps_ctr0 + i * A + j), -1, 1), formed by the env's own thread
  unsigned long long eps_seed, eps_ctr0;
  // rider: the member's noise of the NEXT vector step into its slice of the group's noise64 block (float64); noise_on == 0: none
  int noise_on;
  unsigned long long noise_seed, noise_ctr0; double noise_scale;
};
// One vector step of every member on `st`, m[0 .. P), one launch: env_step_pop_kernel for P > 1, and for a one-member group
// env_step_kernel with the arguments built here from member 0's slices (no member table)
int env_group_step_launch(gcrl_env_group* g, const EnvPopMember* m, hipStream_t st);
// A one-member group's step from actions [N][A], float32 (f64 == 0) or the float64 the acting kernels write (rounded to float32 first)
int env_step_launch(gcrl_env_group* g, const void* actions_dev, int f64, hipStream_t st);
// the same with the collect loop's rider into a block of the caller's: the env's thread also writes the NEXT vector step's exploration
// noise, A elements per env — noise[i * A + c] = hash_normal(noise_seed, noise_ctr0 + i * A + c) (as double) * noise_scale, stored as
// float64 or rounded to float32
int env_step_launch_noise(gcrl_env_group* g, const void* actions_dev, int f64, void* noise, int noise_f64, unsigned long long noise_seed,
                          unsigned long long noise_ctr0, double noise_scale, hipStream_t st);

// ---- dev_env.hip's small launches
// proc_pack_kernel: raw | pay from separate contiguous [n][.] float32 device tensors (the payload's t word: t[i] from device words, or t0 for every
// env when t == null).  ag may be null (then that block and next_ag's are left as they are: no goal normaliser reads them).
struct ProcPack {
  const float *obs, *nobs, *dg, *ndg, *ag, *nag, *act, *rew;
  const int* t;      // [n] device words, or null: t0 for every env
  float* raw; float* pay;
  int n, D, G, A, t0;
};
int proc_pack_launch(const ProcPack& p, hipStream_t st);
// out[i] = clamp(hash_normal(seed, ctr0 + i), -1, 1) for i < n  (the epsilon step of a DDPG collect)
int clipped_normal_fill(float* out, int n, unsigned long long seed, unsigned long long ctr0, hipStream_t st);
// out[i] = double(hash_normal(seed, ctr0 + i)) * scale for i < n, stored as float64 (f64 != 0) or rounded to float32
int normal_fill(void* out, int f64, int n, unsigned long long seed, unsigned long long ctr0, double scale, hipStream_t st);
// out32[i] = float(in64[i]) for i < n
int round_to_f32(const double* in64, float* out32, int n, hipStream_t st);
// env_scripted_kernel (dev_env_script.hip) on `st` for a one-member group: the pick or glide kind's scripted controller, float32 actions [N][A] to out;
// noise_std > 0 adds float(double(hash_normal(seed, ctr0 + i * A + c)) * noise_std) before a final clamp to [-1, 1]
int env_scripted_launch(gcrl_env_group* g, float* out, double noise_std, unsigned long long seed, unsigned long long ctr0, hipStream_t st);

}  // namespace gcrl
