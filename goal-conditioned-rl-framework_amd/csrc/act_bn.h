// act_bn.h — one vector-env step of acting with the BatchNorm actor (SAC / TQC: SACActorModel in eval mode,
// src/model.py:118-141) as ONE launch: normalize_state_batch (src/agent.py:1435-1447) on the raw rows, L x [Linear ->
// BatchNorm1d(running statistics) -> ReLU], the mean and log-std heads, select_action's tanh of the mean (eval) or the
// tanh-Gaussian sample from the supplied eps, float64 actions out.  4 rows per workgroup, activations in LDS; the weights are read
// as stored, W[out][in] (the BatchNorm actor has no [in][out] copies and gets none).
#pragma once
#include <hip/hip_runtime.h>

#include "rowchain.h"   // kActInlineFloats / kActInlineNoise: the inline forms of every agent kind share their limits

namespace gcrl {

constexpr int kActBnThreads = 512, kActBnRows = 4;

struct ActBnArgs {
  const float* P;                       // the actor's live parameter vector (make_net's order: per hidden layer W, b, gamma, beta; then the two heads)
  const float* rmean; const float* rvar;   // running statistics [L][H]
  int S, H, L, A, n, D;                 // state_dim, hidden_dim, layer_count, action_dim, rows, observation columns of a row
  int ldl;                              // floats per LDS activation row (>= max(S, H), a multiple of 4)
  // normalisers (null: that part of the row stays raw) and their norm_math.h regime bits
  const double* nz_mean; const double* nz_var; double nz_clip;
  const double* nzg_mean; const double* nzg_var; double nzg_clip;
  int nz_mode, nzg_mode;
  int warm;                             // != 0: each pass touches the next pass's weight lines first (act_bn.hip warm_lines)
  // staged form: raw rows [n][S], eps [n][A] (null: the deterministic action), actions [n][A]
  const float* rows; const float* eps; double* out64;
};
int launch_act_bn(hipStream_t st, const ActBnArgs& a);

// rows and eps inside the kernel arguments, the float64 actions to host-visible memory followed by one flag per workgroup
// (flag_host[workgroup] = seq once that workgroup's rows are out).  n * S <= kActInlineFloats, n * A <= kActInlineNoise.
struct ActBnInline {
  ActBnArgs base;                       // rows / eps / out64 are ignored
  double* out_host;
  unsigned long long* flag_host;
  unsigned long long seq;
  int with_eps;
  float obs_inl[kActInlineFloats];
  double eps_inl[kActInlineNoise];      // the eps as the ABI carries it; used as (float)
};
int launch_act_bn_inline(hipStream_t st, const ActBnInline& a);

// Population forms (gcrl_pop_observe_act_bn): grid (ceil(n / kActBnRows), members), member = blockIdx.y.  Member m's workgroups read
// tab[m] (its own parameter vector, running statistics, normaliser views and the shared shapes; rows / eps / out64 there are ignored) and
// its slices of rows / eps / out: [members][stride_n][S] floats, [members][stride_n][A] doubles (the eps as the ABI carries it; used as
// (float)), [members][stride_n][A] doubles.  What changes from call to call travels in the kernel arguments, so the table stays the
// same call after call.  Fast form (flags != null): rows, eps, out and flags are the device addresses of a pinned, mapped, coherent
// block the host fills before the launch and polls after it (flags[m * workgroups + workgroup] = seq once that workgroup's rows are
// out); rows and eps are read by system-scope loads.  Staged form (flags == null): device buffers, plain loads and stores.
struct ActBnPop {
  const ActBnArgs* tab;
  const float* rows; const double* eps; double* out;
  unsigned long long* flags;
  unsigned long long seq;
  int with_eps, stride_n;
};
// `shape`: a host copy of one member's arguments, for the shape checks and the LDS size (the members share S, H, L, A, n, ldl)
int launch_act_bn_pop(hipStream_t st, const ActBnPop& c, const ActBnArgs& shape, int members);

}  // namespace gcrl
