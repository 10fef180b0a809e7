// pbt_host.h — host side of the population's in-place clone / re-tune / replace entries (include/gcrl.h gcrl_pop_clone,
// gcrl_agent_set_hparams, gcrl_pop_replace): argument checks and the segment table of pop_clone_kernel.  No HIP in this file: the same
// code is compiled by the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer (tools/pbt_host_check.cc).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/gcrl.h"

namespace gcrl {

constexpr int kMaxClonePairs = 16;

// one copy of pop_clone_kernel: `bytes` from src to dst (device addresses; a segment never overlaps another one's destination)
struct CloneSeg {
  const void* src;
  void* dst;
  unsigned long long bytes;
};

// gcrl_pop_clone's arguments; on refusal the message (naming the argument) is left in `why` and false is returned
inline bool pop_clone_check(int members, const int32_t* src, const int32_t* dst, int32_t pairs, uint32_t what, char* why, size_t n) {
  if (!src) { std::snprintf(why, n, "src: null array"); return false; }
  if (!dst) { std::snprintf(why, n, "dst: null array"); return false; }
  if (pairs < 1 || pairs > kMaxClonePairs) { std::snprintf(why, n, "pairs: %d pairs in one call (1..%d)", pairs, kMaxClonePairs); return false; }
  if (what == 0 || (what & ~(uint32_t)(GCRL_CLONE_AGENT | GCRL_CLONE_RING)) != 0) {
    std::snprintf(why, n, "what: mask 0x%x (bits: GCRL_CLONE_AGENT 1, GCRL_CLONE_RING 2; at least one)", what);
    return false;
  }
  uint32_t is_src = 0, is_dst = 0;
  for (int k = 0; k < pairs; ++k) {
    if (src[k] < 0 || src[k] >= members) { std::snprintf(why, n, "src: pair %d names member %d of %d", k, src[k], members); return false; }
    if (dst[k] < 0 || dst[k] >= members) { std::snprintf(why, n, "dst: pair %d names member %d of %d", k, dst[k], members); return false; }
  }
  for (int k = 0; k < pairs; ++k) {
    if ((is_dst >> dst[k]) & 1u) { std::snprintf(why, n, "dst: member %d is a destination twice", dst[k]); return false; }
    is_dst |= 1u << dst[k];
    is_src |= 1u << src[k];
  }
  if (is_src & is_dst) {
    int m = 0;
    while (!(((is_src & is_dst) >> m) & 1u)) ++m;
    std::snprintf(why, n, "dst: member %d is both a source and a destination in one call", m);
    return false;
  }
  return true;
}

inline void clone_add(std::vector<CloneSeg>& t, const void* src, void* dst, unsigned long long bytes) {
  if (bytes) t.push_back(CloneSeg{src, dst, bytes});
}

// a ring's rows in logical (oldest-first) order into the destination from physical row 0 on — what gcrl_her_save_state followed by
// gcrl_her_load_state leaves (head 0): at most two segments, only the filled part
inline void clone_add_ring_rows(std::vector<CloneSeg>& t, const float* src_ring, float* dst_ring, long long head, long long len, long long capacity,
                                int row_floats) {
  const long long first = len < capacity - head ? len : capacity - head;
  const unsigned long long row = (unsigned long long)row_floats * sizeof(float);
  clone_add(t, src_ring + head * row_floats, dst_ring, (unsigned long long)first * row);
  if (len > first) clone_add(t, src_ring, dst_ring + first * row_floats, (unsigned long long)(len - first) * row);
}

// chunks of 16 KiB per segment along grid.x (every workgroup strides over its segment, so any count is correct), at most `cap`
inline unsigned clone_chunks(const std::vector<CloneSeg>& t, unsigned cap) {
  unsigned long long most = 0;
  for (const CloneSeg& s : t) most = s.bytes > most ? s.bytes : most;
  const unsigned long long want = (most + 16383) / 16384;
  return (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
}

// the fields gcrl_agent_set_hparams changes.  The creating entries validate none of them, so only what cannot be stepped with is refused:
// a value that is not a number, a learning rate that is not finite and > 0, a negative minimum, a scheduler length < 1 (gamma, tau and
// grad_clip are taken as a constructor takes them; grad_clip < 0 means no clipping)
inline bool hparams_check(const gcrl_hparams* h, bool sac, char* why, size_t n) {
  if (!h) { std::snprintf(why, n, "h: null hyper-parameters"); return false; }
  struct { const char* name; double v, min_v; } rates[] = {{"actor_lr", h->actor_lr, h->actor_lr_min}, {"critic_lr", h->critic_lr, h->critic_lr_min}};
  for (auto& r : rates) {
    if (!std::isfinite(r.v) || r.v <= 0.0) { std::snprintf(why, n, "%s: %g (a learning rate is finite and > 0)", r.name, r.v); return false; }
    if (!std::isfinite(r.min_v) || r.min_v < 0.0) { std::snprintf(why, n, "%s_min: %g (a minimum rate is finite and >= 0)", r.name, r.min_v); return false; }
  }
  if (h->ac_scheduler_steps < 1) { std::snprintf(why, n, "ac_scheduler_steps: %lld (>= 1)", (long long)h->ac_scheduler_steps); return false; }
  if (h->cr_scheduler_steps < 1) { std::snprintf(why, n, "cr_scheduler_steps: %lld (>= 1)", (long long)h->cr_scheduler_steps); return false; }
  if (std::isnan(h->gamma)) { std::snprintf(why, n, "gamma: not a number"); return false; }
  if (std::isnan(h->tau)) { std::snprintf(why, n, "tau: not a number"); return false; }
  if (std::isnan(h->grad_clip)) { std::snprintf(why, n, "grad_clip: not a number"); return false; }
  if (sac) {
    if (!std::isfinite(h->alpha_lr) || h->alpha_lr <= 0.0) { std::snprintf(why, n, "alpha_lr: %g (a learning rate is finite and > 0)", h->alpha_lr); return false; }
    if (std::isnan(h->alpha_min_steps)) { std::snprintf(why, n, "alpha_min_steps: not a number"); return false; }
  }
  return true;
}

// first field in which two members' configurations may not differ (nullptr: none) — what every population entry compares
inline const char* pop_mismatch(const gcrl_agent_config& a, const gcrl_agent_config& b) {
#define GCRL_POP_SAME(f) if (a.f != b.f) return #f;
  GCRL_POP_SAME(kind) GCRL_POP_SAME(obs_dim) GCRL_POP_SAME(ac_dim) GCRL_POP_SAME(hidden_dim) GCRL_POP_SAME(layer_count)
  GCRL_POP_SAME(batch_size) GCRL_POP_SAME(num_critics) GCRL_POP_SAME(gradient_step) GCRL_POP_SAME(ac_update_freq)
  GCRL_POP_SAME(polyak_every) GCRL_POP_SAME(pipeline_steps) GCRL_POP_SAME(use_graph) GCRL_POP_SAME(device) GCRL_POP_SAME(n_quantiles)
#undef GCRL_POP_SAME
  return nullptr;
}

// the re-tunable fields of a configuration, as gcrl_agent_set_hparams takes them
inline gcrl_hparams hparams_of(const gcrl_agent_config& c) {
  return gcrl_hparams{c.actor_lr, c.actor_lr_min, c.critic_lr, c.critic_lr_min, c.ac_scheduler_steps, c.cr_scheduler_steps,
                      c.gamma, c.tau, c.grad_clip, c.alpha_lr, c.alpha_min_steps};
}

// the rate a cosine schedule (lr_sched.cc, recursive form) holds after `t` scheduler steps from `base`: what an agent constructed with
// this schedule has in its optimiser after t steps, bit for bit (the recursion is replayed, not its closed form)
inline double cosine_lr_at(double base, double eta_min, int64_t t_max, int64_t t) {
  double lr = base;
  for (int64_t e = 1; e <= t; ++e) lr = gcrl_cosine_lr_next(lr, base, eta_min, t_max, e);
  return lr;
}

}  // namespace gcrl
