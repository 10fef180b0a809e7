// per_tree.h — device-resident prioritised replay on a replay ring (per_tree.hip): the priority tree in HBM and the entries
// the update engine calls between its gather and its step.  Layout and host arithmetic: per_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/gcrl.h"
#include "per_host.h"

struct gcrl_her;

struct gcrl_per_tree {
  gcrl::PerLayout L;
  float* tree = nullptr;        // all levels, L.total floats
  float alpha = 0.6f, eps = 1e-6f;
  uint64_t draws = 0;           // draw counter: draw number of the next batch
  uint64_t synced_rows = 0;     // the ring's rows_pushed as of the last refresh
  bool stale = false;           // the ring was reloaded: the leaves belong to another physical order until set_priorities
  float* p_drawn = nullptr;     // [p_cap] leaf priorities of the last draw
  int p_cap = 0;
  std::vector<float> betas;     // per-step beta values queued for the engine's next steps (gcrl_per_set_betas)
  size_t beta_pos = 0;
  int64_t launches = 0;         // kernel launches issued by this tree
  int source = 0;               // gcrl::kPerSourceTd (leaves = (|td| + eps)^alpha, fed back by the update engine) or kPerSourceEnergy
  gcrl_energy_config energy{};  // kPerSourceEnergy (her_prio.hip): leaves written once, by the ring's flush
  uint64_t prio_ctr = 0;        // kPerSourceEnergy: rows ever drawn (the draw stream's counter)
  bool her_td = false;          // kPerSourceTd on a sample-mode HER ring (her_td.hip): new rows enter at p_max, seeded by the flush
  float* p_max = nullptr;       // her_td: ONE fp32 word on the device, the largest finite priority an update has written (initially 1.0f)
};

namespace gcrl {

constexpr uint64_t kPerKey = 0x5045525f54524545ull;   // "PER_TREE": key of the draw's uniform stream

constexpr int kPerSourceTd = 0, kPerSourceEnergy = 1;
inline bool per_is_td(const gcrl_per_tree* t) { return t && t->source == kPerSourceTd; }
inline bool per_is_energy(const gcrl_per_tree* t) { return t && t->source == kPerSourceEnergy; }
inline bool per_is_her_td(const gcrl_per_tree* t) { return per_is_td(t) && t->her_td; }   // a TD tree all the same: per_is_td routes it

void per_release(gcrl_her* h);
// a zeroed tree for the ring's capacity, not yet attached (*out; freed by the caller on a later failure: per_tree_free)
int per_tree_alloc(gcrl_her* h, const char* who, gcrl_per_tree** out);
void per_tree_free(gcrl_per_tree* t);
// every level above the leaves recomputed, one launch per level
int per_rebuild(gcrl_per_tree* t, hipStream_t st);
// priority 1.0 for the rows pushed since the last refresh, their ancestors recomputed: at most one launch up to kPerRefreshOne
// pending rows (beyond that: one fill launch and a rebuild)
int per_refresh(gcrl_her* h, hipStream_t st);
// refresh, then B proportional draws -> idx_dev[B] (logical indices), then their importance-sampling weights -> w_dev[B]
int per_draw(gcrl_her* h, int B, float beta, uint32_t* idx_dev, float* w_dev, hipStream_t st);
// leaves of idx_dev[B] <- (|td| + eps)^alpha, last occurrence wins, ancestors recomputed; hist_dev (may be null) <- td
int per_update(gcrl_her* h, const uint32_t* idx_dev, const float* td_dev, int B, float* hist_dev, hipStream_t st);
// her_td.hip: per_update's launch for the TD tree of a sample-mode HER ring (her_td == true), which also raises p_max
int her_td_update(gcrl_her* h, const uint32_t* idx_dev, const float* td_dev, int B, float* hist_dev, hipStream_t st);
// next queued beta of the engine's steps; false: none queued
bool per_next_beta(gcrl_her* h, float* beta);

}  // namespace gcrl
