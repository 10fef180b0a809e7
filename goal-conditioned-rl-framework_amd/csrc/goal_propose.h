// goal_propose.h — practice goals: the handle of goal_propose.hip and what the collect loop (agent.hip) takes of it.
// The rule is restated in numpy in tests/goal_propose_ref.py, which is its definition.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_env.h"

constexpr int kGoalMaxCap = 65536;       // archive entries
constexpr int kGoalMaxCand = 64;         // candidates per proposal
constexpr int kGoalTile = 1024;          // archive slots goal_propose_kernel stages per pass (a multiple of 4: a tile starts on 16 bytes)

struct gcrl_goal_proposer {
  // settings
  int cap = 0, C = 0, min_fill = 0, device = 0;
  float radius = 0.f, share = 0.f;
  uint64_t seed = 0;
  // the binding: one env handle (its token; null after a load into a fresh handle, until the first use) of N envs
  const void* env_token = nullptr;
  int N = 0;
  int64_t seen_vsteps = -1;              // the env's step count at this handle's last step: a step is consumed once
  // the archive: [cap][3] float32 at physical slots, logical index j at slot (head + j) mod cap
  float* archive = nullptr;              // cap * 3 floats, rounded up to 16 bytes, plus 16
  int head = 0, len = 0;
  uint64_t q = 0;                        // roll-over steps seen
  int64_t appended = 0, roll_steps = 0, patched = 0;
};

namespace gcrl {

// whether p may serve env, naming the field that forbids it (gcrl.h's table); consumes nothing
int goal_proposer_bind_check(const gcrl_goal_proposer* p, const gcrl_env_group* env, const char* who);
// the same, and that the env has stepped since p's last step (GCRL_ERR_STATE naming `env` otherwise)
int goal_proposer_check(const gcrl_goal_proposer* p, const gcrl_env_group* env, const char* who);
// the env's last step into p on st: the append launch and, when an env rolled over and the archive holds min_fill entries, the
// propose launch.  *launches grows by what was issued.  No copy, no synchronisation.  The caller has run one of the checks above.
int goal_proposer_step_launch(gcrl_goal_proposer* p, gcrl_env_group* env, hipStream_t st, long long* launches);

}  // namespace gcrl
