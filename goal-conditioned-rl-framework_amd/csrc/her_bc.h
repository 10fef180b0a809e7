// her_bc.h — Q-filtered behaviour cloning on the prior-data rows of a batch (bc_weight / q_filter).
#pragma once
#include <hip/hip_runtime.h>

#include "ops.h"

namespace gcrl {

// One actor step's behaviour-cloning term on rows [B - Bd, B) of the step's batch slot (tests/her_bc_ref.py is the definition).
struct BcArgs {
  const StepCtrl* cur;      // batch slot and metrics slot of the step
  const float* spa;         // [slots][B][ldx]: pi(s) in columns [col0, col0 + A)
  const float* sa;          // [slots][B][ldx]: the stored action in the same columns
  long long slot_x;         // floats per batch slot
  int ldx, col0;
  const float* q_pi;        // [B] Q0(s, pi(s))
  const float* q_a;         // [B] Q0(s, a), rows [B - Bd, B) valid; null: no filter, every demonstration row is accepted
  float* dact;              // [B][ld_dact] gradient w.r.t. the pre-tanh action; accepted rows' first A columns are added to
  int ld_dact;
  float* mask;              // [B]: rows [B - Bd, B) written (1 accepted, 0 rejected); null: not kept
  float* metrics;           // records of kMetricFloats floats; words MET_BC_LOSS and MET_BC_PASS of the step's record written
  int B, Bd, A;
  float c;                  // fp32((2 * bc_weight) / Bd)
  float w_bd;               // fp32(bc_weight / Bd)
};

constexpr int kBcThreads = 256;
bool bc_args_ok(const BcArgs& a);
int launch_bc_qfilter(hipStream_t st, const BcArgs& a);

}  // namespace gcrl
