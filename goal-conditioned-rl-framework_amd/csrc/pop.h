// pop.h — launch recording of a DDPG or TD3 population (agent.hip gcrl_pop_*).
//
// A population step issues each member's ordinary launch sequence with a recorder installed on the calling thread: the
// launchers below then record the launch (its arguments, grid, LDS and a closure that would issue it alone) instead of
// issuing it.  The population issues position k of all members' sequences together: as ONE launch of the kernel's
// population form when every member recorded that kernel with the same grid (member blockIdx.y / blockIdx.z reads its own
// arguments from a device table), otherwise as the members' own launches in member order.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

namespace gcrl {

enum PopKind {
  POP_ALONE = 0,       // no population form: each member's own launch, in member order
  POP_ROWCHAIN = 1,    // rowchain_ddpg_kernel<sub> (sub = rows per block / 4)
  POP_DW_ADAM = 2,     // dw_adam_kernel
  POP_BEGIN_STEP = 3,  // begin_step_kernel
  POP_GEMM_BATCH = 4,  // one form's launch of launch_gemm_batch (sub = the form, 1..5; only form 1, gemm_batch_kernel<1, 1, 4>, merges)
  POP_ADAM = 5,        // adam_kernel
  POP_ADAM_PAIR = 6,   // adam_pair_kernel (args: AdamPairArgs)
};
// whether a recorded launch of this kind and sub has a population form
inline bool pop_mergeable(int kind, int sub) { return kind != POP_ALONE && (kind != POP_GEMM_BATCH || sub == 1); }

struct PopOp {
  int kind = POP_ALONE;
  int sub = 0;
  dim3 grid;
  size_t lds = 0;
  std::vector<char> args;                    // the kernel's argument struct, as the single-agent launch would pass it
  std::function<int(hipStream_t)> issue;     // the single-agent launch
};

struct PopRec {
  std::vector<PopOp> ops;
};

// the calling thread's recorder (nullptr: launchers launch)
PopRec*& pop_rec();
// recorders installed in the process: the launchers' fast path is one relaxed load of this count (no thread-local lookup)
extern std::atomic<int> g_pop_recorders;
inline PopRec* pop_recording() { return g_pop_recorders.load(std::memory_order_relaxed) ? pop_rec() : nullptr; }

inline int pop_record(PopRec* r, int kind, int sub, dim3 grid, size_t lds, const void* args, size_t bytes,
                      std::function<int(hipStream_t)> issue) {
  PopOp op;
  op.kind = kind; op.sub = sub; op.grid = grid; op.lds = lds;
  if (bytes) { op.args.resize(bytes); std::memcpy(op.args.data(), args, bytes); }
  op.issue = std::move(issue);
  r->ops.push_back(std::move(op));
  return 0;
}
inline int pop_defer(PopRec* r, std::function<int(hipStream_t)> issue) {
  return pop_record(r, POP_ALONE, 0, dim3(1), 0, nullptr, 0, std::move(issue));
}

// population launches: `tab` is a device array of `members` argument structs
int launch_rowchain_ddpg_pop(hipStream_t st, const void* tab, int members, int rg, dim3 grid, size_t lds);
int launch_dw_adam_pop(hipStream_t st, const void* tab, int members, dim3 grid);
int launch_begin_step_pop(hipStream_t st, const void* tab, int members);
int launch_gemm_batch_pop(hipStream_t st, const void* tab, int members, int shape, dim3 grid);
int launch_adam_pop(hipStream_t st, const void* tab, int members, dim3 grid);
int launch_adam_pair_pop(hipStream_t st, const void* tab, int members, dim3 grid);
long long dw_adam_pop_capacity();   // workgroups of the population form resident at once (0: shared device / query failed)

}  // namespace gcrl
