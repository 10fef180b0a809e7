// pop.h — launch recording of a DDPG, TD3 or SAC population (agent.hip gcrl_pop_*).
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
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace gcrl {

enum PopKind {
  POP_ALONE = 0,       // no population form: each member's own launch, in member order
  POP_ROWCHAIN = 1,    // rowchain_ddpg_kernel<sub & 15, sub & 16> (rows per block / 4; + 16: the LDS-multiplier form; + 32: the stream form)
  POP_DW_ADAM = 2,     // dw_adam_kernel
  POP_BEGIN_STEP = 3,  // begin_step_kernel
  POP_GEMM_BATCH = 4,  // one form's launch of launch_gemm_batch (sub = the form, 1..5; only form 1, gemm_batch_kernel<1, 1, 4>, merges)
  POP_ADAM = 5,        // adam_kernel
  POP_ADAM_PAIR = 6,   // adam_pair_kernel (args: AdamPairArgs)
  // SAC (bn_slab.hip, rowchain.hip, ops_sac.hip): `sub` names the template instance, so only identical forms merge
  POP_BN_FWD = 7,          // bn_linear_fwd_slab_kernel<VEC, NT, WV> (sub = VEC | form << 1 | inputs << 4; form 0: <4, 8>, 1: <1, 4>, 2: <1, 8>)
  POP_BN_BWD = 8,          // bn_linear_bwd_slab_kernel<NT, WV> (sub = form, as above)
  POP_BN_BWD_FOLD = 9,     // bn_linear_bwd_slab_fold_kernel<WV> (sub = WV)
  POP_RC_SPLIT = 10,       // rowchain_split_kernel<RG> (sub = RG | part << 4 | phase << 8; args: RowChainArgs, phase, part)
  POP_RC_SPLIT_HEADS = 11, // rowchain_split_heads_kernel<RG> (sub as above; args: RowChainArgs, phase, part, HeadsFold)
  POP_TG_BWD_SELECT = 12,  // tanh_gauss_bwd_select_kernel (args: TanhGaussBwdArgs, ActorSelArgs, AlphaArgs)
  // TQC on the layer-per-launch schedule (ops_sac.hip)
  POP_TG_FWD = 13,         // tanh_gauss_fwd_kernel (sub = 1; args: TanhGaussArgs) / tanh_gauss_fwd2_kernel (sub = 2; args: two of them)
  POP_TG_BWD = 14,         // tanh_gauss_bwd_kernel (args: TanhGaussBwdArgs)
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

// Device copies of the argument tables of the population ACTING launches (gcrl_pop_observe_act, gcrl_pop_process_step), by content.
// A table repeats call after call (it holds what belongs to the members, not to the call), so the usual call is one memcmp with the
// table of the call before.  A table is never rewritten: a launch still in flight may be reading it.
struct PopTabCache {
  std::map<std::string, void*> tabs;
  const std::string* last = nullptr;
  void* last_dev = nullptr;
  int get(const void* bytes, size_t n, hipStream_t st, void** out) {
    if (last && last->size() == n && std::memcmp(last->data(), bytes, n) == 0) { *out = last_dev; return 0; }
    std::string key((const char*)bytes, n);
    auto it = tabs.find(key);
    if (it == tabs.end()) {
      if (tabs.size() >= 64) {   // (a bound: regimes and modes give a handful of tables)
        if (hipStreamSynchronize(st) != hipSuccess) return -2;
        release();
      }
      void* d = nullptr;
      if (hipMalloc(&d, n) != hipSuccess) return -2;
      if (hipMemcpy(d, bytes, n, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return -2; }
      it = tabs.emplace(std::move(key), d).first;
    }
    last = &it->first; last_dev = it->second;
    *out = last_dev;
    return 0;
  }
  void release() {
    for (auto& kv : tabs) (void)hipFree(kv.second);
    tabs.clear();
    last = nullptr; last_dev = nullptr;
  }
};

// population launches: `tab` is a device array of `members` argument structs
int launch_rowchain_ddpg_pop(hipStream_t st, const void* tab, int members, int sub, dim3 grid, size_t lds);
int launch_dw_adam_pop(hipStream_t st, const void* tab, int members, dim3 grid);
int launch_begin_step_pop(hipStream_t st, const void* tab, int members);
int launch_gemm_batch_pop(hipStream_t st, const void* tab, int members, int shape, dim3 grid);
int launch_adam_pop(hipStream_t st, const void* tab, int members, dim3 grid);
int launch_adam_pair_pop(hipStream_t st, const void* tab, int members, dim3 grid);
// SAC: member = blockIdx.z (slab launches; the row-split forward, whose grid uses all three dimensions, takes member * inputs + input there) or
// blockIdx.y (chain launches, sampling backward)
int launch_bn_fwd_slab_pop(hipStream_t st, const void* tab, int members, int sub, dim3 grid);
int launch_bn_bwd_slab_pop(hipStream_t st, const void* tab, int members, int sub, dim3 grid);
int launch_bn_bwd_slab_fold_pop(hipStream_t st, const void* tab, int members, int sub, dim3 grid);
int launch_rowchain_split_pop(hipStream_t st, const void* tab, int members, int sub, bool heads, dim3 grid, size_t lds);
int launch_tanh_gauss_bwd_select_pop(hipStream_t st, const void* tab, int members, dim3 grid);
// TQC: member = blockIdx.y (the two-input sampling forward, whose grid uses blockIdx.y for the input: blockIdx.z)
int launch_tanh_gauss_fwd_pop(hipStream_t st, const void* tab, int members, int sub, dim3 grid);
int launch_tanh_gauss_bwd_pop(hipStream_t st, const void* tab, int members, dim3 grid);
// gcrl_pop_clone (pop_clone.hip): `tab` is a device array of `segments` CloneSeg (pbt_host.h); grid (chunks, segments)
int launch_pop_clone(hipStream_t st, const void* tab, int segments, unsigned chunks);
// admission of the waiting forms for a population of `members`: the two sides of the comparison (cap 0: shared device or the query failed)
// (*want: `members` times a member's workgroups of the form; *cap: what is resident at once; want 0: the shape does not have the form)
void bn_slab_pop_row_split_terms(int B, int H, int A, int members, long long* want, long long* cap);
void rowchain_pop_merge_terms(int rg, int ldl, int A, int H, int C, int B, int members, long long* want, long long* cap);
long long dw_adam_pop_capacity();   // workgroups of the population form resident at once (0: shared device / query failed)

}  // namespace gcrl
