// dw_adam.hip — the step's two all-row launches as ONE: every dW | db problem of a net (or of two nets: the overlapped DDPG
// step's critic and actor), the global-norm clip, Adam(W), Polyak, the [in][out] weight copies, the riding metrics and the
// control advance.  Protocol and reference lines: ops.h (DwAdamNetArgs).  The arithmetic is shared with the two-launch form
// (gemm_mfma.h gemm_batch_tile, adam_math.h), so the two forms give the same bits.
#include "dw_adam.h"

#include <algorithm>

#include "adam_math.h"
#include "meet.h"
#include "pop.h"

namespace gcrl {
namespace {

constexpr unsigned long long kSlotEmpty = ~0ull;
constexpr int kLeaderMinTiles = 64;
constexpr int kSc1 = 16;      // cache-policy bit of the raw buffer builtins on gfx94x / gfx950: written through to the memory side
constexpr int kImgLd = 20;    // row stride of a regular tile's LDS images: rows stay 16-byte aligned
static_assert(kFusedMaxLayers == 5, "DwNetHead::tile0 holds the first tiles of problems 1..4");   // a negative quiet NaN with every payload bit set: never a sum of squares

// development build (-DGCRL_OF_STAMPS, tools/of_stamps.sh): thread 0 of every workgroup leaves the constant-rate clock (100 MHz) at
// its section boundaries in a.stamps[(net * 2048 + workgroup) * 8 + k]
#ifdef GCRL_OF_STAMPS
#define OF_STAMP(k) of_t[k] = wall_clock64()
#else
#define OF_STAMP(k) do { } while (0)
#endif

// a uniform, read-only-in-this-launch record through the scalar cache (constant address space): one s_load for the whole record
template <class T>
__device__ __forceinline__ T load_uniform(const T* p) {
  static_assert(sizeof(T) % 4 == 0, "whole dwords");
  typedef const unsigned int __attribute__((address_space(4))) cu32;
  cu32* q = reinterpret_cast<cu32*>(reinterpret_cast<uintptr_t>(p));
  union { T v; unsigned int w[sizeof(T) / 4]; } u;
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; ++i) u.w[i] = q[i];
  return u.v;
}

// a pointer that went through pin() is an integer as far as the compiler knows, and what it then dereferences is a FLAT access
// (slower, and counted on the LDS wait counter too): the accesses below go through pointers TYPED as global memory
typedef float __attribute__((address_space(1))) gfloat;
typedef unsigned long long __attribute__((address_space(1))) gu64;
typedef unsigned int __attribute__((address_space(1))) gu32;

// between two polls of a norm slot or result word (s_sleep counts 64 clocks)
__device__ __forceinline__ void poll_pause() {
  __builtin_amdgcn_s_sleep(1);
  __builtin_amdgcn_s_sleep(1);
}

// a POD record copied HERE, every dword of it in a scalar register: the loads of its fields cannot sink to their uses (left to
// itself the compiler fetched every field where it was first needed: a dozen dependent scalar round trips in front of the GEMM)
template <class T>
__device__ __forceinline__ void pin(T& v) {
  static_assert(sizeof(T) % 4 == 0, "whole dwords");
  unsigned int* w = reinterpret_cast<unsigned int*>(&v);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; ++i) asm volatile("" : "+s"(w[i]));
}

// What the kernel is handed: the host-side DwAdamArgs (whole GemmDesc records, 232 bytes each, read field by field where they are
// used) made the kernel start with a dozen DEPENDENT scalar loads — 2.2 us before its first operand request, another microsecond
// inside the tile body.  Here a net is a 48-dword header and 24-dword problems: the header arrives with the first round trip, the
// workgroup's problem, the step's scalars and the launch count with the second.
struct DwProb {
  const float* G; const float* X; float* dW; float* db;   // dW[out][in] = G^T X (G: [K][ldg], X: [K][ldx]), db = column sums of G
  long long pw, pb, wt_dst;                               // DwAdamLayer
  int ldg, ldx, out, in, K, tiles_n, slot0, x_slot;      // x_slot != 0: X lives in the batch array, + batch_slot * x_slot floats
};
struct DwNetHead {   // 16 dwords: the first round trip
  int ntiles, nl, which, slot_stride;
  int tile0[4];      // first tile of problems 1..4 (INT_MAX beyond the net's problems; problem 0 starts at 0)
  const StepCtrl* cur; unsigned int* seq; unsigned long long* slots;
  int polyak, grid_x;   // grid_x: the launch's gridDim.x (from the dispatch packet it would be one more dependent scalar load)
};
struct DwNetPtrs {   // 14 dwords
  float *p, *m, *v, *target, *wt, *wt_target;
  float clip; int pad;
};
struct DwNetK {
  DwNetHead h;
  DwNetPtrs ptr;
  int metric_index, mean_n;
  const float* mean_x; float mean_scale; int mean_index;
  const float* td_q; const float* td_y; int td_n, td_C, td_loss_kind, pad;
  DwProb prob[kFusedMaxLayers];
};
struct DwAdamK {
  float beta2, w1, w2, eps, tau, one_m_tau;
  float* metrics; CtrlBlock* advance; unsigned int* status;
#ifdef GCRL_OF_STAMPS
  unsigned long long* stamps;
#endif
  DwNetK net[2];
};

__global__ __launch_bounds__(256, 5) void dw_adam_kernel(DwAdamK a) {
  const unsigned bx = blockIdx.x, by = blockIdx.y;
#include "dw_adam_body.inc"
}

// population form (agent.hip gcrl_pop_*): member blockIdx.z runs its own arguments tab[blockIdx.z]; its norm slots, launch count and
// control block are its own, so the members' workgroups never wait for each other
__global__ __launch_bounds__(256, 5) void dw_adam_pop_kernel(const DwAdamK* __restrict__ tab) {
  const DwAdamK& a = tab[blockIdx.z];
  const unsigned bx = blockIdx.x, by = blockIdx.y;
#include "dw_adam_body.inc"
}

}  // namespace

long long dw_adam_capacity() { return meet_capacity((const void*)dw_adam_kernel, 256, 0); }

int launch_dw_adam(hipStream_t st, DwAdamArgs& a) {
  GCRL_CHECK_ARG(a.nnets >= 1 && a.nnets <= 2, "dw_adam: %d nets (1 or 2)", a.nnets);
  DwAdamK k;
  std::memset(&k, 0, sizeof(k));
  k.beta2 = a.beta2; k.w1 = a.w1; k.w2 = a.w2; k.eps = a.eps; k.tau = a.tau; k.one_m_tau = a.one_m_tau;
  k.metrics = a.metrics; k.advance = a.advance; k.status = a.status;
#ifdef GCRL_OF_STAMPS
  k.stamps = a.stamps;
#endif
  int widest = 0;
  for (int i = 0; i < a.nnets; ++i) {
    DwAdamNet& n = a.net[i];
    DwNetK& kn = k.net[i];
    GCRL_CHECK_ARG(n.o.nl >= 1 && n.o.nl <= kFusedMaxLayers && n.o.slots && n.o.seq && n.o.cur, "dw_adam: net %d: %d problems / missing slots", i, n.o.nl);
    int tiles = 0;
    for (int l = 0; l < n.o.nl; ++l) {
      GemmDesc& d = n.d[l];
      GCRL_CHECK_ARG(d.M >= 1 && d.N >= 2 && d.K >= 1 && d.A && d.B && d.C && d.ones_col && d.col_out && !d.bias && d.epi == EPI_NONE && d.mul == MUL_NONE &&
                         !d.bn_part && d.ksplit <= 1 && d.shape_hint == 0 && gemm_shape_of(d) == 1,
                     "dw_adam: net %d problem %d is not a dW | db problem of the k-split 16x16 form", i, l);
      // ... in agent.hip bwd_dw's layout: A = G read k-major, B = X read k-major, C = dW [out][in]; a batch-slot lookup only on X,
      // through the control record this net's optimiser reads
      GCRL_CHECK_ARG(d.a_rs == 1 && d.b_cs == 1 && d.c_rs == d.N - 1 && d.a_cs < (1LL << 31) && d.b_rs < (1LL << 31) && d.a_slot == 0 && d.c_slot == 0 &&
                         (!d.slot || (d.slot == &n.o.cur->batch_slot && d.b_slot < (1LL << 31))),
                     "dw_adam: net %d problem %d is not laid out like a dW | db problem", i, l);
      DwProb& p = kn.prob[l];
      p.G = d.A; p.X = d.B; p.dW = d.C; p.db = d.col_out;
      p.pw = n.o.lay[l].pw; p.pb = n.o.lay[l].pb; p.wt_dst = n.o.lay[l].wt_dst;
      p.ldg = (int)d.a_cs; p.ldx = (int)d.b_rs; p.out = d.M; p.in = d.N - 1; p.K = d.K;
      p.tiles_n = (d.N + 15) / 16; p.slot0 = n.o.lay[l].slot0; p.x_slot = d.slot ? (int)d.b_slot : 0;
      if (l >= 1) kn.h.tile0[l - 1] = tiles;
      tiles += ((d.M + 15) / 16) * p.tiles_n;
    }
    n.o.ntiles = tiles;
    GCRL_CHECK_ARG(tiles <= 256 * kFusedMaxSlotsPerThread && tiles + 8 <= n.o.slot_stride, "dw_adam: net %d has %d tiles (slots: %d)", i, tiles, n.o.slot_stride);
    widest = std::max(widest, tiles);
    for (int l = n.o.nl; l < kFusedMaxLayers; ++l) kn.h.tile0[l - 1] = 0x7fffffff;
    kn.h.ntiles = tiles; kn.h.nl = n.o.nl; kn.h.which = n.o.which; kn.h.slot_stride = n.o.slot_stride;
    kn.h.cur = n.o.cur; kn.h.seq = n.o.seq; kn.h.slots = n.o.slots;
    kn.ptr.p = n.o.p; kn.ptr.m = n.o.m; kn.ptr.v = n.o.v; kn.ptr.target = n.o.target; kn.ptr.wt = n.o.wt; kn.ptr.wt_target = n.o.wt_target;
    kn.ptr.clip = n.o.clip; kn.h.polyak = n.o.polyak; kn.metric_index = n.o.metric_index;
    kn.mean_x = n.o.mean_x; kn.mean_n = n.o.mean_n; kn.mean_scale = n.o.mean_scale; kn.mean_index = n.o.mean_index;
    kn.td_q = n.o.td_q; kn.td_y = n.o.td_y; kn.td_n = n.o.td_n; kn.td_C = n.o.td_C; kn.td_loss_kind = n.o.td_loss_kind;
  }
  // (the residency of widest * nnets workgroups is the caller's admission check — dw_adam_capacity — made once per agent)
  for (int i = 0; i < a.nnets; ++i) k.net[i].h.grid_x = widest;
  if (PopRec* r = pop_recording())   // a population step is being recorded (pop.h)
    return pop_record(r, POP_DW_ADAM, 0, dim3((unsigned)widest, (unsigned)a.nnets), 0, &k, sizeof(k), [k, g = dim3((unsigned)widest, (unsigned)a.nnets)](hipStream_t s) -> int {
      hipLaunchKernelGGL(dw_adam_kernel, g, dim3(256), 0, s, k);
      GCRL_HIP(hipGetLastError());
      return GCRL_OK;
    });
  hipLaunchKernelGGL(dw_adam_kernel, dim3((unsigned)widest, (unsigned)a.nnets), dim3(256), 0, st, k);
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

long long dw_adam_pop_capacity() { return meet_capacity((const void*)dw_adam_pop_kernel, 256, 0); }

int launch_dw_adam_pop(hipStream_t st, const void* tab, int members, dim3 grid) {
  GCRL_CHECK_ARG(members >= 1 && members <= 65535 && grid.y >= 1 && grid.y <= 2 && grid.z == 1, "dw_adam population: bad launch");
  hipLaunchKernelGGL(dw_adam_pop_kernel, dim3(grid.x, grid.y, (unsigned)members), dim3(256), 0, st, static_cast<const DwAdamK*>(tab));
  GCRL_HIP(hipGetLastError());
  return GCRL_OK;
}

}  // namespace gcrl
