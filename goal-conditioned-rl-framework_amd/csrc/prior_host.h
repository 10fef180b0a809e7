// prior_host.h — the host-only arithmetic of prior-data replay (her_prior.hip): where the placement launch puts a
// scratch row, and the prior ring's counters of one update call.  No HIP in here apart from the function qualifier: the kernel and
// the engine include it, and tools/prior_host_check.cc compiles it with the host compiler under AddressSanitizer +
// UndefinedBehaviorSanitizer.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GCRL_PRIOR_HD __host__ __device__
#else
#define GCRL_PRIOR_HD
#endif

namespace gcrl {

// The batch matrices of an agent: batch slot j holds its B rows of ldx floats at x + j * slot_x, its rewards / done flags at
// r + j * slot_rd.  The prior ring's gather of batches [b0, b0 + nb) leaves nb * Bd contiguous scratch rows; scratch row t of that
// launch belongs to batch slot b0 + t / Bd, row (B - Bd) + t % Bd.
struct PriorPlace {
  int B, Bd;                     // 1 <= Bd <= B - 1
  int ldx;                       // row stride of sa / nsa / spa in floats, a multiple of 4
  long long slot_x, slot_rd;     // slot strides in floats (>= B * ldx, >= B)
};

GCRL_PRIOR_HD inline bool prior_rows_ok(int B, int Bd) { return Bd >= 1 && B >= 2 && Bd <= B - 1; }

// slot (relative to the launch's first) and row inside it of scratch row t
GCRL_PRIOR_HD inline void prior_slot_row(const PriorPlace& p, long long t, long long* slot, int* row) {
  const long long s = t / p.Bd;
  *slot = s;
  *row = (p.B - p.Bd) + (int)(t - s * p.Bd);
}
// float offsets of that row from the launch's first slot: in sa / nsa / spa, and in r / d
GCRL_PRIOR_HD inline long long prior_x_offset(const PriorPlace& p, long long t) {
  long long s; int row;
  prior_slot_row(p, t, &s, &row);
  return s * p.slot_x + (long long)row * p.ldx;
}
GCRL_PRIOR_HD inline long long prior_rd_offset(const PriorPlace& p, long long t) {
  long long s; int row;
  prior_slot_row(p, t, &s, &row);
  return s * p.slot_rd + row;
}

// The prior ring's counters of one update call of n batches, taken when the call is planned: batch j of the call is the ring's
// draw draw0 + j, its first row the relabel stream's row ctr0 + j * Bd.  A gather part of batches [b0, b0 + nb) — the head gather,
// the deferred rest — starts at prior_part(snap, b0): the parts of a call tile its n batches whatever the split.
struct PriorSnap {
  uint64_t draw0 = 0, ctr0 = 0;
  uint32_t len = 0;      // rows the ring held when the call was planned
  int Bd = 0;
};
struct PriorPart { uint64_t draw, ctr; long long rows; };

GCRL_PRIOR_HD inline PriorPart prior_part(const PriorSnap& s, int b0, int nb) {
  return PriorPart{s.draw0 + (uint64_t)b0, s.ctr0 + (uint64_t)b0 * (uint64_t)s.Bd, (long long)nb * s.Bd};
}
// what planning a call of n batches adds to the ring's batch-draw counter and to its relabel counter
GCRL_PRIOR_HD inline uint64_t prior_draws_of(int n) { return (uint64_t)n; }
GCRL_PRIOR_HD inline uint64_t prior_rows_of(int n, int Bd) { return (uint64_t)n * (uint64_t)Bd; }

}  // namespace gcrl
