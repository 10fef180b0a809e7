// per_host.h — the host-only arithmetic of the device-resident prioritised replay (per_tree.hip): level sizes of the priority
// tree, slot <-> logical index mapping, and the slot ranges that pushes since the last refresh cover.  No HIP in here: the
// stand-alone program tools/per_host_check.cc runs it under AddressSanitizer + UBSan (make -C csrc per_asan).
//
// Tree layout.  Level 0 = the leaves: one fp32 priority per PHYSICAL ring slot, padded with zeros to a multiple of 64.  Level
// k + 1 holds one fp32 sum per 64 entries of level k, again padded with zeros to a multiple of 64; the levels end with the first
// one of at most 64 entries (the top block).  All levels live in one allocation, level k at float offset off[k].
// 1e6 slots: 1 000 000 -> 15 625 (padded 15 680) -> 245 (padded 256) -> 4 (padded 64).
#pragma once
#include <cstdint>

namespace gcrl {

constexpr int kPerFan = 64;         // children per node = lanes per wave
constexpr int kPerMaxLevels = 8;    // 64^8 slots: more than any ring

inline int64_t per_round64(int64_t n) { return (n + kPerFan - 1) / kPerFan * kPerFan; }

struct PerLayout {
  int levels = 0;                        // number of levels, leaves included (>= 1)
  int64_t used[kPerMaxLevels] = {};      // meaningful entries of level k (level 0: the ring's capacity)
  int64_t padded[kPerMaxLevels] = {};    // entries allocated for level k: a multiple of 64
  int64_t off[kPerMaxLevels] = {};       // float offset of level k in the allocation
  int64_t total = 0;                     // floats in the allocation
};

// false: capacity < 1 or too large for kPerMaxLevels levels
inline bool per_layout(int64_t capacity, PerLayout* L) {
  *L = PerLayout{};
  if (capacity < 1) return false;
  int64_t used = capacity, off = 0;
  for (int k = 0; k < kPerMaxLevels; ++k) {
    L->used[k] = used;
    L->padded[k] = per_round64(used);
    L->off[k] = off;
    off += L->padded[k];
    L->levels = k + 1;
    if (L->padded[k] <= kPerFan) { L->total = off; return true; }
    used = L->padded[k] / kPerFan;
  }
  *L = PerLayout{};
  return false;
}

// logical index j (0 = oldest row) <-> physical slot, as the replay ring maps them (her_ring.h)
inline int64_t per_slot_of(int64_t logical, int64_t head, int64_t cap) { return (head + logical) % cap; }
inline int64_t per_logical_of(int64_t slot, int64_t head, int64_t cap) { return (slot - head + cap) % cap; }

// The slots of the last `pending` pushed rows of a ring with `head`, `len`, capacity `cap`: a contiguous range ending at the
// ring's tail, as at most two half-open segments [a0, a1) and [b0, b1) (the second one empty unless the range wraps).
// pending > cap is treated as cap (every slot was overwritten).
struct PerSegs { int64_t a0 = 0, a1 = 0, b0 = 0, b1 = 0; };
inline PerSegs per_pending_segments(int64_t head, int64_t len, int64_t cap, int64_t pending) {
  PerSegs s;
  if (pending <= 0 || len <= 0 || cap <= 0) return s;
  if (pending > len) pending = len;   // (len <= cap: rows pushed and already evicted again leave nothing to refresh)
  const int64_t tail = (head + len) % cap;          // slot the NEXT push writes
  const int64_t first = (tail - pending + cap) % cap;
  if (first + pending <= cap) { s.a0 = first; s.a1 = first + pending; }
  else { s.a0 = first; s.a1 = cap; s.b0 = 0; s.b1 = first + pending - cap; }
  return s;
}

// the nodes of the level above that cover the entries [x0, x1) of a level (empty stays empty)
inline void per_parent_range(int64_t x0, int64_t x1, int64_t* p0, int64_t* p1) {
  if (x1 <= x0) { *p0 = *p1 = 0; return; }
  *p0 = x0 / kPerFan;
  *p1 = (x1 - 1) / kPerFan + 1;
}

}  // namespace gcrl
