// norm_math.h — the arithmetic of the reference's RunningNormalizer (src/utils.py:68-117), shared by every kernel that
// updates or applies one (normalizer.hip, the fused process_step of her_ring.hip, the row-chain act prologue).
//
// numpy's type rules decide the arithmetic, so two things select it (`mode` bits):
//   NORM_F32     the STATISTICS are float32 arrays: a normaliser that was LOADED (load(): np.array(..., dtype=np.float32),
//                :113-114); a created one keeps float64 mean / var (np.zeros / np.ones);
//   NORM_ROWS64  the ROWS the trainer passes are float64 arrays.  They are for observations: the vector env allocates its
//                batches with the observation space's dtype, which TimeFeatureWrapper declares float64 (src/utils.py:156),
//                while the goal spaces stay float32.  (The values are float32-valued either way — panda-gym produces float32
//                — so float32 rows carry them exactly across the ABI.)
// float32 rows (round 2-3, goldens normalizer.npz / normalizer_loaded.npz): batch moments in float32 (numpy's axis-0 sums:
//   sequential for two features or more, pairwise for a one-feature normaliser — see norm_pairwise_sum below); a created normaliser merges and normalises in float64, a loaded one does EVERYTHING in float32 from then on (Python
//   scalars are weak; only the count stays a double).
// float64 rows (round 4, golden normalizer_f64.npz): batch moments and the merge in float64 whatever the statistics' type — only
//   `self.var * self.count` of a loaded normaliser is still a float32 product — so the first update after a load puts the
//   statistics back into float64 (the float32 regime must not be sticky there); normalize subtracts and divides in
//   float64, with the divisor sqrt(var) + 1e-8 a float32 value while the statistics are float32.
// The statistics are stored as doubles either way (float32 values are exact in them).
#pragma once
#include <hip/hip_runtime.h>

namespace gcrl {

enum { NORM_F32 = 1, NORM_ROWS64 = 2 };

// _update_from_moments (:83-93) for one feature: (m, v) <- merge with a batch of `rows` rows whose float32 moments are bm, bv;
// c0 = the count before this batch
__device__ inline void norm_merge(double& m, double& v, float bm, float bv, int rows, double c0, bool f32) {
  const double total = c0 + (double)rows;                       // total_count = self.count + count   (Python floats)
  if (!f32) {
    const double cb = (double)rows;
    const double delta = (double)bm - m;
    const double nm = m + delta * cb / total;                   // (delta * count) / total_count
    // `var * count`: a float32 array times a Python int stays float32 in numpy
    const double M2 = v * c0 + (double)__fmul_rn(bv, (float)rows) + delta * delta * c0 * cb / total;
    m = nm; v = M2 / total;
  } else {
    const float mf = (float)m, vf = (float)v, c0f = (float)c0, cbf = (float)rows, tf = (float)total;
    const float delta = __fsub_rn(bm, mf);
    const float nm = __fadd_rn(mf, __fdiv_rn(__fmul_rn(delta, cbf), tf));
    const float m_a = __fmul_rn(vf, c0f), m_b = __fmul_rn(bv, cbf);
    const float term = __fdiv_rn(__fmul_rn(__fmul_rn(__fmul_rn(delta, delta), c0f), cbf), tf);   // ((square(delta) * self.count) * count) / total_count
    const float M2 = __fadd_rn(__fadd_rn(m_a, m_b), term);
    m = (double)nm; v = (double)__fdiv_rn(M2, tf);
  }
}
// the same with float64 batch moments (float64 rows): everything in float64 except a float32 `self.var * self.count`
__device__ inline void norm_merge64(double& m, double& v, double bm, double bv, int rows, double c0, bool f32) {
  const double total = c0 + (double)rows, cb = (double)rows;
  const double delta = bm - m;
  const double nm = m + delta * cb / total;
  const double m_a = f32 ? (double)__fmul_rn((float)v, (float)c0) : v * c0;
  const double M2 = m_a + bv * cb + delta * delta * c0 * cb / total;
  m = nm; v = M2 / total;
}

// ---- the order of the batch sums.  np.mean / np.var reduce axis 0 of an (n, D) array.  For D >= 2 the reduction's inner loop runs
// ACROSS the features and every feature's sum is sequential in the rows.  A ONE-feature array is different: numpy coalesces the
// contiguous (n, 1) array into one inner reduce of n elements, and that loop is its pairwise sum (tests/numpy_pairwise_ref.py
// restates it and pins it against numpy):
//   n < 8     sequential;
//   n <= 128  eight running sums r[k] over the elements k, k + 8, k + 16, .. of the first n - n % 8, combined as
//             ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 tail elements added one by one;
//   n > 128   sum(first n2) + sum(rest), n2 = n / 2 rounded down to a multiple of 8, each half by the same rule;
//   n > 8192  chunks of 8192 elements, each by the rule above, added to the result one after another.
// Both the sum of the rows and the sum of the squared deviations take that order, for float32 and for float64 rows.
__device__ inline float norm_add(float a, float b) { return __fadd_rn(a, b); }
__device__ inline double norm_add(double a, double b) { return __dadd_rn(a, b); }

// one leaf of the rule above: elements [off, off + n), n <= 128
template <typename T, typename Term>
__device__ inline T norm_pairwise_block(int off, int n, Term t) {
  if (n < 8) {
    T res = (T)0;
    for (int i = 0; i < n; ++i) res = norm_add(res, t(off + i));
    return res;
  }
  T r0 = t(off), r1 = t(off + 1), r2 = t(off + 2), r3 = t(off + 3), r4 = t(off + 4), r5 = t(off + 5), r6 = t(off + 6), r7 = t(off + 7);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 = norm_add(r0, t(off + i));     r1 = norm_add(r1, t(off + i + 1)); r2 = norm_add(r2, t(off + i + 2)); r3 = norm_add(r3, t(off + i + 3));
    r4 = norm_add(r4, t(off + i + 4)); r5 = norm_add(r5, t(off + i + 5)); r6 = norm_add(r6, t(off + i + 6)); r7 = norm_add(r7, t(off + i + 7));
  }
  T res = norm_add(norm_add(norm_add(r0, r1), norm_add(r2, r3)), norm_add(norm_add(r4, r5), norm_add(r6, r7)));
  for (; i < n; ++i) res = norm_add(res, t(off + i));
  return res;
}

// One chunk (n <= 8192, see below) by the whole rule, without recursion and without an indexed array (so: no call stack, no
// per-thread scratch).  The split tree is walked in post-order; where the walk stands is (depth d, one bit per level: 0 = in the left
// half, 1 = in the right half), and the node's [off, off + len) is re-derived from the chunk's start whenever it is needed.  left[k]
// holds the finished left half of the level-k node while its right half is being summed; it is read and written by fully unrolled
// compares, which keeps it in registers.  A level takes the length to at most len / 2 + 4, so 8192 elements need at most 7 levels.
constexpr int kNormPairLevels = 8;
constexpr int kNormPairChunk = 8192;
template <typename T, typename Term>
__device__ inline T norm_pairwise_chunk(int base, int n, Term t) {
  if (n <= 128) return norm_pairwise_block<T>(base, n, t);
  T left[kNormPairLevels];
#pragma unroll
  for (int k = 0; k < kNormPairLevels; ++k) left[k] = (T)0;
  unsigned path = 0;
  int d = 0;
  for (;;) {
    int off = base, len = n;                               // the node at (d, path)
    for (int k = 0; k < d; ++k) {
      int n2 = len / 2; n2 -= n2 % 8;
      if ((path >> k) & 1u) { off += n2; len -= n2; } else len = n2;
    }
    while (len > 128 && d < kNormPairLevels) {             // down its left spine to a leaf
      int n2 = len / 2; n2 -= n2 % 8;
      path &= ~(1u << d); ++d; len = n2;
    }
    T ret = norm_pairwise_block<T>(off, len, t);
    bool turned = false;
    while (d > 0) {                                        // up again: a finished left half waits, a finished right half is added to it
      const int k = d - 1;
      if (!((path >> k) & 1u)) {
#pragma unroll
        for (int q = 0; q < kNormPairLevels; ++q) if (q == k) left[q] = ret;
        path |= 1u << k; turned = true;
        break;
      }
      T lv = (T)0;
#pragma unroll
      for (int q = 0; q < kNormPairLevels; ++q) if (q == k) lv = left[q];
      ret = norm_add(lv, ret);
      path &= ~(1u << k); d = k;
    }
    if (!turned) return ret;
  }
}
// numpy hands its inner loop at most 8192 elements at a time (the ufunc buffer size, which also bounds an unbuffered reduce's inner
// loop) and adds the chunks' sums to the result one after another: ((0 + chunk0) + chunk1) + ...
template <typename T, typename Term>
__device__ inline T norm_pairwise_sum(int n, Term t) {
  T res = (T)0;
  for (int base = 0; base < n; base += kNormPairChunk)
    res = norm_add(res, norm_pairwise_chunk<T>(base, n - base < kNormPairChunk ? n - base : kNormPairChunk, t));
  return res;
}

// RunningNormalizer.update (:75-93) for one feature of rows x(0) .. x(rows - 1) of a normaliser of `width` features; `mode` comes
// back as the statistics' type AFTER the update (float64 rows turn float32 statistics into float64 ones).  width >= 2: the sums run
// sequentially over the rows; width == 1: in numpy's pairwise order (above).  The pairwise sum of the rows and that of the squared
// deviations are two rounds of ONE not-unrolled loop: a second inlined copy of the walk made the process_step kernels a seventh
// longer and their launches 0.8 us slower for every width (instruction fetch), so the rare case keeps its code small.
template <typename Row>
__device__ inline void norm_update_col(double& m, double& v, int rows, int width, double c0, int& mode, Row x) {
  const bool pair = __builtin_expect(width == 1, 0);
  if (mode & NORM_ROWS64) {
    double s = 0.0, bm = 0.0, q = 0.0;
    if (pair) {
#pragma nounroll
      for (int pass = 0; pass < 2; ++pass) {     // pass 0: the sum of the rows; pass 1: of the squared deviations (one copy of the walk)
        const double r = norm_pairwise_sum<double>(rows, [&](int i) { const double xi = (double)x(i); if (pass == 0) return xi; const double d = __dsub_rn(xi, bm); return __dmul_rn(d, d); });
        if (pass == 0) bm = __ddiv_rn(r, (double)rows); else q = r;
      }
    } else {
      for (int i = 0; i < rows; ++i) s = __dadd_rn(s, (double)x(i));
      bm = __ddiv_rn(s, (double)rows);
      for (int i = 0; i < rows; ++i) { const double d = __dsub_rn((double)x(i), bm); q = __dadd_rn(q, __dmul_rn(d, d)); }
    }
    norm_merge64(m, v, bm, __ddiv_rn(q, (double)rows), rows, c0, (mode & NORM_F32) != 0);
    mode &= ~NORM_F32;
  } else {
    float s = 0.f, bm = 0.f, q = 0.f;
    if (pair) {
#pragma nounroll
      for (int pass = 0; pass < 2; ++pass) {
        const float r = norm_pairwise_sum<float>(rows, [&](int i) { const float xi = x(i); if (pass == 0) return xi; const float d = __fsub_rn(xi, bm); return __fmul_rn(d, d); });
        if (pass == 0) bm = __fdiv_rn(r, (float)rows); else q = r;
      }
    } else {
      for (int i = 0; i < rows; ++i) s = __fadd_rn(s, x(i));
      bm = __fdiv_rn(s, (float)rows);
      for (int i = 0; i < rows; ++i) { const float d = __fsub_rn(x(i), bm); q = __fadd_rn(q, __fmul_rn(d, d)); }
    }
    norm_merge(m, v, bm, __fdiv_rn(q, (float)rows), rows, c0, (mode & NORM_F32) != 0);
  }
}

// the divisor of normalize (:96): sqrt(var) + 1e-8 — a float32 value while the statistics are float32
__device__ inline double norm_den(double v, bool f32) {
  // (sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the latter is the NATIVE square root — 1 ulp off numpy's)
  return f32 ? (double)__fadd_rn(sqrtf((float)v), 1e-8f) : sqrt(v) + 1e-8;
}

// clip((x - mean) / den, -clip, clip), rounded to the float32 the trainer casts to (src/env.py:189-190).
// f32 = float32 statistics AND float32 rows: the whole expression in float32; otherwise float64 (den from norm_den above)
__device__ inline float norm_apply(float x, double m, double den, double clip, bool f32) {
  if (!f32) return (float)fmin(fmax(((double)x - m) / den, -clip), clip);
  const float z = __fdiv_rn(__fsub_rn(x, (float)m), (float)den);
  return fminf(fmaxf(z, -(float)clip), (float)clip);
}
__device__ inline bool norm_apply_f32(int mode) { return (mode & NORM_F32) && !(mode & NORM_ROWS64); }

}  // namespace gcrl
