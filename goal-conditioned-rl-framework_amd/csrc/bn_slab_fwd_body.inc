// bn_slab_fwd_body.inc — body of bn_linear_fwd_slab_kernel<VEC, NT, WV> (bn_slab.hip), shared as TEXT with its population form: `g` names the
// launch's FwdArgs (the kernel argument, or the member's entry of the device table), GCRL_SLAB_FWD_PROB the input this workgroup works on.
  __shared__ float red[WV][16];
  __shared__ unsigned int s_flag;
  __shared__ __attribute__((aligned(16))) float stage[WV][16 * NT * kCK];   // wave-private images of the A operand
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  const int prob = GCRL_SLAB_FWD_PROB, rgrp = NT == 1 ? (int)blockIdx.y : 0;
  const FwdProb me = g.p[prob];
  const int B = g.B, H = g.H;
  constexpr int kRowsWg = 16 * NT * WV;
  const int col0 = blockIdx.x * 16, col = col0 + li, row0 = rgrp * kRowsWg + wave * 16 * NT;
  const int nl = min(kRowsWg, B - rgrp * kRowsWg);              // rows of this workgroup (>= 1: launcher)
  const long long sl = (g.slot && me.x_slot) ? (long long)*g.slot : 0;
  v4f acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
  // epilogue operands first: their latency hides behind the GEMM
  const float bias = col < H ? g.bias[col] : 0.f, gm = col < H ? g.gamma[col] : 0.f, bt = col < H ? g.beta[col] : 0.f;
  const int xslot = prob * (H / 16) + (int)blockIdx.x;
  unsigned long long seq = 0;
  if (NT == 1 && g.RS > 1 && g.x.df) seq = slab_seq_load(g.x, xslot);   // (its round trip hides behind the GEMM)
  SLAB_STAMP(0);
  slab_gemm<VEC, true, NT, SlabStages<NT, WV>::value>(acc, stage[wave], me.X + sl * me.x_slot, g.ldx, g.W, g.K, g.K, B, H, row0, col0, lane);
  SLAB_STAMP(1);
  // acc[t][r] = z[row0 + 16 t + 4 lg + r][col] - bias
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[t][r] += bias;
      if (row0 + 16 * t + 4 * lg + r < B) s += acc[t][r];
    }
  asm volatile("" ::"v"(seq));                                      // the launch count has arrived in every wave before the barriers below
  float mean = col_sum<WV>(s, red, wave, li, lg) / (float)nl;      // of this workgroup's rows
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (row0 + 16 * t + 4 * lg + r < B) { const float d = acc[t][r] - mean; q += d * d; }
  float m2 = col_sum<WV>(q, red, wave, li, lg);
  SLAB_STAMP(2);
  if (NT == 1 && g.RS > 1) {
    // merge of the row groups' (n_j, mean_j, M2_j) in index order: mean = sum n_j mean_j / B, M2 = sum (M2_j + n_j (mean_j - mean)^2)
    float pm[8], pq[8];
    const bool ok = g.x.df ? slab_exchange_df(g.x, xslot, g.RS, rgrp, seq, mean, m2, wave, li, lg, pm, pq)
                           : slab_exchange(g.x, xslot, g.RS, rgrp, mean, m2, wave, li, lg, pm, pq, &s_flag);
    float sm = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < g.RS) sm += pm[j] * (float)min(kRowsWg, B - j * kRowsWg);
    mean = sm / (float)B;
    m2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < g.RS) { const float dm = pm[j] - mean; m2 += pq[j] + dm * dm * (float)min(kRowsWg, B - j * kRowsWg); }
    if (!ok) mean = __builtin_nanf("");                        // a timed-out exchange must not pass for a result
  }
  SLAB_STAMP(3);
  const float var = m2 / (float)B;                              // biased: what normalises the batch
  const float invstd = 1.0f / sqrtf(var + kEps);
  if (col < H) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + 16 * t + 4 * lg + r;
        if (row >= B) continue;
        const float xh = (acc[t][r] - mean) * invstd;
        const float y = xh * gm + bt;
        const long long idx = (long long)row * H + col;
        me.h[idx] = y > 0.f ? y : 0.f;
        if (me.xhat) me.xhat[idx] = xh;
      }
    if (rgrp == 0 && wave == 0 && lg == 0) {
      if (me.invstd) me.invstd[col] = invstd;
      me.bstat[col] = mean;
      me.bstat[H + col] = var;
    }
  }
#ifdef GCRL_SLAB_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  SLAB_STAMP(4);
#endif
