// adam_device.inc — the optimiser launches' device functions (riders, the per-net step, the control advance), included inside
// namespace gcrl { namespace { by ops.hip (adam_kernel, adam_pair_kernel) and adam_pop.hip (their population forms).
// riders_here: this launch's metric riders run in workgroup 0 of net 0 (the paired launch); else in a workgroup of their own (adam_kernel).
// nblocks: workgroups stepping elements (the flat form's stride)
__device__ inline void adam_riders(const AdamArgs& a, const StepCtrl& c) {
  if (a.mean_x) rider_mean_metric(a.mean_x, a.mean_n, a.mean_scale, a.metrics + (long long)c.metrics_slot * kMetricFloats + a.mean_index);
  if (a.td_q) rider_td_metrics(a.td_q, a.td_y, a.td_n, a.td_C, a.td_loss_kind, a.metrics + (long long)c.metrics_slot * kMetricFloats);
}
__device__ inline void adam_body(const AdamArgs& a, const int net, const bool riders_here = true, const unsigned nblocks = gridDim.x) {
  __shared__ float s_coef;
  const StepCtrl c = *a.cur;
  const AdamStepScalars sc = adam_scalars(c, a.which);
  const float gscale = c.grad_scale;
  const long long base = (long long)net * a.net_stride;
  float* __restrict__ p = a.p + base;
  const float* __restrict__ g = a.g + base;
  float* __restrict__ m = a.m + base;
  float* __restrict__ v = a.v + base;
  float* __restrict__ tp = a.target ? a.target + base : nullptr;
  // segmented launches: this thread's element is known before anything is loaded, so its operands are
  // requested NOW and arrive while the norm partials are being reduced (one memory round trip less on the
  // critical path of a kernel that is nothing but round trips)
  // (round 5: FOUR elements per thread — a block covers 1 024 flat elements or a 32 x 32 tile as four 16 x 16 sub-tiles.  With one element per
  // thread TD3's twin critics were 1 080 blocks of a few dependent round trips each, four waves of blocks on 256 CUs: 13.2 us for 7.7 MB.)
  AdamSeg sg;
  sg.tiled = 0; sg.nblk = 0;
  int lb = 0;
  long long my_i[kAdamPerThread];
#pragma unroll
  for (int u = 0; u < kAdamPerThread; ++u) my_i[u] = -1;
  if (a.n_seg > 0) {
    int s = 0;
#pragma unroll
    for (int q = 1; q < kMaxAdamSeg; ++q)
      if (q < a.n_seg && (int)blockIdx.x >= a.seg[q].blk0) s = q;
    sg = a.seg[s];
    lb = (int)blockIdx.x - sg.blk0;
    if (lb < sg.nblk) {
      if (!sg.tiled) {
#pragma unroll
        for (int u = 0; u < kAdamPerThread; ++u) {
          const long long i = sg.beg + ((long long)lb * kAdamPerThread + u) * 256 + threadIdx.x;
          if (i < sg.beg + (long long)sg.rows * sg.cols) my_i[u] = i;
        }
      } else {
        const int tiles_k = (sg.cols + kAdamTile - 1) / kAdamTile;
#pragma unroll
        for (int u = 0; u < kAdamPerThread; ++u) {   // sub-tile u: rows + 16 * (u >> 1), columns + 16 * (u & 1)
          const int o = (lb / tiles_k) * kAdamTile + 16 * (u >> 1) + (threadIdx.x >> 4), k = (lb % tiles_k) * kAdamTile + 16 * (u & 1) + (threadIdx.x & 15);
          if (o < sg.rows && k < sg.cols) my_i[u] = sg.beg + (long long)o * sg.cols + k;
        }
      }
    }
  }
  float pre_g[kAdamPerThread], pre_p[kAdamPerThread], pre_m[kAdamPerThread], pre_v[kAdamPerThread], pre_t[kAdamPerThread];
#pragma unroll
  for (int u = 0; u < kAdamPerThread; ++u) {
    pre_g[u] = pre_p[u] = pre_m[u] = pre_v[u] = pre_t[u] = 0.f;
    if (my_i[u] >= 0) {
      pre_g[u] = g[my_i[u]]; pre_p[u] = p[my_i[u]]; pre_m[u] = m[my_i[u]]; pre_v[u] = v[my_i[u]];
      if (tp && a.polyak) pre_t[u] = tp[my_i[u]];
    }
  }
  {
    // ||g||: every block sums the same partials in the same order (deterministic), in fp64
    __shared__ double dred[4];
    const float* part = a.partial + (long long)net * a.part_stride;
    double s = 0.0;
    // independent 16-byte loads (a dependent scalar loop here cost ~4 us of L2 latency per launch)
    const int n4 = ((reinterpret_cast<uintptr_t>(part) & 15) == 0) ? a.nparts >> 2 : 0;
    const float4* part4 = reinterpret_cast<const float4*>(part);
    for (int i = threadIdx.x; i < n4; i += 256) {
      const float4 v = part4[i];
      s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
    for (int i = 4 * n4 + threadIdx.x; i < a.nparts; i += 256) s += (double)part[i];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      s = dred[0] + dred[1] + dred[2] + dred[3];
      float post;
      s_coef = clip_coef(s, gscale, a.clip[net], &post);
      if (blockIdx.x == 0 && a.metrics)
        a.metrics[(long long)c.metrics_slot * kMetricFloats + a.metric_index + net] = post;
    }
  }
  __syncthreads();
  if (riders_here && blockIdx.x == 0 && net == 0) adam_riders(a, c);
  const float gmul = gscale * s_coef;
  const float w1 = a.w1, w2 = a.w2, one_m_tau = a.one_m_tau;
  const bool pk = tp && a.polyak;
  // one element: torch's single-tensor Adam(W) op order; returns the new parameter, *ti the new target
  auto step_vals = [&](long long i, float g_raw, float pi, float mi, float v_old, float t_old, float* ti) -> float {
    const AdamElem e = adam_elem(g_raw, pi, mi, v_old, gmul, sc, a.beta2, w1, w2, a.eps);
    p[i] = e.p; m[i] = e.m; v[i] = e.v;
    if (pk) { *ti = polyak_elem(a.tau, e.p, one_m_tau, t_old); tp[i] = *ti; }
    return e.p;
  };
  if (a.n_seg == 0) {
    float ti;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long long)nblocks * 256)
      step_vals(i, g[i], p[i], m[i], v[i], pk ? tp[i] : 0.f, &ti);
    return;
  }
  if (lb >= sg.nblk) return;   // paired launches are sized for the larger net
  float ti[kAdamPerThread], pi[kAdamPerThread];
#pragma unroll
  for (int u = 0; u < kAdamPerThread; ++u) {
    ti[u] = 0.f; pi[u] = 0.f;
    if (my_i[u] >= 0) pi[u] = step_vals(my_i[u], pre_g[u], pre_p[u], pre_m[u], pre_v[u], pre_t[u], &ti[u]);
  }
  if (!sg.tiled) return;
  __shared__ float tile_p[kAdamPerThread][16][17], tile_t[kAdamPerThread][16][17];
  const int tiles_k = (sg.cols + kAdamTile - 1) / kAdamTile;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
  for (int u = 0; u < kAdamPerThread; ++u) { tile_p[u][ty][tx] = pi[u]; tile_t[u][ty][tx] = ti[u]; }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kAdamPerThread; ++u) {
    const int o0 = (lb / tiles_k) * kAdamTile + 16 * (u >> 1), k0 = (lb % tiles_k) * kAdamTile + 16 * (u & 1);
    const int k = k0 + ty, o = o0 + tx;   // 16 consecutive o per copy row: 64-byte runs
    if (k < sg.cols && o < sg.rows) {
      const long long at = (long long)net * a.wt_net_stride + sg.dst + (long long)k * sg.rows + o;
      a.wt[at] = tile_p[u][tx][ty];
      if (pk && a.wt_target) a.wt_target[at] = tile_t[u][tx][ty];
    }
  }
}

__device__ inline void advance_ctrl(const AdamArgs& a) {
  if (a.advance && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    ctrl_advance(a.advance);
  }
}
