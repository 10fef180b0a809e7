// dw_adam_body.inc — body of the fused dW + optimiser launch, included by dw_adam.hip into dw_adam_kernel (the single-agent
// launch) and dw_adam_pop_kernel (the population launch).  In scope: `a` (the launch's DwAdamK) and `bx`, `by` (the workgroup's
// tile and net in the member's launch).
#ifdef GCRL_OF_STAMPS
  unsigned long long of_t[5];
#endif
  OF_STAMP(0);
  __shared__ float s_ss[4];
  __shared__ double dred[4];
  __shared__ float s_coef;
  __shared__ float tile_p[16][17], tile_t[16][17];
  __shared__ __attribute__((aligned(16))) float img[4][16][kImgLd];   // a regular tile's p / m / v / target: in as loaded, out as stepped
  const DwNetK& on = a.net[by];
  DwNetHead o = on.h;          // first round trip: 16 dwords
  pin(o);
  if ((int)bx >= o.ntiles) return;   // (a paired launch is sized for the larger net; uniform per workgroup, before any barrier)
  // XCD-aware workgroup -> tile order (gemm_mfma.h xcd_tile_of, here for the 2-D grid: workgroup (x, y) runs on XCD
  // (x + y * gridDim.x) % 8): an XCD takes a contiguous range of the net's tiles — whole tile rows of a layer, i.e. that layer's
  // activations enter ONE L2 instead of eight.  A wrong guess about the placement costs speed, never correctness.
  int bid = (int)bx;
  {
    const int per = o.ntiles >> 3;
    if (bid < (per << 3)) bid = ((bid + (int)by * o.grid_x) & 7) * per + (bid >> 3);
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int pi = (bid >= o.tile0[0]) + (bid >= o.tile0[1]) + (bid >= o.tile0[2]) + (bid >= o.tile0[3]);
  const int t0 = pi == 0 ? 0 : o.tile0[0] * (pi == 1) + o.tile0[1] * (pi == 2) + o.tile0[2] * (pi == 3) + o.tile0[3] * (pi == 4);
  // second round trip: the problem, the net's arrays, the step's scalars (the control block's copy, written by the launch in front)
  // and the launch count — the last two through the scalar cache (constant address space): uniform, and nothing in this launch
  // writes them before they are read
  DwProb pr = on.prob[pi];
  DwNetPtrs ptr = on.ptr;
  StepCtrl c = load_uniform(o.cur);
  unsigned long long sq = load_uniform(reinterpret_cast<const unsigned long long*>(o.seq));
  pin(pr); pin(ptr); pin(c); pin(sq);   // (all four requested, then waited for together)
  gfloat* const gp = (gfloat*)ptr.p; gfloat* const gm = (gfloat*)ptr.m; gfloat* const gv = (gfloat*)ptr.v; gfloat* const gt = (gfloat*)ptr.target;
  gfloat* const gwt = (gfloat*)ptr.wt; gfloat* const gwtt = (gfloat*)ptr.wt_target;
  gu64* const gslots = (gu64*)o.slots;
  const unsigned int seq = (unsigned int)sq, fault = (unsigned int)(sq >> 32);   // (fault: the test hook gcrl_agent_debug_meet_fault — workgroup 1's slot never arrives, once)
  const int t = bid - t0;
  const int tn = t % pr.tiles_n, tm = t / pr.tiles_n;
  const int m0 = tm << 4, n0 = tn << 4;
  const int in = pr.in, out = pr.out;   // the problem is [out][in | 1]: column `in` is the bias gradient
  struct { long long pw, pb, wt_dst; int slot0; } lay = {pr.pw, pr.pb, pr.wt_dst, pr.slot0};

  const AdamStepScalars sc = adam_scalars(c, o.which);
  const int em = m0 + 4 * lg + wave, en = n0 + li;   // this lane's element of the tile (gemm_batch_tile's k-split layout)
  long long my_i = -1;
  if (em < out) {
    if (en < in) my_i = lay.pw + (long long)em * in + en;
    else if (en == in) my_i = lay.pb + em;
  }
  const bool pk = ptr.target && o.polyak;

  // the problem as the batched launch's tile body wants it (agent.hip bwd_dw): everything else of the record is a literal here
  GemmDesc d;
  d.A = pr.G; d.a_rs = 1; d.a_cs = pr.ldg;
  d.B = pr.X + (pr.x_slot ? (long long)c.batch_slot * pr.x_slot : 0); d.b_rs = pr.ldx; d.b_cs = 1;
  // (ones_col through an opaque register: as a literal, the compiler turned the tile body's `ones column ? 1 : loaded value` selects
  // into a branch around the B loads of every chunk and drained the loads in flight — s_waitcnt vmcnt(0) — at each of them)
  int one = 1;
  asm volatile("" : "+s"(one));
  d.C = pr.dW; d.c_rs = pr.in; d.col_out = pr.db; d.ones_col = one;
  d.M = pr.out; d.N = pr.in + 1; d.K = pr.K;
  d.bias = nullptr; d.H = nullptr; d.h_rs = 0; d.epi = EPI_NONE; d.mul = MUL_NONE;
  d.slot = nullptr; d.a_slot = d.b_slot = d.c_slot = d.h_slot = 0;
  d.sumsq_out = nullptr; d.bn_part = nullptr;
  d.a_vec = d.b_vec = d.a_rvec = d.b_rvec = 0;   // (operands are batch-major: k runs along rows)
  d.tile0 = 0; d.tiles_n = pr.tiles_n; d.ntiles = 0x7fffffff;
  d.shape_hint = 0; d.ksplit = 0; d.kpart = nullptr; d.kticket = nullptr;
  float x, ss;
  OF_STAMP(1);
  gemm_batch_tile<1, 1, 4>(d, t, x, ss);   // (the gradient element is also stored: get("grad:...") reads it)

  // the tile's sum of squares in the order adam_kernel adds up the batched launch's four per-wave partials of a tile
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_down(ss, off, 64);
  if (lane == 0) s_ss[wave] = ss;
  __syncthreads();
  gu64* mine = gslots + (long long)(seq & 1u) * o.slot_stride;
  if (threadIdx.x == 0 && !(fault && bid == 1)) {
    const double dt = ((double)s_ss[0] + (double)s_ss[1]) + ((double)s_ss[2] + (double)s_ss[3]);
    const int slot = lay.slot0 + t;
    __hip_atomic_store(mine + slot, (unsigned long long)__double_as_longlong(dt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // write-through
    gslots[(long long)((seq & 1u) ^ 1u) * o.slot_stride + slot] = kSlotEmpty;   // nobody reads the other array in this launch; the kernel boundary publishes it
  }
  // A regular tile — all 16 x 16 elements are weights of a layer whose rows are whole 16-byte runs — moves its parameter traffic as
  // ONE 16-byte access per lane and array: wave w takes array w (p, m, v; target on a Polyak step), lane -> row lane >> 2, columns
  // 4 * (lane & 3) ..+3, through an LDS image, and the new values leave written through (sc1): nothing of them stays dirty in this
  // XCD's L2 for the kernel boundary to write back.  (16-byte sc1 stores cost what plain ones do; 4-byte ones six times that.)
  // Every other tile — first layers with odd rows, the bias column, head rows, partial tiles — keeps the element-per-lane path.
  // (Worked out HERE, behind the tile body, from operands the compiler cannot see through: in front of it the operand requests
  // left 0.4 us later.  And the 16-byte pre-load stands in front of the other path's loads, not in an else branch: laid out behind
  // them, its zero-initialised registers were those loads' destinations and the compiler drained every access in flight —
  // s_waitcnt vmcnt(0), the gradient tile's stores included — before requesting it.)
  int in_q = in, out_q = out;
  asm volatile("" : "+s"(in_q), "+s"(out_q) :: "memory");
  const bool wt_wide = lay.wt_dst < 0 || ((out_q & 3) == 0 && (lay.wt_dst & 3) == 0 &&
                                          (((unsigned long long)ptr.wt | (pk ? (unsigned long long)ptr.wt_target : 0ull)) & 15) == 0);
  const bool regular = (in_q & 3) == 0 && n0 + 16 <= in_q && m0 + 16 <= out_q && (lay.pw & 3) == 0 && wt_wide &&
                       (((unsigned long long)ptr.p | (unsigned long long)ptr.m | (unsigned long long)ptr.v | (pk ? (unsigned long long)ptr.target : 0ull)) & 15) == 0;
  const bool mover = wave < 3 || pk;              // (uniform per wave) this wave has an array to move
  const int r4 = lane >> 2, c4 = (lane & 3) << 2;
  const float* const my_arr = wave == 0 ? ptr.p : wave == 1 ? ptr.m : wave == 2 ? ptr.v : ptr.target;
  // this lane's parameter, moments and target: requested now, they arrive while the slots are awaited.  (In front of the tile body
  // they cost it a round trip: its k-loop's header waits for every load in flight — the registers its loads return in are reused
  // per iteration — and so the operand requests went out only after these had landed.)
  float pre_p = 0.f, pre_m = 0.f, pre_v = 0.f, pre_t = 0.f;
  v4u pre4 = {0u, 0u, 0u, 0u};
  if (regular && mover) pre4 = __builtin_amdgcn_raw_buffer_load_b128(wave_uniform_rsrc_n(my_arr + lay.pw + (long long)m0 * in + n0, 15LL * in + 16), (r4 * in + c4) * 4, 0, 0);
  if (!regular && my_i >= 0) {
    pre_p = gp[my_i]; pre_m = gm[my_i]; pre_v = gv[my_i];
    if (pk) pre_t = gt[my_i];
  }
  OF_STAMP(2);
  // riders of the net's first workgroup, while the other workgroups' slots arrive
  float* met = a.metrics + (long long)c.metrics_slot * kMetricFloats;
  if (bid == 0) {
    if (on.mean_x) rider_mean_metric(on.mean_x, on.mean_n, on.mean_scale, met + on.mean_index);
    if (on.td_q) rider_td_metrics(on.td_q, on.td_y, on.td_n, on.td_C, on.td_loss_kind, met);
  }
  // ||g||: the net's slots summed in ONE order (thread t: slots t, t + 256, ...; then lanes, then waves), in fp64.  Nets of
  // >= kLeaderMinTiles tiles: only the first eight workgroups of the net — one per XCD under round-robin dispatch — sweep the
  // slots; each leaves the sum in a result word (again its own flag), and every other workgroup polls the ONE word of the leader
  // that shares its XCD.  With every workgroup sweeping every slot the early finishers kept ~5 MB of slot loads per round in
  // flight in front of the operand loads of the workgroups still working (measured: the last tile done at 10-15 us instead of
  // 7.5); a leader's sweep is 37 lines.  Smaller nets: every workgroup sweeps (a few KB in all).
  {
    const bool lead_mode = o.ntiles >= kLeaderMinTiles;
    const bool sweeper = !lead_mode || bx < 8;
    const int xc = ((int)bx + (int)by * o.grid_x) & 7;
    gu64* res = mine + (o.slot_stride - 8);
    bool ok = true;
    double s = 0.0;
    if (sweeper) {
      // a lane re-loads only the slots it has not seen yet
      unsigned long long w[kFusedMaxSlotsPerThread];
      int spins = 0;
#pragma unroll
      for (int u = 0; u < kFusedMaxSlotsPerThread; ++u) {
        const int i = (int)threadIdx.x + 256 * u;
        w[u] = i < o.ntiles ? __hip_atomic_load(mine + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
      }
      for (;;) {
        bool all = true;
#pragma unroll
        for (int u = 0; u < kFusedMaxSlotsPerThread; ++u) all = all && w[u] != kSlotEmpty;
        if (all) break;
        if (++spins >= kMeetSpinMax) { ok = false; break; }
        poll_pause();
#pragma unroll
        for (int u = 0; u < kFusedMaxSlotsPerThread; ++u)
          if (w[u] == kSlotEmpty) w[u] = __hip_atomic_load(mine + (int)threadIdx.x + 256 * u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int u = 0; u < kFusedMaxSlotsPerThread; ++u)
        if ((int)threadIdx.x + 256 * u < o.ntiles) s += __longlong_as_double((long long)w[u]);
      if (!ok) s = __longlong_as_double(0x7ff8000000000000ll);   // a slot never arrived: the step is poisoned (and reported below)
      s = wave_sum_d(s);
      if (lane == 0) dred[wave] = s;
      __syncthreads();
      if (threadIdx.x == 0) {
        s = dred[0] + dred[1] + dred[2] + dred[3];
        if (lead_mode) {
          __hip_atomic_store(res + xc, (unsigned long long)__double_as_longlong(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // write-through
          gslots[(long long)((seq & 1u) ^ 1u) * o.slot_stride + (o.slot_stride - 8) + xc] = kSlotEmpty;
        }
      }
    } else if (threadIdx.x == 0) {
      // (measured: four polls in flight, a quarter of a round trip apart, instead of one at a time — no gain, 52.5-52.7 vs
      // 52.2 us/step: the hop costs the store's way to the memory side plus one load round trip, not the sampling period)
      unsigned long long w = __hip_atomic_load(res + xc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int spins = 0; w == kSlotEmpty; ) {
        if (++spins >= kMeetSpinMax) { ok = false; w = 0x7ff8000000000000ull; break; }
        poll_pause();
        w = __hip_atomic_load(res + xc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      s = __longlong_as_double((long long)w);
    }
    if (!ok && a.status) __hip_atomic_fetch_or(a.status, (unsigned int)MEET_ERR_DW_ADAM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // the host learns it (meet.h)
    if (threadIdx.x == 0) {
      float post;
      s_coef = clip_coef(s, c.grad_scale, ptr.clip, &post);
      if (bid == 0 && a.metrics) met[on.metric_index] = post;
    }
  }
  if (regular && mover) *reinterpret_cast<v4u*>(&img[wave][r4][c4]) = pre4;
  __syncthreads();
  OF_STAMP(3);
  const float gmul = c.grad_scale * s_coef;
  float p_new = 0.f, t_new = 0.f;
  if (regular) {
    const int r = 4 * lg + wave;
    const AdamElem e = adam_elem(x, img[0][r][li], img[1][r][li], img[2][r][li], gmul, sc, a.beta2, a.w1, a.w2, a.eps);
    if (pk) img[3][r][li] = polyak_elem(a.tau, e.p, a.one_m_tau, img[3][r][li]);
    img[0][r][li] = e.p; img[1][r][li] = e.m; img[2][r][li] = e.v;   // (each lane overwrites what it alone read)
    __syncthreads();
    if (mover)
      __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const v4u*>(&img[wave][r4][c4]), wave_uniform_rsrc_n(my_arr + lay.pw + (long long)m0 * in + n0, 15LL * in + 16),
                                             (r4 * in + c4) * 4, 0, kSc1);
    // the [in][out] copies: 16 x 16 again, a lane's run is four consecutive outputs of input n0 + r4 — wave 3 the online copy, wave 2 the target's
    const bool cp_t = wave == 2 && pk && ptr.wt_target;
    if (lay.wt_dst >= 0 && (wave == 3 || cp_t)) {
      const float (*src)[kImgLd] = cp_t ? img[3] : img[0];
      const v4u run = {__float_as_uint(src[c4][r4]), __float_as_uint(src[c4 + 1][r4]), __float_as_uint(src[c4 + 2][r4]), __float_as_uint(src[c4 + 3][r4])};
      __builtin_amdgcn_raw_buffer_store_b128(run, wave_uniform_rsrc_n((cp_t ? ptr.wt_target : ptr.wt) + lay.wt_dst + (long long)n0 * out + m0, 15LL * out + 16),
                                             (r4 * out + c4) * 4, 0, kSc1);
    }
  } else if (my_i >= 0) {
    const AdamElem e = adam_elem(x, pre_p, pre_m, pre_v, gmul, sc, a.beta2, a.w1, a.w2, a.eps);
    gp[my_i] = e.p; gm[my_i] = e.m; gv[my_i] = e.v;
    p_new = e.p;
    if (pk) { t_new = polyak_elem(a.tau, e.p, a.one_m_tau, pre_t); gt[my_i] = t_new; }
  }
  if (!regular && lay.wt_dst >= 0) {   // (uniform per workgroup) the [in][out] copy of a hidden layer's weight: 16 consecutive outputs per run
    tile_p[4 * lg + wave][li] = p_new;
    tile_t[4 * lg + wave][li] = t_new;
    __syncthreads();
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int k = n0 + ty, oo = m0 + tx;
    if (k < in && oo < out) {
      const long long at = lay.wt_dst + (long long)k * out + oo;
      gwt[at] = tile_p[tx][ty];
      if (pk && ptr.wt_target) gwtt[at] = tile_t[tx][ty];
    }
  }
  OF_STAMP(4);
#ifdef GCRL_OF_STAMPS
  if (a.stamps && threadIdx.x == 0)
    for (int k = 0; k < 5; ++k) a.stamps[((long long)by * 2048 + bx) * 8 + k] = of_t[k];
#endif
  if (bid == 0 && threadIdx.x == 0) {
    ((gu32*)o.seq)[1] = 0u;
    ((gu32*)o.seq)[0] = seq + 1u;   // every workgroup of this launch read it before it published, and this workgroup has seen every slot
    if (by == 0 && a.advance) ctrl_advance(a.advance);
  }
