// rowchain_ddpg_body.inc — body of the fused DDPG row-chain launch, included by rowchain.hip into rowchain_ddpg_kernel (the
// single-agent launch) and rowchain_ddpg_pop_kernel (the population launch).  In scope: template <int RG>, `a` (the launch's
// RowChainArgs) and blockIdx.x (the workgroup's index in the member's launch); template <bool LM>: the LDS-multiplier form (rowchain.h
// rowchain_lds_bytes_mul) — the hidden activations of every net with a backward chain keep LDS rows of their own behind the head biases,
// KP = [L - 1][R][ldl] per net, and the chains read their multipliers there.  hA / gA / hC / gC still leave for the dW launch; hC2, which
// only this launch read, is neither written nor read.  The SAC form (p_critic_only) is never launched with LM (launch_rowchain_ddpg).
// constexpr bool ST: the stream form of the actor phase's chained passes (rowchain_ddpg_kernel_stream, RG = 1); RC_STAMP: development stamps.
// constexpr bool WR: the launch may carry L2-warming riders behind its roles (the single-agent stream kernel only; a.reserved0 of them).
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // k_split (round 4, DDPG): the critic phase K as TWO roles in this launch — its target chain (target actor -> target critic -> Q')
  // and its online critic's forward are independent, so K's critical path shrinks from 11 layer passes to 6 + 2 (the split kernel's
  // phase 0, part 3, producers / consumers form: workgroups [0, nblk_k) the target role, [nblk_k, 2 nblk_k) the online critic, which
  // waits for its rows' Q' only) and the launch is bounded by the actor phase's 10 passes instead.  Same per-row arithmetic.
  if (a.k_split && a.nblk_k) {
    if ((int)blockIdx.x < 2 * a.nblk_k) {
      if (a.clk && threadIdx.x == 0 && blockIdx.x == 0) atomicMin(&a.clk[0], (unsigned long long)wall_clock64());
      rowchain_split_body<RG, false, LM>(a, 0, 3, (int)blockIdx.x);
      if (a.clk && threadIdx.x == 0) atomicMax(&a.clk[1], (unsigned long long)wall_clock64());
      return;
    }
  }
  const int kblocks = (a.k_split && a.nblk_k) ? 2 * a.nblk_k : a.nblk_k;
  if constexpr (WR) {
    // the launch's last a.reserved0 workgroups: L2-warming riders (rowchain.hip rc_warm_rider), behind every role's workgroups
    if ((int)blockIdx.x >= kblocks + a.nblk_p) { rc_warm_rider(a, (int)blockIdx.x - kblocks - a.nblk_p); return; }
  }
  constexpr int R = 4 * RG;
  const int ldl = a.ldl, H = a.critic[0].H, S = a.S, A = a.A, B = a.B;
  float* X0 = lds;
  float* X1 = X0 + R * ldl;
  float* X2 = X1 + R * ldl;
  float* XS = X2 + R * ldl;               // second input rows (K) / last actor activation (P)
  float* part = XS + R * ldl;
  float* sm = part + R * 16 + (RG == 1 ? 2 : 1) * 4 * R * kRowChunk;   // [R][16] head outputs (part[0..R*16): smoothing noise; then 2 exchange buffers)
  float* sm2 = sm + R * 16;               // [R][16] second small array
  float* sm3 = sm2 + R * 16;              // [R][16] reward / done
  float* hw = sm3 + R * 16;               // head weights of the role: [A*H | H | max(A*H, H)], then head biases [16 | 16]
  float* hb = hw + max(max(2 * A + 1, A + 2 * a.C), a.C * (A + 1)) * H;
  [[maybe_unused]] float* KP = hb + 96;                                // LM: kept layers of the role's first chained net (K: critic k, P: actor)
  [[maybe_unused]] float* KPC = KP + max(a.actor.L - 1, 0) * R * ldl;  // LM, P: the critic's, behind the actor's
  // Which role, which row block: the roles in launch order, K's workgroups first
  const bool role_k = (int)blockIdx.x < kblocks;
  const int blk = role_k ? (int)blockIdx.x : (int)blockIdx.x - kblocks;
  const long long row0 = (long long)blk * R;
  const int rv = min(R, B - (int)row0);
  const long long BH = (long long)B * H;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) { a.cb->cur_b = a.cb->cur; a.cb->prev_b = a.cb->prev; }
  if (a.clk && tid == 0 && blk == 0) atomicMin(&a.clk[0], (unsigned long long)wall_clock64());

  // Everything that does not depend on computed data is requested NOW (inputs, rewards, head
  // weights and biases): each of these was a separate exposed memory round trip (~1 us) in the
  // middle of the chain.
  if (role_k) {
    const StepCtrl c = *a.cur_k;
    const int C = a.C;
    const float* ns_rows = a.nsa + (long long)c.batch_slot * a.slot_x + row0 * a.ldx;
    const float* sa_rows = a.sa + (long long)c.batch_slot * a.slot_x + row0 * a.ldx;
    const float* rr = a.rbuf + (long long)c.batch_slot * a.slot_rd + row0;
    const float* dd = a.dbuf + (long long)c.batch_slot * a.slot_rd + row0;
    constexpr int NX = 2 * RG;   // covers row widths up to 128 floats
    const int jp_ns = max(a.tactor.jpad0, a.tcritic[0].jpad0), nc_ns = a.given_next ? S + A : S;
    float* hw_ta = hw; float* hw_tc = hw + A * H; float* hw_c = hw_tc + C * H;
    const float* src_ta = a.tactor.P + a.tactor.w[a.tactor.L];
    // phase 1: request everything
    Staged<NX> s_ns, s_sa;
    rows_load<RG>(s_ns, ns_rows, a.ldx, nc_ns, jp_ns, rv);
    rows_load<RG>(s_sa, sa_rows, a.ldx, S + A, a.critic[0].jpad0, rv);
    float v_r = 0.f, v_d = 0.f, v_lp = 0.f, v_hb = 0.f;
    if (tid < R && tid < rv) { v_r = rr[tid]; v_d = dd[tid]; if (a.logp_next) v_lp = a.logp_next[row0 + tid]; }
    if (tid < A && !a.given_next) v_hb = a.tactor.P[a.tactor.b[a.tactor.L] + tid];
    if (tid >= 32 && tid < 32 + C) v_hb = a.tcritic[tid - 32].P[a.tcritic[tid - 32].b[a.tcritic[tid - 32].L]];
    if (tid >= 64 && tid < 64 + C) v_hb = a.critic[tid - 64].P[a.critic[tid - 64].b[a.critic[tid - 64].L]];
    Staged<8> s_ta, s_tc[2], s_c[2];
    if (!a.given_next) seg_load(s_ta, src_ta, A * H);
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (k < C) {
        seg_load(s_tc[k], a.tcritic[k].P + a.tcritic[k].w[a.tcritic[k].L], H);
        seg_load(s_c[k], a.critic[k].P + a.critic[k].w[a.critic[k].L], H);
      }
    // phase 2: into LDS
    rows_store<RG>(s_ns, X0, ldl, ns_rows, a.ldx, nc_ns, jp_ns, rv);
    rows_store<RG>(s_sa, XS, ldl, sa_rows, a.ldx, S + A, a.critic[0].jpad0, rv);
    if (tid < R) { sm3[tid * 16] = v_r; sm3[tid * 16 + 1] = v_d; sm3[tid * 16 + 2] = v_lp; }
    if (tid < A && !a.given_next) hb[tid] = v_hb;
    if (tid >= 32 && tid < 32 + C) hb[16 + (tid - 32)] = v_hb;
    if (tid >= 64 && tid < 64 + C) hb[18 + (tid - 64)] = v_hb;
    if (!a.given_next) seg_store(s_ta, hw_ta, src_ta, A * H);
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (k < C) {
        seg_store(s_tc[k], hw_tc + k * H, a.tcritic[k].P + a.tcritic[k].w[a.tcritic[k].L], H);
        seg_store(s_c[k], hw_c + k * H, a.critic[k].P + a.critic[k].w[a.critic[k].L], H);
      }
    if (a.target_kind == TGT_MIN && !a.given_next && tid < R * A) {
      // smoothing noise of this block's rows, same draw as td3_smooth_kernel (element i = row*A + j)
      const int r = tid / A, o = tid - r * A;
      const long long i = (row0 + r) * A + o;
      float e = 0.f;
      if (r < rv) e = a.noise ? a.noise[i] : hash_normal(a.seed, (((unsigned long long)c.rng_hi << 32) | c.rng_lo) + (unsigned long long)i);
      part[tid] = fminf(fmaxf(__fmul_rn(e, a.policy_noise), -a.noise_clamp), a.noise_clamp);
    }
    __syncthreads();
    float* h;
    if (!a.given_next) {
      // target actor on ns (+ clipped smoothing noise, TD3)
      h = mlp_hidden<RG>(a.tactor, X0, X1, X2, ldl, part + R * 16, nullptr, BH, row0, rv);
      rows_head<RG>(h, ldl, H, hw_ta, H, hb, A, EPI_TANH, sm);
      __syncthreads();
      if (tid < R * A) {
        const int r = tid / A, o = tid - r * A;
        float act = sm[r * 16 + o];
        if (a.target_kind == TGT_MIN) act = fminf(fmaxf(__fadd_rn(act, part[tid]), -1.0f), 1.0f);
        X0[r * ldl + S + o] = act;
      }
      __syncthreads();
    }
    // target critic(s) on [ns | a']
    for (int k = 0; k < C; ++k) {
      h = mlp_hidden<RG>(a.tcritic[k], X0, X1, X2, ldl, part + R * 16, nullptr, BH, row0, rv);
      rows_head<RG>(h, ldl, H, hw_tc + k * H, H, hb + 16 + k, 1, EPI_NONE, sm + 4 + k);   // sm[r*16 + 4 + k]
      __syncthreads();
    }
    if (tid < R) {
      // y = r + gamma*(1-d)*tq, tq = Q' (DDPG, y clamped to [-1/(1-gamma), 0]) or min(Q1', Q2') (TD3):
      // same roundings as td_loss_kernel
      const int r = tid;
      float tq = a.target_kind == TGT_DDPG ? sm[r * 16 + 4] : fminf(sm[r * 16 + 4], sm[r * 16 + 5]);
      if (a.target_kind == TGT_MIN_ENT) tq = __fsub_rn(tq, __fmul_rn(a.alpha, sm3[r * 16 + 2]));
      float y = __fadd_rn(sm3[r * 16], __fmul_rn(__fmul_rn(a.gamma, __fsub_rn(1.0f, sm3[r * 16 + 1])), tq));
      if (a.target_kind == TGT_DDPG) y = fminf(fmaxf(y, a.clamp_lo), 0.0f);
      sm2[r * 16 + 1] = y;
      if (r < rv) a.y[row0 + r] = y;
    }
    // online critic(s) on [s | a]: forward (activations saved), loss gradient, input-gradient chain
    for (int k = 0; k < C; ++k) {
      if constexpr (LM) h = mlp_hidden_keep<RG>(a.critic[k], XS, KP, X1, ldl, part + R * 16, a.hC + (long long)k * a.critic[k].L * BH, BH, row0, rv);
      else h = mlp_hidden<RG>(a.critic[k], XS, X1, X2, ldl, part + R * 16, a.hC + (long long)k * a.critic[k].L * BH, BH, row0, rv);
      rows_head<RG>(h, ldl, H, hw_c + k * H, H, hb + 18 + k, 1, EPI_NONE, sm);
      __syncthreads();
      if (tid < R) {
        const int r = tid;
        const float q = sm[r * 16], y = sm2[r * 16 + 1];
        const float diff = __fsub_rn(q, y);
        float g;
        if (a.loss_kind == LOSS_MSE) g = (2.0f / (float)B) * diff;            // d mse_loss / dq
        else { const float n1 = 1.0f / (float)B; g = (diff < -1.0f) ? -n1 : (diff > 1.0f ? n1 : n1 * diff); }   // smooth-L1
        if (r >= rv) g = 0.f;
        sm2[r * 16] = g;
        if (r < rv) { a.q[(long long)k * B + row0 + r] = q; a.dq[(long long)k * B + row0 + r] = g; }
      }
      __syncthreads();
      float* gsave = a.gC + (long long)k * a.critic[k].L * BH;
      head_backward<RG>(h, ldl, H, hw_c + k * H, 1, sm2, gsave + (a.critic[k].L - 1) * BH + row0 * H, rv);
      __syncthreads();
      if constexpr (LM) grad_chain_keep<RG>(a.critic[k], h, X1, X2, ldl, part + R * 16, KP, gsave, BH, row0, rv);
      else grad_chain<RG>(a.critic[k], h, X1, X2, ldl, part + R * 16, a.hC + (long long)k * a.critic[k].L * BH, gsave, BH, row0, rv);
    }
  } else if (a.p_critic_only) {
    const StepCtrl c = *a.cur_p;
    const int C = a.C;
    const float* s_rows = a.sa + (long long)c.batch_slot * a.slot_x + row0 * a.ldx;
    {
      const int jpad = a.critic[0].jpad0;
      for (int i = tid; i < R * jpad; i += kRowThreads) {
        const int r = i / jpad, cc = i - r * jpad;
        float v = 0.f;
        if (r < rv) {
          if (cc < S) v = s_rows[(long long)r * a.ldx + cc];
          else if (cc < S + A) v = a.pi[(row0 + r) * a.Apad + (cc - S)];
        }
        X0[r * ldl + cc] = v;
      }
    }
    float* hw_c = hw; float* hw_da = hw + C * H;   // heads [C][H], then rows S..S+A-1 of each W0^T [C][A][H]
    for (int k = 0; k < C; ++k) {
      stage(hw_c + k * H, a.critic[k].P + a.critic[k].w[a.critic[k].L], H);
      stage(hw_da + k * A * H, a.critic[k].Wt + a.critic[k].wt[0] + (long long)S * H, A * H);
    }
    if (tid < C) hb[tid] = a.critic[tid].P[a.critic[tid].b[a.critic[tid].L]];
    __syncthreads();
    for (int k = 0; k < C; ++k) {
      float* h = mlp_hidden<RG>(a.critic[k], X0, X1, X2, ldl, part + R * 16, a.hC2 + (long long)k * a.critic[k].L * BH, BH, row0, rv);
      rows_head<RG>(h, ldl, H, hw_c + k * H, H, hb + k, 1, EPI_NONE, sm + k);   // sm[r*16 + k]
      __syncthreads();
    }
    if (tid < R) {
      // d(-mean min(q1, q2))/dq: to the smaller, split on ties (actor_select_kernel)
      const int r = tid;
      const float q0 = sm[r * 16], q1 = C > 1 ? sm[r * 16 + 1] : INFINITY;
      const float gb = r < rv ? -1.0f / (float)B : 0.f;
      const float w0 = q0 < q1 ? 1.f : (q0 == q1 ? 0.5f : 0.f);
      sm2[r * 16] = gb * w0;
      sm2[r * 16 + 1] = gb * (1.f - w0);
      if (r < rv) { a.q2[row0 + r] = q0; if (C > 1) a.q2[(long long)B + row0 + r] = q1; }
    }
    __syncthreads();
    for (int k = 0; k < C; ++k) {
      const float* hs = a.hC2 + (long long)k * a.critic[k].L * BH;
      const float* hsrc = hs + (a.critic[k].L - 1) * BH + row0 * H;
      for (int i = tid; i < R * H; i += kRowThreads) {
        const int r = i / H, kk = i - r * H;
        XS[r * ldl + kk] = r < rv ? hsrc[(long long)r * H + kk] : 0.f;
      }
      __syncthreads();
      head_backward<RG>(XS, ldl, H, hw_c + k * H, 1, sm2 + k, nullptr, rv);
      __syncthreads();
      float* g0 = grad_chain<RG>(a.critic[k], XS, X1, X2, ldl, part + R * 16, hs, nullptr, BH, row0, rv);
      rows_head<RG>(g0, ldl, H, hw_da + k * A * H, H, nullptr, A, EPI_NONE, sm);
      __syncthreads();
      if (tid < R * A) {
        const int r = tid / A, o = tid - r * A;
        if (r < rv) a.dz[((long long)k * B + row0 + r) * a.Apad + o] = sm[r * 16 + o];
      }
      __syncthreads();
    }
  } else if constexpr (ST) {
    // The actor phase in the stream form (rowchain.h WStream; 4 rows per workgroup, walks of two layers or more: rowchain_stream_ok) —
    // the branch below with one weight stream carried through the role's passes: the prologue requests the first stage of the actor's
    // layer 0 with its other requests, every pass requests its successor, and the last pass in front of a head section requests the
    // first pass behind it (actor -> critic layer 0 -> critic's first backward matrix -> actor's first backward matrix).  The whole
    // role runs in a branch of its own per dispatched H: no join of differently compiled passes while the stream is live.
    auto p_role = [&](auto ks_tag) {
      constexpr int KS = decltype(ks_tag)::value;   // H / 4 at H = 64, 128, 256; 0: any other H
      RC_STAMP(0);
      const StepCtrl c = *a.cur_p;
      const float* sa_rows = a.sa + (long long)c.batch_slot * a.slot_x + row0 * a.ldx;
      constexpr int NX = 2 * RG;
      const int jp_s = max(a.actor.jpad0, a.critic[0].jpad0);
      float* hw_a = hw; float* hw_c = hw + A * H; float* hw_da = hw_c + H;
      const float* src_a = a.actor.P + a.actor.w[a.actor.L];
      const float* src_c = a.critic[0].P + a.critic[0].w[a.critic[0].L];
      const float* src_da = a.critic[0].Wt + a.critic[0].wt[0] + (long long)S * H;   // rows S..S+A-1 of W0^T
      Staged<NX> s_s;
      rows_load<RG>(s_s, sa_rows, a.ldx, S, jp_s, rv);
      Staged<8> s_a, s_hc, s_da;
      seg_load(s_a, src_a, A * H);
      seg_load(s_hc, src_c, H);
      seg_load(s_da, src_da, A * H);
      float v_hb = 0.f;
      if (tid < A) v_hb = a.actor.P[a.actor.b[a.actor.L] + tid];
      if (tid == 32) v_hb = a.critic[0].P[a.critic[0].b[a.critic[0].L]];
      WStream<8> ws;
      ws.eb = (v4f){0.f, 0.f, 0.f, 0.f};
      ws.template prime<true>(a.actor.Wt + a.actor.wt[0], H, a.actor.jpad0, H, a.actor.P + a.actor.b[0]);
      const WNext nx_c0 = {a.critic[0].Wt + a.critic[0].wt[0], H, a.critic[0].jpad0, H, a.critic[0].P + a.critic[0].b[0]};   // critic, layer 0
      const WNext nx_cb = {a.critic[0].P + a.critic[0].w[a.critic[0].L - 1], H, H, H, nullptr};                            // critic, first backward matrix
      const WNext nx_ab = {a.actor.P + a.actor.w[a.actor.L - 1], H, H, H, nullptr};                                        // actor, first backward matrix
      const WNext nx_none = {nullptr, 0, 0, 0, nullptr};
      rows_store<RG>(s_s, X0, ldl, sa_rows, a.ldx, S, jp_s, rv);
      seg_store(s_a, hw_a, src_a, A * H);
      seg_store(s_hc, hw_c, src_c, H);
      seg_store(s_da, hw_da, src_da, A * H);
      if (tid < A) hb[tid] = v_hb;
      if (tid == 32) hb[16] = v_hb;
      const bool fuse_q = head_fusable(H);
      if (fuse_q && tid < R) sm2[tid * 16] = (tid < rv) ? -1.0f / (float)B : 0.f;   // d(-mean Q)/dq, constant
      __syncthreads();
      RC_STAMP(1);
      float* h;
      if constexpr (LM) h = mlp_hidden_st<KS, true, TAIL_ANY, true>(ws, a.actor, X0, KP, nullptr, XS, ldl, part + R * 16, a.hA, BH, row0, rv, nx_c0);
      else h = mlp_hidden_st<KS, false, TAIL_ANY, true>(ws, a.actor, X0, X1, X2, XS, ldl, part + R * 16, a.hA, BH, row0, rv, nx_c0);
      RC_STAMP(2);
      rows_head<RG>(h, ldl, H, hw_a, H, hb, A, EPI_TANH, sm);
      __syncthreads();
      if (tid < R * A) { const int r = tid / A, o = tid - r * A; X0[r * ldl + S + o] = sm[r * 16 + o]; }
      __syncthreads();
      RC_STAMP(3);
      if constexpr (LM) h = mlp_hidden_st<KS, true, TAIL_FULL, false>(ws, a.critic[0], X0, KPC, nullptr, X1, ldl, part + R * 16, nullptr, BH, row0, rv, nx_cb);
      else h = mlp_hidden_st<KS, false, TAIL_FULL, false>(ws, a.critic[0], X0, X1, X2, nullptr, ldl, part + R * 16, a.hC2, BH, row0, rv, nx_cb);
      RC_STAMP(4);
      if (fuse_q) {
        head_backward<RG>(h, ldl, H, hw_c, 1, sm2, nullptr, rv, sm3, hb[16]);
        __syncthreads();
        if (tid < rv) a.q2[row0 + tid] = sm3[tid * 16];
      } else {
        rows_head<RG>(h, ldl, H, hw_c, H, hb + 16, 1, EPI_NONE, sm2);
        __syncthreads();
        if (tid < R) {
          if (tid < rv) a.q2[row0 + tid] = sm2[tid * 16];
          sm2[tid * 16] = (tid < rv) ? -1.0f / (float)B : 0.f;   // d(-mean Q)/dq
        }
        __syncthreads();
        head_backward<RG>(h, ldl, H, hw_c, 1, sm2, nullptr, rv);
        __syncthreads();
      }
      RC_STAMP(6);
      float* g0;
      if constexpr (LM) g0 = grad_chain_st<KS, true, TAIL_FULL, false>(ws, a.critic[0], h, X1, X2, ldl, part + R * 16, KPC, nullptr, BH, row0, rv, nx_ab);
      else g0 = grad_chain_st<KS, false, TAIL_FULL, false>(ws, a.critic[0], h, X1, X2, ldl, part + R * 16, a.hC2, nullptr, BH, row0, rv, nx_ab);
      RC_STAMP(7);
      rows_head<RG>(g0, ldl, H, hw_da, H, nullptr, A, EPI_NONE, sm2);
      __syncthreads();
      if (tid < R * A) {
        const int r = tid / A, o = tid - r * A;
        const float act = sm[r * 16 + o];
        const float g = sm2[r * 16 + o] * act_deriv(act, MUL_DTANH);
        sm2[r * 16 + o] = g;
        if (r < rv) a.dz[(row0 + r) * a.Apad + o] = g;
      }
      __syncthreads();
      head_backward<RG>(XS, ldl, H, hw_a, A, sm2, a.gA + (a.actor.L - 1) * BH + row0 * H, rv);
      __syncthreads();
      RC_STAMP(9);
      if constexpr (LM) grad_chain_st<KS, true, TAIL_NONE, false>(ws, a.actor, XS, X1, X2, ldl, part + R * 16, KP, a.gA, BH, row0, rv, nx_none);
      else grad_chain_st<KS, false, TAIL_NONE, false>(ws, a.actor, XS, X1, X2, ldl, part + R * 16, a.hA, a.gA, BH, row0, rv, nx_none);
      RC_STAMP(10);
    };
    if (H == 256) p_role(std::integral_constant<int, 64>{});
    else if (H == 128) p_role(std::integral_constant<int, 32>{});
    else if (H == 64) p_role(std::integral_constant<int, 16>{});
    else p_role(std::integral_constant<int, 0>{});
  } else {
    const StepCtrl c = *a.cur_p;
    const float* sa_rows = a.sa + (long long)c.batch_slot * a.slot_x + row0 * a.ldx;
    constexpr int NX = 2 * RG;
    const int jp_s = max(a.actor.jpad0, a.critic[0].jpad0);
    float* hw_a = hw; float* hw_c = hw + A * H; float* hw_da = hw_c + H;
    const float* src_a = a.actor.P + a.actor.w[a.actor.L];
    const float* src_c = a.critic[0].P + a.critic[0].w[a.critic[0].L];
    const float* src_da = a.critic[0].Wt + a.critic[0].wt[0] + (long long)S * H;   // rows S..S+A-1 of W0^T
    Staged<NX> s_s;
    rows_load<RG>(s_s, sa_rows, a.ldx, S, jp_s, rv);
    Staged<8> s_a, s_hc, s_da;
    seg_load(s_a, src_a, A * H);
    seg_load(s_hc, src_c, H);
    seg_load(s_da, src_da, A * H);
    float v_hb = 0.f;
    if (tid < A) v_hb = a.actor.P[a.actor.b[a.actor.L] + tid];
    if (tid == 32) v_hb = a.critic[0].P[a.critic[0].b[a.critic[0].L]];
    rows_store<RG>(s_s, X0, ldl, sa_rows, a.ldx, S, jp_s, rv);
    seg_store(s_a, hw_a, src_a, A * H);
    seg_store(s_hc, hw_c, src_c, H);
    seg_store(s_da, hw_da, src_da, A * H);
    if (tid < A) hb[tid] = v_hb;
    if (tid == 32) hb[16] = v_hb;
    const bool fuse_q = head_fusable(H);   // Q(s, pi(s)) feeds a metric only: its head pass rides in the head's backward pass (below)
    if (fuse_q && tid < R) sm2[tid * 16] = (tid < rv) ? -1.0f / (float)B : 0.f;   // d(-mean Q)/dq, constant
    __syncthreads();
    // the last actor activation lands in XS and stays there: the critic chain reuses X1 / X2
    float* h;
    if constexpr (LM) h = mlp_hidden_keep<RG>(a.actor, X0, KP, XS, ldl, part + R * 16, a.hA, BH, row0, rv);
    else h = mlp_hidden<RG>(a.actor, X0, X1, X2, ldl, part + R * 16, a.hA, BH, row0, rv, XS);
    rows_head<RG>(h, ldl, H, hw_a, H, hb, A, EPI_TANH, sm);
    __syncthreads();
    if (tid < R * A) { const int r = tid / A, o = tid - r * A; X0[r * ldl + S + o] = sm[r * 16 + o]; }
    __syncthreads();
    // critic on [s | pi(s)]
    if constexpr (LM) h = mlp_hidden_keep<RG>(a.critic[0], X0, KPC, X1, ldl, part + R * 16, nullptr, BH, row0, rv);
    else h = mlp_hidden<RG>(a.critic[0], X0, X1, X2, ldl, part + R * 16, a.hC2, BH, row0, rv);
    if (fuse_q) {
      head_backward<RG>(h, ldl, H, hw_c, 1, sm2, nullptr, rv, sm3, hb[16]);
      __syncthreads();
      if (tid < rv) a.q2[row0 + tid] = sm3[tid * 16];
    } else {
      rows_head<RG>(h, ldl, H, hw_c, H, hb + 16, 1, EPI_NONE, sm2);
      __syncthreads();
      if (tid < R) {
        if (tid < rv) a.q2[row0 + tid] = sm2[tid * 16];
        sm2[tid * 16] = (tid < rv) ? -1.0f / (float)B : 0.f;   // d(-mean Q)/dq
      }
      __syncthreads();
      head_backward<RG>(h, ldl, H, hw_c, 1, sm2, nullptr, rv);
      __syncthreads();
    }
    float* g0;
    if constexpr (LM) g0 = grad_chain_keep<RG>(a.critic[0], h, X1, X2, ldl, part + R * 16, KPC, nullptr, BH, row0, rv);
    else g0 = grad_chain<RG>(a.critic[0], h, X1, X2, ldl, part + R * 16, a.hC2, nullptr, BH, row0, rv);
    // da[r][j] = g0[r][:] . W0[:, S+j]  (row S+j of the [in][out] copy), then through the tanh
    rows_head<RG>(g0, ldl, H, hw_da, H, nullptr, A, EPI_NONE, sm2);
    __syncthreads();
    if (tid < R * A) {
      const int r = tid / A, o = tid - r * A;
      const float act = sm[r * 16 + o];
      const float g = sm2[r * 16 + o] * act_deriv(act, MUL_DTANH);
      sm2[r * 16 + o] = g;
      if (r < rv) a.dz[(row0 + r) * a.Apad + o] = g;
    }
    __syncthreads();
    head_backward<RG>(XS, ldl, H, hw_a, A, sm2, a.gA + (a.actor.L - 1) * BH + row0 * H, rv);
    __syncthreads();
    if constexpr (LM) grad_chain_keep<RG>(a.actor, XS, X1, X2, ldl, part + R * 16, KP, a.gA, BH, row0, rv);
    else grad_chain<RG>(a.actor, XS, X1, X2, ldl, part + R * 16, a.hA, a.gA, BH, row0, rv);
  }
  if (a.clk && tid == 0) atomicMax(&a.clk[1], (unsigned long long)wall_clock64());
