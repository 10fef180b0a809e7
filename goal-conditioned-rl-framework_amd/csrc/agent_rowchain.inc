// agent_rowchain.inc — host side of the row-block path (rowchain.h), included into agent.hip's
// anonymous namespace ahead of the phase builders: both the per-step phases (DDPG Polyak steps,
// TD3) and the software-pipelined DDPG schedule (agent_pipeline.inc) launch through it.

struct PipeCtx {
  const StepCtrl* cur;
  const int* slot;
};


// ---- row-block form (rowchain.h): the forward / input-gradient chains of K and P are ONE launch
// (blocks of 4-16 batch rows walk every layer with the activations resident in LDS), followed by
// one batched launch of all dW|db GEMMs and the optimiser:
//   begin, rowchain[K | P], dW[K | P], Adam pair      = 4 launches per overlapped step
// which: 0 actor, 1 target actor, 2 critic c, 3 target critic c
RowNet make_rownet(gcrl_agent* a, const NetSpec& n, const float* P, int which, int c = 0) {
  RowNet r;
  std::memset(&r, 0, sizeof(r));
  r.P = P;
  r.Wt = a->wt + a->wt_net[which] + (which >= 2 ? c * a->wt_cstride : 0);
  r.in = n.in_dim; r.jpad0 = round_up(n.in_dim, 4); r.H = n.H; r.L = n.L; r.out = n.out_dim;
  long long off = 0;
  for (int l = 0; l <= n.L; ++l) {
    r.w[l] = n.lin[l].w; r.b[l] = n.lin[l].b;
    if (l < n.L) { r.wt[l] = off; off += (long long)(l == 0 ? r.jpad0 : n.H) * n.H; }
  }
  return r;
}

// targets_only: after a Polyak update issued outside the optimiser kernel
int rc_rebuild_wt(gcrl_agent* a, hipStream_t st, bool targets_only = false) {
  auto one = [&](const RowNet& r) { return launch_wt_rebuild(st, r, const_cast<float*>(r.Wt)); };
  if (!targets_only && !a->sac) TRY(one(make_rownet(a, a->actor, a->P_actor(), 0)));
  if (a->has_target_actor) TRY(one(make_rownet(a, a->actor, a->P_tactor(), 1)));
  for (int c = 0; c < a->C; ++c) {
    if (!targets_only) TRY(one(make_rownet(a, a->critic, a->P_critic(c), 2, c)));
    TRY(one(make_rownet(a, a->critic, a->P_tcritic(c), 3, c)));
  }
  if (!targets_only) a->wt_dirty = false;
  return GCRL_OK;
}

int prof_drain(gcrl_agent* a) {
  if (a->prof_used == 0) return GCRL_OK;
  for (int i = 0; i < a->prof_used; ++i) {
    float ms = 0.f;
    GCRL_HIP(hipEventSynchronize(a->prof_b[i]));
    GCRL_HIP(hipEventElapsedTime(&ms, a->prof_a[i], a->prof_b[i]));
    a->prof_ms += ms;
  }
  std::vector<unsigned long long> clk(2 * (size_t)a->prof_used);
  GCRL_HIP(hipMemcpy(clk.data(), a->prof_clk, clk.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (int i = 0; i < a->prof_used; ++i)
    if (clk[2 * i + 1] > clk[2 * i]) a->prof_ticks += (double)(clk[2 * i + 1] - clk[2 * i]);
  a->prof_used = 0;
  return GCRL_OK;
}

// which of the agent's fused DDPG launches (rowchain_ddpg_kernel) take the LDS-multiplier form (rowchain.h): bit 0 a launch of critic-phase
// workgroups only, bit 1 of actor-phase workgroups only, bit 2 the overlapped launch of both; 0: none, or no launch goes through that kernel
int rc_lds_mul_forms(const gcrl_agent* a) {
  if (!a->rowchain || a->sac || a->split_roles || a->rc_global_mul) return 0;
  const long long nblk = (a->B + 4 * a->row_rg - 1) / (4 * a->row_rg), nk = (a->ddpg_ksplit ? 2 : 1) * nblk;
  auto ok = [&](bool actor_phase, long long wgs) { return rowchain_lds_mul_ok(a->row_rg, a->row_ldl, a->A, a->H, a->C, a->L, actor_phase, wgs); };
  const bool k_fused = !a->split_k;   // (TD3's split critic phase runs in the role-parallel kernels)
  return ((k_fused && ok(false, nk)) ? 1 : 0) | (ok(true, nblk) ? 2 : 0) | ((k_fused && ok(true, nk + nblk)) ? 4 : 0);
}

// whether the agent's fused DDPG launches take the stream form of their chained passes (rowchain.h rowchain_stream_ok, in the agent's terms)
bool rc_stream_form(const gcrl_agent* a) {
  return a->rowchain && !a->sac && !a->split_roles && !a->split_k && !a->rc_no_stream && a->cfg.kind == GCRL_AGENT_DDPG && a->row_rg == 1 &&
         a->C == 1 && a->H <= kRowChunk && a->L >= 2;
}

// L2-warming rider workgroups of the agent's fused DDPG launches (rowchain.hip rc_warm_rider): the stream form's launches only, and only
// where a launch of `wgs` role workgroups leaves them CUs of their own (the two-role admission's count, one workgroup per CU); 0: none.
// They wait for nothing, so meetings being off or the device being shared does not take them away.  GCRL_RC_NO_WARM=1 at creation: none.
// The count is against the CUs (n_cus, as the two-role admission 3 * nblk <= n_cus counts), not against meet_capacity: riders carry the launch's
// last indices and wait for nobody, so nothing depends on their being resident — the rule only keeps them off CUs that hold a role workgroup.
int rc_warm_riders(const gcrl_agent* a, long long wgs) {
  if (!rc_stream_form(a) || a->rc_warm <= 0) return 0;
  return wgs + a->rc_warm <= std::max(a->n_cus, 1) ? a->rc_warm : 0;
}

// SAC on the role-parallel row-chain launches: the BatchNorm actor's heads and its sampling run inside them (rowchain.h HeadsFold)
bool heads_fold_on(const gcrl_agent* a) {
  return a->rowchain && a->cfg.kind == GCRL_AGENT_SAC && a->split_roles && a->slab_on() && !a->heads_fold_off && a->A <= 16 && a->bn_sync.world <= 1;
}

int rc_launch_chain(gcrl_agent* a, hipStream_t st, const PipeCtx& k, const PipeCtx& p, int what, const float* noise = nullptr) {
  RowChainArgs rc;
  std::memset(&rc, 0, sizeof(rc));
  rc.cur_k = k.cur; rc.cur_p = p.cur; rc.cb = a->ctrl();
  rc.actor = make_rownet(a, a->actor, a->P_actor(), 0);
  rc.tactor = make_rownet(a, a->actor, a->P_tactor(), 1);
  rc.C = a->C;
  for (int c = 0; c < a->C; ++c) {
    rc.critic[c] = make_rownet(a, a->critic, a->P_critic(c), 2, c);
    rc.tcritic[c] = make_rownet(a, a->critic, a->P_tcritic(c), 3, c);
  }
  const bool td3 = a->cfg.kind == GCRL_AGENT_TD3;
  rc.target_kind = a->sac ? TGT_MIN_ENT : (td3 ? TGT_MIN : TGT_DDPG);
  rc.loss_kind = td3 ? LOSS_SMOOTH_L1 : LOSS_MSE;
  if (a->sac) {   // the BatchNorm actor runs outside the row-block kernel
    rc.given_next = 1; rc.p_critic_only = 1;
    rc.logp_next = a->logp_next; rc.alpha = 0.2f;   // SAC: literal 0.2 (src/agent.py:569)
    rc.pi = a->pi_buf;
  }
  rc.noise = noise; rc.policy_noise = (float)a->cfg.policy_noise; rc.noise_clamp = (float)a->cfg.noise_clamp;
  rc.seed = a->cfg.seed;
  rc.sa = a->sa; rc.nsa = a->nsa; rc.rbuf = a->rbuf; rc.dbuf = a->dbuf;
  rc.slot_x = a->slot_x; rc.slot_rd = a->slot_rd;
  rc.ldx = a->ldx; rc.ldl = a->row_ldl; rc.B = a->B; rc.S = a->S; rc.A = a->A; rc.Apad = a->Apad;
  const int nblk = (a->B + 4 * a->row_rg - 1) / (4 * a->row_rg);
  // (roles in launch order.  By XCD, K on XCDs 0-3 and P on 4-7: HBM-side traffic 32.3 -> 23.4 MB but the step 56.03 -> 56.53 us, round 4)
  rc.nblk_k = (what & 1) ? nblk : 0;
  rc.nblk_p = (what & 2) ? nblk : 0;
  rc.hC = a->hC; rc.gC = a->rc_gC; rc.q = a->q; rc.y = a->ybuf; rc.dq = a->dq;
  rc.hA = a->hA; rc.gA = a->rc_gA; rc.hC2 = a->hC2; rc.q2 = a->q2; rc.dz = a->dact;
  rc.gamma = (float)a->cfg.gamma;
  rc.clamp_lo = (float)(-1.0 / (1.0 - a->cfg.gamma));
  rc.qt = a->qt;
  rc.reserved0 = rc_warm_riders(a, (long long)((a->ddpg_ksplit && (what & 1)) ? 2 : 1) * rc.nblk_k + rc.nblk_p);
  if (a->split_roles) {
    // twin critics at a latency-bound batch size: each network's chain in its own workgroups (rowchain.h)
    HeadsFold hfold;
    std::memset(&hfold, 0, sizeof(hfold));
    if (heads_fold_on(a)) {
      const NetSpec& an = a->actor;
      const long long BH = (long long)a->B * a->H;
      hfold.on = 1;
      hfold.P = a->P_actor();
      hfold.w_mean = an.lin[an.L].w; hfold.b_mean = an.lin[an.L].b; hfold.w_ls = an.lin[an.L + 1].w; hfold.b_ls = an.lin[an.L + 1].b;
      hfold.h_next = a->hN + (long long)((an.L - 1) & 1) * BH;     // (the no-grad pass keeps two ping-pong buffers: sac_actor_forward_multi hbuf)
      hfold.h_cur = a->hA + (long long)(an.L - 1) * BH;
      hfold.eps_next = a->hf_eps_next; hfold.eps_cur = a->hf_eps_cur;
      hfold.logp_next = a->logp_next;
      hfold.pi = a->pi_buf; hfold.logp = a->logp; hfold.save_eps = a->epsbuf; hfold.save_std = a->stdbuf; hfold.head = a->headA;
      if (what & 1) {   // (field by field into the zeroed record: a temporary's padding would reach the population's content-keyed table cache)
        BnRunning& r = hfold.run;
        r.bstat[0] = a->bn_bstat; r.bstat[1] = a->hf_nf == 2 ? a->bn_bstat + (long long)an.L * 2 * a->H : nullptr;
        r.n = a->hf_nf; r.rmean = a->bn_rmean; r.rvar = a->bn_rvar; r.layers = an.L; r.H = a->H; r.B = a->B;
      }
    }
    // actor steps: pi(s) by the critic phase's online roles (rowchain.h cur_in_k; GCRL_HEADS_CUR_IN_P=1: by the actor phase's critic roles)
    static const bool cur_in_p = std::getenv("GCRL_HEADS_CUR_IN_P") != nullptr;
    hfold.cur_in_k = (hfold.on && a->hf_nf == 2 && !cur_in_p) ? 1 : 0;
    const HeadsFold* hfp = hfold.on ? &hfold : nullptr;
    const HeadsFold* hfp_p = (hfold.on && !hfold.cur_in_k) ? &hfold : nullptr;   // phase 1 runs on the stored pi otherwise
    if (a->rc_merge) {   // forward and backward parts of a phase in ONE launch: the role workgroups of a row block meet inside it (rowchain.h)
      rc.bar = reinterpret_cast<unsigned int*>(a->rc_bar); rc.status = a->status_dev;
      if (what & 1) TRY(launch_rowchain_split(st, rc, a->row_rg, 0, 3, hfp));
      if (what & 2) TRY(launch_rowchain_split(st, rc, a->row_rg, 1, 3, hfp_p));
      return GCRL_OK;
    }
    if (what & 1) { TRY(launch_rowchain_split(st, rc, a->row_rg, 0, 1, hfp)); TRY(launch_rowchain_split(st, rc, a->row_rg, 0, 2)); }
    if (what & 2) { TRY(launch_rowchain_split(st, rc, a->row_rg, 1, 1, hfp_p)); TRY(launch_rowchain_split(st, rc, a->row_rg, 1, 2)); }
    return GCRL_OK;
  }
  if (a->split_k) {
    // TD3 at a chip-filling batch: the critic phase's four networks in their own workgroups — not for parallelism
    // (every CU already has a workgroup) but for two resident workgroups per CU: two waves per SIMD lift the measured
    // 4x4x1 MFMA issue ceiling from 89 to 114 TFLOP/s (profiles/r02_mfma_issue_ceiling.txt).  The actor phase keeps the fused kernel.
    if ((what & 1) && a->rc_merge_k) {
      rc.bar = reinterpret_cast<unsigned int*>(a->rc_bar); rc.status = a->status_dev; rc.producers_first = 1;
      TRY(launch_rowchain_split(st, rc, a->row_rg, 0, 3));
    } else if (what & 1) { TRY(launch_rowchain_split(st, rc, a->row_rg, 0, 1)); TRY(launch_rowchain_split(st, rc, a->row_rg, 0, 2)); }
    if (what & 2) { rc.nblk_k = 0; TRY(launch_rowchain_ddpg(st, rc, a->row_rg, !a->rc_global_mul, !a->rc_no_stream)); }
    return GCRL_OK;
  }
  if (a->ddpg_ksplit && (what & 1)) {   // the critic phase as two roles of the fused launch (rowchain.hip: k_split)
    rc.k_split = 1; rc.producers_first = 1;
    rc.bar = reinterpret_cast<unsigned int*>(a->rc_bar); rc.status = a->status_dev;
  }
  if (!a->prof || what != 3) return launch_rowchain_ddpg(st, rc, a->row_rg, !a->rc_global_mul, !a->rc_no_stream);
  // measurement mode (never inside a graph capture): the overlapped launch, bracketed
  if (a->prof_used == gcrl_agent::kProfPairs) TRY(prof_drain(a));
  const unsigned long long init[2] = {~0ull, 0ull};
  rc.clk = a->prof_clk + 2 * a->prof_used;
  GCRL_HIP(hipMemcpyAsync(rc.clk, init, sizeof(init), hipMemcpyHostToDevice, st));
  GCRL_HIP(hipEventRecord(a->prof_a[a->prof_used], st));
  TRY(launch_rowchain_ddpg(st, rc, a->row_rg, !a->rc_global_mul, !a->rc_no_stream));
  GCRL_HIP(hipEventRecord(a->prof_b[a->prof_used], st));
  a->prof_used++;
  a->prof_launches++;
  return GCRL_OK;
}

// all dW|db problems of a phase in one launch index (critic: every critic of the K role)
void rc_add_dw(gcrl_agent* a, Launches& ls, const PipeCtx& c, bool critic, bool fused) {
  const int B = a->B, L = a->L, H = a->H;
  const NetSpec& net = critic ? a->critic : a->actor;
  const long long BH = (long long)B * H;
  for (int k = 0; k < (critic ? a->C : 1); ++k) {
    float* Gp = critic ? a->G_critic(k) : a->G_actor();
    const float* hid = critic ? a->hC + (long long)k * L * BH : a->hA;
    const float* gr = critic ? a->rc_gC + (long long)k * L * BH : a->rc_gA;
    const float* x0 = a->sa;   // the actor's first layer reads the s columns of the same rows
    for (int l = L; l >= 0; --l) {
      const float* G = l == L ? (critic ? a->dq + (long long)k * B : a->dact) : gr + (long long)l * BH;
      const long long ldg = l == L ? (critic ? 1 : a->Apad) : H;
      GemmDesc dw = bwd_dw(G, ldg, l == 0 ? x0 : hid + (long long)(l - 1) * BH, l == 0 ? a->ldx : H, Gp, net.lin[l], B);
      if (l == 0) { dw.slot = c.slot; dw.b_slot = a->slot_x; }
      if (fused) dw.sumsq_out = critic ? a->parts_c + (long long)k * a->nparts_c + a->part_off_c[l] : a->parts_a + a->part_off_a[l];
      dw_split_form(a, dw, critic ? k : -1, l);
      ls.add(0, dw);
    }
  }
}

// extras of the optimiser launches on the row-block path: [in][out] copies (and the Polyak
// destination's), TD metrics of the critic step
void rc_adam_extras(gcrl_agent* a, AdamArgs& ad, bool critic) {
  const NetSpec& net = critic ? a->critic : a->actor;
  ad.wt = a->wt + a->wt_net[critic ? 2 : 0];
  ad.wt_target = a->wt + a->wt_net[critic ? 3 : 1];
  ad.wt_net_stride = critic ? a->wt_cstride : 0;
  // segment table: hidden-layer weights as 16x16 tiles (their [in][out] copies get written through an
  // LDS transpose), everything between them (biases, head) as flat 256-element chunks
  ad.n_seg = 0;
  int blk = 0;
  long long pos = 0, off = 0;
  auto flat = [&](long long beg, long long end) {
    if (end <= beg) return;
    AdamSeg& s = ad.seg[ad.n_seg++];
    s.beg = beg; s.dst = 0; s.rows = 1; s.cols = (int)(end - beg); s.tiled = 0; s.pad = 0;
    s.blk0 = blk; s.nblk = (int)((end - beg + 256 * kAdamPerThread - 1) / (256 * kAdamPerThread)); blk += s.nblk;
  };
  for (int l = 0; l < net.L; ++l) {
    const Lin& ln = net.lin[l];
    flat(pos, ln.w);
    AdamSeg& s = ad.seg[ad.n_seg++];
    s.beg = ln.w; s.dst = off; s.rows = ln.out; s.cols = ln.in; s.tiled = 1; s.pad = 0;
    s.blk0 = blk; s.nblk = ((ln.out + kAdamTile - 1) / kAdamTile) * ((ln.in + kAdamTile - 1) / kAdamTile); blk += s.nblk;
    pos = ln.w + (long long)ln.out * ln.in;
    off += (long long)(l == 0 ? round_up(net.in_dim, 4) : net.H) * net.H;
  }
  flat(pos, net.numel);
  ad.seg_blocks = blk;
  if (critic) {
    ad.td_q = a->q; ad.td_y = a->ybuf; ad.td_n = a->B; ad.td_C = a->C;
    ad.td_loss_kind = a->cfg.kind == GCRL_AGENT_TD3 ? LOSS_SMOOTH_L1 : LOSS_MSE;
  }
}

// ---- the dW | db problems, the clip and the optimiser step of a phase's net(s) as ONE launch (dw_adam.hip; round 5).
// net: critic k (critic = true) or the actor.  `cur`: the control record's COPY (cur_b / prev_b, refreshed by the row-chain
// launch in front): the launch may advance the originals, so nothing in it — the first layers' batch-slot lookups included —
// reads them.  Same problems, in the same order, as rc_add_dw; same optimiser arguments as pipe_adam_*_args + rc_adam_extras.
void of_fill_net(gcrl_agent* a, DwAdamNet& n, bool critic, int k, const StepCtrl* cur, bool polyak) {
  const int B = a->B, L = a->L, H = a->H;
  const NetSpec& net = critic ? a->critic : a->actor;
  const long long BH = (long long)B * H;
  std::memset(&n, 0, sizeof(n));
  float* Gp = critic ? a->G_critic(k) : a->G_actor();
  const float* hid = critic ? a->hC + (long long)k * L * BH : a->hA;
  const float* gr = critic ? a->rc_gC + (long long)k * L * BH : a->rc_gA;
  const std::vector<int>& poff = critic ? a->part_off_c : a->part_off_a;
  std::vector<long long> wt_off((size_t)L + 1, -1);
  long long off = 0;
  for (int l = 0; l < L; ++l) { wt_off[l] = off; off += (long long)(l == 0 ? round_up(net.in_dim, 4) : H) * H; }
  int q = 0;
  for (int l = L; l >= 0; --l, ++q) {
    const float* G = l == L ? (critic ? a->dq + (long long)k * B : a->dact) : gr + (long long)l * BH;
    const long long ldg = l == L ? (critic ? 1 : a->Apad) : H;
    GemmDesc dw = bwd_dw(G, ldg, l == 0 ? a->sa : hid + (long long)(l - 1) * BH, l == 0 ? a->ldx : H, Gp, net.lin[l], B);
    if (l == 0) { dw.slot = &cur->batch_slot; dw.b_slot = a->slot_x; }
    n.d[q] = dw;
    n.o.lay[q] = DwAdamLayer{net.lin[l].w, net.lin[l].b, wt_off[l], poff[l] / 4, 0};
  }
  n.o.nl = L + 1;
  n.o.cur = cur;
  n.o.which = critic ? 1 : 0;
  const long long go = critic ? a->goff_critic + (long long)k * a->critic_stride : a->goff_actor;
  n.o.p = critic ? a->P_critic(k) : a->P_actor();
  n.o.m = a->adam_m + go; n.o.v = a->adam_v + go;
  n.o.target = critic ? a->P_tcritic(k) : (polyak ? a->P_tactor() : nullptr);
  n.o.wt = a->wt + a->wt_net[critic ? 2 : 0] + (critic ? (long long)k * a->wt_cstride : 0);
  n.o.wt_target = a->wt + a->wt_net[critic ? 3 : 1] + (critic ? (long long)k * a->wt_cstride : 0);
  n.o.clip = (critic && k == 0 && a->cfg.kind == GCRL_AGENT_TD3) ? -1.f : (float)a->cfg.grad_clip;   // TD3's critic_1 is not clipped (src/agent.py:201)
  n.o.polyak = polyak ? 1 : 0;
  n.o.metric_index = critic ? MET_CRITIC_GRAD + k : MET_ACTOR_GRAD;
  const int ni = critic ? k : a->C;
  n.o.slots = reinterpret_cast<unsigned long long*>(a->of_slots) + (long long)ni * 2 * a->of_stride;
  n.o.slot_stride = (int)a->of_stride;
  n.o.seq = reinterpret_cast<unsigned int*>(a->of_seq) + ni * 32;
  if (critic) {
    if (k == 0) {
      n.o.td_q = a->q; n.o.td_y = a->ybuf; n.o.td_n = a->B; n.o.td_C = a->C;
      n.o.td_loss_kind = a->cfg.kind == GCRL_AGENT_TD3 ? LOSS_SMOOTH_L1 : LOSS_MSE;
    }
  } else {
    n.o.mean_x = a->q2; n.o.mean_n = a->B; n.o.mean_scale = -1.0f; n.o.mean_index = MET_ACTOR_LOSS;   // -Q.mean()
  }
}

void of_common(gcrl_agent* a, DwAdamArgs& da) {
  std::memset(&da, 0, sizeof(da));
  da.beta2 = (float)kBeta2; da.w1 = (float)(1.0 - kBeta1); da.w2 = (float)(1.0 - kBeta2); da.eps = (float)kAdamEps;
  da.tau = (float)a->cfg.tau; da.one_m_tau = (float)(1.0 - a->cfg.tau);
  da.metrics = a->metrics_dev;
  da.status = a->status_dev;
}

// TD3 / SAC on the row-chain path (per-step phases, agent.hip): every critic's dW | db + clip + AdamW (+ Polyak) in ONE launch at the
// end of phase 0 (src/agent.py:199-222, :583-606), and — TD3 — the actor's at the end of phase 1 (:149-162).  The step's control
// record is read from its copy; `adv`: this is the step's last launch and advances the original for the next step.
bool of_phase_critics(const gcrl_agent* a, int variant) {
  return a->opt_fuse && a->cfg.kind != GCRL_AGENT_DDPG && (variant & V_FUSED_NORM) && !(variant & V_XCHG) && !(variant & V_WEIGHTS);
}
bool of_phase_actor(const gcrl_agent* a, int variant) { return of_phase_critics(a, variant) && !a->sac; }
int of_launch_critics(gcrl_agent* a, hipStream_t st, int variant) {
  DwAdamArgs da;
  of_common(a, da);
  for (int k = 0; k < a->C; ++k) of_fill_net(a, da.net[k], true, k, &a->ctrl()->cur_b, (variant & V_POLYAK_C) != 0);
  da.nnets = a->C;
  if ((variant & V_ADV) && !(variant & V_ACTOR)) da.advance = a->ctrl();
  return launch_dw_adam(st, da);
}
int of_launch_actor(gcrl_agent* a, hipStream_t st, int variant) {
  DwAdamArgs da;
  of_common(a, da);
  of_fill_net(a, da.net[0], false, 0, &a->ctrl()->cur_b, a->cfg.kind == GCRL_AGENT_TD3 && (variant & V_POLYAK_A) != 0);
  da.nnets = 1;
  if (variant & V_ADV) da.advance = a->ctrl();
  return launch_dw_adam(st, da);
}

// what: 1 = the critic phase's net, 2 = the actor phase's, 3 = both (the overlapped step: critic of step i+1 | actor of step i)
int of_launch_ddpg(gcrl_agent* a, hipStream_t st, int what, bool adv, bool polyak) {
  DwAdamArgs da;
  of_common(a, da);
  int n = 0;
  if (what & 1) of_fill_net(a, da.net[n++], true, 0, &a->ctrl()->cur_b, polyak);
  if (what & 2) of_fill_net(a, da.net[n++], false, 0, what == 3 ? &a->ctrl()->prev_b : &a->ctrl()->cur_b, polyak);
  da.nnets = n;
  if (adv) da.advance = a->ctrl();   // (what & 1 always holds then: net 0 is the critic, as in adam_pair_kernel)
#ifdef GCRL_OF_STAMPS
  // development build: the merged launches number GCRL_OF_STAMPS_AT .. +7 leave their per-workgroup clock stamps in the file GCRL_OF_STAMPS
  static unsigned long long* stamps = nullptr;
  static long long launches = 0;
  static const long long at = std::getenv("GCRL_OF_STAMPS_AT") ? std::atoll(std::getenv("GCRL_OF_STAMPS_AT")) : 3000;
  const char* path = std::getenv("GCRL_OF_STAMPS");
  if (path && !stamps) { GCRL_HIP(hipMalloc((void**)&stamps, 2 * 2048 * 8 * sizeof(unsigned long long))); }
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cs);
  const bool take = path && what == 3 && cs == hipStreamCaptureStatusNone && launches >= at && launches < at + 8;
  if (what == 3 && cs == hipStreamCaptureStatusNone) ++launches;
  da.stamps = take ? stamps : nullptr;
  if (take) {
    GCRL_HIP(hipMemsetAsync(stamps, 0, 2 * 2048 * 8 * sizeof(unsigned long long), st));
    TRY(launch_dw_adam(st, da));
    GCRL_HIP(hipStreamSynchronize(st));
    std::vector<unsigned long long> h(2 * 2048 * 8);
    GCRL_HIP(hipMemcpy(h.data(), stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    FILE* f = std::fopen(path, launches - 1 == at ? "wb" : "ab");
    if (f) { std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f); std::fclose(f); }
    return GCRL_OK;
  }
#endif
  return launch_dw_adam(st, da);
}

