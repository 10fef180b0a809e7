// agent_pipeline.inc — software-pipelined DDPG steps (included into agent.hip's anonymous
// namespace).
//
// In DDPG the critic phase K of step i+1 (target actor/critic pass, online critic pass, TD loss,
// critic backward, critic Adam) reads the TARGET actor, not the actor that step i's actor phase P
// (actor forward, critic forward/backward through the stepped critic, actor backward, actor Adam)
// is updating (reference src/agent.py:1311-1317 vs :1288-1300).  P(i) and K(i+1) are therefore
// independent except for one ordering constraint — K(i+1)'s optimiser step may overwrite the
// critic only after P(i) has finished reading it — and, on Polyak steps (step % 40 == 0), the
// target-actor update, where the pair is simply not overlapped.
//
// A step is launch/latency-bound at B=256 (1.8 us launch floor + ~2 us of dependent memory round
// trips per GEMM launch, 4 TFLOP/s of 157), and independent hipGraph branches do NOT run
// concurrently on this runtime (measured: two parallel 16-GEMM chains take as long as 32 in a
// row).  So the overlap is done by CO-SCHEDULING: launch j of P(i) and launch j of K(i+1) are one
// batched-GEMM launch (more tiles, same latency):
//
//   begin(shift)      prev <- cur (step i), cur <- table[..] (step i+1)
//   2L+2 launches     [target-actor l | critic l]  then [target-critic l]   +  [actor l] then [critic' l]
//   td_loss           K
//   L+1 launches      K critic backward (dW|db, dX)                         +  P critic' input-gradient
//   L+1 launches      P actor backward (dW|db, dX)
//   Adam pair         K critic (after P's last read of the critic parameters) and P actor, one launch
//
// = 3L+7 launches (16 at L=3) instead of 6L+13 (31) for the two phases run back to back.  The
// arithmetic of each step is untouched (same kernels, same operands, same order inside a chain),
// so update_many stays bitwise equal to repeated update() — tests/test_gpu_parity.py checks it.
//
// How a call's steps reach the GPU (run_steps_ddpg): at the default use_graph = 1 the row-block path issues PLAIN launches
// (graph_on(), agent.hip) — two per overlapped step, no graph launch anywhere in the call.  Measured (round 17,
// profiles/r17_trace_gaps_ddpg_parent.txt): with the host ahead, plain launches follow each other with 0.0 us of idle GPU, the
// same as kernels inside a graph, while every graph launch idles the GPU for 8.3-8.8 us; the graph pieces below (use_graph = 2)
// therefore cannot beat the plain form, however few they are.  The call's idle time sat in front of the main gather instead
// (finish_deferred_draw, agent.hip).

// forward launches of K: [TA l | C l] at l = 0..L, [TC l] at L+1..2L+1
void pipe_add_K_fwd(gcrl_agent* a, Launches& f, const PipeCtx& k) {
  const int B = a->B, S = a->S, L = a->L;
  chain_mlp(a, f, 0, a->critic, a->P_critic(0), a->sa, a->ldx, a->slot_x, hid_C, 0, a->q, 1, 0, EPI_NONE, B, k.slot);
  chain_mlp(a, f, 0, a->actor, a->P_tactor(), a->nsa, a->ldx, a->slot_x, hid_TA, 0, a->nsa + S, a->ldx, a->slot_x, EPI_TANH, B, k.slot);
  chain_mlp(a, f, (size_t)L + 1, a->critic, a->P_tcritic(0), a->nsa, a->ldx, a->slot_x, hid_TC, 0, a->qt, 1, 0, EPI_NONE, B, k.slot);
}

// forward launches of P: [A l] at 0..L, [C' l] at L+1..2L+1 (critic 0 on [s | pi(s)], own buffers)
void pipe_add_P_fwd(gcrl_agent* a, Launches& f, const PipeCtx& p) {
  const int B = a->B, S = a->S, L = a->L;
  chain_mlp(a, f, 0, a->actor, a->P_actor(), a->spa, a->ldx, a->slot_x, hid_A, 0, a->spa + S, a->ldx, a->slot_x, EPI_TANH, B, p.slot);
  chain_mlp(a, f, (size_t)L + 1, a->critic, a->P_critic(0), a->spa, a->ldx, a->slot_x, hid_C2, 0, a->q2, 1, 0, EPI_NONE, B, p.slot);
}

int pipe_td_loss(gcrl_agent* a, hipStream_t st, const PipeCtx& k) {
  TdLossArgs td;
  std::memset(&td, 0, sizeof(td));
  td.cur = k.cur;
  td.r = a->rbuf; td.d = a->dbuf; td.slot_stride = a->slot_rd;
  td.qt = a->qt; td.q = a->q; td.dq = a->dq;
  td.metrics = a->metrics_dev;
  td.B = a->B; td.C = 1; td.drop = 0;
  td.gamma = (float)a->cfg.gamma;
  td.loss_kind = LOSS_MSE;
  td.target_kind = TGT_DDPG;
  td.clamp_lo = (float)(-1.0 / (1.0 - a->cfg.gamma));
  return launch_td_loss(st, td);
}

// K critic backward, layer L..0 at launches 0..L (fused-norm partials)
void pipe_add_K_bwd(gcrl_agent* a, Launches& bw, const PipeCtx& k, bool fused) {
  const int B = a->B, L = a->L, H = a->H;
  float* Gp = a->G_critic(0);
  const float* P = a->P_critic(0);
  for (int l = L; l >= 0; --l) {
    const size_t at = (size_t)(L - l);
    const float* G = l == L ? a->dq : a->gC_at(0, l & 1);
    const long long ldg = l == L ? 1 : H;
    GemmDesc dw = bwd_dw(G, ldg, l == 0 ? a->sa : a->hC_at(0, l - 1), l == 0 ? a->ldx : H, Gp, a->critic.lin[l], B);
    if (l == 0) { dw.slot = k.slot; dw.b_slot = a->slot_x; }
    if (fused) dw.sumsq_out = a->parts_c + a->part_off_c[l];
    bw.add(at, dw);
    if (l > 0) bw.add(at, bwd_dx(G, ldg, P, a->critic.lin[l], 0, H, a->gC_at(0, (l - 1) & 1), H, B, MUL_DLEAKY, a->hC_at(0, l - 1), H));
  }
}

// P: input gradient of critic 0 down to the action columns, layer L..0 at launches 0..L
void pipe_add_P_c2bwd(gcrl_agent* a, Launches& bw, const PipeCtx& p) {
  const int B = a->B, L = a->L, H = a->H, S = a->S, A = a->A;
  const float* P = a->P_critic(0);
  for (int l = L; l >= 1; --l) {
    const float* G = l == L ? a->dq2 : a->gC2_at(l & 1);
    bw.add((size_t)(L - l), bwd_dx(G, l == L ? 1 : H, P, a->critic.lin[l], 0, H, a->gC2_at((l - 1) & 1), H, B, MUL_DLEAKY, a->hC2_at(l - 1), H));
  }
  GemmDesc d0 = bwd_dx(a->gC2_at(0), H, P, a->critic.lin[0], S, A, a->dact, a->Apad, B, MUL_DTANH, a->spa + S, a->ldx);
  d0.slot = p.slot; d0.h_slot = a->slot_x;
  bw.add((size_t)L, d0);
}

void pipe_add_P_abwd(gcrl_agent* a, Launches& ab, const PipeCtx& p, bool fused) {
  const int B = a->B, L = a->L, H = a->H;
  float* Ga = a->G_actor();
  const float* Pa = a->P_actor();
  for (int l = L; l >= 0; --l) {
    const size_t at = (size_t)(L - l);
    const float* G = l == L ? a->dact : a->gA[l & 1];
    const long long ldg = l == L ? a->Apad : H;
    GemmDesc dw = bwd_dw(G, ldg, l == 0 ? a->spa : a->hA_at(l - 1), l == 0 ? a->ldx : H, Ga, a->actor.lin[l], B);
    if (l == 0) { dw.slot = p.slot; dw.b_slot = a->slot_x; }
    if (fused) dw.sumsq_out = a->parts_a + a->part_off_a[l];
    ab.add(at, dw);
    if (l > 0) ab.add(at, bwd_dx(G, ldg, Pa, a->actor.lin[l], 0, H, a->gA[(l - 1) & 1], H, B, MUL_DLEAKY, a->hA_at(l - 1), H));
  }
}

void pipe_adam_critic_args(gcrl_agent* a, const PipeCtx& k, AdamArgs& ad, bool fused) {
  std::memset(&ad, 0, sizeof(ad));
  adam_common(a, ad);   // default partial source: norm_partial[0..64) from the sumsq kernel
  ad.cur = k.cur;
  if (fused) { ad.partial = a->parts_c; ad.nparts = a->nparts_c; ad.part_stride = a->nparts_c; }
  ad.which = 1;
  ad.p = a->P_critic(0); ad.g = a->G_critic(0);
  ad.m = a->adam_m + a->goff_critic; ad.v = a->adam_v + a->goff_critic;
  ad.target = a->P_tcritic(0);
  ad.n = a->critic.numel; ad.net_stride = a->critic_stride; ad.nets = 1;
  for (int c = 0; c < kMaxCritics; ++c) ad.clip[c] = (float)a->cfg.grad_clip;
  ad.polyak = 0;  // (PIPE_POLYAK turns it on for the overlapped step whose critic phase is a Polyak step)
  ad.metric_index = MET_CRITIC_GRAD;
}

void pipe_adam_actor_args(gcrl_agent* a, const PipeCtx& p, AdamArgs& ad, bool fused) {
  std::memset(&ad, 0, sizeof(ad));
  adam_common(a, ad);
  ad.cur = p.cur;
  if (fused) { ad.partial = a->parts_a; ad.nparts = a->nparts_a; ad.part_stride = a->nparts_a; }
  else ad.partial = a->norm_partial + kNormBlocks;   // the actor's slot of the unfused pair
  ad.which = 0;
  ad.p = a->P_actor(); ad.g = a->G_actor();
  ad.m = a->adam_m + a->goff_actor; ad.v = a->adam_v + a->goff_actor;
  ad.n = a->actor.numel; ad.net_stride = 0; ad.nets = 1;
  for (int c = 0; c < kMaxCritics; ++c) ad.clip[c] = (float)a->cfg.grad_clip;
  ad.metric_index = MET_ACTOR_GRAD;
  ad.mean_x = a->q2; ad.mean_n = a->B; ad.mean_scale = -1.0f; ad.mean_index = MET_ACTOR_LOSS;  // -Q.mean()
}

// what: 1 = K only (with a plain begin), 2 = P only (reads `cur`: the step K just ran for),
//       3 = P(prev) || K(cur) overlapped (begin with shift)
// seg:  -1 = the whole thing, gradient-norm partials fused into the dW epilogues (single GPU);
//        0 = everything up to the gradients, 1 = norm + optimiser step(s): data-parallel runs
//        all-reduce the gradient block between the two (ONE exchange per overlapped step: the
//        critic gradients of K(i+1) and the actor gradients of P(i) are adjacent in memory)
// flags (in `what`, above the two phase bits):
//   PIPE_PRE  cur/prev were already advanced by the previous segment's optimiser kernel: no begin launch
//   PIPE_ADV  this segment's optimiser kernel advances them for the next one (which must be P||K)
//   PIPE_POLYAK  the segment's critic phase K belongs to a Polyak step (step % 40 == 0, row-block path): the
//             reference updates BOTH targets between that step's critic update and its actor update
//             (src/agent.py:1397-1401), i.e. right where the overlapped step P(s-1) || K(s) runs its
//             optimiser launch: target critic <- critic just stepped, target actor <- actor just stepped by
//             P(s-1) (the actor that step s's actor update will start from).  K(s+1) then reads the new
//             targets, P(s) does not care: Polyak steps stay inside the overlapped schedule at no extra launch.
enum { PIPE_PRE = 4, PIPE_ADV = 8, PIPE_POLYAK = 16 };

int enqueue_ddpg_pipe(gcrl_agent* a, hipStream_t st, int what_flags, int seg) {
  const int what = what_flags & 3;
  const bool pre = (what_flags & PIPE_PRE) != 0, adv = (what_flags & PIPE_ADV) != 0;
  const bool polyak = (what_flags & PIPE_POLYAK) != 0;
  const PipeCtx kc{a->cur(), &a->ctrl()->cur.batch_slot};
  const PipeCtx pc = what == 3 ? PipeCtx{a->prev(), &a->ctrl()->prev.batch_slot} : kc;
  const bool xc = seg < 0 && a->xchg != nullptr;   // whole segments issued by the update entry points: the exchange is a launch of the sequence
  const bool fused = seg < 0 && !xc;
  if (seg <= 0 && a->rowchain) {
    if ((what & 1) && !pre) TRY(launch_begin_step(st, a->ctrl(), what == 3 ? 1 : 0));
    TRY(rc_launch_chain(a, st, kc, pc, what));
    // dW | db, clip, optimiser, Polyak, weight copies, metrics and the control advance as ONE launch (dw_adam.hip) — not
    // under data parallelism (the exchange sits between the gradients and the step) and not while measuring the chain launch
    if (fused && a->opt_fuse) return of_launch_ddpg(a, st, what, adv, polyak);
    Launches dw;
    if (what & 1) rc_add_dw(a, dw, kc, true, fused);
    if (what & 2) rc_add_dw(a, dw, pc, false, fused);
    TRY(dw.run(st));
    if (xc) TRY(xchg_launch(a, st, what));   // ONE exchange per overlapped step: critic | actor are adjacent segments
    if (seg == 0) return GCRL_OK;
  } else if (seg <= 0) {
    if ((what & 1) && !pre) TRY(launch_begin_step(st, a->ctrl(), what == 3 ? 1 : 0));
    Launches f;
    if (what & 1) pipe_add_K_fwd(a, f, kc);
    if (what & 2) pipe_add_P_fwd(a, f, pc);
    TRY(f.run(st));
    if (what & 1) TRY(pipe_td_loss(a, st, kc));
    Launches bw;
    if (what & 1) pipe_add_K_bwd(a, bw, kc, fused);
    if (what & 2) pipe_add_P_c2bwd(a, bw, pc);
    TRY(bw.run(st));
    if (what & 2) {
      Launches ab;
      pipe_add_P_abwd(a, ab, pc, fused);
      TRY(ab.run(st));
    }
    if (xc) TRY(xchg_launch(a, st, what));
    if (seg == 0) return GCRL_OK;
  }
  const bool xcp = xc && !a->xchg_sep_norm;   // the clip norm's partials come from the exchange kernel
  const float* g_c = xc ? xg(a, a->G_critic(0)) : a->G_critic(0);   // after an exchange the optimiser reads the receive buffer
  const float* g_a = xc ? xg(a, a->G_actor()) : a->G_actor();
  if (!fused && !xcp) {
    if (what == 3) TRY(launch_sumsq2(st, g_c, a->critic.numel, a->norm_partial, g_a, a->actor.numel, a->norm_partial + kNormBlocks));
    else if (what & 1) TRY(launch_sumsq(st, g_c, a->critic.numel, 0, 1, a->norm_partial));
    else TRY(launch_sumsq(st, g_a, a->actor.numel, 0, 1, a->norm_partial + kNormBlocks));
  }
  AdamArgs ac, aa;
  if (what & 1) pipe_adam_critic_args(a, kc, ac, fused);
  if (what & 2) pipe_adam_actor_args(a, pc, aa, fused);
  if (xc && (what & 1)) ac.g = g_c;
  if (xc && (what & 2)) aa.g = g_a;
  if (xcp && (what & 1)) { TRY(xchg_parts(a, true, &ac.partial, &ac.nparts)); ac.part_stride = ac.nparts; }
  if (xcp && (what & 2)) { TRY(xchg_parts(a, false, &aa.partial, &aa.nparts)); aa.part_stride = aa.nparts; }
  if (a->rowchain) {
    if (what & 1) rc_adam_extras(a, ac, true);
    if (what & 2) rc_adam_extras(a, aa, false);
  }
  if (polyak) {   // what == 3 on the row-block path (the optimiser also writes the targets' [in][out] copies)
    ac.polyak = 1;
    aa.polyak = 1; aa.target = a->P_tactor();
  }
  if (a->rowchain) {   // the optimiser reads the copies, so that it may advance the originals
    ac.cur = &a->ctrl()->cur_b;
    aa.cur = what == 3 ? &a->ctrl()->prev_b : &a->ctrl()->cur_b;
    if (adv) ac.advance = a->ctrl();   // (what & 1) always holds here
  }
  // the critic's optimiser step only has to precede the NEXT step's passes (P never reads the
  // critic after its input-gradient launches), so in the overlapped form it shares a launch with
  // the actor's
  if (what == 3) TRY(launch_adam_pair(st, ac, aa));
  else if (what == 1) TRY(launch_adam(st, ac));
  else TRY(launch_adam(st, aa));
  return GCRL_OK;
}

// n consecutive segments of the same kind (n > 1: overlapped steps P||K, whole, chained by the
// optimiser's control advance) captured as ONE graph: a graph launch costs ~8 us of idle GPU
// between graphs, as much as two kernels of the 4-launch step
int run_ddpg_pipe(gcrl_agent* a, hipStream_t st, int what_flags, int seg = -1, int n = 1) {
  if (a->rowchain && a->wt_dirty) TRY(rc_rebuild_wt(a, st));
  auto enqueue = [&](hipStream_t s) -> int {
    for (int i = 0; i < n; ++i) {
      int wf = what_flags;
      if (n > 1 && a->rowchain) {   // inside a chain every step is pre-advanced and advances; the ends keep the caller's flags
        if (i > 0) wf |= PIPE_PRE;
        if (i + 1 < n) wf |= PIPE_ADV;
      }
      TRY(enqueue_ddpg_pipe(a, s, wf, seg));
    }
    return GCRL_OK;
  };
  if (!graph_on(a) || a->prof || pop_recording()) return enqueue(st);
  const int key = 0x100000 | what_flags | ((seg + 1) << 5) | (n << 8);
  auto it = a->graphs.find(key);
  if (it == a->graphs.end()) {
    hipGraph_t g = nullptr;
    GCRL_HIP(hipStreamBeginCapture(a->cap_stream, hipStreamCaptureModeThreadLocal));
    int rc = enqueue(a->cap_stream);
    hipError_t e = hipStreamEndCapture(a->cap_stream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    GCRL_HIP(e);
    hipGraphExec_t ex = nullptr;
    GCRL_HIP(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    it = a->graphs.emplace(key, ex).first;
  }
  GCRL_HIP(hipGraphLaunch(it->second, st));
  return GCRL_OK;
}

// Drive m planned steps.  A step whose K or P involves a Polyak update (variant bits) runs through
// the ordinary per-step graph; runs of plain actor steps are overlapped pairwise.
int run_steps_ddpg(gcrl_agent* a, hipStream_t st, const int* variants, int m, bool first_pre = false) {
  const int plain = V_ACTOR;                                   // actor step, no Polyak, nothing injected
  const int polyak = V_ACTOR | V_POLYAK_C | V_POLYAK_A;        // DDPG's step % 40 == 0
  const bool rc = a->rowchain;   // only the row-block path can advance the control block in its optimiser launch
                                 // and keep Polyak steps inside the overlapped schedule
  auto joins = [&](int v) { return v == plain || (rc && v == polyak); };
  // the call's other batches are drawn once the critic phases of the head's steps have been issued (`issued` = how many)
  auto drawn_after = [&](int issued) -> int { return (a->deferred.her && issued >= a->deferred.next) ? finish_deferred_draw(a, st) : GCRL_OK; };
  int i = 0;
  while (i < m) {
    const int pre0 = (first_pre && i == 0) ? 1 : 0;   // the call's first step starts from the uploaded control block
    if (variants[i] != plain) { TRY(run_step(a, st, variants[i] | norm_bits(a) | (pre0 ? V_PRE : 0), 7)); TRY(drawn_after(i + 1)); ++i; continue; }
    // maximal run [i, j): starts at a plain step, continues over plain and (row-block path) Polyak steps
    int j = i + 1;
    while (j < m && joins(variants[j])) ++j;
    if (j - i == 1 && !rc) { TRY(run_step(a, st, variants[i] | norm_bits(a) | (pre0 ? V_PRE : 0), 7)); TRY(drawn_after(i + 1)); i = j; continue; }
    TRY(run_ddpg_pipe(a, st, 1 | (rc && j - i > 1 ? PIPE_ADV : 0) | (pre0 ? PIPE_PRE : 0)));   // K(i)
    TRY(drawn_after(i + 1));
    int s = i + 1;                                                     // overlapped steps P(s-1) || K(s)
    while (s < j) {
      const int adv_after = [&](int last) { return rc && last + 1 < j ? PIPE_ADV : 0; }(s);
      if (variants[s] == polyak) {
        TRY(run_ddpg_pipe(a, st, 3 | PIPE_PRE | PIPE_POLYAK | adv_after));
        ++s;
        TRY(drawn_after(s));
        continue;
      }
      int e = s;                                                       // stretch of plain steps [s, e)
      while (e < j && variants[e] == plain) ++e;
      // whole stretches as one graph when graphs are on (a trainer cycle has one pattern, so few graphs get
      // built); very long ones fall back to chains of 16 / 4 / 1
      int left = e - s;
      while (left > 0) {
        // (the call's other batches still to be drawn: one overlapped step at a time until the head's steps are queued)
        const int n = a->deferred.her ? 1 : (left <= 64 ? left : (left >= 16 ? 16 : (left >= 4 ? 4 : 1)));
        TRY(run_ddpg_pipe(a, st, 3 | (rc ? PIPE_PRE : 0) | (rc && s + n < j ? PIPE_ADV : 0), -1, n));
        s += n;
        left -= n;
        TRY(drawn_after(s));
      }
    }
    TRY(finish_deferred_draw(a, st));
    TRY(run_ddpg_pipe(a, st, 2));                                   // P(j-1)
    i = j;
  }
  return GCRL_OK;
}

// ---- data-parallel schedule: the same step sequence as a list of segments, each followed by the
// gradient block the caller must all-reduce (sum) before running the next segment
void dp_build_schedule(gcrl_agent* a) {
  a->dp_segs.clear();
  a->dp_pos = 0;
  const int m = (int)a->dp_plans.size();
  float* crit = a->grads + a->goff_critic;
  const long long n_crit = (long long)a->C * a->critic_stride;
  float* act = a->grads + a->goff_actor;
  const long long n_act = (a->goff_alpha - a->goff_actor) + (a->sac ? 1 : 0);
  const long long n_both = (a->goff_actor - a->goff_critic) + n_act;   // critics | actor are adjacent
  auto phases = [&](int i) {
    const bool actor = (a->dp_plans[i].variant & V_ACTOR) != 0;
    a->dp_segs.push_back({0, i, 0, crit, n_crit});
    a->dp_segs.push_back({0, i, 1, actor ? act : nullptr, actor ? n_act : 0});
    a->dp_segs.push_back({0, i, 2, nullptr, 0});
  };
  const bool pipe = a->cfg.kind == GCRL_AGENT_DDPG && a->cfg.pipeline_steps != 0;
  int i = 0;
  while (i < m) {
    const bool rc = a->rowchain;
    const int polyak = V_ACTOR | V_POLYAK_C | V_POLYAK_A;
    int j = i;   // a run starts at a plain step and, on the row-block path, continues over Polyak steps
    while (pipe && j < m && (a->dp_plans[j].variant == V_ACTOR || (rc && j > i && a->dp_plans[j].variant == polyak))) ++j;
    if (j - i < 2) { phases(i); ++i; continue; }
    a->dp_segs.push_back({1, 1 | (rc ? PIPE_ADV : 0), 0, crit, n_crit});       // K(i)
    a->dp_segs.push_back({1, 1 | (rc ? PIPE_ADV : 0), 1, nullptr, 0});
    for (int s = i + 1; s < j; ++s) {                     // P(s-1) || K(s): ONE exchange
      const int wf = 3 | (rc ? PIPE_PRE : 0) | (rc && s + 1 < j ? PIPE_ADV : 0) | (a->dp_plans[s].variant == polyak ? PIPE_POLYAK : 0);
      a->dp_segs.push_back({1, wf, 0, crit, n_both});
      a->dp_segs.push_back({1, wf, 1, nullptr, 0});
    }
    a->dp_segs.push_back({1, 2, 0, act, n_act});         // P(j-1)
    a->dp_segs.push_back({1, 2, 1, nullptr, 0});
    i = j;
  }
}
