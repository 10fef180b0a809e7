// agent_pop.inc — DDPG, TD3, SAC and TQC populations (include/gcrl.h gcrl_pop_*; included at the end of agent.hip).
//
// P independent DDPG, TD3 or SAC agents of one kind and equal shapes whose update steps share launches.  Each member is an ordinary gcrl_agent (its own
// parameters, optimiser state, control block, metric ring and meeting counters), so every single-agent entry works on it.  A
// population call records each member's launch sequence of the call (pop.h: the launchers record instead of launching), then
// issues position k of all sequences together: one launch of the kernel's population form (rowchain_ddpg_pop_kernel,
// dw_adam_pop_kernel, begin_step_pop_kernel, gemm_batch_pop_kernel<1, 1, 4>, adam_pop_kernel, adam_pair_pop_kernel; SAC: the slab launches' bn_linear_*_slab_*pop_kernel, rowchain_split_[heads_]pop_kernel, tanh_gauss_bwd_select_pop_kernel), in which member m's workgroups read member m's own argument struct — the same
// arithmetic in the same order as the member's own launch, so each member computes bit for bit what it computes alone.
// Launches without a population form are issued member by member at their position.
// TQC (gcrl_pop_create_layered): members on the layer-per-launch schedule; new forms tanh_gauss_fwd[2]_pop_kernel and tanh_gauss_bwd_pop_kernel;
// the TD-loss launch and the single-workgroup metric launch of a step have none yet (DESIGN.md 4f).
// The acting side (one launch per vector-env step for all members): gcrl_pop_observe_act (row-chain actors), gcrl_pop_observe_act_bn
// (SAC's BatchNorm actors), gcrl_pop_process_step.  On a gcrl_env_group (dev_env.h) the same three stages run without the host in the
// loop: gcrl_pop_collect (acting launch, env_step_pop_kernel, device-block process-step: three launches per vector step for all
// members) and gcrl_pop_evaluate (acting launch in eval mode, env step).
//
// Admission (meet.h): a launch whose workgroups wait for each other is issued in its waiting form only when the WHOLE population
// launch is resident at once; otherwise the members record the no-wait form of that stage (same bits — except SAC's slab launches, whose
// row-split and one-workgroup forms sum a column in different orders: gcrl_pop_forms says which the population runs, and a member is bitwise a
// standalone agent running the same forms).

struct gcrl_pop {
  std::vector<gcrl_agent*> m;
  std::map<std::string, void*> tabs;   // device argument tables of the population launches, by content (they repeat call after call)
  std::vector<PopRec> rec;
  // SAC: whether P x a member's workgroups of the row-split slab launches / of part 3 of the split chain launch are resident at once (fixed at
  // creation: a function of P, the shapes and whether the device is shared)
  // admission of the waiting forms, per form bit (1 row-split slab launches, 2 merged chain launch / DDPG's k-split critic phase, 8 fused
  // optimiser launch): P x a member's workgroups of the form against what is resident at once (gcrl_pop_forms_terms)
  long long want[3] = {0, 0, 0}, cap[3] = {0, 0, 0};
  bool no_waits = false;               // GCRL_POP_NO_WAITS=1 at creation: the population admits no waiting form (A/B knob)
  int64_t merged = 0, alone = 0;       // recorded positions issued as one population launch / member by member (gcrl_pop_launch_counts)
  // replay side of an update call (gcrl_pop_set_gather_merge, gcrl_pop_gather_counts): the members' gathers as one population launch
  bool gather_merge = false;
  int64_t upd_calls = 0, gather_merged = 0, gather_alone = 0;
  // acting side (gcrl_pop_observe_act, gcrl_pop_observe_act_bn, gcrl_pop_process_step; counts: gcrl_pop_acting_counts)
  PopTabCache act_tabs;                // device tables of the members' RowActArgs (SAC: ActBnArgs)
  // fast form: one pinned, mapped block [noise | actions | flags | rows] for kPopActRows rows per member (rowchain.h RowActPop)
  char *act_blk_host = nullptr, *act_blk_dev = nullptr;
  unsigned long long act_seq = 0;
  // staged form (more rows per member than the block holds): pinned staging and its device twin, batch_size rows per member
  char *act_st_host = nullptr, *act_st_dev = nullptr;
  std::vector<int64_t> act_ordered;    // per member: its `calls` when the acting stream last waited for its update work
  PopProcStep proc;
  int64_t act_calls = 0, act_launches = 0, act_staged = 0;
  PopTabCache clone_tabs;              // device segment tables of gcrl_pop_clone (pbt_host.h CloneSeg), by content
  // gcrl_pop_collect / gcrl_pop_evaluate on a gcrl_env_group (dev_env.h): what the loops have issued (gcrl_pop_collect_counts), and the
  // group's counters as of the start of an evaluate call with reset == 0 (device copy)
  int64_t col_calls = 0, col_steps = 0, col_launches = 0, col_copies = 0, col_syncs = 0;
  char* eval_snap = nullptr;
};

namespace {

constexpr int kMaxPopMembers = 16;
constexpr int kPopActRows = 32;   // rows per member the pinned block of gcrl_pop_observe_act holds (more: the staged form)

// [members][stride_n] rows of S floats, noise and actions of A doubles, one flag per workgroup: offsets into one block (doubles first)
struct PopActLayout {
  size_t noise, out, flags, rows, bytes;
  PopActLayout(int P, int stride_n, int S, int A) {
    const size_t d = (size_t)P * stride_n * A * sizeof(double);
    noise = 0; out = d; flags = 2 * d;
    rows = flags + (size_t)P * ((stride_n + 3) / 4) * sizeof(unsigned long long);
    bytes = rows + (size_t)P * stride_n * S * sizeof(float);
  }
};

// (pop_mismatch — the first field in which two members' configurations may not differ — lives in pbt_host.h)

// device copy of the members' argument structs of one population launch (cached: the same pointers every call)
int pop_table(gcrl_pop* p, const std::vector<const PopOp*>& ops, hipStream_t st, void** out) {
  std::string key;
  for (const PopOp* o : ops) key.append(o->args.data(), o->args.size());
  auto it = p->tabs.find(key);
  if (it == p->tabs.end()) {
    if (p->tabs.size() >= 256) {   // (a bound, never reached by the step's fixed launch pattern)
      GCRL_HIP(hipStreamSynchronize(st));
      for (auto& kv : p->tabs) (void)hipFree(kv.second);
      p->tabs.clear();
    }
    void* d = nullptr;
    GCRL_HIP(hipMalloc(&d, key.size()));
    GCRL_HIP(hipMemcpy(d, key.data(), key.size(), hipMemcpyHostToDevice));
    it = p->tabs.emplace(std::move(key), d).first;
  }
  *out = it->second;
  return GCRL_OK;
}

// position k of every member's recorded sequence: one population launch, or the members' own launches in member order
int pop_issue(gcrl_pop* p, size_t k, hipStream_t st) {
  const size_t P = p->m.size();
  std::vector<const PopOp*> ops(P);
  bool merge = true;
  for (size_t i = 0; i < P; ++i) {
    ops[i] = &p->rec[i].ops[k];
    const PopOp& o = *ops[i];
    const PopOp& o0 = *ops[0];
    merge = merge && pop_mergeable(o.kind, o.sub) && o.kind == o0.kind && o.sub == o0.sub && o.grid.x == o0.grid.x && o.grid.y == o0.grid.y &&
            o.grid.z == o0.grid.z && o.lds == o0.lds && o.args.size() == o0.args.size();
  }
  if (!merge || P == 1) {
    for (const PopOp* o : ops) TRY(o->issue(st));
    p->alone++;
    return GCRL_OK;
  }
  void* tab = nullptr;
  TRY(pop_table(p, ops, st, &tab));
  const PopOp& o = *ops[0];
  p->merged++;
  switch (o.kind) {
    case POP_ROWCHAIN: return launch_rowchain_ddpg_pop(st, tab, (int)P, o.sub, o.grid, o.lds);
    case POP_DW_ADAM: return launch_dw_adam_pop(st, tab, (int)P, o.grid);
    case POP_BEGIN_STEP: return launch_begin_step_pop(st, tab, (int)P);
    case POP_GEMM_BATCH: return launch_gemm_batch_pop(st, tab, (int)P, o.sub, o.grid);
    case POP_ADAM: return launch_adam_pop(st, tab, (int)P, o.grid);
    case POP_ADAM_PAIR: return launch_adam_pair_pop(st, tab, (int)P, o.grid);
    case POP_BN_FWD: return launch_bn_fwd_slab_pop(st, tab, (int)P, o.sub, o.grid);
    case POP_BN_BWD: return launch_bn_bwd_slab_pop(st, tab, (int)P, o.sub, o.grid);
    case POP_BN_BWD_FOLD: return launch_bn_bwd_slab_fold_pop(st, tab, (int)P, o.sub, o.grid);
    case POP_RC_SPLIT: return launch_rowchain_split_pop(st, tab, (int)P, o.sub, false, o.grid, o.lds);
    case POP_RC_SPLIT_HEADS: return launch_rowchain_split_pop(st, tab, (int)P, o.sub, true, o.grid, o.lds);
    case POP_TG_BWD_SELECT: return launch_tanh_gauss_bwd_select_pop(st, tab, (int)P, o.grid);
    case POP_TG_FWD: return launch_tanh_gauss_fwd_pop(st, tab, (int)P, o.sub, o.grid);
    case POP_TG_BWD: return launch_tanh_gauss_bwd_pop(st, tab, (int)P, o.grid);
    default: return fail(GCRL_ERR_STATE, "gcrl_pop_update_n: launch kind %d has no population form", o.kind);
  }
}

// record member a's launches of m planned steps (stream capture around the recording: a launch that bypassed the recorder would
// land in the captured graph instead of running out of order — refused below).  DDPG: the overlapped schedule of
// gcrl_agent_update_n (run_steps_ddpg); TD3 and SAC: their per-step phases with the variant bits gcrl_agent_update_n gives them on the
// row-chain path (every step pre-advanced, its last launch advancing the control block); TQC: the layer-per-launch schedule with the bits
// pop_layer_adv gives (gcrl_agent_update_n's rule)
bool pop_layer_adv(const gcrl_agent* a) { return a->sac && !a->rowchain && a->Q == 1 && a->cfg.ac_update_freq == 1 && !a->layer_adv_off; }
int pop_record_steps(gcrl_agent* a, hipStream_t cs, const std::vector<StepPlan>& plans, PopRec* rec) {
  rec->ops.clear();
  std::vector<int> variants(plans.size());
  for (size_t i = 0; i < plans.size(); ++i) variants[i] = plans[i].variant;
  GCRL_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
  pop_rec() = rec;
  g_pop_recorders.fetch_add(1);
  int rc = GCRL_OK;
  if (a->cfg.kind == GCRL_AGENT_TD3 || a->cfg.kind == GCRL_AGENT_SAC) {
    for (size_t i = 0; i < variants.size() && !rc; ++i) rc = run_step(a, cs, variants[i] | norm_bits(a) | V_ADV | V_PRE, 7, 1);
  } else if (a->cfg.kind == GCRL_AGENT_TQC) {
    // every step starts with its begin_step launch — unless every step is an actor step: then the actor's optimiser launch advances the
    // control block and the TD-loss launch refreshes the copies it reads, as in the standalone agent's call
    const int adv = pop_layer_adv(a) ? (V_ADV | V_PRE) : 0;
    for (size_t i = 0; i < variants.size() && !rc; ++i) rc = run_step(a, cs, variants[i] | norm_bits(a) | adv, 7, 1);
  } else {
    rc = run_steps_ddpg(a, cs, variants.data(), (int)variants.size(), /*first_pre=*/true);
  }
  g_pop_recorders.fetch_sub(1);
  pop_rec() = nullptr;
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(cs, &g);
  size_t stray = 0;
  if (g) {
    (void)hipGraphGetNodes(g, nullptr, &stray);
    (void)hipGraphDestroy(g);
  }
  if (rc) return rc;
  GCRL_HIP(e);
  if (stray) return fail(GCRL_ERR_STATE, "gcrl_pop_update_n: %zu launch(es) of a member's step bypassed the population recorder", stray);
  return GCRL_OK;
}

// the waiting forms the next update call records (bits as gcrl_agent_get_meetings: 1 row-split slab launches, 2 merged chain launch, 8 fused
// optimiser launch): every member has the form on, the device is this process's own, and the WHOLE population launch is resident at once
int pop_forms_now(const gcrl_pop* p) {
  const int P = (int)p->m.size();
  bool on[3];
  for (int f = 0; f < 3; ++f) on[f] = !meet_device_shared() && !p->no_waits && (P == 1 || (p->want[f] > 0 && p->want[f] <= p->cap[f]));
  for (gcrl_agent* a : p->m) {
    on[0] = on[0] && a->bn_rsplit > 1;
    on[1] = on[1] && (a->sac ? a->rc_merge : a->ddpg_ksplit);
    on[2] = on[2] && a->opt_fuse;
  }
  return (on[0] ? 1 : 0) | (on[1] ? 2 : 0) | (on[2] ? 8 : 0);
}

}  // namespace

std::atomic<int> gcrl::g_pop_recorders{0};

PopRec*& gcrl::pop_rec() {
  static thread_local PopRec* r = nullptr;
  return r;
}

namespace {

// same_forms: the caller accepts "bitwise a standalone agent RUNNING THE SAME FORMS" (gcrl_pop_create_forms) — the only guarantee a SAC
// population can give; gcrl_pop_create promises bit for bit a standalone agent whatever its forms, and keeps refusing SAC
gcrl_pop* pop_create(const gcrl_agent_config* cfgs, int32_t members, bool same_forms) {
  auto bad = [](const char* field, const char* why) -> gcrl_pop* {
    fail(GCRL_ERR_ARG, "gcrl_pop_create: %s: %s", field, why);
    return nullptr;
  };
  // every refusal before any device work
  if (!cfgs) return bad("cfgs", "null config array");
  if (members < 1 || members > kMaxPopMembers) return bad("members", "a population has 1..16 members");
  for (int i = 0; i < members; ++i) {
    const gcrl_agent_config& c = cfgs[i];
    if (c.kind != GCRL_AGENT_DDPG && c.kind != GCRL_AGENT_TD3 && c.kind != GCRL_AGENT_SAC) return bad("kind", "populations are DDPG, TD3 or SAC (TQC populations are not implemented)");
    if (c.kind == GCRL_AGENT_SAC && !same_forms)
      return bad("kind", "a SAC population is bitwise a standalone agent running the same launch forms only (gcrl_pop_forms): create it with gcrl_pop_create_forms");
    if (const char* f = pop_mismatch(cfgs[0], c)) return bad(f, "members must share kind, shapes, batch_size, gradient_step, ac_update_freq, polyak_every, pipeline_steps, use_graph and device");
    if (c.pipeline_steps != 2) return bad("pipeline_steps", "the population runs the row-chain step: pipeline_steps = 2");
    if (c.hidden_dim < 4 || c.hidden_dim % 4 != 0) return bad("hidden_dim", "the row-chain step needs hidden_dim % 4 == 0");
    if (c.ac_dim < 1 || c.ac_dim > 16 || c.obs_dim < 1 || c.layer_count < 1 || c.layer_count > 8 || c.batch_size < 1) return bad("shape", "bad obs_dim / ac_dim / layer_count / batch_size");
    if (c.use_graph >= 2) return bad("use_graph", "the population issues its launches itself (use_graph 0 or 1)");
  }
  const bool td3 = cfgs[0].kind == GCRL_AGENT_TD3, sac = cfgs[0].kind == GCRL_AGENT_SAC;
  const int C = (td3 || sac) ? 2 : 1;
  if (td3 && cfgs[0].num_critics != 2) return bad("num_critics", "a TD3 agent has two critics");
  if (sac) {
    // the path cfg 5 runs (agent.hip build: the same rules): BatchNorm slab launches, role-split chain launches with the actor's heads folded in
    const gcrl_agent_config& c = cfgs[0];
    if (c.num_critics != 2) return bad("num_critics", "a SAC population runs the twin-critic role-split chain launches: num_critics = 2");
    if (c.batch_size > 512) return bad("batch_size", "SAC populations run the BatchNorm slab launches: batch_size <= 512");
    if (c.hidden_dim < 16 || c.hidden_dim % 16 != 0) return bad("hidden_dim", "SAC populations run the BatchNorm slab launches: hidden_dim % 16 == 0");
    if (!sac_slab_rule(c.batch_size, c.hidden_dim)) return bad("GCRL_NO_BN_SLAB", "SAC populations run the BatchNorm slab launches, which this environment switches off");
    if (!sac_split_roles_rule(c.num_critics, c.batch_size, row_rg_of(c.kind, c.batch_size))) return bad("GCRL_NO_SPLIT_ROLES", "SAC populations run the role-split chain launches, which this environment switches off");
    if (sac_heads_fold_env_off()) return bad("GCRL_NO_HEADS_FOLD", "SAC populations run the chain launches with the actor's heads folded in, which this environment switches off");
  }
  // the row-chain launch (agent.hip build: the same rules, row_rg_of / td3_split_k_rule): its rows per workgroup and LDS
  const gcrl_agent_config& c0 = cfgs[0];
  const int H = c0.hidden_dim, ldx = round_up(c0.obs_dim + c0.ac_dim, 4);
  const int ldl = round_up(std::max(H, ldx), 4) + 4;
  const int rg = row_rg_of(c0.kind, c0.batch_size);
  if (rowchain_lds_bytes(rg, ldl, c0.ac_dim, H, C) > 160 * 1024) return bad("hidden_dim", "the row-chain launch of this shape does not fit the LDS");
  if (td3) {
    // TD3 at a batch that fills the chip runs forms without a population form: the split dW problems (B >= 2048) and the
    // role-split critic phase (split_k / rc_merge_k: >= 256 row blocks)
    if (c0.batch_size >= 2048) return bad("batch_size", "TD3 populations run batch_size < 2048 (the split dW form has no population form)");
    if (td3_split_k_rule(c0.batch_size, rg))
      return bad("batch_size", "at this batch TD3 runs the role-split critic phase (split_k / rc_merge_k), which has no population form");
  }
  gcrl_pop* p = new gcrl_pop;
  for (int i = 0; i < members; ++i) {
    gcrl_agent* a = gcrl_agent_create(&cfgs[i]);
    if (!a) { gcrl_pop_destroy(p); return nullptr; }
    p->m.push_back(a);
    if (!a->rowchain) { gcrl_pop_destroy(p); return bad("hidden_dim", "this configuration does not run the row-chain step"); }
    if (td3 && i == 0 && (a->split_k || a->rc_merge_k || a->dw_split_c > 1 || a->dw_split_a > 1)) {
      gcrl_pop_destroy(p);
      return bad("batch_size", "this TD3 configuration runs the role-split critic phase or the split dW form, which have no population form");
    }
  }
  if (sac) {
    for (gcrl_agent* a : p->m)
      if (!(a->split_roles && a->slab_on() && heads_fold_on(a))) {
        gcrl_pop_destroy(p);
        return bad("kind", "this SAC configuration does not run the slab launches and the role-split chain launches with folded heads");
      }
  }
  {
    gcrl_agent* a0 = p->m[0];
    const long long nblk = (a0->B + 4 * a0->row_rg - 1) / (4 * a0->row_rg);
    if (sac) {
      bn_slab_pop_row_split_terms(a0->B, a0->H, a0->A, members, &p->want[0], &p->cap[0]);
      rowchain_pop_merge_terms(a0->row_rg, a0->row_ldl, a0->A, a0->H, a0->C, a0->B, members, &p->want[1], &p->cap[1]);
    } else {   // DDPG's k-split critic phase: three roles per row block, one workgroup per CU
      p->want[1] = (long long)members * 3 * nblk; p->cap[1] = std::max(a0->n_cus, 1);
    }
    p->want[2] = (long long)members * a0->of_wgs; p->cap[2] = dw_adam_pop_capacity();
    p->no_waits = std::getenv("GCRL_POP_NO_WAITS") != nullptr;
  }
  p->rec.resize(members);
  return p;
}

// TQC populations (gcrl_pop_create_layered): members on the layer-per-launch schedule — scalar critics, the BatchNorm actor's slab launches
gcrl_pop* pop_create_layered(const gcrl_agent_config* cfgs, int32_t members) {
  auto bad = [](const char* field, const char* why) -> gcrl_pop* {
    fail(GCRL_ERR_ARG, "gcrl_pop_create_layered: %s: %s", field, why);
    return nullptr;
  };
  // every refusal before any device work
  if (!cfgs) return bad("cfgs", "null config array");
  if (members < 1 || members > kMaxPopMembers) return bad("members", "a population has 1..16 members");
  bool any_tqc = false;
  for (int i = 0; i < members; ++i) any_tqc = any_tqc || cfgs[i].kind == GCRL_AGENT_TQC;
  for (int i = 0; i < members; ++i) {
    const gcrl_agent_config& c = cfgs[i];
    if (c.kind != GCRL_AGENT_TQC)
      return bad("kind", any_tqc ? "members must share kind: every member of this population is a TQC agent"
                                 : "this entry creates TQC populations (DDPG and TD3: gcrl_pop_create; SAC: gcrl_pop_create_forms)");
    if (c.n_quantiles > 1) return bad("n_quantiles", "TQC populations run the scalar critics: n_quantiles = 1 (the distributional variant has no population)");
    if (c.num_critics < 2 || c.num_critics > kMaxCritics) return bad("num_critics", "a TQC population has 2..8 critics");
    if (const char* f = pop_mismatch(cfgs[0], c)) return bad(f, "members must share kind, shapes, batch_size, num_critics, gradient_step, ac_update_freq, polyak_every, pipeline_steps, use_graph and device");
    if (c.top_drop < 0 || c.top_drop >= c.num_critics) return bad("top_drop", "0 <= top_drop < num_critics");
    if (c.ac_dim < 1 || c.ac_dim > 16 || c.obs_dim < 1 || c.layer_count < 1 || c.layer_count > 8 || c.batch_size < 1) return bad("shape", "bad obs_dim / ac_dim / layer_count / batch_size");
    if (c.batch_size > 512) return bad("batch_size", "TQC populations run the BatchNorm slab launches: batch_size <= 512");
    if (c.hidden_dim < 16 || c.hidden_dim % 16 != 0) return bad("hidden_dim", "TQC populations run the BatchNorm slab launches: hidden_dim % 16 == 0");
    if (!sac_slab_rule(c.batch_size, c.hidden_dim)) return bad("GCRL_NO_BN_SLAB", "TQC populations run the BatchNorm slab launches, which this environment switches off");
    if (c.use_graph >= 2) return bad("use_graph", "the population issues its launches itself (use_graph 0 or 1)");
  }
  gcrl_pop* p = new gcrl_pop;
  for (int i = 0; i < members; ++i) {
    gcrl_agent* a = gcrl_agent_create(&cfgs[i]);
    if (!a) { gcrl_pop_destroy(p); return nullptr; }
    p->m.push_back(a);
    if (a->rowchain || !a->slab_on() || a->Q != 1) {
      gcrl_pop_destroy(p);
      return bad("kind", "this TQC configuration does not run the layer-per-launch step with the slab launches");
    }
  }
  gcrl_agent* a0 = p->m[0];
  // form bit 1: the row-split slab launches; bit 2 has no meaning on this schedule (want 0); bit 8: no TQC agent runs the fused optimiser
  // launch (a row-chain form), so its terms only say what the launch would take
  bn_slab_pop_row_split_terms(a0->B, a0->H, a0->A, members, &p->want[0], &p->cap[0]);
  p->want[1] = 0; p->cap[1] = 0;
  p->want[2] = a0->opt_fuse_can ? (long long)members * a0->of_wgs : 0; p->cap[2] = a0->opt_fuse_can ? dw_adam_pop_capacity() : 0;
  p->no_waits = std::getenv("GCRL_POP_NO_WAITS") != nullptr;
  p->rec.resize(members);
  return p;
}

}  // namespace

extern "C" {

gcrl_pop* gcrl_pop_create_layered(const gcrl_agent_config* cfgs, int32_t members) { return pop_create_layered(cfgs, members); }
gcrl_pop* gcrl_pop_create(const gcrl_agent_config* cfgs, int32_t members) { return pop_create(cfgs, members, false); }
gcrl_pop* gcrl_pop_create_forms(const gcrl_agent_config* cfgs, int32_t members) { return pop_create(cfgs, members, true); }

int gcrl_pop_member(gcrl_pop* p, int32_t i, gcrl_agent** out) {
  GCRL_CHECK_ARG(p && out, "gcrl_pop_member: null argument");
  GCRL_CHECK_ARG(i >= 0 && i < (int32_t)p->m.size(), "gcrl_pop_member: member %d of %d", i, (int)p->m.size());
  *out = p->m[i];
  return GCRL_OK;
}

int32_t gcrl_pop_size(const gcrl_pop* p) { return p ? (int32_t)p->m.size() : -1; }

int gcrl_pop_launch_counts(const gcrl_pop* p, int64_t* merged, int64_t* alone) {
  GCRL_CHECK_ARG(p, "gcrl_pop_launch_counts: null handle");
  if (merged) *merged = p->merged;
  if (alone) *alone = p->alone;
  return GCRL_OK;
}

int gcrl_pop_set_gather_merge(gcrl_pop* p, int32_t on) {
  GCRL_CHECK_ARG(p, "gcrl_pop_set_gather_merge: pop: null handle");
  p->gather_merge = on != 0;
  return GCRL_OK;
}

int gcrl_pop_gather_counts(const gcrl_pop* p, int64_t* calls, int64_t* merged, int64_t* alone) {
  GCRL_CHECK_ARG(p, "gcrl_pop_gather_counts: pop: null handle");
  if (calls) *calls = p->upd_calls;
  if (merged) *merged = p->gather_merged;
  if (alone) *alone = p->gather_alone;
  return GCRL_OK;
}

int gcrl_pop_forms(gcrl_pop* p) {
  GCRL_CHECK_ARG(p, "gcrl_pop_forms: pop: null handle");
  return pop_forms_now(p);
}

int gcrl_pop_forms_terms(const gcrl_pop* p, int64_t* want, int64_t* capacity) {
  GCRL_CHECK_ARG(p && want && capacity, "gcrl_pop_forms_terms: null argument");
  for (int f = 0; f < 3; ++f) { want[f] = p->want[f]; capacity[f] = p->cap[f]; }
  return GCRL_OK;
}

int gcrl_pop_update_n(gcrl_pop* p, gcrl_her* const* rings, int64_t step0, int32_t n, int64_t* tickets_out, int32_t* tuple_len_out,
                      void* stream) {
  GCRL_CHECK_ARG(p && rings, "gcrl_pop_update_n: null handle");
  GCRL_CHECK_ARG(n >= 1, "gcrl_pop_update_n: n must be >= 1");
  const int P = (int)p->m.size();
  for (int i = 0; i < P; ++i) {
    gcrl_agent* a = p->m[i];
    GCRL_CHECK_ARG(rings[i], "gcrl_pop_update_n: member %d has no replay ring", i);
    if (her_prio_on(rings[i]))
      return fail(GCRL_ERR_STATE, "gcrl_pop_update_n: prioritise: member %d's ring has an energy tree; populations do not draw from one", i);
    if (her_td_on(rings[i]))
      return fail(GCRL_ERR_STATE, "gcrl_pop_update_n: prioritise: member %d's ring has a TD-error tree; populations do not draw from one", i);
    GCRL_CHECK_ARG(!a->xchg && a->bn_sync.world <= 1, "gcrl_pop_update_n: member %d is in a data-parallel group", i);
    GCRL_CHECK_ARG(!a->prof, "gcrl_pop_update_n: member %d has launch profiling on", i);
    if (a->bc_weight > 0.0) return fail(GCRL_ERR_STATE, "gcrl_pop_update_n: bc_weight: member %d has the behaviour-cloning term on; populations do not step it", i);
    TRY(prior_precheck(a, rings[i], "gcrl_pop_update_n"));   // prior-data replay: every member's prior ring, before any member's ticket
    // (members may share a ring: its index stream — the ring's generator, or draws_done in device-RNG mode — is then consumed in
    // member order, as by standalone agents that share the ring and are called in that order)
    // a process that arrived on this device after the handle was built: the forms with waits go off (as gcrl_agent_update_n)
    if ((a->calls & 31) == 0 && !meet_device_shared()) { const int rc = gcrl_agent_get_meetings(a); if (rc < 0) return rc; }
  }
  gcrl_agent* a0 = p->m[0];
  hipStream_t st = a0->pick(stream);
  // admission of the forms whose workgroups wait for each other: the whole population launch resident at once
  const int forms = pop_forms_now(p);
  const bool tqc = a0->cfg.kind == GCRL_AGENT_TQC;
  const bool sac = a0->cfg.kind == GCRL_AGENT_SAC || tqc;   // (the BatchNorm actors: their slab launches have the row-split form)
  const bool ksplit = !sac && (forms & 2) != 0, ofuse = (forms & 8) != 0, rsplit = (forms & 1) != 0, merge = sac && (forms & 2) != 0;
  struct Forms { bool ksplit, ofuse, rc_merge; int bn_rsplit; };
  std::vector<Forms> saved(P);
  for (int i = 0; i < P; ++i) {
    gcrl_agent* a = p->m[i];
    saved[i] = Forms{a->ddpg_ksplit, a->opt_fuse, a->rc_merge, a->bn_rsplit};
  }
  auto restore = [&]() {
    for (int i = 0; i < P; ++i) {
      gcrl_agent* a = p->m[i];
      a->ddpg_ksplit = saved[i].ksplit; a->opt_fuse = saved[i].ofuse; a->rc_merge = saved[i].rc_merge; a->bn_rsplit = saved[i].bn_rsplit;
    }
  };
  const int chunk = std::min(kMaxStepsPerCall, a0->Mmax);
  for (int done = 0; done < n; done += chunk) {
    const int m = std::min(chunk, n - done);
    std::vector<std::vector<StepPlan>> plans(P);
    // every member's batches first (their rings' index streams in member order), then the gathers: one population launch for all
    // members' rings, or — gather_merge off — each member's own launch
    CallGather cgs[kMaxPopMembers];
    for (int i = 0; i < P; ++i) {
      gcrl_agent* a = p->m[i];
      if (a->wt_dirty) TRY(rc_rebuild_wt(a, st));
      TRY(begin_call_plan(a, rings[i], step0 + done, m, nullptr, 1.0f, st, plans[i], tickets_out ? tickets_out + (size_t)i * n + done : nullptr,
                          tuple_len_out ? tuple_len_out + (size_t)i * n + done : nullptr, /*defer_rest=*/false, /*pre_advanced=*/!tqc || pop_layer_adv(a),
                          &cgs[i]));
    }
    bool one = false;
    TRY(begin_call_issue_pop(p->m.data(), cgs, P, p->gather_merge, st, &one));
    p->upd_calls++;
    if (one) p->gather_merged++;
    else p->gather_alone += P;
    int rc = GCRL_OK;
    for (int i = 0; i < P && !rc; ++i) {
      gcrl_agent* a = p->m[i];
      a->ddpg_ksplit = ksplit; a->opt_fuse = ofuse;
      if (sac) { a->rc_merge = merge; if (!rsplit) a->bn_rsplit = 1; }
      rc = pop_record_steps(a, a0->cap_stream, plans[i], &p->rec[i]);
    }
    restore();
    if (rc) return rc;
    const size_t K = p->rec[0].ops.size();
    for (int i = 1; i < P; ++i)
      if (p->rec[i].ops.size() != K) return fail(GCRL_ERR_STATE, "gcrl_pop_update_n: member %d's step has %zu launches, member 0's %zu", i, p->rec[i].ops.size(), K);
    for (size_t k = 0; k < K; ++k) TRY(pop_issue(p, k, st));
    for (gcrl_agent* a : p->m) TRY(end_call(a, st));
  }
  return GCRL_OK;
}

int gcrl_pop_observe_act(gcrl_pop* p, gcrl_normalizer* const* nz_obs, gcrl_normalizer* const* nz_dg, const float* obs_host, int32_t obs_dim,
                         const float* dg_host, int32_t goal_dim, int32_t n, const double* noise_host, const int32_t* modes, double* out_host,
                         void* stream) {
  // every refusal before any device work
  GCRL_CHECK_ARG(obs_host, "gcrl_pop_observe_act: obs_host: null array");
  GCRL_CHECK_ARG(dg_host, "gcrl_pop_observe_act: dg_host: null array");
  GCRL_CHECK_ARG(modes, "gcrl_pop_observe_act: modes: null array");
  GCRL_CHECK_ARG(out_host, "gcrl_pop_observe_act: out_host: null array");
  GCRL_CHECK_ARG(modes[0] >= -1 && modes[0] <= 2, "gcrl_pop_observe_act: modes: member 0 has mode %d (-1 skipped, 0, 1 or 2)", modes[0]);
  GCRL_CHECK_ARG(p, "gcrl_pop_observe_act: pop: null handle");
  const int P = (int)p->m.size();
  gcrl_agent* a0 = p->m[0];
  // (a BatchNorm actor has no row-chain network to build the launch's table from: its members act through gcrl_agent_observe_act)
  GCRL_CHECK_ARG(!a0->sac, "gcrl_pop_observe_act: kind: a SAC population has no merged acting launch (call gcrl_agent_observe_act on each member)");
  const int D = obs_dim, G = goal_dim, A = a0->A, S = a0->S;
  GCRL_CHECK_ARG(n >= 1 && n <= a0->B, "gcrl_pop_observe_act: n: %d rows per member (1..batch_size = %d)", n, a0->B);
  GCRL_CHECK_ARG(D >= 1 && G >= 0 && D + G == S, "gcrl_pop_observe_act: obs_dim %d + goal_dim %d != state_dim %d", D, G, S);
  unsigned int live = 0, noisy = 0;
  for (int i = 0; i < P; ++i) {
    GCRL_CHECK_ARG(modes[i] >= -1 && modes[i] <= 2, "gcrl_pop_observe_act: modes: member %d has mode %d (-1 skipped, 0, 1 or 2)", i, modes[i]);
    gcrl_normalizer* zo = nz_obs ? nz_obs[i] : nullptr;
    gcrl_normalizer* zg = nz_dg ? nz_dg[i] : nullptr;
    // the kernel indexes mean[j] / var[j] for j < obs_dim (goal_dim): a normaliser of another size is an argument error, never an out-of-bounds access
    GCRL_CHECK_ARG(!zo || gcrl_normalizer_size(zo) == D, "gcrl_pop_observe_act: nz_obs: member %d's observation normaliser has size %d for obs_dim %d", i, gcrl_normalizer_size(zo), D);
    GCRL_CHECK_ARG(!zg || gcrl_normalizer_size(zg) == G, "gcrl_pop_observe_act: nz_dg: member %d's goal normaliser has size %d for goal_dim %d", i, gcrl_normalizer_size(zg), G);
    if (modes[i] >= 0) live |= 1u << i;
    if (modes[i] == 1 && noise_host) noisy |= 1u << i;
  }
  GCRL_CHECK_ARG(4 * round_up(S, 4) <= 2 * kRowThreads || !(nz_obs || nz_dg), "gcrl_pop_observe_act: obs_dim: fused normalisation supports state_dim <= 128");
  p->act_calls++;
  const size_t oD = (size_t)n * D, oG = (size_t)n * G, oA = (size_t)n * A;
  if (P == 1) {   // nothing to merge: the member's own entry
    if (!live) return GCRL_OK;
    return gcrl_agent_observe_act(a0, nz_obs ? nz_obs[0] : nullptr, nz_dg ? nz_dg[0] : nullptr, obs_host, D, dg_host, G, n, noise_host, modes[0], out_host, stream);
  }
  if (!live) return GCRL_OK;   // every member on the epsilon-random branch: no network, no launch
  hipStream_t st = a0->pick(stream);
  // after every member's last update call (DESIGN.md 4c: the event that closes a handle's update work), and on fresh [in][out] copies
  p->act_ordered.resize(P, 0);
  for (int i = 0; i < P; ++i) {
    gcrl_agent* a = p->m[i];
    if (a->calls != p->act_ordered[i]) {
      GCRL_HIP(hipStreamWaitEvent(st, a->call_ev[(a->calls - 1) % kEventRing], 0));
      p->act_ordered[i] = a->calls;
    }
    if (((live >> i) & 1u) && a->wt_dirty) TRY(rc_rebuild_wt(a, st));
  }
  // the members' table: what belongs to the member (a skipped member keeps a slot; its post mode there is never read)
  RowActArgs tab[kMaxPopMembers];
  int fill = 1;
  for (int i = P - 1; i >= 0; --i) if (modes[i] >= 0) fill = modes[i];   // (the first live member's mode: the table then repeats whoever is skipped)
  for (int i = 0; i < P; ++i) {
    gcrl_agent* a = p->m[i];
    RowActArgs& ra = tab[i];
    std::memset(&ra, 0, sizeof(ra));
    ra.actor = make_rownet(a, a->actor, a->P_actor(), 0);
    ra.ld_obs = S; ra.out = a->dact; ra.ld_out = a->Apad;
    ra.n = n; ra.S = S; ra.A = A; ra.ldl = a->row_ldl;
    ra.D = D;
    gcrl::normalizer_view(nz_obs ? nz_obs[i] : nullptr, &ra.nz_mean, &ra.nz_var, nullptr, &ra.nz_clip, &ra.nz_mode);
    gcrl::normalizer_view(nz_dg ? nz_dg[i] : nullptr, &ra.nzg_mean, &ra.nzg_var, nullptr, &ra.nzg_clip, &ra.nzg_mode);
    const int mode = modes[i] < 0 ? fill : modes[i];
    ra.post = mode == 1 ? 1 : (mode == 0 ? 2 : 3);
  }
  void* tab_dev = nullptr;
  if (p->act_tabs.get(tab, sizeof(RowActArgs) * P, st, &tab_dev)) return fail(GCRL_ERR_HIP, "gcrl_pop_observe_act: argument table upload failed");
  const bool fast = n <= kPopActRows;
  const int stride_n = fast ? kPopActRows : a0->B;
  const PopActLayout lay(P, stride_n, S, A);
  char* host = nullptr;
  if (fast) {
    if (!p->act_blk_host) {
      GCRL_HIP(hipHostMalloc((void**)&p->act_blk_host, lay.bytes, hipHostMallocMapped | hipHostMallocCoherent));
      std::memset(p->act_blk_host, 0, lay.bytes);
      GCRL_HIP(hipHostGetDevicePointer((void**)&p->act_blk_dev, p->act_blk_host, 0));
    }
    host = p->act_blk_host;
  } else {
    if (!p->act_st_host) {
      GCRL_HIP(hipHostMalloc((void**)&p->act_st_host, lay.bytes, hipHostMallocDefault));
      GCRL_HIP(hipMalloc((void**)&p->act_st_dev, lay.bytes));
    }
    host = p->act_st_host;
  }
  char* dev = fast ? p->act_blk_dev : p->act_st_dev;
  float* h_rows = reinterpret_cast<float*>(host + lay.rows);
  double* h_noise = reinterpret_cast<double*>(host + lay.noise);
  for (int i = 0; i < P; ++i) {
    if (!((live >> i) & 1u)) continue;
    float* r = h_rows + (size_t)i * stride_n * S;
    for (int e = 0; e < n; ++e) {
      std::memcpy(r + (size_t)e * S, obs_host + i * oD + (size_t)e * D, sizeof(float) * D);
      std::memcpy(r + (size_t)e * S + D, dg_host + i * oG + (size_t)e * G, sizeof(float) * G);
    }
    if ((noisy >> i) & 1u) std::memcpy(h_noise + (size_t)i * stride_n * A, noise_host + i * oA, sizeof(double) * oA);
  }
  RowActPop c;
  c.tab = static_cast<const RowActArgs*>(tab_dev);
  c.rows = reinterpret_cast<const float*>(dev + lay.rows);
  c.noise = reinterpret_cast<const double*>(dev + lay.noise);
  c.out = reinterpret_cast<double*>(dev + lay.out);
  c.flags = fast ? reinterpret_cast<unsigned long long*>(dev + lay.flags) : nullptr;
  c.seq = ++p->act_seq;
  c.live = live; c.noisy = noisy; c.stride_n = stride_n;
  const double* h_out = reinterpret_cast<const double*>(host + lay.out);
  if (fast) {
    // ONE launch and nothing else: the host's stores to the block precede the launch, the kernel reads them there, and the host
    // waits for the live members' flags (a bounded spin; then the ordinary synchronisation says what happened)
    __atomic_thread_fence(__ATOMIC_RELEASE);
    TRY(launch_rowchain_act_pop(st, c, P, n, a0->row_ldl, A, a0->H));
    p->act_launches++;
    const int nwg = (n + 3) / 4;
    volatile unsigned long long* flags = reinterpret_cast<volatile unsigned long long*>(host + lay.flags);
    bool seen = false;
    for (long spin = 0; spin < 4000000 && !seen; ++spin) {
      seen = true;
      for (int i = 0; i < P && seen; ++i)
        if ((live >> i) & 1u)
          for (int w = 0; w < nwg; ++w) seen = seen && flags[(size_t)i * nwg + w] == c.seq;
      if (!seen) __builtin_ia32_pause();
    }
    if (!seen) GCRL_HIP(hipStreamSynchronize(st));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
  } else {
    // the exception: copies up, the same one launch, copy down, one synchronisation (noise, actions and flags lie before the rows)
    if (noisy) GCRL_HIP(hipMemcpyAsync(dev + lay.noise, host + lay.noise, lay.out - lay.noise, hipMemcpyHostToDevice, st));
    GCRL_HIP(hipMemcpyAsync(dev + lay.rows, host + lay.rows, lay.bytes - lay.rows, hipMemcpyHostToDevice, st));
    TRY(launch_rowchain_act_pop(st, c, P, n, a0->row_ldl, A, a0->H));
    p->act_launches++;
    p->act_staged++;
    GCRL_HIP(hipMemcpyAsync(host + lay.out, dev + lay.out, lay.flags - lay.out, hipMemcpyDeviceToHost, st));
    GCRL_HIP(hipStreamSynchronize(st));
  }
  for (int i = 0; i < P; ++i)
    if ((live >> i) & 1u) std::memcpy(out_host + i * oA, h_out + (size_t)i * stride_n * A, sizeof(double) * oA);
  return GCRL_OK;
}

// The BatchNorm actors' (SAC) population acting: the population forms of act_bn.hip on the members' live parameter vectors and running
// statistics — no [in][out] copies are involved.  The pinned block, the staging pair, the sequence number and the table cache are the
// ones of gcrl_pop_observe_act (a population is of one kind: the two entries never share a block in use).
int gcrl_pop_observe_act_bn(gcrl_pop* p, gcrl_normalizer* const* nz_obs, gcrl_normalizer* const* nz_dg, const float* obs_host, int32_t obs_dim,
                            const float* dg_host, int32_t goal_dim, int32_t n, const double* eps_host, double* out_host, void* stream) {
  // every refusal before any device work
  GCRL_CHECK_ARG(obs_host, "gcrl_pop_observe_act_bn: obs_host: null array");
  GCRL_CHECK_ARG(dg_host, "gcrl_pop_observe_act_bn: dg_host: null array");
  GCRL_CHECK_ARG(out_host, "gcrl_pop_observe_act_bn: out_host: null array");
  GCRL_CHECK_ARG(p, "gcrl_pop_observe_act_bn: pop: null handle");
  const int P = (int)p->m.size();
  gcrl_agent* a0 = p->m[0];
  GCRL_CHECK_ARG(a0->sac, "gcrl_pop_observe_act_bn: kind: the members are not BatchNorm actors (call gcrl_pop_observe_act)");
  const int D = obs_dim, G = goal_dim, A = a0->A, S = a0->S;
  GCRL_CHECK_ARG(n >= 1 && n <= a0->B, "gcrl_pop_observe_act_bn: n: %d rows per member (1..batch_size = %d)", n, a0->B);
  GCRL_CHECK_ARG(D >= 1 && G >= 0 && D + G == S, "gcrl_pop_observe_act_bn: obs_dim %d + goal_dim %d != state_dim %d", D, G, S);
  for (int i = 0; i < P; ++i) {
    gcrl_normalizer* zo = nz_obs ? nz_obs[i] : nullptr;
    gcrl_normalizer* zg = nz_dg ? nz_dg[i] : nullptr;
    // the kernel indexes mean[j] / var[j] for j < obs_dim (goal_dim): a normaliser of another size is an argument error, never an out-of-bounds access
    GCRL_CHECK_ARG(!zo || gcrl_normalizer_size(zo) == D, "gcrl_pop_observe_act_bn: nz_obs: member %d's observation normaliser has size %d for obs_dim %d", i, gcrl_normalizer_size(zo), D);
    GCRL_CHECK_ARG(!zg || gcrl_normalizer_size(zg) == G, "gcrl_pop_observe_act_bn: nz_dg: member %d's goal normaliser has size %d for goal_dim %d", i, gcrl_normalizer_size(zg), G);
  }
  p->act_calls++;
  const size_t oD = (size_t)n * D, oG = (size_t)n * G, oA = (size_t)n * A;
  if (P == 1)   // nothing to merge: the member's own entry
    return gcrl_agent_observe_act(a0, nz_obs ? nz_obs[0] : nullptr, nz_dg ? nz_dg[0] : nullptr, obs_host, D, dg_host, G, n, eps_host, 2, out_host, stream);
  hipStream_t st = a0->pick(stream);
  // after every member's last update call (DESIGN.md 4c: the event that closes a handle's update work)
  p->act_ordered.resize(P, 0);
  for (int i = 0; i < P; ++i) {
    gcrl_agent* a = p->m[i];
    if (a->calls != p->act_ordered[i]) {
      GCRL_HIP(hipStreamWaitEvent(st, a->call_ev[(a->calls - 1) % kEventRing], 0));
      p->act_ordered[i] = a->calls;
    }
  }
  // the members' table: what belongs to the member, filled as gcrl_agent_observe_act fills its own arguments
  ActBnArgs tab[kMaxPopMembers];
  for (int i = 0; i < P; ++i) {
    gcrl_agent* a = p->m[i];
    ActBnArgs& ba = tab[i];
    std::memset(&ba, 0, sizeof(ba));
    ba.P = a->P_actor(); ba.rmean = a->bn_rmean; ba.rvar = a->bn_rvar;
    ba.S = S; ba.H = a->H; ba.L = a->L; ba.A = A; ba.n = n; ba.D = D;
    ba.ldl = (std::max(S, a->H) + 3) / 4 * 4;
    ba.warm = 0;   // (as gcrl_agent_observe_act: measured slower)
    gcrl::normalizer_view(nz_obs ? nz_obs[i] : nullptr, &ba.nz_mean, &ba.nz_var, nullptr, &ba.nz_clip, &ba.nz_mode);
    gcrl::normalizer_view(nz_dg ? nz_dg[i] : nullptr, &ba.nzg_mean, &ba.nzg_var, nullptr, &ba.nzg_clip, &ba.nzg_mode);
  }
  void* tab_dev = nullptr;
  if (p->act_tabs.get(tab, sizeof(ActBnArgs) * P, st, &tab_dev)) return fail(GCRL_ERR_HIP, "gcrl_pop_observe_act_bn: argument table upload failed");
  const bool fast = n <= kPopActRows;
  const int stride_n = fast ? kPopActRows : a0->B;
  const PopActLayout lay(P, stride_n, S, A);
  char* host = nullptr;
  if (fast) {
    if (!p->act_blk_host) {
      GCRL_HIP(hipHostMalloc((void**)&p->act_blk_host, lay.bytes, hipHostMallocMapped | hipHostMallocCoherent));
      std::memset(p->act_blk_host, 0, lay.bytes);
      GCRL_HIP(hipHostGetDevicePointer((void**)&p->act_blk_dev, p->act_blk_host, 0));
    }
    host = p->act_blk_host;
  } else {
    if (!p->act_st_host) {
      GCRL_HIP(hipHostMalloc((void**)&p->act_st_host, lay.bytes, hipHostMallocDefault));
      GCRL_HIP(hipMalloc((void**)&p->act_st_dev, lay.bytes));
    }
    host = p->act_st_host;
  }
  char* dev = fast ? p->act_blk_dev : p->act_st_dev;
  float* h_rows = reinterpret_cast<float*>(host + lay.rows);
  double* h_eps = reinterpret_cast<double*>(host + lay.noise);
  for (int i = 0; i < P; ++i) {
    float* r = h_rows + (size_t)i * stride_n * S;
    for (int e = 0; e < n; ++e) {
      std::memcpy(r + (size_t)e * S, obs_host + i * oD + (size_t)e * D, sizeof(float) * D);
      std::memcpy(r + (size_t)e * S + D, dg_host + i * oG + (size_t)e * G, sizeof(float) * G);
    }
    if (eps_host) std::memcpy(h_eps + (size_t)i * stride_n * A, eps_host + i * oA, sizeof(double) * oA);
  }
  ActBnPop c;
  c.tab = static_cast<const ActBnArgs*>(tab_dev);
  c.rows = reinterpret_cast<const float*>(dev + lay.rows);
  c.eps = reinterpret_cast<const double*>(dev + lay.noise);
  c.out = reinterpret_cast<double*>(dev + lay.out);
  c.flags = fast ? reinterpret_cast<unsigned long long*>(dev + lay.flags) : nullptr;
  c.seq = ++p->act_seq;
  c.with_eps = eps_host ? 1 : 0; c.stride_n = stride_n;
  const double* h_out = reinterpret_cast<const double*>(host + lay.out);
  if (fast) {
    // ONE launch and nothing else: the host's stores to the block precede the launch, the kernel reads them there, and the host
    // waits for the members' flags (a bounded spin; then the ordinary synchronisation says what happened)
    __atomic_thread_fence(__ATOMIC_RELEASE);
    TRY(launch_act_bn_pop(st, c, tab[0], P));
    p->act_launches++;
    const int nwg = (n + kActBnRows - 1) / kActBnRows;
    volatile unsigned long long* flags = reinterpret_cast<volatile unsigned long long*>(host + lay.flags);
    bool seen = false;
    for (long spin = 0; spin < 4000000 && !seen; ++spin) {
      seen = true;
      for (int w = 0; w < P * nwg && seen; ++w) seen = flags[w] == c.seq;
      if (!seen) __builtin_ia32_pause();
    }
    if (!seen) GCRL_HIP(hipStreamSynchronize(st));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
  } else {
    // the exception: copies up, the same one launch, copy down, one synchronisation (eps, actions and flags lie before the rows)
    if (eps_host) GCRL_HIP(hipMemcpyAsync(dev + lay.noise, host + lay.noise, lay.out - lay.noise, hipMemcpyHostToDevice, st));
    GCRL_HIP(hipMemcpyAsync(dev + lay.rows, host + lay.rows, lay.bytes - lay.rows, hipMemcpyHostToDevice, st));
    TRY(launch_act_bn_pop(st, c, tab[0], P));
    p->act_launches++;
    p->act_staged++;
    GCRL_HIP(hipMemcpyAsync(host + lay.out, dev + lay.out, lay.flags - lay.out, hipMemcpyDeviceToHost, st));
    GCRL_HIP(hipStreamSynchronize(st));
  }
  for (int i = 0; i < P; ++i) std::memcpy(out_host + i * oA, h_out + (size_t)i * stride_n * A, sizeof(double) * oA);
  return GCRL_OK;
}

int gcrl_pop_process_step(gcrl_pop* p, gcrl_her* const* rings, gcrl_normalizer* const* nz_obs, int32_t update_stats, gcrl_normalizer* const* nz_dg,
                          int32_t update_goal_stats, const float* obs_host, const float* next_obs_host, int32_t obs_dim, const float* dg_host,
                          const float* next_dg_host, const float* ag_host, const float* next_ag_host, const float* actions_host,
                          const float* rewards_host, const uint8_t* dones_host, int32_t env0, int32_t n, int64_t* rows_out, void* stream) {
  // every refusal before any device work (the per-member ones: her_process_step_pop)
  GCRL_CHECK_ARG(rings, "gcrl_pop_process_step: rings: null array");
  GCRL_CHECK_ARG(obs_host && next_obs_host, "gcrl_pop_process_step: obs_host / next_obs_host: null array");
  GCRL_CHECK_ARG(dg_host && next_dg_host && next_ag_host, "gcrl_pop_process_step: dg_host / next_dg_host / next_ag_host: null array");
  GCRL_CHECK_ARG(actions_host && rewards_host && dones_host, "gcrl_pop_process_step: actions_host / rewards_host / dones_host: null array");
  GCRL_CHECK_ARG(rows_out, "gcrl_pop_process_step: rows_out: null array");
  GCRL_CHECK_ARG(p, "gcrl_pop_process_step: pop: null handle");
  return her_process_step_pop(&p->proc, (int)p->m.size(), rings, nz_obs, update_stats, nz_dg, update_goal_stats, obs_host, next_obs_host, obs_dim,
                              dg_host, next_dg_host, ag_host, next_ag_host, actions_host, rewards_host, dones_host, env0, n, rows_out, stream);
}

int gcrl_pop_acting_counts(const gcrl_pop* p, int64_t* act_calls, int64_t* act_launches, int64_t* proc_calls, int64_t* proc_launches,
                           int64_t* act_staged) {
  GCRL_CHECK_ARG(p, "gcrl_pop_acting_counts: pop: null handle");
  if (act_calls) *act_calls = p->act_calls;
  if (act_launches) *act_launches = p->act_launches;
  if (proc_calls) *proc_calls = p->proc.calls;
  if (proc_launches) *proc_launches = p->proc.launches;
  if (act_staged) *act_staged = p->act_staged;
  return GCRL_OK;
}

// ---------------------------------------------------------------- population-based training: clone, re-tune, replace (pbt_host.h)

int gcrl_pop_clone(gcrl_pop* p, gcrl_her* const* rings, const int32_t* src, const int32_t* dst, int32_t pairs, uint32_t what, void* stream) {
  // every refusal before any device work
  GCRL_CHECK_ARG(p, "gcrl_pop_clone: pop: null handle");
  const int P = (int)p->m.size();
  char why[256];
  if (!pop_clone_check(P, src, dst, pairs, what, why, sizeof(why))) return fail(GCRL_ERR_ARG, "gcrl_pop_clone: %s", why);
  const bool with_agent = (what & GCRL_CLONE_AGENT) != 0, with_ring = (what & GCRL_CLONE_RING) != 0;
  for (int k = 0; k < pairs; ++k)
    for (const int i : {src[k], dst[k]})
      if (p->m[i]->bc_weight > 0.0) return fail(GCRL_ERR_STATE, "gcrl_pop_clone: bc_weight: member %d has the behaviour-cloning term on; populations do not carry it", i);
  if (with_ring) {
    GCRL_CHECK_ARG(rings, "gcrl_pop_clone: rings: null array with GCRL_CLONE_RING");
    for (int k = 0; k < pairs; ++k) {
      const gcrl_her* s = rings[src[k]];
      const gcrl_her* d = rings[dst[k]];
      GCRL_CHECK_ARG(s, "gcrl_pop_clone: rings: member %d has no replay ring", src[k]);
      GCRL_CHECK_ARG(d, "gcrl_pop_clone: rings: member %d has no replay ring", dst[k]);
      GCRL_CHECK_ARG(s != d, "gcrl_pop_clone: rings: members %d and %d share a replay ring", src[k], dst[k]);
      if (her_prio_on(s) || her_prio_on(d))
        return fail(GCRL_ERR_STATE, "gcrl_pop_clone: prioritise: a ring with an energy tree is not cloned (members %d, %d)", src[k], dst[k]);
      if (her_td_on(s) || her_td_on(d))
        return fail(GCRL_ERR_STATE, "gcrl_pop_clone: prioritise: a ring with a TD-error tree is not cloned (members %d, %d)", src[k], dst[k]);
#define GCRL_RING_SAME(expr, field) \
  GCRL_CHECK_ARG(s->expr == d->expr, "gcrl_pop_clone: %s: member %d's ring has %lld, member %d's %lld", field, src[k], (long long)s->expr, dst[k], (long long)d->expr)
      GCRL_RING_SAME(cfg.capacity, "capacity");
      GCRL_RING_SAME(S, "state_dim"); GCRL_RING_SAME(A, "action_dim"); GCRL_RING_SAME(G, "goal_dim");
      if (s->relabel_mode != d->relabel_mode)   // (sample-time relabelling: the records carry tails the other mode's do not)
        return fail(GCRL_ERR_STATE, "gcrl_pop_clone: relabel: member %d's ring has relabel mode %d, member %d's %d", src[k], s->relabel_mode, dst[k], d->relabel_mode);
      if (s->goal_strategy != d->goal_strategy)   // (the record widths differ, and a goal pick of one strategy reads tails the other's lack)
        return fail(GCRL_ERR_STATE, "gcrl_pop_clone: goal_strategy: member %d's ring has goal strategy %d, member %d's %d", src[k], s->goal_strategy, dst[k], d->goal_strategy);
      if (s->normalize_mode != d->normalize_mode)   // (raw rows in a ring whose gathers do not normalise, or the reverse)
        return fail(GCRL_ERR_STATE, "gcrl_pop_clone: normalize: member %d's ring has normalize mode %d, member %d's %d", src[k], s->normalize_mode, dst[k], d->normalize_mode);
      GCRL_RING_SAME(RS, "record_floats"); GCRL_RING_SAME(RG, "staged_record_floats");
      GCRL_RING_SAME(cfg.nenvs, "nenvs"); GCRL_RING_SAME(cfg.flush_len, "flush_len"); GCRL_RING_SAME(cfg.k_future, "k_future");
#undef GCRL_RING_SAME
    }
  }
  uint32_t involved = 0;
  for (int k = 0; k < pairs; ++k) involved |= (1u << src[k]) | (1u << dst[k]);
  for (int i = 0; i < P; ++i)
    if ((involved >> i) & 1u) GCRL_CHECK_ARG(!p->m[i]->deferred.her, "gcrl_pop_clone: member %d is inside an update call", i);
  // the segment table: one entry per state allocation and pair (what gcrl_agent_save_state puts in its blob), then the rings' filled parts
  std::vector<CloneSeg> segs;
  for (int k = 0; k < pairs; ++k) {
    gcrl_agent* s = p->m[src[k]];
    gcrl_agent* d = p->m[dst[k]];
    if (with_agent) {
      const unsigned long long bn = (unsigned long long)std::max(1, s->L * s->H) * sizeof(float);
      clone_add(segs, s->params, d->params, (unsigned long long)s->n_params * sizeof(float));
      clone_add(segs, s->adam_m, d->adam_m, (unsigned long long)s->n_grads * sizeof(float));
      clone_add(segs, s->adam_v, d->adam_v, (unsigned long long)s->n_grads * sizeof(float));
      clone_add(segs, s->bn_rmean, d->bn_rmean, bn);
      clone_add(segs, s->bn_rvar, d->bn_rvar, bn);
      clone_add(segs, s->alpha_dev, d->alpha_dev, sizeof(float));
    }
    if (with_ring) {
      const gcrl_her* hs = rings[src[k]];
      gcrl_her* hd = rings[dst[k]];
      clone_add(segs, hs->stage, hd->stage, (unsigned long long)hs->cfg.nenvs * hs->cfg.flush_len * hs->RG * sizeof(float));
      clone_add_ring_rows(segs, hs->ring, hd->ring, hs->head, hs->len, hs->cfg.capacity, hs->RS);
    }
  }
  gcrl_agent* a0 = p->m[0];
  hipStream_t st = a0->pick(stream);
  // after the last update call of every member involved (DESIGN.md 4c: the event that closes a handle's update work)
  for (int i = 0; i < P; ++i) {
    gcrl_agent* a = p->m[i];
    if (((involved >> i) & 1u) && a->calls > 0) GCRL_HIP(hipStreamWaitEvent(st, a->call_ev[(a->calls - 1) % kEventRing], 0));
  }
  void* tab_dev = nullptr;
  if (p->clone_tabs.get(segs.data(), segs.size() * sizeof(CloneSeg), st, &tab_dev)) return fail(GCRL_ERR_HIP, "gcrl_pop_clone: segment table upload failed");
  TRY(launch_pop_clone(st, tab_dev, (int)segs.size(), clone_chunks(segs, 128)));
  // host state, and the destination's derived state as gcrl_agent_load_state / gcrl_her_load_state leave it
  for (int k = 0; k < pairs; ++k) {
    const gcrl_agent* s = p->m[src[k]];
    gcrl_agent* d = p->m[dst[k]];
    if (with_agent) {
      d->t_actor = s->t_actor; d->t_critic = s->t_critic; d->t_alpha = s->t_alpha;
      d->lr_actor = s->lr_actor; d->lr_critic = s->lr_critic; d->rng_ctr = s->rng_ctr;
      d->wt_dirty = true;
    }
    if (with_ring) {
      const gcrl_her* hs = rings[src[k]];
      gcrl_her* hd = rings[dst[k]];
      hd->staged = hs->staged;
      hd->head = 0; hd->len = hs->len;
      hd->episodes_flushed = hs->episodes_flushed; hd->draws_done = hs->draws_done; hd->mutation_epoch = hs->mutation_epoch + 1;
      hd->relabel_ctr = hs->relabel_ctr;
    }
  }
  // the launch closes the work so far of every member involved: a destination's next update, acting or metrics call, and a source's
  // next write, are ordered after it on whatever stream they run
  for (int i = 0; i < P; ++i)
    if ((involved >> i) & 1u) TRY(end_call(p->m[i], st));
  return GCRL_OK;
}

int gcrl_agent_set_hparams(gcrl_agent* a, const gcrl_hparams* h) {
  GCRL_CHECK_ARG(a, "gcrl_agent_set_hparams: agent: null handle");
  char why[256];
  if (!hparams_check(h, a->sac, why, sizeof(why))) return fail(GCRL_ERR_ARG, "gcrl_agent_set_hparams: %s", why);
  GCRL_CHECK_ARG(!a->deferred.her && a->dp_pos >= a->dp_segs.size(), "gcrl_agent_set_hparams: agent: the handle is inside an update call");
  if (!a->graphs.empty()) {   // captured steps hold the old gamma / tau / clip as kernel arguments
    GCRL_HIP(hipDeviceSynchronize());
    for (auto& kv : a->graphs) (void)hipGraphExecDestroy(kv.second);
    a->graphs.clear();
  }
  gcrl_agent_config& c = a->cfg;
  c.actor_lr = h->actor_lr; c.actor_lr_min = h->actor_lr_min; c.ac_scheduler_steps = h->ac_scheduler_steps;
  c.critic_lr = h->critic_lr; c.critic_lr_min = h->critic_lr_min; c.cr_scheduler_steps = h->cr_scheduler_steps;
  c.gamma = h->gamma; c.tau = h->tau; c.grad_clip = h->grad_clip;
  if (a->sac) { c.alpha_lr = h->alpha_lr; c.alpha_min_steps = h->alpha_min_steps; }
  // positions kept: the rate an agent constructed with the new schedule holds after the same number of scheduler steps
  a->lr_actor = cosine_lr_at(c.actor_lr, c.actor_lr_min, c.ac_scheduler_steps, a->t_actor);
  a->lr_critic = cosine_lr_at(c.critic_lr, c.critic_lr_min, c.cr_scheduler_steps, a->t_critic);
  return GCRL_OK;
}

int gcrl_pop_replace(gcrl_pop* p, int32_t i, const gcrl_agent_config* cfg) {
  // every refusal before any device work
  GCRL_CHECK_ARG(p, "gcrl_pop_replace: pop: null handle");
  GCRL_CHECK_ARG(i >= 0 && i < (int32_t)p->m.size(), "gcrl_pop_replace: i: member %d of %d", i, (int)p->m.size());
  GCRL_CHECK_ARG(cfg, "gcrl_pop_replace: cfg: null config");
  gcrl_agent* a = p->m[i];
  // (the member's own configuration holds every shared field of the population, and everything the creating entry checked about shapes)
  if (const char* f = pop_mismatch(a->cfg, *cfg)) return fail(GCRL_ERR_ARG, "gcrl_pop_replace: %s: the new member must share it with the population", f);
  if (cfg->kind == GCRL_AGENT_TQC) GCRL_CHECK_ARG(cfg->top_drop >= 0 && cfg->top_drop < cfg->num_critics, "gcrl_pop_replace: top_drop: 0 <= top_drop < num_critics");
  {   // the re-tunable fields as gcrl_agent_set_hparams takes them
    const gcrl_hparams h = hparams_of(*cfg);
    char why[256];
    if (!hparams_check(&h, a->sac, why, sizeof(why))) return fail(GCRL_ERR_ARG, "gcrl_pop_replace: %s", why);
  }
  GCRL_CHECK_ARG(!a->deferred.her && !a->xchg && a->bn_sync.world <= 1, "gcrl_pop_replace: i: member %d is inside an update call or a data-parallel group", i);
  GCRL_HIP(hipDeviceSynchronize());
  TRY(meet_check(a));
  for (auto& kv : a->graphs) (void)hipGraphExecDestroy(kv.second);   // captured steps hold the old gamma / tau / clip as kernel arguments
  a->graphs.clear();
  a->cfg = *cfg;
  a->lr_actor = cfg->actor_lr; a->lr_critic = cfg->critic_lr;
  a->t_actor = a->t_critic = a->t_alpha = 0;
  a->rng_ctr = 0;
  GCRL_HIP(hipMemset(a->adam_m, 0, (size_t)a->n_grads * sizeof(float)));
  GCRL_HIP(hipMemset(a->adam_v, 0, (size_t)a->n_grads * sizeof(float)));
  GCRL_HIP(hipMemset(a->grads, 0, (size_t)a->n_grads * sizeof(float)));
  GCRL_HIP(hipMemset(a->params, 0, (size_t)a->n_params * sizeof(float)));
  // step counts are zero: the call below takes its construction path (BatchNorm affine and statistics, hard-copied targets, log_alpha)
  return gcrl_agent_init_weights(a, cfg->seed, 1);
}

}  // extern "C"

// ---------------------------------------------------------------- population collect and evaluation on a gcrl_env_group (dev_env.h)
namespace {

// what gcrl_pop_collect and gcrl_pop_evaluate share of their checks: the group against the members (field names as gcrl_agent_collect's)
int pop_group_check(gcrl_pop* p, gcrl_env_group* g, gcrl_normalizer* const* nz_obs, gcrl_normalizer* const* nz_dg, int eval_mode, const char* who) {
  const int P = (int)p->m.size();
  gcrl_agent* a0 = p->m[0];
  GCRL_CHECK_ARG(g->P == P, "%s: env: the group has %d members, the population %d", who, g->P, P);
  GCRL_CHECK_ARG(g->device == a0->cfg.device, "%s: env: it lives on device %d, the population on device %d", who, g->device, a0->cfg.device);
  GCRL_CHECK_ARG(g->N <= a0->B, "%s: env: %d envs per member exceed batch_size %d (the acting launch takes 1..batch_size rows)", who, g->N, a0->B);
  GCRL_CHECK_ARG(g->N <= kEnvMaxN, "%s: env: %d envs per member (at most %d)", who, g->N, kEnvMaxN);
  GCRL_CHECK_ARG(g->D + kEnvG == a0->S && g->A == a0->A, "%s: env: obs_dim %d + goal_dim %d / action_dim %d, the members have state_dim %d / action_dim %d", who,
                 g->D, kEnvG, g->A, a0->S, a0->A);
  GCRL_CHECK_ARG(4 * round_up(a0->S, 4) <= 2 * kRowThreads || a0->sac || !(nz_obs || nz_dg), "%s: env: fused normalisation supports state_dim <= 128", who);
  for (int i = 0; i < P; ++i)
    TRY(act_dev_check(p->m[i], nz_obs ? nz_obs[i] : nullptr, nz_dg ? nz_dg[i] : nullptr, g->D, g->N, eval_mode, who));
  return GCRL_OK;
}

// The population acting launch on the group's rows: float64 actions of the members in `live` to the group's action block.  mode: 1 with the
// group's noise block added (SAC / TQC: its eps), else the eval mode.  After every member's last update call and on fresh weight copies,
// as gcrl_pop_observe_act orders and rebuilds them.
int pop_group_act(gcrl_pop* p, gcrl_env_group* g, gcrl_normalizer* const* nz_obs, gcrl_normalizer* const* nz_dg, unsigned int live, bool explore,
                  int eval_mode, hipStream_t st, int64_t* launches) {
  const int P = (int)p->m.size();
  gcrl_agent* a0 = p->m[0];
  const int N = g->N, D = g->D, S = a0->S, A = a0->A;
  p->act_ordered.resize(P, 0);
  for (int i = 0; i < P; ++i) {
    gcrl_agent* a = p->m[i];
    if (a->calls != p->act_ordered[i]) {
      GCRL_HIP(hipStreamWaitEvent(st, a->call_ev[(a->calls - 1) % kEventRing], 0));
      p->act_ordered[i] = a->calls;
    }
    if (!a0->sac && ((live >> i) & 1u) && a->wt_dirty) {
      *launches += 1 + (a->has_target_actor ? 1 : 0) + 2 * a->C;
      TRY(rc_rebuild_wt(a, st));
    }
  }
  void* tab_dev = nullptr;
  if (a0->sac) {
    ActBnArgs tab[kMaxPopMembers];
    for (int i = 0; i < P; ++i) {
      gcrl_agent* a = p->m[i];
      ActBnArgs& ba = tab[i];
      std::memset(&ba, 0, sizeof(ba));
      ba.P = a->P_actor(); ba.rmean = a->bn_rmean; ba.rvar = a->bn_rvar;
      ba.S = S; ba.H = a->H; ba.L = a->L; ba.A = A; ba.n = N; ba.D = D;
      ba.ldl = (std::max(S, a->H) + 3) / 4 * 4;
      gcrl::normalizer_view(nz_obs ? nz_obs[i] : nullptr, &ba.nz_mean, &ba.nz_var, nullptr, &ba.nz_clip, &ba.nz_mode);
      gcrl::normalizer_view(nz_dg ? nz_dg[i] : nullptr, &ba.nzg_mean, &ba.nzg_var, nullptr, &ba.nzg_clip, &ba.nzg_mode);
    }
    if (p->act_tabs.get(tab, sizeof(ActBnArgs) * P, st, &tab_dev)) return fail(GCRL_ERR_HIP, "gcrl_pop_collect: argument table upload failed");
    ActBnPop c;
    c.tab = static_cast<const ActBnArgs*>(tab_dev);
    c.rows = g->rows; c.eps = g->noise64; c.out = g->act64; c.flags = nullptr;
    c.seq = ++p->act_seq;
    c.with_eps = explore ? 1 : 0; c.stride_n = g->stride_n;
    TRY(launch_act_bn_pop(st, c, tab[0], P));
  } else {
    const int mode = explore ? 1 : eval_mode;
    RowActArgs tab[kMaxPopMembers];
    for (int i = 0; i < P; ++i) {
      gcrl_agent* a = p->m[i];
      RowActArgs& ra = tab[i];
      std::memset(&ra, 0, sizeof(ra));
      ra.actor = make_rownet(a, a->actor, a->P_actor(), 0);
      ra.ld_obs = S; ra.out = a->dact; ra.ld_out = a->Apad;
      ra.n = N; ra.S = S; ra.A = A; ra.ldl = a->row_ldl;
      ra.D = D;
      gcrl::normalizer_view(nz_obs ? nz_obs[i] : nullptr, &ra.nz_mean, &ra.nz_var, nullptr, &ra.nz_clip, &ra.nz_mode);
      gcrl::normalizer_view(nz_dg ? nz_dg[i] : nullptr, &ra.nzg_mean, &ra.nzg_var, nullptr, &ra.nzg_clip, &ra.nzg_mode);
      ra.post = mode == 1 ? 1 : (mode == 0 ? 2 : 3);
    }
    if (p->act_tabs.get(tab, sizeof(RowActArgs) * P, st, &tab_dev)) return fail(GCRL_ERR_HIP, "gcrl_pop_collect: argument table upload failed");
    RowActPop c;
    c.tab = static_cast<const RowActArgs*>(tab_dev);
    c.rows = g->rows; c.noise = g->noise64; c.out = g->act64; c.flags = nullptr;
    c.seq = ++p->act_seq;
    c.live = live; c.noisy = explore ? live : 0u; c.stride_n = g->stride_n;
    TRY(launch_rowchain_act_pop(st, c, P, N, a0->row_ldl, A, a0->H));
  }
  *launches += 1;
  return GCRL_OK;
}

}  // namespace

extern "C" {

int gcrl_pop_collect(gcrl_pop* p, gcrl_env_group* g, gcrl_her* const* rings, gcrl_normalizer* const* nz_obs, int32_t update_stats,
                     gcrl_normalizer* const* nz_dg, int32_t update_goal_stats, int32_t steps, int32_t explore, int32_t eval_mode, int64_t* rows_out,
                     void* stream) {
  const char* who = "gcrl_pop_collect";
  // every refusal comes before a counter, a ring slot or a draw of an exploration stream is consumed
  GCRL_CHECK_ARG(p, "%s: pop: null handle", who);
  GCRL_CHECK_ARG(g, "%s: env: null group handle", who);
  GCRL_CHECK_ARG(rings, "%s: rings: null array", who);
  GCRL_CHECK_ARG(rows_out, "%s: rows_out: null array", who);
  GCRL_CHECK_ARG(steps >= 1, "%s: steps: %d (>= 1 required)", who, steps);
  const int P = (int)p->m.size();
  gcrl_agent* a0 = p->m[0];
  TRY(pop_group_check(p, g, nz_obs, nz_dg, eval_mode, who));
  const int N = g->N;
  for (int i = 0; i < P; ++i) {
    gcrl_her* h = rings[i];
    GCRL_CHECK_ARG(h, "%s: rings: member %d has no replay ring", who, i);
    for (int j = 0; j < i; ++j)
      GCRL_CHECK_ARG(rings[j] != h, "%s: shared_ring: members %d and %d share a replay ring; one ring and one normaliser pair cannot take the merged staging launch", who, j, i);
    GCRL_CHECK_ARG(N <= h->cfg.nenvs, "%s: env: %d envs per member for a ring of %d episode slots (member %d)", who, N, h->cfg.nenvs, i);
    GCRL_CHECK_ARG(g->D + kEnvG == h->S && g->A == h->A && kEnvG == h->G, "%s: env: obs_dim %d + goal_dim %d / action_dim %d, member %d's ring has state_dim %d / action_dim %d / goal_dim %d",
                   who, g->D, kEnvG, g->A, i, h->S, h->A, h->G);
    GCRL_CHECK_ARG(g->T == h->cfg.flush_len, "%s: max_steps: the group's horizon %d differs from the flush length %d of member %d's ring", who, g->T, h->cfg.flush_len, i);
    GCRL_CHECK_ARG(h->cfg.reward_kind == GCRL_REWARD_SPARSE, "%s: compute_reward: the reward kind of member %d's ring is %s; the env's reward is the built-in sparse kind", who, i,
                   h->cfg.reward_kind == GCRL_REWARD_HOST ? "a host callback" : "dense");
    GCRL_CHECK_ARG(std::memcmp(&g->thr, &h->cfg.reward_threshold, sizeof(float)) == 0, "%s: threshold: the group's %g differs from the %g of member %d's ring", who, g->thr,
                   h->cfg.reward_threshold, i);
    GCRL_CHECK_ARG(h->normalize_mode == rings[0]->normalize_mode, "%s: normalize: member %d's ring has normalize mode %d, member 0's %d", who, i, h->normalize_mode,
                   rings[0]->normalize_mode);
    GCRL_CHECK_ARG(!update_stats || (nz_obs && nz_obs[i]), "%s: nz_obs: update_stats without an observation normaliser (member %d)", who, i);
    GCRL_CHECK_ARG(!update_goal_stats || (nz_dg && nz_dg[i]), "%s: nz_dg: update_goal_stats without a goal normaliser (member %d)", who, i);
  }
  for (int i = 0; i < P; ++i)
    for (int e = 0; e < N; ++e)
      if (g->t_host[(size_t)i * N + e] != rings[i]->staged[e])
        return gcrl::fail(GCRL_ERR_STATE, "%s: t: env %d of member %d is at step %d of its episode, the member's ring has %d transitions staged for it", who, e, i,
                          g->t_host[(size_t)i * N + e], rings[i]->staged[e]);
  if (P == 1) {   // nothing to merge: the member's own loop on the group's one member
    const long long s0 = a0->col_steps, l0 = a0->col_launches;
    const int rc = agent_collect_group(a0, g, rings[0], nz_obs ? nz_obs[0] : nullptr, update_stats, nz_dg ? nz_dg[0] : nullptr, update_goal_stats, steps, explore,
                                       eval_mode, rows_out, stream);
    p->col_calls += 1; p->col_steps += a0->col_steps - s0; p->col_launches += a0->col_launches - l0;
    return rc;
  }
  hipStream_t st = a0->pick(stream);
  void* sarg = stream ? stream : (void*)a0->stream;   // one stream for all handles: the loop is stream-ordered
  p->col_calls += 1;
  const bool ddpg = a0->cfg.kind == GCRL_AGENT_DDPG;
  const unsigned long long per_step = (unsigned long long)N * g->A;
  int flush_mul[kMaxPopMembers];
  for (int i = 0; i < P; ++i) { flush_mul[i] = 1 + (gcrl::her_prio_on(rings[i]) ? 1 : 0) + (gcrl::her_td_on(rings[i]) ? 1 : 0); rows_out[i] = 0; }
  gcrl::EnvPopMember mem[kMaxPopMembers];
  int64_t rows_step[kMaxPopMembers];
  for (int s = 0; s < steps; ++s) {
    unsigned int live = 0;
    std::memset(mem, 0, sizeof(mem));
    for (int i = 0; i < P; ++i) {
      gcrl_agent* a = p->m[i];
      const unsigned long long c = a->col_ctr;
      const double scale = a->sac ? 1.0 : a->col_noise_std;
      double* noise_i = g->noise64 + (size_t)i * g->stride_n * g->A;
      const bool eps_step = explore && ddpg && a->col_epsilon > 0.0 &&
                            (double)gcrl::hash_below(a->col_seed, kEpsStream, c, 1u << 24) * (1.0 / 16777216.0) < a->col_epsilon;
      gcrl::EnvPopMember& em = mem[i];
      if (eps_step) {   // the member's envs form clip(randn) themselves: no network, no fill
        em.src = gcrl::kEnvActEps; em.eps_ctr0 = c * per_step;
      } else {
        live |= 1u << i;
        if (explore && !(a->col_noise_valid && a->col_noise_env == g->token && a->col_noise_ctr == c)) {   // (a first call, or after the stream was set)
          TRY(gcrl::normal_fill(noise_i, 1, (int)per_step, a->col_seed, c * per_step, scale, st));
          p->col_launches += 1;
        }
        em.src = gcrl::kEnvActF64; em.act = g->act64 + (size_t)i * g->stride_n * g->A;
      }
      em.eps_seed = a->col_seed ^ kEpsStream;
      em.noise_on = explore ? 1 : 0; em.noise_seed = a->col_seed; em.noise_ctr0 = (c + 1) * per_step; em.noise_scale = scale;
    }
    if (live) TRY(pop_group_act(p, g, nz_obs, nz_dg, live, explore != 0, eval_mode, st, &p->col_launches));
    TRY(gcrl::env_group_step_launch(g, mem, st));
    p->col_launches += 1;
    for (int i = 0; i < P; ++i) {
      gcrl_agent* a = p->m[i];
      if (explore) { a->col_noise_valid = true; a->col_noise_env = g->token; a->col_noise_ctr = a->col_ctr + 1; }
      a->col_ctr += 1;
    }
    p->col_steps += 1;
    int64_t f0[kMaxPopMembers];
    for (int i = 0; i < P; ++i) f0[i] = rings[i]->flush_calls;
    const int rc = gcrl::her_process_step_pop_dev(&p->proc, P, rings, nz_obs, update_stats, nz_dg, update_goal_stats, g->data, g->stride, g->raw_floats, g->D, N,
                                                  rows_step, sarg);
    p->col_launches += 1;
    for (int i = 0; i < P; ++i) p->col_launches += (rings[i]->flush_calls - f0[i]) * flush_mul[i];
    if (rc) return rc;
    for (int i = 0; i < P; ++i) rows_out[i] += rows_step[i];
  }
  return GCRL_OK;
}

int gcrl_pop_collect_counts(const gcrl_pop* p, int64_t* calls, int64_t* steps, int64_t* launches, int64_t* copies, int64_t* syncs) {
  GCRL_CHECK_ARG(p, "gcrl_pop_collect_counts: pop: null handle");
  if (calls) *calls = p->col_calls;
  if (steps) *steps = p->col_steps;
  if (launches) *launches = p->col_launches;
  if (copies) *copies = p->col_copies;
  if (syncs) *syncs = p->col_syncs;
  return GCRL_OK;
}

int gcrl_pop_evaluate(gcrl_pop* p, gcrl_env_group* g, gcrl_normalizer* const* nz_obs, gcrl_normalizer* const* nz_dg, int32_t episodes, int32_t reset,
                      int32_t eval_mode, int64_t* episodes_out, int64_t* successes_out, double* reward_sum_out, void* stream) {
  const char* who = "gcrl_pop_evaluate";
  GCRL_CHECK_ARG(p, "%s: pop: null handle", who);
  GCRL_CHECK_ARG(g, "%s: env: null group handle", who);
  GCRL_CHECK_ARG(episodes >= 1, "%s: episodes: %d (>= 1 required)", who, episodes);
  const int P = (int)p->m.size();
  gcrl_agent* a0 = p->m[0];
  TRY(pop_group_check(p, g, nz_obs, nz_dg, eval_mode, who));
  const int N = g->N;
  const size_t PN = (size_t)P * N;
  if (!reset)
    for (size_t e = 0; e < PN; ++e)
      if (g->t_host[e] != 0)
        return gcrl::fail(GCRL_ERR_STATE, "%s: t: env %d of member %d is at step %d of its episode; reset == 0 scores whole episodes only", who, (int)(e % N),
                          (int)(e / N), g->t_host[e]);
  hipStream_t st = a0->pick(stream);
  void* sarg = stream ? stream : (void*)a0->stream;
  const size_t cn_b = PN * 3 * sizeof(unsigned long long), rs_b = PN * sizeof(double);
  if (reset) {
    TRY(gcrl_env_group_reset(g, nullptr, sarg));
  } else {   // the counters as they stand, kept on the device: the call's one synchronisation comes at its end
    if (!p->eval_snap) GCRL_HIP(hipMalloc((void**)&p->eval_snap, (size_t)kMaxPopMembers * kEnvMaxN * (3 * sizeof(unsigned long long) + sizeof(double))));
    GCRL_HIP(hipMemcpyAsync(p->eval_snap, g->cnt, cn_b, hipMemcpyDeviceToDevice, st));
    GCRL_HIP(hipMemcpyAsync(p->eval_snap + cn_b, g->rsum, rs_b, hipMemcpyDeviceToDevice, st));
  }
  gcrl::EnvPopMember mem[kMaxPopMembers];
  std::memset(mem, 0, sizeof(mem));
  for (int i = 0; i < P; ++i) { mem[i].src = gcrl::kEnvActF64; mem[i].act = g->act64 + (size_t)i * g->stride_n * g->A; }
  const int rounds = (episodes + N - 1) / N;
  const unsigned int live = P >= 32 ? ~0u : ((1u << P) - 1u);
  int64_t launches = 0;
  for (int s = 0; s < rounds * g->T; ++s) {
    TRY(pop_group_act(p, g, nz_obs, nz_dg, live, false, eval_mode, st, &launches));
    TRY(gcrl::env_group_step_launch(g, mem, st));
  }
  std::vector<unsigned long long> cn0(PN * 3, 0ull), cn1(PN * 3);
  std::vector<double> rs0(PN, 0.0), rs1(PN);
  if (!reset) {
    GCRL_HIP(hipMemcpyAsync(cn0.data(), p->eval_snap, cn_b, hipMemcpyDeviceToHost, st));
    GCRL_HIP(hipMemcpyAsync(rs0.data(), p->eval_snap + cn_b, rs_b, hipMemcpyDeviceToHost, st));
  }
  GCRL_HIP(hipMemcpyAsync(cn1.data(), g->cnt, cn_b, hipMemcpyDeviceToHost, st));
  GCRL_HIP(hipMemcpyAsync(rs1.data(), g->rsum, rs_b, hipMemcpyDeviceToHost, st));
  GCRL_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < P; ++k) {
    int64_t ep = 0, su = 0; double r1 = 0.0, r0 = 0.0;
    for (int i = 0; i < N; ++i) {
      const size_t e = (size_t)k * N + i;
      ep += (int64_t)(cn1[e * 3 + 1] - cn0[e * 3 + 1]); su += (int64_t)(cn1[e * 3 + 2] - cn0[e * 3 + 2]);
      r1 += rs1[e]; r0 += rs0[e];
    }
    if (episodes_out) episodes_out[k] = ep;
    if (successes_out) successes_out[k] = su;
    if (reward_sum_out) reward_sum_out[k] = r1 - r0;
  }
  return GCRL_OK;
}

void gcrl_pop_destroy(gcrl_pop* p) {
  if (!p) return;
  for (gcrl_agent* a : p->m) gcrl_agent_destroy(a);   // (synchronises the device)
  p->act_tabs.release();
  p->clone_tabs.release();
  if (p->act_blk_host) (void)hipHostFree(p->act_blk_host);
  if (p->act_st_host) (void)hipHostFree(p->act_st_host);
  if (p->act_st_dev) (void)hipFree(p->act_st_dev);
  her_process_step_pop_release(&p->proc);
  if (p->eval_snap) (void)hipFree(p->eval_snap);
  for (auto& kv : p->tabs) (void)hipFree(kv.second);
  delete p;
}

}  // extern "C"
