// agent_pop.inc — DDPG and TD3 populations (include/gcrl.h gcrl_pop_*; included at the end of agent.hip).
//
// P independent DDPG or TD3 agents of one kind and equal shapes whose update steps share launches.  Each member is an ordinary gcrl_agent (its own
// parameters, optimiser state, control block, metric ring and meeting counters), so every single-agent entry works on it.  A
// population call records each member's launch sequence of the call (pop.h: the launchers record instead of launching), then
// issues position k of all sequences together: one launch of the kernel's population form (rowchain_ddpg_pop_kernel,
// dw_adam_pop_kernel, begin_step_pop_kernel, gemm_batch_pop_kernel<1, 1, 4>, adam_pop_kernel, adam_pair_pop_kernel), in which member m's workgroups read member m's own argument struct — the same
// arithmetic in the same order as the member's own launch, so each member computes bit for bit what it computes alone.
// Launches without a population form are issued member by member at their position.
//
// Admission (meet.h): a launch whose workgroups wait for each other is issued in its waiting form only when the WHOLE population
// launch is resident at once; otherwise the members record the no-wait form of that stage (same bits).

struct gcrl_pop {
  std::vector<gcrl_agent*> m;
  std::map<std::string, void*> tabs;   // device argument tables of the population launches, by content (they repeat call after call)
  std::vector<PopRec> rec;
  int64_t merged = 0, alone = 0;       // recorded positions issued as one population launch / member by member (gcrl_pop_launch_counts)
};

namespace {

constexpr int kMaxPopMembers = 16;

const char* pop_mismatch(const gcrl_agent_config& a, const gcrl_agent_config& b) {
#define GCRL_POP_SAME(f) if (a.f != b.f) return #f;
  GCRL_POP_SAME(kind) GCRL_POP_SAME(obs_dim) GCRL_POP_SAME(ac_dim) GCRL_POP_SAME(hidden_dim) GCRL_POP_SAME(layer_count)
  GCRL_POP_SAME(batch_size) GCRL_POP_SAME(num_critics) GCRL_POP_SAME(gradient_step) GCRL_POP_SAME(ac_update_freq)
  GCRL_POP_SAME(polyak_every) GCRL_POP_SAME(pipeline_steps) GCRL_POP_SAME(use_graph) GCRL_POP_SAME(device) GCRL_POP_SAME(n_quantiles)
#undef GCRL_POP_SAME
  return nullptr;
}

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
    default: return fail(GCRL_ERR_STATE, "gcrl_pop_update_n: launch kind %d has no population form", o.kind);
  }
}

// record member a's launches of m planned steps (stream capture around the recording: a launch that bypassed the recorder would
// land in the captured graph instead of running out of order — refused below).  DDPG: the overlapped schedule of
// gcrl_agent_update_n (run_steps_ddpg); TD3: its per-step phases with the variant bits gcrl_agent_update_n gives them on the
// row-chain path (every step pre-advanced, its last launch advancing the control block)
int pop_record_steps(gcrl_agent* a, hipStream_t cs, const std::vector<StepPlan>& plans, PopRec* rec) {
  rec->ops.clear();
  std::vector<int> variants(plans.size());
  for (size_t i = 0; i < plans.size(); ++i) variants[i] = plans[i].variant;
  GCRL_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
  pop_rec() = rec;
  g_pop_recorders.fetch_add(1);
  int rc = GCRL_OK;
  if (a->cfg.kind == GCRL_AGENT_TD3) {
    for (size_t i = 0; i < variants.size() && !rc; ++i) rc = run_step(a, cs, variants[i] | norm_bits(a) | V_ADV | V_PRE, 7, 1);
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

}  // namespace

std::atomic<int> gcrl::g_pop_recorders{0};

PopRec*& gcrl::pop_rec() {
  static thread_local PopRec* r = nullptr;
  return r;
}

extern "C" {

gcrl_pop* gcrl_pop_create(const gcrl_agent_config* cfgs, int32_t members) {
  auto bad = [](const char* field, const char* why) -> gcrl_pop* {
    fail(GCRL_ERR_ARG, "gcrl_pop_create: %s: %s", field, why);
    return nullptr;
  };
  // every refusal before any device work
  if (!cfgs) return bad("cfgs", "null config array");
  if (members < 1 || members > kMaxPopMembers) return bad("members", "a population has 1..16 members");
  for (int i = 0; i < members; ++i) {
    const gcrl_agent_config& c = cfgs[i];
    if (c.kind != GCRL_AGENT_DDPG && c.kind != GCRL_AGENT_TD3) return bad("kind", "populations are DDPG or TD3 (SAC / TQC populations are not implemented)");
    if (const char* f = pop_mismatch(cfgs[0], c)) return bad(f, "members must share kind, shapes, batch_size, gradient_step, ac_update_freq, polyak_every, pipeline_steps, use_graph and device");
    if (c.pipeline_steps != 2) return bad("pipeline_steps", "the population runs the row-chain DDPG step: pipeline_steps = 2");
    if (c.hidden_dim < 4 || c.hidden_dim % 4 != 0) return bad("hidden_dim", "the row-chain DDPG step needs hidden_dim % 4 == 0");
    if (c.ac_dim < 1 || c.ac_dim > 16 || c.obs_dim < 1 || c.layer_count < 1 || c.layer_count > 8 || c.batch_size < 1) return bad("shape", "bad obs_dim / ac_dim / layer_count / batch_size");
    if (c.use_graph >= 2) return bad("use_graph", "the population issues its launches itself (use_graph 0 or 1)");
  }
  const bool td3 = cfgs[0].kind == GCRL_AGENT_TD3;
  const int C = td3 ? 2 : 1;
  if (td3 && cfgs[0].num_critics != 2) return bad("num_critics", "a TD3 agent has two critics");
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
    if (!a->rowchain) { gcrl_pop_destroy(p); return bad("hidden_dim", "this configuration does not run the row-chain DDPG step"); }
    if (td3 && i == 0 && (a->split_k || a->rc_merge_k || a->dw_split_c > 1 || a->dw_split_a > 1)) {
      gcrl_pop_destroy(p);
      return bad("batch_size", "this TD3 configuration runs the role-split critic phase or the split dW form, which have no population form");
    }
  }
  p->rec.resize(members);
  return p;
}

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

int gcrl_pop_update_n(gcrl_pop* p, gcrl_her* const* rings, int64_t step0, int32_t n, int64_t* tickets_out, int32_t* tuple_len_out,
                      void* stream) {
  GCRL_CHECK_ARG(p && rings, "gcrl_pop_update_n: null handle");
  GCRL_CHECK_ARG(n >= 1, "gcrl_pop_update_n: n must be >= 1");
  const int P = (int)p->m.size();
  for (int i = 0; i < P; ++i) {
    gcrl_agent* a = p->m[i];
    GCRL_CHECK_ARG(rings[i], "gcrl_pop_update_n: member %d has no replay ring", i);
    GCRL_CHECK_ARG(!a->xchg && a->bn_sync.world <= 1, "gcrl_pop_update_n: member %d is in a data-parallel group", i);
    GCRL_CHECK_ARG(!a->prof, "gcrl_pop_update_n: member %d has launch profiling on", i);
    for (int j = 0; j < i; ++j) GCRL_CHECK_ARG(rings[j] != rings[i], "gcrl_pop_update_n: members %d and %d share a replay ring", j, i);
    // a process that arrived on this device after the handle was built: the forms with waits go off (as gcrl_agent_update_n)
    if ((a->calls & 31) == 0 && !meet_device_shared()) { const int rc = gcrl_agent_get_meetings(a); if (rc < 0) return rc; }
  }
  gcrl_agent* a0 = p->m[0];
  hipStream_t st = a0->pick(stream);
  // admission of the forms whose workgroups wait for each other: the whole population launch resident at once
  const long long nblk = (a0->B + 4 * a0->row_rg - 1) / (4 * a0->row_rg);
  bool ksplit = true, ofuse = true;
  for (gcrl_agent* a : p->m) { ksplit = ksplit && a->ddpg_ksplit; ofuse = ofuse && a->opt_fuse; }
  ksplit = ksplit && !meet_device_shared() && (long long)P * 3 * nblk <= std::max(a0->n_cus, 1);
  ofuse = ofuse && !meet_device_shared() && (P == 1 || (long long)P * a0->of_wgs <= dw_adam_pop_capacity());
  struct Forms { bool ksplit, ofuse, rowtile; };
  std::vector<Forms> saved(P);
  for (int i = 0; i < P; ++i) {
    gcrl_agent* a = p->m[i];
    saved[i] = Forms{a->ddpg_ksplit, a->opt_fuse, a->rowtile};
  }
  auto restore = [&]() { for (int i = 0; i < P; ++i) { p->m[i]->ddpg_ksplit = saved[i].ksplit; p->m[i]->opt_fuse = saved[i].ofuse; p->m[i]->rowtile = saved[i].rowtile; } };
  const int chunk = std::min(kMaxStepsPerCall, a0->Mmax);
  for (int done = 0; done < n; done += chunk) {
    const int m = std::min(chunk, n - done);
    std::vector<std::vector<StepPlan>> plans(P);
    // every member's batches first (their rings' index streams in member order), each gathered by its ring
    for (int i = 0; i < P; ++i) {
      gcrl_agent* a = p->m[i];
      if (a->wt_dirty) TRY(rc_rebuild_wt(a, st));
      TRY(begin_call(a, rings[i], step0 + done, m, nullptr, 1.0f, st, plans[i], tickets_out ? tickets_out + (size_t)i * n + done : nullptr,
                     tuple_len_out ? tuple_len_out + (size_t)i * n + done : nullptr, /*defer_rest=*/false, /*pre_advanced=*/true));
    }
    int rc = GCRL_OK;
    for (int i = 0; i < P && !rc; ++i) {
      gcrl_agent* a = p->m[i];
      a->ddpg_ksplit = ksplit; a->opt_fuse = ofuse; a->rowtile = false;
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

void gcrl_pop_destroy(gcrl_pop* p) {
  if (!p) return;
  for (gcrl_agent* a : p->m) gcrl_agent_destroy(a);   // (synchronises the device)
  for (auto& kv : p->tabs) (void)hipFree(kv.second);
  delete p;
}

}  // extern "C"
