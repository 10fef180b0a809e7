"""GPU (-m gpu): every optimiser launch form audited against torch's own Adam / AdamW ON THE GRADIENT THE ENGINE REPORTS.

The clip, the Adam(W) step, Polyak and the log-alpha step (csrc/adam_math.h, adam_device.inc, dw_adam_body.inc, adam_pop.hip,
`alpha_step` in csrc/ops.h) are otherwise checked only end to end, through gradients that carry fp32 reordering noise, and bit
for bit between launch forms that all include the same header.  Given the gradient the step is a deterministic function, so
here each audited `update(step)` is bracketed by reads of everything the optimiser reads and writes — parameters, moments,
targets, log_alpha and its moments before; the same and `grad:<net>` after — and (before, gradient, t, lr) goes to
tests/adam_ref.py: torch.optim.Adam / AdamW with clip_grad_norm_ in front, on the CPU in fp32 and fp64, and `held_step`'s bound
on the parameter step, the target's step, m, v (max-norm and per element in ulps) and the logged post-clip norm.  t and lr are
tracked per optimiser by the reference's rules (oracle/agent_oracle.py, SURVEY a14-a19: critics step every update, the actor
when step % ac_update_freq == 0, log_alpha on actor steps with step > alpha_min_steps; CosineAnnealingLR stepped after each
optimiser step), never read from the engine.

It is not a bitwise comparison with torch: torch's CPU lerp_ / addcmul_ fuse the multiply-add, adam_elem rounds every product;
about one moment word in eight differs in the last place.  "Same op order as torch" (adam_math.h) is about the order.  What IS
held bitwise, on top of the bound:
  * a net that does not step keeps p, m, v; a target keeps its words on a step without Polyak;
  * entries with an exactly zero gradient and zero moments move by the decay alone: fl(p * decay), p itself under Adam;
  * under an inactive clip the coefficient is exactly 1: m and v are then the unfused fp32 arithmetic on g itself, bit for bit
    (which also says that the gradient a launch reports is the one it consumed, the fused dW + optimiser launch included:
    tests/test_gpu_write_through.py states that against the two-launch form).

The per-element figures are judged per net and step against torch fp32's own figure of that step; the active-clip steps of a
net are judged together, against torch's worst figure over them (adam_ref.judge_units): there the figure is mostly the rounding
of the clip coefficient, one draw per net and step for either side.

Every case prints what it reached (clip active / inactive, entries where eps is visible, exact-zero gradients, Polyak and
non-Polyak steps, alpha and non-alpha steps, norms below 1e-3 above their clip) and fails when a count it claims is zero.  The
worst err/bound per kind, form and quantity, and the per-element unit figures (the device's and torch fp32's), go to
test_records/optimiser_audit.json in the tree, rewritten after every case.
"""
import json
import os

import numpy as np
import pytest
import torch

import adam_ref as ar
from adam_ref import F32
from oracle import her_oracle
from oracle.agent_oracle import make_config

pytestmark = pytest.mark.gpu

CLIP_ACTIVE, CLIP_INACTIVE = 1e-3, 1e3
RECORD = dict(worst={}, units={})


@pytest.fixture(autouse=True)
def _reference_on_one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _record(kind, form, rows):
    from conftest import ROOT
    for r in rows:
        key = f"{kind}/{form}/{r['quantity']}"
        RECORD["worst"][key] = max(RECORD["worst"].get(key, 0.0), r["ratio"])
        if "units" in r:
            u = RECORD["units"].setdefault(key, dict(device=0.0, torch_fp32=0.0))
            u["device"], u["torch_fp32"] = max(u["device"], r["units"]), max(u["torch_fp32"], r["units_torch32"])
    os.makedirs(os.path.join(ROOT, "test_records"), exist_ok=True)
    with open(os.path.join(ROOT, "test_records", "optimiser_audit.json"), "w") as f:
        json.dump(dict(note="optimiser launches vs torch Adam / AdamW on the engine's own gradient (tests/adam_ref.py held_step): worst "
                            "err/bound per kind / form / quantity (<= 1 passes); units: worst per-element error of m and v in ulps, the "
                            "device's and torch fp32's own", worst_err_over_bound=RECORD["worst"], units=RECORD["units"]), f, indent=1, sort_keys=True)


def covers(claims, counts):
    print("  covers " + " ".join(f"{k}={int(v)}" for k, v in counts.items()) + f"  (claims {sorted(claims)})")
    zero = [k for k in claims if int(counts[k]) == 0]
    assert not zero, f"the case misses {zero}"


# ------------------------------------------------------------------------------------------------------------------ the audit
class Audit:
    """Brackets `update(step)` of one agent (a standalone one or a population member)."""

    def __init__(self, ag, kind, cfg, gstep, form):
        self.ag, self.kind, self.cfg, self.gstep, self.form = ag, kind, cfg, gstep, form
        self.C = len(ag.critics)
        self.t = dict(actor=0, critic=0, alpha=0)
        self.lr_actor = ar.cosine_lrs(cfg.actor_lr, cfg.actor_lr_min, cfg.ac_scheduler_steps, 16)
        self.lr_critic = ar.cosine_lrs(cfg.critic_lr, cfg.critic_lr_min, cfg.cr_scheduler_steps, 16)
        self.counts = dict(clip_active=0, clip_inactive=0, eps_visible=0, zero_grad=0, still=0, polyak=0, no_polyak=0, alpha=0, no_alpha=0,
                           small_norm_above_clip=0, not_stepped=0)
        self.rows = []
        self.nets = ["actor"] + [f"critic_{i}" for i in range(self.C)]
        self.targets = ([] if ag._sac else ["target_actor"]) + [f"target_critic_{i}" for i in range(self.C)]

    def get(self, name):
        return self.ag.actor._get(name)

    def snapshot(self):
        s = {}
        for n in self.nets + (["log_alpha"] if self.ag._sac else []):
            s[n] = dict(p=self.get(n), m=self.get("adam_m:" + n), v=self.get("adam_v:" + n))
        for n in self.targets:
            s[n] = self.get(n)
        return s

    def clip_of(self, net):
        if net == "log_alpha" or self.cfg.grad_clip is None or (self.kind == "TD3" and net == "critic_0"):   # src/agent.py:201
            return -1.0
        return float(self.cfg.grad_clip)

    def check(self, step, before, info):
        """After `update(step)` returned `info`: audit every net."""
        kind, cfg = self.kind, self.cfg
        after = self.snapshot()
        tup = [float(x) for x in info]
        do_actor = step % cfg.ac_update_freq == 0
        do_alpha = self.ag._sac and do_actor and step > cfg.alpha_min_steps
        polyak_c = dict(DDPG=step % 40 == 0, TD3=True, SAC=step % self.gstep == 0, TQC=True)[kind]
        expect_len = dict(DDPG=(4, 6), TD3=(6, 8), SAC=(6, 9), TQC=(6, 9))[kind][1 if do_actor else 0]
        assert len(tup) == expect_len, (step, len(tup), expect_len)
        norm_at = {}          # net -> position of its post-clip norm in the tuple
        if kind == "DDPG":
            norm_at = {"critic_0": 4 if do_actor else 3, "actor": 5}
        elif kind in ("TD3", "SAC"):
            norm_at = {"critic_0": 5 if do_actor else 4, "critic_1": 6 if do_actor else 5, "actor": 7}
        else:
            norm_at = {"actor": 7}
        tqc_norms = []
        self.t["critic"] += 1                     # the optimisers' own step counts, by the reference's rules
        self.t["actor"] += int(do_actor)
        self.t["alpha"] += int(do_alpha)

        def same(x, y):
            return np.array_equal(ar.bits(x), ar.bits(y))

        def audit(net, which, target, polyak):
            t = self.t[which]
            lr = dict(actor=self.lr_actor, critic=self.lr_critic)[which][t - 1] if which != "alpha" else float(cfg.alpha_lr)
            b = dict(before[net], g=self.get("grad:" + net), grad_scale=1.0)
            if polyak:
                b["target"] = before[target]
            clip = self.clip_of(net)
            r32, r64, t32, t64 = ar.references(kind, b, t, lr, clip, cfg.tau if polyak else None)
            a = dict(after[net])
            if polyak:
                a["target"] = after[target]
            if net in norm_at:
                a["post_norm"] = tup[norm_at[net]]
            elif net.startswith("critic"):
                tqc_norms.append((r32.post_norm, r64.post_norm))
            what = f"s{step} {net}"
            active = clip >= 0 and r64.coef < 1.0
            rows = ar.held_step(what, b, a, r32, r64, t32, t64, check=False)
            self.rows += [dict(r, what=what, net=net, active=active) for r in rows]
            # exact expectations
            still = ar.still_entries(b)
            assert same(a["p"][still], ar.decayed(b["p"], kind, lr)[still]), f"{what}: an entry with g = m = v = 0 moved by more than the decay"
            assert not a["m"][still].any() and not a["v"][still].any(), what
            if not active:
                assert r32.coef == 1.0
                mm, vv = ar.unfused_moments(b["m"], b["v"], b["g"])
                assert same(a["m"], mm) and same(a["v"], vv), (f"{what}: inactive clip, but m / v are not the unfused fp32 step on g itself "
                                                                f"({int((ar.bits(a['m']) != ar.bits(mm)).sum())} m, {int((ar.bits(a['v']) != ar.bits(vv)).sum())} v "
                                                                f"words differ): the coefficient is not exactly 1")
            if target is not None and not polyak:
                assert same(after[target], before[target]), f"{what}: {target} changed on a step without Polyak"
            c = self.counts
            if net != "log_alpha":
                c["clip_active"] += int(active)
                c["clip_inactive"] += int(not active)
                c["small_norm_above_clip"] += int(active and r64.norm < 1e-3)
                c["eps_visible"] += int((np.sqrt(r64.v) / np.sqrt(1.0 - ar.BETA2 ** t) < 100.0 * ar.EPS).sum())
                c["zero_grad"] += int((b["g"] == 0).sum())
                c["still"] += int(still.sum())
                if target is not None:
                    c["polyak" if polyak else "no_polyak"] += 1

        def unchanged(net, target):
            for k in ("p", "m", "v"):
                assert same(after[net][k], before[net][k]), f"s{step} {net}: {k} changed on a step that does not step it"
            if target is not None:
                assert same(after[target], before[target]), f"s{step}: {target} changed although {net} did not step"
            self.counts["not_stepped"] += 1

        for i in range(self.C):
            audit(f"critic_{i}", "critic", f"target_critic_{i}", polyak_c)
        if tqc_norms:      # TQC logs the mean of the critics' norms (src/agent.py:1013-1042), in both norm positions
            n32, n64 = (float(np.mean([x[k] for x in tqc_norms])) for k in (0, 1))
            for at in (5, 6) if do_actor else (4, 5):
                self.rows.append(dict(ar.held(f"s{step} critics", "post_norm", [tup[at]], [n32], [n64]), what=f"s{step} critics"))
        if kind == "DDPG":
            # the actor's target moves BEFORE the actor steps (src/agent.py:1397-1401): Polyak of the actor as the step found it
            if polyak_c:
                p0, t0 = before["actor"]["p"], before["target_actor"].astype(np.float64)
                r32, r64 = (ar.reference_polyak(dt, cfg.tau, p0.astype(np.float64), before["target_actor"]) for dt in (torch.float32, torch.float64))
                got = after["target_actor"].astype(np.float64)
                self.rows.append(dict(ar.held(f"s{step} target_actor", "dtarget", got - t0, r32 - t0, r64 - t0), what=f"s{step} target_actor"))
                self.counts["polyak"] += 1
            else:
                assert same(after["target_actor"], before["target_actor"]), f"s{step}: target_actor changed on a step without Polyak"
                self.counts["no_polyak"] += 1
        if do_actor:
            audit("actor", "actor", "target_actor" if kind == "TD3" else None, kind == "TD3")
        else:
            unchanged("actor", "target_actor" if kind == "TD3" else None)
            if kind == "TD3":
                self.counts["no_polyak"] += 1
        if self.ag._sac:
            if do_alpha:
                audit("log_alpha", "alpha", None, False)
                la = np.float64(after["log_alpha"]["p"][0])
                assert abs(self.ag.alpha.item() - np.exp(la)) <= 4e-7 * np.exp(la)      # alpha = expf(log_alpha): three fp32 ulps
                self.counts["alpha"] += 1
            else:
                unchanged("log_alpha", None)
                self.counts["no_alpha"] += 1

    def finish(self, claims):
        ar.judge_units(self.rows)         # m and v per element on active-clip steps: against torch fp32's worst over the net's such steps
        _record(self.kind, self.form, self.rows)
        covers(claims, self.counts)
        bad = [(r["what"], r["quantity"], r["err"], r["ref32_err"], r["scale"], round(r["ratio"], 3)) for r in self.rows if not r["ok"]]
        print(f"  worst err/bound {max(r['ratio'] for r in self.rows):.3f} over {len(self.rows)} quantities")
        assert not bad, bad[:12]


# ------------------------------------------------------------------------------------------------------------------ the agents
def _cls(gcrl, kind):
    return dict(DDPG=gcrl.DDPG, TD3=gcrl.TD3Agent, SAC=gcrl.SACAgent, TQC=gcrl.TQCAgent)[kind]


def _cfg(kind, H, L, B, clip, cosine=False):
    over = dict(hidden_dim=H, layer_count=L, batch_size=B, max_len=2000, grad_clip=clip, policy_noise=0.2, noise_clamp=0.5,
                ac_update_freq=2 if kind == "TD3" else 1, tau=0.05, actor_lr=1e-3, critic_lr=7e-4)
    if cosine:
        over.update(actor_lr_min=2e-4, critic_lr_min=1e-4, ac_scheduler_steps=3, cr_scheduler_steps=3)
    else:
        over.update(actor_lr_min=1e-3, critic_lr_min=7e-4)
    if kind in ("SAC", "TQC"):
        over.update(alpha_min_steps=2.0, alpha_lr=1e-2)
    return make_config(kind, **over)


def _inputs(kind, seed, steps, B, S, A, zero_reward=False, zero_cols=()):
    """Injected batches and noise, one set per step (numpy float32)."""
    gen = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        s, ns = gen.standard_normal((B, S)).astype(F32), gen.standard_normal((B, S)).astype(F32)
        for k in zero_cols:
            s[:, k] = 0.0
        a = np.tanh(gen.standard_normal((B, A))).astype(F32)
        r = np.zeros((B, 1), F32) if zero_reward else -(gen.random((B, 1)) < 0.7).astype(F32)
        d = (gen.random((B, 1)) < 0.2).astype(F32)
        kw = dict(batch=tuple(torch.from_numpy(x).cuda() for x in (s, a, r, ns, d)))
        if kind == "TD3":
            kw["noise"] = torch.from_numpy(gen.standard_normal((B, A)).astype(F32))
        if kind in ("SAC", "TQC"):
            kw["eps_next"] = torch.from_numpy(gen.standard_normal((B, A)).astype(F32))
            kw["eps_cur"] = torch.from_numpy(gen.standard_normal((B, A)).astype(F32))
        out.append(kw)
    return out


def _steps(kind):
    return list(range(38, 44)) if kind == "DDPG" else list(range(1, 7))     # DDPG: Polyak on step % 40 == 0 (src/agent.py:1397)


def _make(gcrl, monkeypatch, kind, dims, form, clip, cosine=False, scale=None):
    H, L, B, S, A = dims
    if form == "no_opt_fuse":
        monkeypatch.setenv("GCRL_NO_OPT_FUSE", "1")
    else:
        monkeypatch.delenv("GCRL_NO_OPT_FUSE", raising=False)
    cfg = _cfg(kind, H, L, B, clip, cosine)
    kw = dict(pipeline=0) if form == "flat" else {}
    ag = _cls(gcrl, kind)(S, A, cfg, None, nenvs=1, gradient_step=2, rng="engine", seed=7, **kw)
    if scale is not None:
        for v in [ag.actor] + list(ag.critics):
            v.set_flat((v.flat() * F32(scale)).astype(F32))
        ag.update_target_network()
    fused = bool(ag.meetings() & 8)            # the fused dW + optimiser launch (csrc/dw_adam.hip)
    print(f"  {kind} {dims} form {form}: launch forms with waits active: {ag.meetings()}")
    if form != "default" or kind == "TQC" or dims in FALLBACK_SHAPES:
        # two launches (GCRL_NO_OPT_FUSE), the flat launch_sumsq + launch_adam (pipeline 0; TQC's layer-per-launch step), and the
        # shapes past kFusedMaxLayers / 256 * kFusedMaxSlotsPerThread tiles: the case must not have run the fused launch
        assert not fused, f"{kind} {dims} form {form} ran the fused optimiser launch"
    elif not fused:
        pytest.skip("the fused optimiser launch is not admissible on this device (shared GPU, or too few CUs for its workgroups)")
    return ag, cfg


def _run(gcrl, monkeypatch, kind, dims, form, clip, claims, cosine=False, scale=None, zero_reward=False, crafted=False):
    H, L, B, S, A = dims
    steps = _steps(kind)
    zero_cols = (0, 1) if crafted else ()
    inputs = _inputs(kind, 100 + H + B, len(steps), B, S, A, zero_reward, zero_cols)
    ag, cfg = _make(gcrl, monkeypatch, kind, dims, form, clip, cosine, scale)
    if crafted:
        # the coming gradient, from a twin that takes the first step: moments set against it, so that m_new cancels; v from 1e-30
        # to 1e4; the first layer's weights of state column 0 keep zero moments (their gradient is exactly zero: the column is)
        twin, _ = _make(gcrl, monkeypatch, kind, dims, form, clip, cosine, scale)
        for net in ["actor"] + [f"critic_{i}" for i in range(len(ag.critics))]:
            assert np.array_equal(twin.actor._get(net), ag.actor._get(net))
        twin.update(steps[0], **inputs[0])
        gen = np.random.default_rng(5)
        for net, view in [("actor", ag.actor)] + [(f"critic_{i}", c) for i, c in enumerate(ag.critics)]:
            g = twin.actor._get("grad:" + net)
            n = g.size
            m = np.where(gen.random(n) < 0.5, -g / F32(9.0), -0.5 * g).astype(F32)       # 0.9 m + 0.1 g ~ 0 for half of them
            v = (10.0 ** gen.uniform(-30.0, 4.0, n)).astype(F32)
            col0 = np.arange(H) * view.in_dim
            assert not g[col0].any() and not g[col0 + 1].any(), f"{net}: the gradient of a zero state column is not exactly zero"
            m[col0], v[col0] = 0.0, 0.0
            ag.actor._set("adam_m:" + net, m)
            ag.actor._set("adam_v:" + net, v)
        del twin
    au = Audit(ag, kind, cfg, 2, form)
    for step, kw in zip(steps, inputs):
        before = au.snapshot()
        info = ag.update(step, **kw)
        au.check(step, before, info)
    au.finish(claims)


FALLBACK_SHAPES = [(128, 8, 17, 30, 6), (520, 2, 40, 12, 2)]     # DDPG shapes the fused launch does not take
DDPG_SHAPES = [(4, 2, 3, 3, 1), (32, 2, 32, 10, 3), (36, 4, 70, 10, 3), (64, 3, 30, 41, 7), (128, 8, 17, 30, 6), (520, 2, 40, 12, 2)]
TD3_SHAPES = [(32, 2, 32, 10, 3), (64, 1, 7, 5, 16), (128, 3, 130, 23, 4)]
BN_SHAPE = (64, 2, 40, 11, 3)
CLIPS = [("active", CLIP_ACTIVE), ("inactive", CLIP_INACTIVE)]


def _claims(kind, clip_name):
    c = {"clip_" + clip_name}
    if kind == "TD3":
        c |= {"clip_inactive", "not_stepped"}          # critic_1 is never clipped; the actor rests every other step
    if kind in ("DDPG", "TD3", "SAC"):
        c |= {"polyak", "no_polyak"}
    else:
        c |= {"polyak"}
    if kind in ("SAC", "TQC"):
        c |= {"alpha", "no_alpha", "eps_visible"}      # a Linear bias in front of BatchNorm has a noise-only gradient
    return c


@pytest.mark.parametrize("clip_name,clip", CLIPS)
@pytest.mark.parametrize("form", ["default", "no_opt_fuse", "flat"])
@pytest.mark.parametrize("dims", DDPG_SHAPES)
def test_ddpg_optimiser_steps_are_torch_adam(gcrl, monkeypatch, dims, form, clip_name, clip):
    """Adam (no decay), Polyak on step 40 of steps 38..43: nets below one 32 x 32 tile, exact tiles, ragged tiles at the fused launch's
    layer limit, the cosine schedule (scheduler_steps 3), and the two shapes past the fused launch's limits (the fallback form)."""
    _run(gcrl, monkeypatch, "DDPG", dims, form, clip, _claims("DDPG", clip_name), cosine=dims == (64, 3, 30, 41, 7))


@pytest.mark.parametrize("clip_name,clip", CLIPS)
@pytest.mark.parametrize("form", ["default", "no_opt_fuse", "flat"])
@pytest.mark.parametrize("dims", TD3_SHAPES)
def test_td3_optimiser_steps_are_torch_adamw(gcrl, monkeypatch, dims, form, clip_name, clip):
    """AdamW, both critics in one launch with critic_1 unclipped, the actor every second step (ac_update_freq 2) with its target."""
    _run(gcrl, monkeypatch, "TD3", dims, form, clip, _claims("TD3", clip_name))


@pytest.mark.parametrize("clip_name,clip", CLIPS)
@pytest.mark.parametrize("form", ["default", "no_opt_fuse"])
@pytest.mark.parametrize("kind", ["SAC", "TQC"])
def test_bn_actor_agents_optimiser_steps_are_torch_adamw(gcrl, monkeypatch, kind, form, clip_name, clip):
    """SAC (Polyak on even steps: gradient_step 2) and TQC (five critics in one launch: nets = 5, net_stride), the log-alpha step
    from step 3 on (alpha_min_steps 2)."""
    _run(gcrl, monkeypatch, kind, BN_SHAPE, form, clip, _claims(kind, clip_name))


@pytest.mark.parametrize("form", ["default", "no_opt_fuse", "flat"])
@pytest.mark.parametrize("kind,dims", [("DDPG", (32, 2, 32, 10, 3)), ("TD3", (32, 2, 32, 10, 3))])
def test_small_norm_makes_the_1e_6_of_the_coefficient_visible(gcrl, monkeypatch, kind, dims, form):
    """Parameters scaled by 1e-2 and zero rewards: the critic's gradient norm falls below 1e-3, the clip (1e-6) lies below it, and
    clip / (norm + 1e-6) differs from clip / norm by 0.1 % and more — nowhere else is the 1e-6 observable."""
    _run(gcrl, monkeypatch, kind, dims, form, 1e-6, _claims(kind, "active") | {"small_norm_above_clip"}, scale=1e-2, zero_reward=True)


@pytest.mark.parametrize("kind,dims,form", [(k, d, f) for k, d in [("DDPG", (36, 4, 70, 10, 3)), ("TD3", (32, 2, 32, 10, 3)), ("SAC", BN_SHAPE),
                                                                    ("TQC", BN_SHAPE)]
                                            for f in ["default", "no_opt_fuse"] + (["flat"] if k in ("DDPG", "TD3") else [])])
def test_crafted_moments_and_a_zero_state_column(gcrl, monkeypatch, kind, dims, form):
    """Before step 1, through the views' _set: adam_v from 1e-30 to 1e4, adam_m against the coming gradient (m_new cancels), two
    state columns of every injected batch exactly zero (the first layer's gradient columns are then exactly zero; one of them
    keeps zero moments and must move by the decay alone) — under every launch form of the kind."""
    _run(gcrl, monkeypatch, kind, dims, form, CLIP_INACTIVE, _claims(kind, "inactive") | {"eps_visible", "zero_grad", "still"}, crafted=True)


# ------------------------------------------------------------------------------------------------------------------ populations
@pytest.mark.parametrize("kind", ["DDPG", "TD3"])
def test_population_optimiser_steps_are_torch_adam(gcrl, monkeypatch, kind):
    """adam_pop.hip and launch_dw_adam_pop: three members at (36, 2, 30, 10, 3) with distinct learning rates and clips (active, none,
    inactive), four steps through the population's update, every member audited through its own views.  State column 0 of every
    pushed row is zero, so the first layers hold entries that move by the decay alone under these forms too."""
    monkeypatch.delenv("GCRL_NO_OPT_FUSE", raising=False)
    H, L, B, S, A = 36, 2, 30, 10, 3
    cfgs = []
    for i, clip in enumerate([CLIP_ACTIVE, None, CLIP_INACTIVE]):
        c = _cfg(kind, H, L, B, clip, cosine=True)
        c.actor_lr, c.critic_lr = 1e-3 * (1 + 0.25 * i), 7e-4 * (1 + 0.5 * i)
        cfgs.append(c)
    Pop = dict(DDPG=gcrl.DDPGPopulation, TD3=gcrl.TD3Population)[kind]
    pop = Pop(S, A, cfgs, 1, 2, rng="engine", seeds=[31, 32, 33])
    for i, m in enumerate(pop.members):
        gen = np.random.default_rng(50 + i)
        for _ in range(2):
            for st in her_oracle.synthetic_episode(gen, 50, S, A):
                s0, ns = st[0].copy(), st[2].copy()
                s0[0] = ns[0] = 0.0           # state column 0 exactly zero in every stored row: the decay-only entries of the first layers
                m.push_her(0, s0, st[1], ns, *st[3:])
    audits = [Audit(m, kind, c, 2, "population") for m, c in zip(pop.members, cfgs)]
    steps = [39, 40, 41, 42] if kind == "DDPG" else [1, 2, 3, 4]
    for step in steps:
        before = [au.snapshot() for au in audits]
        infos = pop.update(step)
        for au, b, info in zip(audits, before, infos):
            au.check(step, b, info)
    for au, name in zip(audits, ["active", "inactive", "inactive"]):
        au.finish(_claims(kind, name) | {"zero_grad", "still"})
