"""Off-GPU pins of tests/grad_ref.py (the definition the GPU gradient audit holds the engine to) and of the audit's case table
(tests/grad_cases.py):

  * its fp32 run against OracleAgent on the same parameters, batch and noise, per kind, with and without importance weights: the
    same torch ops in the same order, so the pre-clip gradients, the target, the per-row TD error and the tuple are bitwise the
    oracle's — but for SAC's actor, whose min(Q_0, Q_1) backward accumulates the two critics' input gradients in another order
    (measured: 1 ulp of the vector's max on the actor's gradient and its norm; allowed: 4);
  * its fp64 run against the REAL reference's recorded fp64 numbers: g64_* / gnorm64_* / tuple64 of two full-size fixtures (inputs
    rebuilt through tests/fullsize.Case), the gradpre arrays and tuples of update_sac_fp64.npz / update_tqc_fp64.npz.  fp64 against
    fp64: the deviations measured here are at most 1.7e-13 of each vector's max (tuple entries: 1e-13 relative); asserted at 2e-12 —
    a decade above the worst, and five below anything fp32;
  * a flip vector of one hand-picked unit against a finite re-run with that unit's derivative forced;
  * every case of the GPU table: the chosen seed gives the coverage counts the case claims, at most KINK_CAP units near a kink,
    none at B <= 64 — so the table is verified before the first GPU run.
"""
import random

import numpy as np
import pytest
import torch

import grad_cases as gc
import grad_ref as gr
from adam_ref import ulp32
from conftest import hparams_from_golden, load_golden
from fullsize import Case as FullCase
from oracle.agent_oracle import OracleAgent, make_config

FP64_PIN = 2e-12


@pytest.fixture(autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _hp(cfg, kind, A, top_drop=2):
    return dict(gamma=cfg.gamma, grad_clip=cfg.grad_clip, critic_lr=cfg.critic_lr, policy_noise=cfg.policy_noise, noise_clamp=cfg.noise_clamp,
                top_drop=top_drop if kind == "TQC" else 0, target_entropy={"SAC": -0.5 * A, "TQC": -float(A)}.get(kind, 0.0))


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", gr.KINDS)
def test_fp32_run_is_the_oracles(kind, weighted):
    S, A, H, L, B, step = 10, 3, 32, 2, 40, 2
    cfg = make_config(kind, hidden_dim=H, layer_count=L, batch_size=B, max_len=2000, grad_clip=0.7, ac_update_freq=1, policy_noise=0.2,
                      noise_clamp=0.5, critic_lr=7e-4)
    torch.manual_seed(3)
    orc = OracleAgent(kind, S, A, cfg, nenvs=1, gradient_step=2, rng=random.Random(1))
    gen = np.random.default_rng(5)
    modules = {"actor": orc.actor}
    if orc.target_actor is not None:
        modules["target_actor"] = orc.target_actor
    for i, (c, t) in enumerate(zip(orc.critics, orc.target_critics)):
        modules[f"critic_{i}"], modules[f"target_critic_{i}"] = c, t
    nets = {}
    for n, m in modules.items():
        nets[n] = (0.3 * gen.standard_normal(orc.flat_params(m).size)).astype(np.float32)
        orc.set_flat_params(m, nets[n])
    f32 = np.float32
    batch = (gen.standard_normal((B, S)).astype(f32), np.tanh(gen.standard_normal((B, A))).astype(f32), -(gen.random((B, 1)) < 0.7).astype(f32),
             gen.standard_normal((B, S)).astype(f32), (gen.random((B, 1)) < 0.2).astype(f32))
    noise, e1, e2 = ((k * gen.standard_normal((B, A))).astype(f32) for k in (2.0, 1.0, 1.0))
    w = gen.uniform(0.2, 1.0, (B, 1)).astype(f32) if weighted else None
    kw = {}
    if kind == "TD3":
        kw["noise"] = torch.from_numpy(noise)
    if kind in ("SAC", "TQC"):
        kw.update(eps_next=torch.from_numpy(e1), eps_cur=torch.from_numpy(e2))
        with torch.no_grad():
            orc.log_alpha.fill_(-0.3)
        orc.alpha = orc.log_alpha.exp()
    want = orc.update(step, tuple(torch.from_numpy(x) for x in batch), weights=None if w is None else torch.from_numpy(w), **kw)
    want = np.array([float(np.asarray(x)) for x in want])
    st = gr.Step(kind, S, A, H, L, _hp(cfg, kind, A), nets, batch, log_alpha=-0.3, weights=w, noise=noise, eps_next=e1, eps_cur=e2,
                 actor_step=True, alpha_step=True)
    R = st.run(torch.float32)
    got = np.array(R.tuple)
    assert got.shape == want.shape
    loose = {7} if kind == "SAC" else set()                    # the actor's norm
    for j in range(len(want)):
        d = abs(got[j] - want[j])
        print(f"{kind} tuple[{j}] |diff| {d:.3e} = {d / ulp32(want[j]):.2f} ulp32")
        assert d <= (4 * ulp32(want[j]) if j in loose else 0.0), (j, got[j], want[j])
    for i, pre in enumerate(orc.last["critic_grads_pre"]):
        assert np.array_equal(st.flat(R, f"critic_{i}").astype(f32), pre), f"critic_{i}"
    g, pre = st.flat(R, "actor"), orc.last["actor_grads_pre"]
    d = float(np.abs(g - pre).max())
    print(f"{kind} actor gradient: worst |diff| {d:.3e} = {d / ulp32(np.abs(pre).max()):.2f} ulp32 of the vector's max")
    assert d <= (4 * ulp32(np.abs(pre).max()) if kind == "SAC" else 0.0)
    assert np.array_equal(R.y.astype(f32), orc.last["target"].reshape(-1))
    assert np.array_equal(R.td_abs.astype(f32), orc.last["td_per_sample"].reshape(-1))
    if kind in ("SAC", "TQC"):
        assert R.g_log_alpha == orc.last["alpha_grad"]
        bns = [m for m in orc.actor.base_net if isinstance(m, torch.nn.BatchNorm1d)]
        for (m, v), bn in zip(R.bn_running, bns):
            assert np.array_equal(m.astype(f32), bn.running_mean.numpy()) and np.array_equal(v.astype(f32), bn.running_var.numpy())


# ------------------------------------------------------------------------------------------------------------------ the real reference, fp64
def _pin(what, got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    rel = float(np.max(np.abs(got - want))) / max(float(np.max(np.abs(want))), 1e-300)
    print(f"  {what:<28} |diff| / max {rel:.2e}")
    assert rel <= FP64_PIN, (what, rel)


@pytest.mark.parametrize("name", ["ddpg_pickplace_b256", "cfg5_sac_slide_b512"])
def test_fp64_run_is_the_references_full_size_fixture(name):
    c = FullCase(name)
    g, cfg, kind = c.g, c.cfg, c.kind
    nets = {n: c.init_vector(n) for n in c.net_names}
    st = gr.Step(kind, c.S, c.A, c.H, c.L, _hp(cfg, kind, c.A), nets, c.batch, log_alpha=0.0, noise=c.noise, eps_next=c.eps_next, eps_cur=c.eps_cur,
                 actor_step=c.step % cfg.ac_update_freq == 0, alpha_step=kind in ("SAC", "TQC") and c.step > cfg.alpha_min_steps)
    R = st.run(torch.float64)
    assert len(R.tuple) == len(g["tuple64"])
    for j, (x, y) in enumerate(zip(R.tuple, g["tuple64"])):
        _pin(f"tuple[{j}]", [x], [y])
    for n in R.grads:
        flat = st.flat(R, n)
        _pin(f"grad {n}", flat[g[f"gidx_{n}"]], g[f"g64_{n}"])
        _pin(f"gnorm {n}", [np.sqrt(np.square(flat).sum())], g[f"gnorm64_{n}"])
    if kind == "SAC":
        _pin("bn_mean", np.concatenate([m for m, _ in R.bn_running]), g["bn_mean64"])
        _pin("bn_var", np.concatenate([v for _, v in R.bn_running]), g["bn_var64"])


@pytest.mark.parametrize("tag", ["sac", "tqc"])
def test_fp64_run_is_the_references_recorded_first_step(tag):
    g, g64 = load_golden(f"update_{tag}.npz"), load_golden(f"update_{tag}_fp64.npz")
    kind = str(g["kind"][0])
    S, A, B, gstep = (int(x) for x in g["dims"])
    cfg = hparams_from_golden(g)
    step = int(g["steps"][0])
    C = gr.n_critics(kind)
    nets = {"actor": g["init_actor"]}
    for i in range(C):
        nets[f"critic_{i}"] = g[f"init_critic_{i}"]
        k = f"init_target_critic_{i}"
        nets[f"target_critic_{i}"] = g[k] if k in g.files else g[f"init_critic_{i}"]
    batch = tuple(g[f"step0_{k}"] for k in ("s", "a", "r", "ns", "d"))
    st = gr.Step(kind, S, A, cfg.hidden_dim, cfg.layer_count, _hp(cfg, kind, A), nets, batch, log_alpha=0.0, eps_next=g["step0_eps_next"],
                 eps_cur=g["step0_eps_cur"], actor_step=step % cfg.ac_update_freq == 0, alpha_step=step > cfg.alpha_min_steps)
    R = st.run(torch.float64)
    assert len(R.tuple) == len(g64["step0_tuple"])
    for j, (x, y) in enumerate(zip(R.tuple, g64["step0_tuple"])):
        _pin(f"tuple[{j}]", [x], [y])
    for n in R.grads:
        _pin(f"gradpre {n}", st.flat(R, n), g64[f"step0_gradpre_{n}"])


# ------------------------------------------------------------------------------------------------------------------ flip vectors
@pytest.mark.parametrize("kind,ps", [("DDPG", "critic_0"), ("DDPG", "critic_0@actor"), ("SAC", "actor")])
def test_flip_vector_is_the_rerun_with_the_derivative_forced(kind, ps):
    """Unit (layer 0, row 3, unit 5) of one pass: the flip vector against a re-run in which that unit's activation is REPLACED by
    the line through its value with the other side's slope (same value at z, the other derivative: a finite construction, no
    autograd trick), differentiated as usual."""
    case = gc.by_id()[{"DDPG": "ddpg-b20-h72-l4-s23a4", "SAC": "sac-b40-h16-l2-s10a3"}[kind]]
    inp = gc.inputs(case)
    st = gc.step_of(case, inp)
    base = st.run(torch.float64)
    ca = base.critics_after
    unit = (ps, 0, 3, 5)
    vec = st.flip_vectors([unit], base, critics_after=ca)[0]
    z0 = float(base.z[ps][0][3, 5])
    slope = gr.LEAKY if kind == "DDPG" or "critic" in ps else 0.0
    other = slope if z0 > 0 else 1.0
    orig = gr._act

    def forced(z, s, flips):
        out = orig(z, s, None)
        if flips:
            (r, u), = flips
            m = torch.zeros_like(z)
            m[r, u] = 1.0
            line = out.detach() + other * (z - z.detach())           # value kept, slope of the other side
            out = out * (1 - m) + line * m
        return out

    gr._act = forced
    try:
        R2 = st.run(torch.float64, critics_after=ca, flips={ps: [(0, 3, 5)]})
    finally:
        gr._act = orig
    moved = 0
    for n in base.grads:
        want = st.flat(R2, n) - st.flat(base, n)
        assert np.allclose(vec[n], want, rtol=0, atol=1e-12 * max(1.0, float(np.abs(st.flat(base, n)).max()))), n
        moved += int(np.any(want != 0))
    hit = ps.split("@")[0] if "@" not in ps else "actor"
    assert np.any(vec[hit] != 0) and moved == 1, (hit, moved)        # the pass's own net moves, no other


# ------------------------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("case", gc.table(), ids=lambda c: c.id)
def test_case_seed_reaches_its_claims_and_keeps_the_kink_cap(case):
    ref = gc.references(case, gc.inputs(case), flips=False)
    print(f"{case.id}: {case.why}; expects {case.expect}; covers {ref.cover}; {len(ref.units)} units near a kink")
    zero = [k for k in sorted(case.claims) if int(ref.cover.get(k, 0)) == 0]
    assert not zero, f"{case.id} (seed {case.seed}) misses {zero}"
    assert len(ref.units) <= gc.KINK_CAP, (case.id, len(ref.units))
    assert case.B > 64 or not ref.units, (case.id, ref.units)


def test_table_reaches_every_rule_boundary():
    """What the table is for, stated on the table itself: every rows-per-workgroup value, both sides of the two-role critic phase, of
    td3_split_k_rule, of the slab and of its row split, a refused row chain, every switch once."""
    t = gc.table()
    ex = lambda kind, key: {c.expect.get(key) for c in t if c.kind == kind and key in c.expect}
    assert ex("DDPG", "rows_per_workgroup") == {4, 8, 16} and ex("TD3", "rows_per_workgroup") == {4, 8}
    assert ex("DDPG", "ddpg_ksplit") == {0, 1} and ex("TD3", "split_k") == {0, 1} and ex("TD3", "rc_merge_k") == {0, 1}
    assert ex("SAC", "bn_slab") == {0, 1} and ex("SAC", "bn_rsplit") == {1, 4} and ex("SAC", "split_roles") == {0, 1}
    assert {0, 1} <= ex("DDPG", "rowchain") and {0, 1} <= ex("TD3", "rowchain") and {0, 1} <= ex("SAC", "rowchain") and ex("TQC", "rowchain") == {0}
    used = {e for c in t for e in c.env + c.proc}
    assert used == set(gc.CREATION_SWITCHES) | set(gc.PROCESS_SWITCHES), used
    n = gc.MI355X_CUS // 3
    assert {c.B for c in t if c.kind == "DDPG" and c.H == 64 and c.L == 2} == {4 * n, 4 * n + 1}
    assert len({tuple(sorted(c.proc)) for c in t if c.proc}) <= 3       # child processes of the GPU file
    assert max(c.H for c in t) <= 72
