"""GPU (-m gpu): the argument fetch in front of the fused DDPG step's two launches.  rowchain_ddpg_kernel warms its argument lines in one
scalar round trip (csrc/kernarg.h kernarg_warm_once) before any role or row block is chosen; the fused optimiser launch picks its
net by blockIdx.y and its problem by tile.  Such code can only go wrong in WHICH record a workgroup picks up — the role and row
block of its blockIdx.x, the net, the problem, the early exit of the smaller net's surplus workgroups — so the cases vary that,
all through the public handle and all bitwise unless stated:

  * DDPG `update_many(1, 41)` against 41 x `update()`: the K-only first launch and the P-only last one (one net), 39 paired launches
    (two nets of different tile counts), the Polyak step at 40, a partial row block (B = 6);
  * the same call against the two-launch optimiser (GCRL_NO_OPT_FUSE=1) and against the
    one-role critic phase (GCRL_NO_DDPG_KSPLIT=1);
  * the row chain's 8- and 16-row instances (B = 516, 1028);
  * a population of two members against the members stepped alone (the table-pointer launch);
  * TD3 with ac_update_freq 2 (the fused optimiser launch at other points of the step);
  * OracleAgent, five steps, 1e-5.
"""
import random

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import OracleAgent, make_config

pytestmark = pytest.mark.gpu


def _cfg(kind, H, L, B, **over):
    base = dict(hidden_dim=H, layer_count=L, batch_size=B, max_len=4000, grad_clip=1.0, tau=0.05, actor_lr_min=2e-4, ac_scheduler_steps=30,
                critic_lr_min=3e-4, cr_scheduler_steps=25)
    if kind == "TD3":
        base.update(policy_noise=0.2, noise_clamp=0.5, ac_update_freq=2)
    base.update(over)
    return make_config(kind, **base)


def _fill(ag, S, A, seed=3):
    gen = np.random.default_rng(seed)
    ep = 0
    while len(ag.buffer) < ag.batch_size + 500:
        for st in her_oracle.synthetic_episode(gen, 50, S, A):
            ag.push_her(ep % 2, *st)
        ep += 1
    gen2 = np.random.default_rng(seed + 5)
    for v in [ag.actor] + list(ag.critics):
        v.set_flat((v.flat() + 0.05 * gen2.standard_normal(v.numel())).astype(np.float32))
    ag.update_target_network()


def _build(gcrl, kind, S, A, H, L, B, gstep=40, seed=21):
    cls = gcrl.DDPG if kind == "DDPG" else gcrl.TD3Agent
    ag = cls(S, A, _cfg(kind, H, L, B), None, nenvs=2, gradient_step=gstep, rng="engine", seed=seed)
    _fill(ag, S, A)
    return ag


def _blob(ag):
    """the engine state: parameters, targets, Adam moments, schedules, counters"""
    from gcrl_amd._ffi import check, lib
    n = int(lib.gcrl_agent_state_size(ag._h))
    blob = np.empty(n, np.uint8)
    check(lib.gcrl_agent_save_state(ag._h, blob.ctypes.data, n))
    return blob


def _arrays(ag):
    nets = ["actor"] + [f"critic_{i}" for i in range(len(ag.critics))]
    out = [ag.actor.flat()] + [c.flat() for c in ag.critics] + [t.flat() for t in ag.target_critics] + [ag.target_actor.flat()]
    for n in nets:
        out += [ag.actor._get("adam_m:" + n), ag.actor._get("adam_v:" + n), ag.actor._get("grad:" + n)]
    return out


def _tuples(ts):
    """the metric tuples as bit patterns (TD3's critic-only and actor steps differ in length)"""
    return [np.array([float(x) for x in t], np.float64).view(np.uint64).tolist() for t in ts]


def _same(x, y, what):
    assert x[0] == y[0], (what, "tuples", x[0], y[0])
    for i, (p, q) in enumerate(zip(x[1], y[1])):
        assert p.shape == q.shape and np.array_equal(p.view(np.uint32), q.view(np.uint32)), (what, "array", i)
    assert np.array_equal(x[2], y[2]), (what, "engine state")


def _many(ag, n):
    t = _tuples(ag.update_many(1, n))
    return t, _arrays(ag), _blob(ag)


def _one(ag, n):
    t = _tuples([ag.update(step) for step in range(1, n + 1)])
    return t, _arrays(ag), _blob(ag)


# the nets' tile counts differ in each (the actor's head has A rows, the critic's first layer S + A columns); B = 6 leaves a partial
# row block
DDPG_SHAPES = [(B, H, L, S, A) for B in (4, 6, 20) for H in (64, 72) for L in (2, 3) for S, A in ((23, 4), (10, 3))]


@pytest.mark.parametrize("B,H,L,S,A", DDPG_SHAPES)
def test_ddpg_41_steps_in_one_call_are_41_updates(gcrl, B, H, L, S, A):
    many, one = _build(gcrl, "DDPG", S, A, H, L, B), _build(gcrl, "DDPG", S, A, H, L, B)
    assert many.meetings() & 8 and one.meetings() & 8          # the fused optimiser launch ran, and the two-role critic phase
    assert many.meetings() & 2
    got, want = _many(many, 41), _one(one, 41)
    assert np.isfinite(np.array(got[0], np.uint64).view(np.float64)).all()
    _same(got, want, (B, H, L, S, A))


@pytest.mark.parametrize("env,B,H,L,S,A", [("GCRL_NO_OPT_FUSE", 6, 72, 2, 10, 3), ("GCRL_NO_OPT_FUSE", 20, 64, 3, 23, 4),
                                           ("GCRL_NO_DDPG_KSPLIT", 6, 72, 3, 10, 3)])
def test_ddpg_call_is_the_unfused_forms_call(gcrl, monkeypatch, env, B, H, L, S, A):
    monkeypatch.delenv(env, raising=False)
    new = _build(gcrl, "DDPG", S, A, H, L, B)
    monkeypatch.setenv(env, "1")
    old = _build(gcrl, "DDPG", S, A, H, L, B)
    assert new.meetings() & 8 and new.meetings() & 2          # this side: the fused optimiser launch, the two-role critic phase
    if env == "GCRL_NO_OPT_FUSE":
        assert not old.meetings() & 8          # the two-launch optimiser ran on that side
    else:
        assert not old.meetings() & 2          # the one-role critic phase ran on that side
    _same(_many(new, 41), _many(old, 41), (env, B, H, L))


@pytest.mark.parametrize("B", [516, 1028])
def test_ddpg_8_and_16_row_instances(gcrl, B):
    S, A, H, L = 10, 3, 64, 3
    many, one = _build(gcrl, "DDPG", S, A, H, L, B), _build(gcrl, "DDPG", S, A, H, L, B)
    _same(_many(many, 5), _one(one, 5), B)


def test_population_of_two_is_its_members_alone(gcrl):
    S, A, H, L, B, gstep = 10, 3, 64, 3, 20, 10
    cfgs = [_cfg("DDPG", H, L, B), _cfg("DDPG", H, L, B, actor_lr=1.5e-3, grad_clip=None)]
    seeds = [61, 62]
    pop = gcrl.DDPGPopulation(S, A, cfgs, 2, gstep, rng="engine", seeds=seeds)
    solo = [gcrl.DDPG(S, A, c, None, nenvs=2, gradient_step=gstep, rng="engine", seed=s) for c, s in zip(cfgs, seeds)]
    for i, (m, a) in enumerate(zip(pop.members, solo)):
        _fill(m, S, A, seed=100 + i)
        _fill(a, S, A, seed=100 + i)
    got = pop.update_many(1, 10)
    for i, a in enumerate(solo):
        want = _tuples(a.update_many(1, 10))
        g = _tuples(got[i])
        assert g == want, (i, g, want)
        assert np.array_equal(_blob(pop.members[i]), _blob(a)), f"member {i}: engine state differs from the standalone agent"


def test_td3_ten_steps_in_one_call_are_ten_updates(gcrl):
    S, A, H, L, B = 10, 3, 64, 3, 20
    many, one = _build(gcrl, "TD3", S, A, H, L, B, gstep=5), _build(gcrl, "TD3", S, A, H, L, B, gstep=5)
    got, want = _many(many, 10), _one(one, 10)
    assert {len(t) for t in want[0]} == {6, 8}          # critic-only and actor steps both occurred
    _same(got, want, "TD3")


def test_ddpg_five_steps_track_the_oracle(gcrl):
    """the oracle draws its initial weights from torch's global generator: seeded, so that every run compares the same numbers"""
    S, A, H, L, B, seed = 10, 3, 64, 3, 64, 1898
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        cfg = make_config("DDPG", hidden_dim=H, layer_count=L, batch_size=B, max_len=2000)
        ag = gcrl.DDPG(S, A, cfg, None, nenvs=2, gradient_step=5, rng="engine", seed=seed)
        torch.manual_seed(seed)
        orc = OracleAgent("DDPG", S, A, cfg, nenvs=2, gradient_step=5, rng=random.Random(seed))
        ag.buffer.compute_reward = her_oracle.sparse_reward
        gen = np.random.default_rng(0)
        for ep in range(3):
            for st in her_oracle.synthetic_episode(gen, 50, S, A):
                ag.push_her(ep % 2, *st)
                orc.push_her(ep % 2, *st)
        ag.actor.set_flat(orc.flat_params(orc.actor))
        ag.critic.set_flat(orc.flat_params(orc.critics[0]))
        ag.update_target_network()
        orc.hard_update()
        for k, info in enumerate(ag.update_many(1, 5)):
            got = np.array([float(x) for x in info])
            want = np.array([float(np.asarray(x)) for x in orc.update(k + 1)])
            print("  step", k + 1, "max |got - want| / max(|want|, 1):", float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))))
            assert np.allclose(got, want, rtol=1e-5, atol=1e-5), (k + 1, got, want)
    finally:
        torch.set_num_threads(n)
