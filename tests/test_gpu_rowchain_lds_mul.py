"""GPU (-m gpu): the fused DDPG row-chain launch reads its backward chains' act' multipliers from LDS (csrc/rowchain.hip
mlp_hidden_keep / grad_chain_keep, round 21).  Every hidden layer's output of a net with a backward chain in the workgroup keeps LDS
rows of its own instead of ping-ponging through two buffers, the chain multiplies by act' of those rows instead of loading the global
save back, the actor phase's critic activations (hC2: read by nobody else) are not written at all, and the online role of the
two-role critic phase keeps its last activation across the meeting instead of reloading it.  Only where a value is read from
changed: act_deriv sees the same fp32 number, so everything must be the BITS of the global-multiplier form (GCRL_RC_GLOBAL_MUL=1:
the parent's kernel text), and the reference's arithmetic within the flat 1e-5 of tests/test_gpu_full_size.py.

Shapes: S = 5, A = 3; batches of 4, 6 and 20 rows at 4 rows per workgroup (6 and 20 leave a partial row block), 516 rows at 8 per
workgroup (last block 4 of 8) and 1028 at 16 (last block 4 of 16); H = 64 and 72; L = 2, 3 and 4 (L = 4: more kept layers than
the two ping-pong buffers the old form has).  Each shape once with the two-role critic phase (the default) and once with the
one-role form (GCRL_NO_DDPG_KSPLIT=1).  Agent.rowchain_form() says which form an agent's launches take, so no case passes on the
old form by accident."""
import random

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import OracleAgent, make_config
from test_gpu_optfuse import _agent, _everything
from test_gpu_parity import _ddpg_for_schedules

pytestmark = pytest.mark.gpu

S, A = 5, 3

SHAPES = [(B, H, L) for L in (2, 3, 4) for H in (64, 72) for B in (4, 6, 20)] + [(516, 64, 3), (1028, 64, 3)]


@pytest.fixture(autouse=True, scope="module")
def _oracle_on_one_thread():
    """(the oracle's fp32 sums depend on torch's thread count: tests/test_gpu_multistep.py)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _tuples(tickets):
    return [tuple(float(x) for x in t) for t in tickets]


def _pair(gcrl, monkeypatch, H, L, B, two_role, fused=True):
    """(global-multiplier agent, default agent) of one shape, both on the asked critic-phase form (fused: and on the fused optimiser
    launch, as _agent insists; else whatever optimiser launches the shape gets)"""
    def make():
        ag = _agent(gcrl, monkeypatch, True, H, L, B, S=S, A=A) if fused else _ddpg_for_schedules(gcrl, H, L, 2, B=B, S=S, A=A)
        gen = np.random.default_rng(6)      # (the helpers push 738 rows: more episodes, the same for both agents, where the batch is larger)
        while len(ag.buffer) < B:
            for st in her_oracle.synthetic_episode(gen, 50, S, A):
                ag.push_her(0, *st)
        return ag

    if two_role:
        monkeypatch.delenv("GCRL_NO_DDPG_KSPLIT", raising=False)
    else:
        monkeypatch.setenv("GCRL_NO_DDPG_KSPLIT", "1")
    monkeypatch.setenv("GCRL_RC_GLOBAL_MUL", "1")
    old = make()
    monkeypatch.delenv("GCRL_RC_GLOBAL_MUL")
    new = make()
    for ag in (old, new):
        if two_role and not (ag.meetings() & 2):
            pytest.skip("the two-role critic phase is not admissible on this device (shared GPU, or too few CUs)")
        assert two_role or not (ag.meetings() & 2)
    return old, new


def _same_bits(old, new, ref, got):
    for i, (x, y) in enumerate(zip(ref, got)):
        assert x == y, (i + 1, x, y)
    for i, (x, y) in enumerate(zip(_everything(old), _everything(new))):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), i
    assert np.all(np.isfinite(np.array(got)))


@pytest.mark.parametrize("two_role", [True, False], ids=["two_role_k", "one_role_k"])
@pytest.mark.parametrize("B,H,L", SHAPES)
def test_lds_multiplier_form_is_bitwise_the_global_form(gcrl, monkeypatch, B, H, L, two_role):
    """41 steps of update_many from the same seed (gradient_step 40: step 40 is a Polyak step): every returned tuple, parameter,
    target, Adam moment and stored gradient bitwise equal to the global-multiplier form; the default agent reports the LDS form for
    all three of its launches (critic phase alone, actor phase alone, both overlapped), the switched one none."""
    old, new = _pair(gcrl, monkeypatch, H, L, B, two_role)
    assert old.rowchain_form() == 0
    assert new.rowchain_form() == 7, new.rowchain_form()
    ref = _tuples(old.update_many(1, 41))
    got = _tuples(new.update_many(1, 41))
    assert len(got) == len(ref) == 41
    _same_bits(old, new, ref, got)


def test_a_shape_the_lds_rule_refuses_keeps_the_global_form(gcrl, monkeypatch):
    """B = 1028, H = 256, L = 3: 16 rows per workgroup at 260 floats per LDS row is 144 KB already, two more buffers do not fit the
    160 KB.  The agent is created, reports the global-multiplier form, and five steps are bitwise those of the switch."""
    old, new = _pair(gcrl, monkeypatch, 256, 3, 1028, True, fused=False)
    assert old.rowchain_form() == 0 and new.rowchain_form() == 0
    ref = _tuples(old.update_many(1, 5))
    got = _tuples(new.update_many(1, 5))
    assert len(got) == len(ref) == 5
    _same_bits(old, new, ref, got)


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("B", [4, 6, 20])
def test_lds_multiplier_form_tracks_the_oracle(gcrl, monkeypatch, B, L):
    """Five steps at H = 64 against OracleAgent fed the same pushes, the same parameters and the same index stream: every entry of
    every returned tuple within 1e-5 of the oracle's, relative to that entry (the flat bound of tests/test_gpu_full_size.py)."""
    monkeypatch.delenv("GCRL_RC_GLOBAL_MUL", raising=False)
    monkeypatch.delenv("GCRL_NO_DDPG_KSPLIT", raising=False)
    monkeypatch.delenv("GCRL_NO_OPT_FUSE", raising=False)
    seed = 1898
    cfg = make_config("DDPG", hidden_dim=64, layer_count=L, batch_size=B, max_len=3000, grad_clip=0.5)
    orc = OracleAgent("DDPG", S, A, cfg, nenvs=1, gradient_step=40, rng=random.Random(seed))
    ag = gcrl.DDPG(S, A, cfg, None, nenvs=1, gradient_step=40, rng="engine", seed=seed)
    gen = np.random.default_rng(4)
    for _ in range(3):
        for st in her_oracle.synthetic_episode(gen, 50, S, A):
            ag.push_her(0, *st)
            orc.push_her(0, *st)
    ag.actor.set_flat(orc.flat_params(orc.actor))
    ag.critic.set_flat(orc.flat_params(orc.critics[0]))
    ag.update_target_network()
    orc.hard_update()
    assert ag.rowchain_form() == 7, ag.rowchain_form()
    worst = 0.0
    rows = []
    for k, info in enumerate(ag.update_many(1, 5)):
        got = np.array([float(x) for x in info])
        want = np.array([float(np.asarray(x)) for x in orc.update(k + 1)])
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        print(f"B {B} L {L} step {k + 1}: worst relative deviation {rel.max():.3e}")
        rows.append((k + 1, got, want))
        worst = max(worst, float(rel.max()))
    assert worst <= 1e-5, (worst, rows)


def test_td3_actor_phase_is_bitwise_the_global_form(gcrl, monkeypatch):
    """TD3 at B = 20, H = 64 with ac_update_freq = 2, six steps (three of them with an actor phase): its actor phase is the fused
    kernel with no critic-phase workgroups, its critic phase the same kernel's one-role form with two critics — tuples and every
    parameter and target bitwise those of the switch."""
    import test_gpu_multistep as ms
    cfg = ms._cfg("TD3", 64, 3, 20, ac_update_freq=2)

    def build():
        ag = gcrl.TD3Agent(S, A, cfg, None, nenvs=2, gradient_step=5, rng="engine", seed=21)
        gen = np.random.default_rng(3)
        for ep in range(4):
            for st in her_oracle.synthetic_episode(gen, 50, S, A):
                ag.push_her(ep % 2, *st)
        gen2 = np.random.default_rng(8)
        for v in [ag.actor] + ag.critics:
            v.set_flat((v.flat() + 0.05 * gen2.standard_normal(v.numel())).astype(np.float32))
        ag.update_target_network()
        return ag

    monkeypatch.setenv("GCRL_RC_GLOBAL_MUL", "1")
    old = build()
    assert old.rowchain_form() == 0
    monkeypatch.delenv("GCRL_RC_GLOBAL_MUL")
    new = build()
    assert new.rowchain_form() & 2, new.rowchain_form()
    t_old, t_new = _tuples(old.update_many(1, 6)), _tuples(new.update_many(1, 6))
    assert {len(t) for t in t_new} == {6, 8}            # critic-only and actor steps both occurred
    for step, (x, y) in enumerate(zip(t_old, t_new), start=1):
        assert x == y, (step, x, y)
    for x, y in zip(ms._state(old), ms._state(new)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert all(np.isfinite(v) for t in t_new for v in t)


def test_population_of_two_is_bitwise_its_members_alone(gcrl, monkeypatch):
    """A DDPG population of two members at B = 20 (rowchain_ddpg_pop_kernel includes the same body; the members' launches choose the
    form), six steps: every member's tuples and engine state bitwise equal to the same agent stepped on its own."""
    import test_gpu_population as tp
    monkeypatch.delenv("GCRL_RC_GLOBAL_MUL", raising=False)
    monkeypatch.delenv("GCRL_NO_OPT_FUSE", raising=False)
    pop, solo = tp._pair(gcrl, S, A, tp._cfgs(2, 64, 20), 5, [71, 72])
    for ag in solo:
        assert ag.rowchain_form() == 7, ag.rowchain_form()
    tp._run_and_compare(pop, solo, [(1, 6)])
