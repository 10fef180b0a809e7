"""GPU (-m gpu): the stream form of the fused DDPG row-chain launch's chained layer passes (csrc/rowchain.h WStream, rows_pass_st /
rows_pass_rt; round 37).  A pass no longer ends its weight stream with a stage of loads nobody reads: the free stage registers take the
first stage of the wave's share of the NEXT pass's matrix (within a net, and in the actor phase across the head sections), with that
pass's bias items in front, and the next pass starts with its first stage in flight.  The MFMA sequence of every accumulator, the
partial-sum exchange and the epilogue are the parent's, so everything must be the BITS of the loop form (GCRL_RC_NO_STREAM=1: the
parent's kernel text), and the reference's arithmetic within the flat 1e-5 of tests/test_gpu_full_size.py.

Shapes: S = 5, A = 3.  H = 64 (k-share 16: one stage pair, a dispatched size), 72 (shares 20 / 20 / 20 / 12: a partial stage and an
uneven last wave, the run-time variant), 36 (shares 12 / 12 / 12 / 0: a wave with an empty share requests and consumes nothing), 256
(the headline's four stage pairs); L = 2 (a backward chain of one pass: the request across a head section comes straight after a
forward one), 3, 4 (more layers than ping-pong buffers); B = 4, 6 (partial row block), 20 (several blocks).  Each shape with the
two-role critic phase and with GCRL_NO_DDPG_KSPLIT=1: the stream form is the ACTOR phase's (the critic-phase roles keep the loop form
in both), so the two cases differ in which workgroups run beside the stream-form ones.  Agent.rowchain_stream() says which form an
agent's launches take, so no case passes on the loop form by accident."""
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

SHAPES = [(B, H, L) for L in (2, 3, 4) for H in (64, 72, 36) for B in (4, 6, 20)] + [(4, 256, 3), (6, 256, 3)]


@pytest.fixture(autouse=True, scope="module")
def _oracle_on_one_thread():
    """(the oracle's fp32 sums depend on torch's thread count: tests/test_gpu_multistep.py)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _tuples(tickets):
    return [tuple(float(x) for x in t) for t in tickets]


def _pair(gcrl, monkeypatch, H, L, B, two_role, fused=True, global_mul=False):
    """(loop-form agent, default agent) of one shape, both on the asked critic-phase form and multiplier form"""
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
    if global_mul:
        monkeypatch.setenv("GCRL_RC_GLOBAL_MUL", "1")
    else:
        monkeypatch.delenv("GCRL_RC_GLOBAL_MUL", raising=False)
    monkeypatch.setenv("GCRL_RC_NO_STREAM", "1")
    old = make()
    monkeypatch.delenv("GCRL_RC_NO_STREAM")
    new = make()
    for ag in (old, new):
        if two_role and not (ag.meetings() & 2):
            pytest.skip("the two-role critic phase is not admissible on this device (shared GPU, or too few CUs)")
        assert two_role or not (ag.meetings() & 2)
    assert old.rowchain_form() == new.rowchain_form()
    return old, new


def _same_bits(old, new, ref, got):
    for i, (x, y) in enumerate(zip(ref, got)):
        assert x == y, (i + 1, x, y)
    for i, (x, y) in enumerate(zip(_everything(old), _everything(new))):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), i
    assert np.all(np.isfinite(np.array(got)))


@pytest.mark.parametrize("two_role", [True, False], ids=["two_role_k", "one_role_k"])
@pytest.mark.parametrize("B,H,L", SHAPES)
def test_stream_form_is_bitwise_the_loop_form(gcrl, monkeypatch, B, H, L, two_role):
    """41 steps of update_many from the same seed (gradient_step 40: step 40 is a Polyak step): every returned tuple, parameter,
    target, Adam moment and stored gradient bitwise equal to the loop form; the default agent reports the stream form, the switched
    one does not."""
    old, new = _pair(gcrl, monkeypatch, H, L, B, two_role)
    assert old.rowchain_stream() is False
    assert new.rowchain_stream() is True
    ref = _tuples(old.update_many(1, 41))
    got = _tuples(new.update_many(1, 41))
    assert len(got) == len(ref) == 41
    _same_bits(old, new, ref, got)


@pytest.mark.parametrize("H", [64, 72])
def test_stream_form_agrees_under_the_global_multiplier_form(gcrl, monkeypatch, H):
    """The same comparison with GCRL_RC_GLOBAL_MUL=1 on both sides (the chains' multipliers loaded back from the global saves, next to
    the carried stage), L = 3, B = 6."""
    old, new = _pair(gcrl, monkeypatch, H, 3, 6, True, global_mul=True)
    assert old.rowchain_form() == 0 and new.rowchain_form() == 0
    assert old.rowchain_stream() is False and new.rowchain_stream() is True
    ref = _tuples(old.update_many(1, 41))
    got = _tuples(new.update_many(1, 41))
    assert len(got) == len(ref) == 41
    _same_bits(old, new, ref, got)


@pytest.mark.parametrize("B", [516, 1028])
def test_other_row_counts_keep_the_loop_form(gcrl, monkeypatch, B):
    """B = 516 runs 8 rows per workgroup, B = 1028 sixteen (H = 64, L = 3): neither takes the stream form, and five steps are bitwise
    those of the switch."""
    old, new = _pair(gcrl, monkeypatch, 64, 3, B, True, fused=False)
    assert old.update_forms()["rows_per_workgroup"] == new.update_forms()["rows_per_workgroup"] == (8 if B == 516 else 16)
    assert old.rowchain_stream() is False and new.rowchain_stream() is False
    ref = _tuples(old.update_many(1, 5))
    got = _tuples(new.update_many(1, 5))
    assert len(got) == len(ref) == 5
    _same_bits(old, new, ref, got)


def test_population_of_two_is_bitwise_its_members_alone(gcrl, monkeypatch):
    """A DDPG population of two members at H = 64, L = 3, B = 6 (rowchain_ddpg_pop_kernel_stream includes the same body; the members'
    launches choose the form), six steps: every member's tuples and engine state bitwise equal to the same agent stepped on its own."""
    import test_gpu_population as tp
    for name in ("GCRL_RC_NO_STREAM", "GCRL_RC_GLOBAL_MUL", "GCRL_NO_OPT_FUSE", "GCRL_NO_DDPG_KSPLIT"):
        monkeypatch.delenv(name, raising=False)
    pop, solo = tp._pair(gcrl, S, A, tp._cfgs(2, 64, 6), 5, [71, 72])
    for ag in solo:
        assert ag.rowchain_stream() is True
    tp._run_and_compare(pop, solo, [(1, 6)])


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("B", [4, 6, 20])
@pytest.mark.parametrize("H", [64, 72])
def test_stream_form_tracks_the_oracle(gcrl, monkeypatch, H, B, L):
    """Five steps against OracleAgent fed the same pushes, the same parameters and the same index stream: every entry of every
    returned tuple within 1e-5 of the oracle's, relative to that entry (the flat bound of tests/test_gpu_full_size.py)."""
    for name in ("GCRL_RC_NO_STREAM", "GCRL_RC_GLOBAL_MUL", "GCRL_NO_OPT_FUSE", "GCRL_NO_DDPG_KSPLIT"):
        monkeypatch.delenv(name, raising=False)
    seed = 1898
    torch.manual_seed(seed)   # (the oracle draws its initial parameters from torch's global generator: the same ones every run)
    cfg = make_config("DDPG", hidden_dim=H, layer_count=L, batch_size=B, max_len=3000, grad_clip=0.5)
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
    assert ag.rowchain_stream() is True
    worst = 0.0
    rows = []
    for k, info in enumerate(ag.update_many(1, 5)):
        got = np.array([float(x) for x in info])
        want = np.array([float(np.asarray(x)) for x in orc.update(k + 1)])
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        print(f"H {H} B {B} L {L} step {k + 1}: worst relative deviation {rel.max():.3e}")
        rows.append((k + 1, got, want))
        worst = max(worst, float(rel.max()))
    assert worst <= 1e-5, (worst, rows)
