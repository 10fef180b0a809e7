"""GPU (-m gpu): the L2-warming rider workgroups of the fused DDPG row-chain launch (csrc/rowchain.hip rc_warm_rider; round 38).  The
single-agent stream-form launch grows by a few workgroups with its last indices, on CUs the roles leave idle, that only load — and
discard — the weight matrices the roles are about to stream.  A rider stores nothing, meets nobody and stamps nothing, so everything
must be the BITS of the launch without riders (GCRL_RC_NO_WARM=1, read at agent creation), and the reference's arithmetic within the flat
1e-5 of tests/test_gpu_full_size.py.

Shapes: S = 5, A = 3.  H = 36 (a matrix of 5 184 bytes: smaller than one rider's sweep, most of whose requests lie past its end and must
read nothing; wave 3's share of a pass is empty), 64, 72 (a matrix that ends inside a 4 KB piece), 256 (the headline's: 64 pieces a
matrix); L = 2 (one matrix per net and layout), 3, 4; B = 4 (one row block: the riders outnumber the role workgroups), 6, 20.  Each
shape with the two-role critic phase and with GCRL_NO_DDPG_KSPLIT=1 (the riders' indices start behind 3 or 2 workgroups per row
block).  Agent.rowchain_warm() says how many riders an agent's launch carries, so no case passes without them by accident."""
import random

import numpy as np
import pytest
import torch

import test_gpu_rowchain_stream as rs
from oracle import her_oracle
from oracle.agent_oracle import OracleAgent, make_config
from test_gpu_optfuse import _agent
from test_gpu_parity import _ddpg_for_schedules

pytestmark = pytest.mark.gpu

S, A = rs.S, rs.A
NW = 16     # csrc/rowchain.h kRowChainWarm: two riders per XCD, each takes every other 4 KB piece of a matrix

SHAPES = [(B, H, L) for L in (2, 3, 4) for H in (36, 64, 72, 256) for B in (4, 6, 20)]
KNOBS = ("GCRL_RC_NO_WARM", "GCRL_RC_NO_STREAM", "GCRL_RC_GLOBAL_MUL", "GCRL_NO_OPT_FUSE", "GCRL_NO_DDPG_KSPLIT")


@pytest.fixture(autouse=True, scope="module")
def _oracle_on_one_thread():
    """(the oracle's fp32 sums depend on torch's thread count: tests/test_gpu_multistep.py)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _pair(gcrl, monkeypatch, H, L, B, two_role, fused=True):
    """(agent without riders, default agent) of one shape, both on the asked critic-phase form"""
    def make():
        ag = _agent(gcrl, monkeypatch, True, H, L, B, S=S, A=A) if fused else _ddpg_for_schedules(gcrl, H, L, 2, B=B, S=S, A=A)
        gen = np.random.default_rng(6)      # (the helpers push 738 rows: more episodes, the same for both agents, where the batch is larger)
        while len(ag.buffer) < B:
            for st in her_oracle.synthetic_episode(gen, 50, S, A):
                ag.push_her(0, *st)
        return ag

    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    if not two_role:
        monkeypatch.setenv("GCRL_NO_DDPG_KSPLIT", "1")
    monkeypatch.setenv("GCRL_RC_NO_WARM", "1")
    old = make()
    monkeypatch.delenv("GCRL_RC_NO_WARM")
    new = make()
    for ag in (old, new):
        if two_role and not (ag.meetings() & 2):
            pytest.skip("the two-role critic phase is not admissible on this device (shared GPU, or too few CUs)")
        assert two_role or not (ag.meetings() & 2)
    assert old.rowchain_form() == new.rowchain_form()
    assert old.rowchain_stream() == new.rowchain_stream()
    return old, new


@pytest.mark.parametrize("two_role", [True, False], ids=["two_role_k", "one_role_k"])
@pytest.mark.parametrize("B,H,L", SHAPES)
def test_riders_change_no_bit(gcrl, monkeypatch, B, H, L, two_role):
    """41 steps of update_many from the same seed (gradient_step 40: step 40 is a Polyak step): every returned tuple, parameter,
    target, Adam moment and stored gradient bitwise equal to the launch without riders; the default agent reports its riders, the
    switched one reports none."""
    old, new = _pair(gcrl, monkeypatch, H, L, B, two_role)
    assert new.rowchain_stream() is True
    assert old.rowchain_warm() == 0
    assert new.rowchain_warm() == NW
    ref = rs._tuples(old.update_many(1, 41))
    got = rs._tuples(new.update_many(1, 41))
    assert len(got) == len(ref) == 41
    rs._same_bits(old, new, ref, got)


def test_a_launch_off_the_stream_form_gets_no_riders(gcrl, monkeypatch):
    """B = 516 runs 8 rows per workgroup (H = 64, L = 3) and keeps the loop form: no riders on either agent, and five steps are
    bitwise those of the switch."""
    old, new = _pair(gcrl, monkeypatch, 64, 3, 516, True, fused=False)
    assert new.update_forms()["rows_per_workgroup"] == 8
    assert new.rowchain_stream() is False
    assert old.rowchain_warm() == 0 and new.rowchain_warm() == 0
    ref = rs._tuples(old.update_many(1, 5))
    got = rs._tuples(new.update_many(1, 5))
    assert len(got) == len(ref) == 5
    rs._same_bits(old, new, ref, got)


def test_population_of_two_is_bitwise_its_members_alone(gcrl, monkeypatch):
    """A DDPG population of two members at H = 64, L = 3, B = 6, six steps: the members stepped on their own run with riders, the
    population kernel runs without, and every member's tuples and engine state are bitwise equal."""
    import test_gpu_population as tp
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    pop, solo = tp._pair(gcrl, S, A, tp._cfgs(2, 64, 6), 5, [71, 72])
    for ag in solo:
        assert ag.rowchain_stream() is True and ag.rowchain_warm() == NW
    tp._run_and_compare(pop, solo, [(1, 6)])


def test_riders_track_the_oracle(gcrl, monkeypatch):
    """Five steps at H = 64, B = 6, L = 3 against OracleAgent fed the same pushes, the same parameters and the same index stream:
    every entry of every returned tuple within 1e-5 of the oracle's, relative to that entry (the flat bound of
    tests/test_gpu_full_size.py)."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    H, B, L = 64, 6, 3
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
    assert ag.rowchain_warm() == NW
    worst = 0.0
    rows = []
    for k, info in enumerate(ag.update_many(1, 5)):
        got = np.array([float(x) for x in info])
        want = np.array([float(np.asarray(x)) for x in orc.update(k + 1)])
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        print(f"step {k + 1}: worst relative deviation {rel.max():.3e}")
        rows.append((k + 1, got, want))
        worst = max(worst, float(rel.max()))
    assert worst <= 1e-5, (worst, rows)
