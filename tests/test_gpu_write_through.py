"""GPU (-m gpu): the fused dW + optimiser launch moves a regular tile's parameter traffic in 16-byte runs and writes its results
through (csrc/dw_adam_body.inc, round 19).  A tile is regular when all 16 x 16 of its elements are weights of a layer whose rows
are whole 16-byte runs; every other tile — first layers with rows of 5 (actor: S) and 8 (critic: S + A) floats, the bias column,
head rows, the partial tiles of H = 72 — keeps the element-per-lane path.  Only where values live and how they are stored changed:
the same bits as the two-launch form (GCRL_NO_OPT_FUSE=1: batched dW | db GEMMs, then adam_kernel — untouched), the reference's
arithmetic within the north star's flat 1e-5, and the TD3 and population launches that include the same body.

Shapes: S = 5, A = 3 throughout; batches of 4, 6 and 20 rows (6 and 20 leave a partial row block), H = 64 (regular tiles only in
the hidden layers) and H = 72 (partial 16-wide tiles beside regular ones), L = 2 and 3."""
import random

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import OracleAgent, make_config
from test_gpu_optfuse import _agent, _everything

pytestmark = pytest.mark.gpu

S, A = 5, 3


@pytest.fixture(autouse=True, scope="module")
def _oracle_on_one_thread():
    """(the oracle's fp32 sums depend on torch's thread count: tests/test_gpu_multistep.py)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _tuples(tickets):
    return [tuple(float(x) for x in t) for t in tickets]


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("H", [64, 72])
@pytest.mark.parametrize("B", [4, 6, 20])
def test_default_form_is_bitwise_the_two_launch_form(gcrl, monkeypatch, B, H, L):
    """41 steps of update_many from the same seed (gradient_step 40: step 40 is a Polyak step, so the target / wt_target path runs,
    and step 41's target chain reads the [in][out] copy it wrote): every returned tuple, parameter, target, Adam moment and stored
    gradient bitwise equal to the two-launch form."""
    two = _agent(gcrl, monkeypatch, False, H, L, B, S=S, A=A)
    ref = _tuples(two.update_many(1, 41))
    one = _agent(gcrl, monkeypatch, True, H, L, B, S=S, A=A)
    got = _tuples(one.update_many(1, 41))
    assert len(got) == len(ref) == 41
    for i, (x, y) in enumerate(zip(ref, got)):
        assert x == y, (i + 1, x, y)
    for i, (x, y) in enumerate(zip(_everything(two), _everything(one))):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), i
    assert np.all(np.isfinite(np.array(got)))


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("B", [4, 6, 20])
def test_default_form_tracks_the_oracle(gcrl, monkeypatch, B, L):
    """Five steps at H = 64 against OracleAgent fed the same pushes, the same parameters and the same index stream: every entry of
    every returned tuple within 1e-5 of the oracle's, relative to that entry (the flat bound of tests/test_gpu_full_size.py)."""
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
    if not (ag.meetings() & 8):
        pytest.skip("the fused optimiser launch is not admissible on this device (shared GPU, or too few CUs for its workgroups)")
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


def test_td3_actor_phase_is_bitwise_the_two_launch_form(gcrl, monkeypatch):
    """TD3 at B = 6, H = 64 with ac_update_freq = 2, six steps (three of them with an actor phase): both critics' launch and the
    actor's against GCRL_NO_OPT_FUSE=1 — tuples and every parameter and target bitwise."""
    import test_gpu_multistep as ms
    cfg = ms._cfg("TD3", 64, 3, 6, ac_update_freq=2)

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

    monkeypatch.setenv("GCRL_NO_OPT_FUSE", "1")
    two = build()
    assert not (two.meetings() & 8)
    monkeypatch.delenv("GCRL_NO_OPT_FUSE")
    one = build()
    if not (one.meetings() & 8):
        pytest.skip("the fused optimiser launch is not admissible on this device")
    t_two, t_one = _tuples(two.update_many(1, 6)), _tuples(one.update_many(1, 6))
    assert {len(t) for t in t_one} == {6, 8}            # critic-only and actor steps both occurred
    for step, (x, y) in enumerate(zip(t_two, t_one), start=1):
        assert x == y, (step, x, y)
    for x, y in zip(ms._state(two), ms._state(one)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert all(np.isfinite(v) for t in t_one for v in t)


def test_population_of_two_is_bitwise_its_members_alone(gcrl, monkeypatch):
    """A DDPG population of two members (dw_adam_pop_kernel includes the same body), six steps: every member's tuples and engine
    state bitwise equal to the same agent stepped on its own."""
    import test_gpu_population as tp
    monkeypatch.delenv("GCRL_NO_OPT_FUSE", raising=False)
    pop, solo = tp._pair(gcrl, S, A, tp._cfgs(2, 64, 6), 5, [71, 72])
    tp._run_and_compare(pop, solo, [(1, 6)])
