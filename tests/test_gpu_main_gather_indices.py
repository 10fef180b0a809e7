"""GPU (-m gpu): the main gather of an `update_many` call reads the deferred batches' indices straight from the call's pinned
upload block (csrc/agent.hip finish_deferred_draw) instead of from a staged copy.  What can go wrong is the block's lifetime —
the host reuses it kCtrlSlots (4) calls later and may only do so once the gather has read it — and the index offset of the
first deferred batch.  Both forms (`GCRL_MAIN_IDX_STAGED=1` selects the copy) are held bitwise to repeated `update()`, which
draws and gathers one batch per call through the head gather."""
import numpy as np
import pytest

from oracle import her_oracle
from oracle.agent_oracle import make_config

pytestmark = pytest.mark.gpu

S, A, H, L, B = 10, 3, 64, 2, 8
HEAD = 4   # batches of a pipelined DDPG call's head gather (csrc/agent.hip build()): the main gather takes the rest


def _build(gcrl):
    cfg = make_config("DDPG", hidden_dim=H, layer_count=L, batch_size=B, max_len=2000, grad_clip=1.0, tau=0.05)
    ag = gcrl.DDPG(S, A, cfg, None, nenvs=2, gradient_step=40, rng="engine", seed=5)
    gen = np.random.default_rng(3)
    for ep in range(6):
        for st in her_oracle.synthetic_episode(gen, 50, S, A):
            ag.push_her(ep % 2, *st)
    return ag


def _state(ag):
    out = [v.flat() for v in [ag.actor, ag.target_actor] + ag.critics + ag.target_critics]
    out += [ag.actor._get(n) for n in ("adam_m:actor", "adam_v:actor", "adam_m:critic_0", "adam_v:critic_0")]
    return [x.view(np.uint32) for x in out]


@pytest.fixture(scope="module")
def twin(gcrl):
    """Repeated update() over the steps every case below runs: the tuples of each step, and the state after each call's last one."""
    calls = [HEAD + 1, 9, 9, 9, 9, 9, 41]   # one deferred batch; more calls in a row than upload slots; a whole trainer cycle
    one = _build(gcrl)
    tuples, states, step = [], [], 1
    for n in calls:
        tuples.append([tuple(float(x) for x in one.update(step + i)) for i in range(n)])
        states.append(_state(one))
        step += n
    return calls, tuples, states


@pytest.mark.parametrize("staged", [False, True])
def test_back_to_back_calls_match_repeated_update(gcrl, monkeypatch, twin, staged):
    """Seven calls issued without reading anything back in between (the host runs ahead of the GPU and comes round to the first
    call's upload block while later gathers are still queued), then every call's tuples and the final state: bitwise."""
    calls, tuples, states = twin
    if staged:
        monkeypatch.setenv("GCRL_MAIN_IDX_STAGED", "1")
    many = _build(gcrl)
    res, step = [], 1
    for n in calls:
        res.append(many.update_many(step, n))
        step += n
    for c, (want, got) in enumerate(zip(tuples, res)):
        got = [tuple(float(x) for x in t) for t in got]
        assert got == want, (c, calls[c])
    for x, y in zip(states[-1], _state(many)):
        assert np.array_equal(x, y)


def test_each_call_matches_repeated_update(gcrl, twin):
    """The same calls with the state compared after every one: a wrong row in any call's main gather shows in that call."""
    calls, tuples, states = twin
    many = _build(gcrl)
    step = 1
    for c, n in enumerate(calls):
        got = [tuple(float(x) for x in t) for t in many.update_many(step, n)]
        assert got == tuples[c], (c, n)
        for x, y in zip(states[c], _state(many)):
            assert np.array_equal(x, y), (c, n)
        step += n
