"""GPU (-m gpu): pop.collect / pop.evaluate on a DeviceGoalEnvGroup and agent.evaluate (csrc/agent_pop.inc gcrl_pop_collect,
gcrl_pop_evaluate; csrc/agent.hip gcrl_agent_evaluate) held BIT FOR BIT to the project's own standalone path, which
tests/test_gpu_collect.py holds to the host loop: member m of the population against a standalone twin of the same config and seed
running agent.collect on DeviceGoalEnv(seeds[m]) under the same exploration stream.

  (a) collect against twins: ring save blob, normalisers, env state and stats, stream counter, rows returned, a following update_many
      tuple for tuple, and all of it again after that update (the weight-copy rebuild, the event ordering) — four kinds x {push ring +
      engine rng, relabel="sample" + device rng}, P = 2 and 3 at N = 1, 5, 33, and a normalize="sample" ring with the goal normaliser;
  (b) DDPG's epsilon branch with steps on which every member, some members and no member take it, asserted from the oracle;
  (c) a second call of K steps issues 3 K launches, less the acting launches of all-epsilon steps, plus the declared flush launches;
  (d) evaluate against the twins' agent.evaluate, and agent.evaluate against the host loop observe_act(eval_action=True) ->
      tests/dev_env_ref.py; normalisers, ring and exploration counter untouched; reset=False off a boundary refused by `t`;
  (e) refusals by field name with nothing consumed, a bitwise resume, the example's device-env loop.

Shapes: H 32, L 3, B 64, T 50 (the smallest flush length the ring accepts), thr 0.05.  No case provokes a fault."""
import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import make_config

import dev_env_ref as E
import evaluate_ref as V
import test_gpu_collect as TC
import test_gpu_her_prior as TP
import test_gpu_her_relabel as T0
import test_gpu_her_strategy as TS

pytestmark = pytest.mark.gpu

f32 = np.float32
B, H, L, T, THR = TC.B, TC.H, TC.L, TC.T, TC.THR
G, A = 3, 3
STEPS = 2 * T + 3
POPS = dict(DDPG="DDPGPopulation", TD3="TD3Population", SAC="SACPopulation", TQC="TQCPopulation")
ENV_SEEDS = [9, 4, 9]
AGENT_SEEDS = [5, 6, 7]


def _pair(gcrl, kind, P, n, env_kind="reach", rng="engine", relabel="push", normalize="push", g_normalize=False, **popkw):
    """a population of P members and its P standalone twins: same configs, seeds, ring settings, normaliser kinds"""
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    S = E.OBS_DIM[env_kind] + G
    cfgs = [make_config(kind, hidden_dim=H, layer_count=L, batch_size=B, max_len=2000, k_future=4, **TS.KINDS[kind]) for _ in range(P)]
    kw = dict(relabel=relabel)
    if normalize == "sample":
        kw.update(normalize="sample", obs_normalize=True, g_normalize=g_normalize)
    pop = getattr(gcrl, POPS[kind])(S, A, cfgs, n, 4, rng=rng, seeds=AGENT_SEEDS[:P], **kw, **popkw)
    for m in pop.members:
        if not popkw.get("shared_ring"):
            m.buffer.obs_normalizer = DeviceRunningNormalizer(S - G)
            m.buffer.dg_normalizer = DeviceRunningNormalizer(G)
            m.buffer.compute_reward = her_oracle.sparse_reward
    twins = [TC._agent(gcrl, kind, seed=s, nenvs=n, state_dim=S, rng=rng, relabel=relabel, normalize=normalize, g_normalize=g_normalize)
             for s in AGENT_SEEDS[:P]]
    return pop, twins


def _envs(gcrl, P, n, env_kind="reach", seeds=ENV_SEEDS):
    group = gcrl.DeviceGoalEnvGroup(env_kind, P, n, seeds[:P], max_steps=T, threshold=THR)
    solo = [gcrl.DeviceGoalEnv(env_kind, n, seed=s, max_steps=T, threshold=THR) for s in seeds[:P]]
    return group, solo


def _compare(pop, twins, group, solo, what):
    stats = group.stats()
    for i, (m, tw) in enumerate(zip(pop.members, twins)):
        assert np.array_equal(TP._blob(m.buffer), TP._blob(tw.buffer)), (what, i, "ring blob")
        assert TC._same_nz(m, tw), (what, i, "normalisers")
        assert np.array_equal(group.member_state(i), solo[i].save_state()), (what, i, "env state")
        assert stats[i] == solo[i].stats(), (what, i)
        assert m._collect_stream() == tw._collect_stream(), (what, i, "exploration stream")
        assert m.buffer.relabel_counter == tw.buffer.relabel_counter and T0._mt_state(m.buffer) == T0._mt_state(tw.buffer), (what, i)
        assert np.array_equal(T0._state(m), T0._state(tw)), (what, i, "agent state")


def _same_forms(pop, kind):
    """SAC / TQC: a member is bitwise a standalone agent running the same launch forms (tests/test_gpu_population_sac.py); at these shapes
    the population and a standalone agent of this process run the same ones"""
    if kind in ("SAC", "TQC"):
        assert pop.forms() == pop.members[0].meetings() & (1 | 2 | 8), (pop.forms(), pop.members[0].meetings(), pop.forms_terms())


def _update_both(pop, twins, step0, n):
    got = pop.update_many(step0, n)
    want = [tw.update_many(step0, n) for tw in twins]
    for i, (g, w) in enumerate(zip(got, want)):
        x, y = T0._tuples(g), T0._tuples(w)
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (i, x, y)


def _pick_stream_seeds(P, n_steps):
    """DDPG: per-member stream seeds whose first n_steps epsilon uniforms give at least one step with every member on the network, one
    mixed step and one with every member on the epsilon branch — found from the oracle, on the CPU"""
    for base in range(1, 400):
        seeds = [base + 1000 * m for m in range(P)]
        on = np.array([[E.epsilon_uniform(s, c) < 0.2 for c in range(n_steps)] for s in seeds])
        k = on.sum(0)
        if (k == 0).any() and (k == P).any() and ((k > 0) & (k < P)).any():
            return seeds, on
    raise AssertionError("no seeds")


CASES = [("DDPG", "push", "engine", 3, 5), ("DDPG", "sample", "device", 2, 1), ("TD3", "push", "engine", 2, 33), ("TD3", "sample", "device", 3, 1),
         ("SAC", "push", "engine", 3, 33), ("SAC", "sample", "device", 2, 5), ("TQC", "push", "engine", 2, 33), ("TQC", "sample", "device", 3, 5)]


# ---------------------------------------------------------------- (a), (b) collect against twins
@pytest.mark.parametrize("kind,relabel,rng,P,n", CASES)
def test_pop_collect_is_the_members_own_collect(gcrl, kind, relabel, rng, P, n):
    assert {(c[3], c[4]) for c in CASES} == {(p, k) for p in (2, 3) for k in (1, 5, 33)}      # N = 5: past a 4-row group; 33: past the 32-row mark
    env_kind = "push" if kind in ("TD3", "TQC") else "reach"
    pop, twins = _pair(gcrl, kind, P, n, env_kind, rng=rng, relabel=relabel)
    group, solo = _envs(gcrl, P, n, env_kind)
    if kind == "DDPG":
        seeds, on = _pick_stream_seeds(P, STEPS)
        k = on.sum(0)
        assert (k == 0).any() and (k == P).any() and ((k > 0) & (k < P)).any()
        for m, tw, s in zip(pop.members, twins, seeds):
            m.set_collect_stream(seed=s); tw.set_collect_stream(seed=s)
            assert m._collect_stream()[2] == 0.2
    rows = pop.collect(group, STEPS)
    want = [tw.collect(e, STEPS) for tw, e in zip(twins, solo)]
    assert rows == want and all(r > 0 for r in rows)
    _compare(pop, twins, group, solo, "explore")
    _same_forms(pop, kind)
    _update_both(pop, twins, 1, 4)
    _compare(pop, twins, group, solo, "after update_many")
    # once more after the parameter write (weight-copy rebuild, event ordering): eval mode, then exploring again
    assert pop.collect(group, 4, explore=False) == [tw.collect(e, 4, explore=False) for tw, e in zip(twins, solo)]
    _compare(pop, twins, group, solo, "eval after update")
    assert pop.collect(group, T) == [tw.collect(e, T) for tw, e in zip(twins, solo)]
    _compare(pop, twins, group, solo, "explore after update")
    assert all(m._collect_stream()[3] == STEPS + 4 + T for m in pop.members)
    c = pop.collect_counts()
    assert c["calls"] == 3 and c["steps"] == STEPS + 4 + T and c["copies"] == 0 and c["syncs"] == 0


def test_pop_collect_into_raw_rings_with_the_goal_normaliser(gcrl):
    """normalize="sample": the raw-store population kernel, with the goal normaliser's statistics updated per member"""
    P, n = 3, 5
    pop, twins = _pair(gcrl, "TD3", P, n, "push", rng="device", relabel="sample", normalize="sample", g_normalize=True)
    group, solo = _envs(gcrl, P, n, "push")
    rows = pop.collect(group, T + 7, g_normalize=True)
    assert rows == [tw.collect(e, T + 7, g_normalize=True) for tw, e in zip(twins, solo)] and all(r > 0 for r in rows)
    _compare(pop, twins, group, solo, "raw rings")
    _update_both(pop, twins, 1, 2)
    assert pop.collect(group, 5, g_normalize=True) == [tw.collect(e, 5, g_normalize=True) for tw, e in zip(twins, solo)]
    _compare(pop, twins, group, solo, "raw rings after update")


def test_a_one_member_population_runs_the_members_own_loop(gcrl):
    pop, twins = _pair(gcrl, "DDPG", 1, 5)
    group, solo = _envs(gcrl, 1, 5)
    assert pop.collect(group, T + 3) == [twins[0].collect(solo[0], T + 3)]
    _compare(pop, twins, group, solo, "P = 1")
    assert pop.collect_counts()["launches"] == pop.members[0].collect_counts()["launches"] == twins[0].collect_counts()["launches"]
    r = pop.evaluate(group, 5)
    assert r == [twins[0].evaluate(solo[0], 5)]


# ---------------------------------------------------------------- (c) counts
@pytest.mark.parametrize("kind", ["DDPG", "SAC"])
def test_a_second_call_is_three_launches_a_step_for_all_members(gcrl, kind):
    from gcrl_amd._ffi import lib
    P, n = 3, 5
    pop, _ = _pair(gcrl, kind, P, n)
    group, _ = _envs(gcrl, P, n)
    seeds = [m._collect_stream()[0] for m in pop.members]
    if kind == "DDPG":
        seeds, _ = _pick_stream_seeds(P, STEPS)
        for m, s in zip(pop.members, seeds):
            m.set_collect_stream(seed=s)
    first = 7
    pop.collect(group, first)                 # a first call: allocations, the first step's noise fills, the weight copies, the tables
    K = STEPS - first
    flushes = lambda: sum(int(lib.gcrl_her_flush_calls(m.buffer.handle)) for m in pop.members)
    c0, f0 = pop.collect_counts(), flushes()
    pop.collect(group, K)
    c1, f1 = pop.collect_counts(), flushes()
    all_eps = 0
    if kind == "DDPG":
        on = np.array([[E.epsilon_uniform(s, c) < 0.2 for c in range(first, first + K)] for s in seeds])
        all_eps = int((on.sum(0) == P).sum())
        assert all_eps >= 1
    assert f1 - f0 >= 2 * P
    assert c1["calls"] - c0["calls"] == 1 and c1["steps"] - c0["steps"] == K
    assert c1["launches"] - c0["launches"] == 3 * K - all_eps + (f1 - f0)
    assert c1["copies"] == 0 and c1["syncs"] == 0


# ---------------------------------------------------------------- (d) evaluate
def _nz_bits(ag):
    return tuple(x.tobytes() for x in TC._nz_state(ag))


@pytest.mark.parametrize("kind", ["DDPG", "TD3", "SAC", "TQC"])
def test_evaluate_against_twins_and_the_host_loop(gcrl, kind):
    P, n = 3, 5
    pop, twins = _pair(gcrl, kind, P, n)
    group, solo = _envs(gcrl, P, n)
    assert pop.collect(group, T) == [tw.collect(e, T) for tw, e in zip(twins, solo)]          # some statistics and a trained step to evaluate
    _same_forms(pop, kind)
    _update_both(pop, twins, 1, 2)
    held, held_solo = _envs(gcrl, P, n, seeds=[21, 21, 22])                                    # held out; members 0 and 1 on identical episodes
    before = [(_nz_bits(m), TP._blob(m.buffer).tobytes(), m._collect_stream(), T0._state(m).tobytes()) for m in pop.members]
    got = pop.evaluate(held, 2 * n)
    want = [tw.evaluate(e, 2 * n) for tw, e in zip(twins, held_solo)]
    assert got == want and all(r["episodes"] == 2 * n for r in got)
    assert all(0 <= r["successes"] <= r["episodes"] and r["success_rate"] == r["successes"] / r["episodes"] for r in got)
    assert before == [(_nz_bits(m), TP._blob(m.buffer).tobytes(), m._collect_stream(), T0._state(m).tobytes()) for m in pop.members]
    for i in range(P):
        assert np.array_equal(held.member_state(i), held_solo[i].save_state()), i
        assert held.stats()[i] == {k: got[i][k] for k in ("episodes", "successes", "reward_sum")}
    # episodes round up to a multiple of N; reset=False goes on from the counters and reports the difference
    more = pop.evaluate(held, n + 1, reset=False)
    assert more == [tw.evaluate(e, n + 1, reset=False) for tw, e in zip(twins, held_solo)] and all(r["episodes"] == 2 * n for r in more)
    assert [s["episodes"] for s in held.stats()] == [4 * n] * P
    # agent.evaluate against the host loop: the eval action of observe_act on the numpy definition
    tw, ref = twins[0], E.RefEnv("reach", n, seed=21, max_steps=T, threshold=THR)
    tw._act_noise = lambda n_, ev: (None, 2 if tw._sac else tw._ACT_MODE_EVAL)
    policy = lambda st: tw.observe_act(st["observation"], st["desired_goal"], eval_action=True).astype(f32)
    host = V.evaluate(ref, policy, n)
    dev = tw.evaluate(held_solo[0], n)
    assert dev == host, (dev, host)
    assert np.array_equal(TC.bits(held_solo[0].acting_rows()["rows"].cpu().numpy()), TC.bits(ref.rows))
    # off an episode boundary reset=False is refused by `t`, with nothing stepped
    held.step(torch.zeros((P, n, 3), device="cuda")); held_solo[0].step(torch.zeros((n, 3), device="cuda"))
    snap = (held.save_state().tobytes(), held_solo[0].save_state().tobytes())
    with pytest.raises(gcrl._ffi.GcrlError, match=" t: "):
        pop.evaluate(held, n, reset=False)
    with pytest.raises(gcrl._ffi.GcrlError, match=" t: "):
        tw.evaluate(held_solo[0], n, reset=False)
    assert snap == (held.save_state().tobytes(), held_solo[0].save_state().tobytes())
    with pytest.raises(ValueError, match="episodes"):
        pop.evaluate(held, 0)
    with pytest.raises(ValueError, match="env"):
        pop.evaluate(held_solo[0], n)
    with pytest.raises(ValueError, match="env"):
        tw.evaluate(held, n)


# ---------------------------------------------------------------- (e) refusals, resume, the example
def _snap(pop, group):
    return ([TC._snap(m, _MemberEnv(group, i))[:-1] for i, m in enumerate(pop.members)], pop.collect_counts()["steps"], group.save_state().tobytes())


class _MemberEnv:
    """what TC._snap reads of an env, for member i of a group"""

    def __init__(self, group, i):
        self.group, self.i = group, i

    def save_state(self):
        return self.group.member_state(self.i)


def test_refusals_name_their_field_and_consume_nothing(gcrl):
    from gcrl_amd.src.utils import RunningNormalizer
    err = gcrl._ffi.GcrlError
    P, n = 2, 3
    pop, twins = _pair(gcrl, "DDPG", P, n)
    group, solo = _envs(gcrl, P, n)
    assert pop.collect(group, 5) == [tw.collect(e, 5) for tw, e in zip(twins, solo)]
    before = _snap(pop, group)
    mk = lambda kind="reach", p=P, k=n, **kw: gcrl.DeviceGoalEnvGroup(kind, p, k, list(range(p)), **dict(dict(max_steps=T, threshold=THR), **kw))
    cases = [("env", mk(p=3)), ("env", mk(k=4)), ("env", mk("push")), ("max_steps", mk(max_steps=T - 1)), ("threshold", mk(threshold=0.06)),
             ("env", solo[0]), ("env", object())]
    for field, other in cases:
        with pytest.raises((ValueError, err), match=field):
            pop.collect(other, 3)
    with pytest.raises(ValueError, match="steps"):
        pop.collect(group, 0)
    big, _ = _pair(gcrl, "DDPG", P, B + 1)
    with pytest.raises((ValueError, err), match="env"):                    # more envs per member than batch_size
        big.collect(mk(k=B + 1), 1)
    # a group that is not where the rings' staging areas are: the member and the env are named
    with pytest.raises(err, match=r" t: env 0 of member 0"):
        pop.collect(mk(), 3)
    # a normaliser flag that asks for a device normaliser that is not there
    keep = pop.members[1].buffer.dg_normalizer
    pop.members[1].buffer.dg_normalizer = RunningNormalizer(G)
    with pytest.raises(err, match="normalize"):
        pop.collect(group, 3, g_normalize=True)
    pop.members[1].buffer.dg_normalizer = keep
    # a member's ring with a dense reward or a host callback
    for fn in (lambda ag_, g_, info=None: -np.ones(np.shape(ag_)[:-1], f32) * 0.5, her_oracle.dense_reward):
        odd, _ = _pair(gcrl, "DDPG", P, n)
        odd.members[1].buffer.compute_reward = fn
        with pytest.raises((ValueError, err), match="compute_reward"):
            odd.collect(mk(), 3)
    # a shared ring, a member under a gradient exchange, and a member's own collect
    shared, _ = _pair(gcrl, "DDPG", P, n, shared_ring=True)
    with pytest.raises(err, match="shared_ring"):
        shared.collect(mk(), 3)
    pop.members[0]._dp_driven = True
    with pytest.raises(err, match="DataParallelUpdater"):
        pop.collect(group, 3)
    del pop.members[0]._dp_driven
    with pytest.raises(err, match=r"pop\.collect"):
        pop.members[0].collect(solo[0], 3)
    assert _snap(pop, group) == before, "a refusal consumed something"
    assert pop.collect(group, T) == [tw.collect(e, T) for tw, e in zip(twins, solo)]
    _compare(pop, twins, group, solo, "after the refusals")


def test_resume_mid_episode_is_bitwise(gcrl, tmp_path):
    P, n = 2, 3
    mkpop = lambda: _pair(gcrl, "TD3", P, n, rng="device", relabel="sample")[0]
    a = mkpop()
    for i, m in enumerate(a.members):
        m.set_collect_stream(seed=1234 + i)              # keys of their own: the resume has to carry them
    group, _ = _envs(gcrl, P, n)
    a.collect(group, T + 17)
    a.update_many(1, 2)
    a.save_state(str(tmp_path / "st"))
    blob = group.save_state()
    b = mkpop()
    for m in b.members:
        m.buffer._ensure(E.OBS_DIM["reach"] + G, A, G)
    bgroup = gcrl.DeviceGoalEnvGroup("reach", P, n, [77, 78], max_steps=T, threshold=THR)
    b.load_state(str(tmp_path / "st"))
    bgroup.load_state(blob)
    assert [m._collect_stream() for m in b.members] == [m._collect_stream() for m in a.members]
    assert a.members[1]._collect_stream()[0] == 1235 and a.members[1]._collect_stream()[3] == T + 17
    assert a.collect(group, T) == b.collect(bgroup, T)
    assert np.array_equal(group.save_state(), bgroup.save_state())
    for x, y in zip(a.members, b.members):
        assert TC._same_nz(x, y)
        for u, v in zip(x.buffer.rows() + x.buffer.tails(), y.buffer.rows() + y.buffer.tails()):
            assert np.array_equal(TC.bits(u), TC.bits(v))
    ta, tb = a.update_many(3, 4), b.update_many(3, 4)
    for x, y in zip(ta, tb):
        assert np.array_equal(T0._tuples(x).view(np.uint64), T0._tuples(y).view(np.uint64))
    for x, y in zip(a.members, b.members):
        assert np.array_equal(T0._state(x), T0._state(y))


def test_the_example_trains_on_a_device_env_with_pbt(gcrl):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("population_trainer", os.path.join(root, "examples", "population_trainer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.train(members=3, cycles=2, device_env="reach", pbt=1, num_envs=4, max_episode=4, gradient_step=4, hidden=H, layers=L, batch=B,
                    eval_episodes=8, verbose=False)
    rates = out["success"]
    assert out["collect_counts"]["steps"] == 2 * T and out["collect_counts"]["copies"] == 0 and out["gradient_steps"] == 2 * 4 * 3
    assert len(rates) == 3 and all(np.isfinite(r) and 0.0 <= r <= 1.0 for r in rates)
