"""GPU (-m gpu): the collect and evaluate loops on the `pick` device environment (state 23 = obs 20 + goal 3, action 4), and the ring filled
from its scripted controller, held bit for bit to the host entries they restate:

  (a) agent.collect(env, 2 T + 3) == the host loop observe_act -> tests/dev_env_pick_ref.py -> process_step under the same noise at
      four components per env, four agent kinds x {push + engine rng, sample + device rng}, DDPG on both sides of epsilon, again
      after an update_many;
  (b) pop.collect(group, 2 T + 3) == the members' own collect on standalone twins, P 2 / 3 x N 1 / 5 / 33, DDPG and SAC;
  (c) agent.evaluate / pop.evaluate against twins and the host loop;
  (d) HERBuffer.collect_scripted(env, 2 T + 3) == the host loop scripted_action -> RefPickEnv.step -> process_step: the ring's save blob
      and the normalisers, both normalize modes, N 1 / 3 / 18, across a flush; its refusals against an untouched snapshot;
  (e) a relabel="sample", prioritise="energy" ring filled by collect_scripted: its priorities are tests/her_energy_ref.py's on the
      ring's own rows, and lifted objects give a potential term;
  (f) the example's --device-env pick with a prior ring filled on the device.

The Gaussian values of the exploration stream come from the device's own gcrl_hash_normal_fill on both sides, as in
tests/test_gpu_collect.py.  No case provokes a fault."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import make_config

import dev_env_pick_ref as P
import dev_env_ref as E
import evaluate_ref as V
import her_energy_ref as EN
import test_gpu_collect as TC
import test_gpu_her_prior as TP
import test_gpu_her_relabel as T0
import test_gpu_her_strategy as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
B, H, L, T, THR = 64, 64, 3, 50, 0.05
D, G, A = 20, 3, 4
STEPS = 2 * T + 3
bits = T0.bits
POPS = dict(DDPG="DDPGPopulation", SAC="SACPopulation")


def _agent(gcrl, kind, seed=5, nenvs=3, rng="engine", relabel="push", normalize="push", g_normalize=False, **kw):
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    cfg = make_config(kind, hidden_dim=H, layer_count=L, batch_size=B, max_len=2000, k_future=4, **TS.KINDS[kind])
    if normalize == "sample":
        kw.update(normalize="sample", obs_normalize=True, g_normalize=g_normalize)
    ag = getattr(gcrl, TC.CLS[kind])(D + G, A, cfg, None, nenvs=nenvs, gradient_step=4, rng=rng, seed=seed, relabel=relabel, **kw)
    ag.buffer.obs_normalizer = DeviceRunningNormalizer(D)
    ag.buffer.dg_normalizer = DeviceRunningNormalizer(G)
    ag.buffer.compute_reward = her_oracle.sparse_reward
    return ag


def _envs(gcrl, n, seed=9):
    return gcrl.DeviceGoalEnv("pick", n, seed=seed, max_steps=T, threshold=THR), P.RefPickEnv(n, seed=seed, max_steps=T, threshold=THR)


def _host_loop(gcrl, ag, ref, steps, explore, c0):
    """observe_act -> numpy definition -> process_step, the noise of vector step c taken from the device stream's definition at A = 4"""
    sd, ns, eps, _ = ag._collect_stream()
    n, rows = ref.n, 0
    for c in range(c0, c0 + steps):
        st = ref.state_dict()
        if explore and eps > 0 and E.epsilon_uniform(sd, c) < eps:
            z = TC._device_normals(gcrl, sd ^ E.EPS_STREAM, c * n * A, n * A).reshape(n, A)
            ag._act_noise = lambda n_, ev, z=z: (np.clip(z, -1, 1).astype(np.float64), None)
        elif explore:
            z = TC._device_normals(gcrl, sd, c * n * A, n * A).reshape(n, A).astype(np.float64) * ns
            ag._act_noise = lambda n_, ev, z=z: (z, 2 if ag._sac else 1)
        else:
            ag._act_noise = lambda n_, ev: (None, 2 if ag._sac else ag._ACT_MODE_EVAL)
        act = ag.observe_act(st["observation"], st["desired_goal"], eval_action=not explore).astype(f32)
        rows += _host_store(ag, ref, st, act)
    return rows


def _host_store(ag, ref, st, act, **flags):
    raw, pay = ref.step(act)
    _, nobs, _, ndg, _, nag = ref.split(raw)
    nx = dict(observation=nobs, desired_goal=ndg, achieved_goal=nag)
    return ag.process_step(st, act, nx, pay[:, 1].copy(), np.zeros(ref.n, bool), **flags)


# ---------------------------------------------------------------- (a) collect against the host loop
@pytest.mark.parametrize("kind", ["DDPG", "TD3", "SAC", "TQC"])
@pytest.mark.parametrize("relabel,rng", [("push", "engine"), ("sample", "device")])
def test_collect_is_the_host_loop(gcrl, kind, relabel, rng):
    n = 3
    seed = TC._pick_seed(STEPS)
    a, b = (_agent(gcrl, kind, seed=seed, relabel=relabel, rng=rng) for _ in range(2))
    env, ref = _envs(gcrl, n)
    if kind == "DDPG":
        u = np.array([E.epsilon_uniform(a._collect_stream()[0], c) for c in range(STEPS)])
        assert (u < 0.2).any() and (u >= 0.2).any()
    rows_a = a.collect(env, STEPS)
    rows_b = _host_loop(gcrl, b, ref, STEPS, True, 0)
    assert rows_a == rows_b > 0
    TC._compare(a, b, env, ref, "explore")
    x, y = T0._tuples(a.update_many(1, 4)), T0._tuples(b.update_many(1, 4))
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (x, y)
    # once more after the parameter write (the weight-copy rebuild), in eval mode and then exploring again
    assert a.collect(env, 4, explore=False) == _host_loop(gcrl, b, ref, 4, False, STEPS)
    TC._compare(a, b, env, ref, "eval after update")
    assert a._collect_stream()[3] == STEPS + 4
    assert a.collect(env, T) == _host_loop(gcrl, b, ref, T, True, STEPS + 4)
    TC._compare(a, b, env, ref, "explore after update")
    c = a.collect_counts()
    assert c["copies"] == 0 and c["syncs"] == 0


# ---------------------------------------------------------------- (b), (c) populations against standalone twins
def _pair(gcrl, kind, members, n):
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    seeds = [5, 6, 7][:members]
    cfgs = [make_config(kind, hidden_dim=H, layer_count=L, batch_size=B, max_len=2000, k_future=4, **TS.KINDS[kind]) for _ in range(members)]
    pop = getattr(gcrl, POPS[kind])(D + G, A, cfgs, n, 4, rng="engine", seeds=seeds, relabel="push")
    for m in pop.members:
        m.buffer.obs_normalizer = DeviceRunningNormalizer(D)
        m.buffer.dg_normalizer = DeviceRunningNormalizer(G)
        m.buffer.compute_reward = her_oracle.sparse_reward
    return pop, [_agent(gcrl, kind, seed=s, nenvs=n) for s in seeds]


def _groups(gcrl, members, n, seeds=(9, 4, 9)):
    seeds = list(seeds[:members])
    return (gcrl.DeviceGoalEnvGroup("pick", members, n, seeds, max_steps=T, threshold=THR),
            [gcrl.DeviceGoalEnv("pick", n, seed=s, max_steps=T, threshold=THR) for s in seeds])


def _compare_pop(pop, twins, group, solo, what):
    stats = group.stats()
    for i, (m, tw) in enumerate(zip(pop.members, twins)):
        assert np.array_equal(TP._blob(m.buffer), TP._blob(tw.buffer)), (what, i, "ring blob")
        assert TC._same_nz(m, tw), (what, i, "normalisers")
        assert np.array_equal(group.member_state(i), solo[i].save_state()), (what, i, "env state")
        assert stats[i] == solo[i].stats(), (what, i)
        assert m._collect_stream() == tw._collect_stream(), (what, i, "exploration stream")
        assert np.array_equal(T0._state(m), T0._state(tw)), (what, i, "agent state")


CASES = [("DDPG", 3, 5), ("DDPG", 2, 1), ("DDPG", 2, 33), ("SAC", 3, 33), ("SAC", 2, 5), ("SAC", 3, 1)]


@pytest.mark.parametrize("kind,members,n", CASES)
def test_pop_collect_is_the_members_own_collect(gcrl, kind, members, n):
    assert {(c[1], c[2]) for c in CASES} == {(p, k) for p in (2, 3) for k in (1, 5, 33)}
    pop, twins = _pair(gcrl, kind, members, n)
    group, solo = _groups(gcrl, members, n)
    if kind == "DDPG":      # per-member stream seeds with a step of every member on the network, a mixed step and one all on the epsilon branch
        import test_gpu_pop_collect as TPC
        seeds, _ = TPC._pick_stream_seeds(members, STEPS)
        for m, tw, s in zip(pop.members, twins, seeds):
            m.set_collect_stream(seed=s); tw.set_collect_stream(seed=s)
    rows = pop.collect(group, STEPS)
    assert rows == [tw.collect(e, STEPS) for tw, e in zip(twins, solo)] and all(r > 0 for r in rows)
    _compare_pop(pop, twins, group, solo, "explore")
    got, want = pop.update_many(1, 4), [tw.update_many(1, 4) for tw in twins]
    for g, w in zip(got, want):
        assert np.array_equal(T0._tuples(g).view(np.uint64), T0._tuples(w).view(np.uint64))
    assert pop.collect(group, 4, explore=False) == [tw.collect(e, 4, explore=False) for tw, e in zip(twins, solo)]
    assert pop.collect(group, T) == [tw.collect(e, T) for tw, e in zip(twins, solo)]
    _compare_pop(pop, twins, group, solo, "after update")
    c = pop.collect_counts()
    assert c["steps"] == STEPS + 4 + T and c["copies"] == 0 and c["syncs"] == 0


@pytest.mark.parametrize("kind", ["DDPG", "SAC"])
def test_evaluate_against_twins_and_the_host_loop(gcrl, kind):
    members, n = 3, 5
    pop, twins = _pair(gcrl, kind, members, n)
    group, solo = _groups(gcrl, members, n)
    assert pop.collect(group, T) == [tw.collect(e, T) for tw, e in zip(twins, solo)]
    for g, w in zip(pop.update_many(1, 2), [tw.update_many(1, 2) for tw in twins]):
        assert np.array_equal(T0._tuples(g).view(np.uint64), T0._tuples(w).view(np.uint64))
    held, held_solo = _groups(gcrl, members, n, seeds=(21, 21, 22))
    got = pop.evaluate(held, 2 * n)
    assert got == [tw.evaluate(e, 2 * n) for tw, e in zip(twins, held_solo)] and all(r["episodes"] == 2 * n for r in got)
    for i in range(members):
        assert np.array_equal(held.member_state(i), held_solo[i].save_state()), i
    more = pop.evaluate(held, n + 1, reset=False)
    assert more == [tw.evaluate(e, n + 1, reset=False) for tw, e in zip(twins, held_solo)] and all(r["episodes"] == 2 * n for r in more)
    # agent.evaluate against the host loop: the eval action of observe_act on the numpy definition
    tw, ref = twins[0], P.RefPickEnv(n, seed=21, max_steps=T, threshold=THR)
    tw._act_noise = lambda n_, ev: (None, 2 if tw._sac else tw._ACT_MODE_EVAL)
    policy = lambda st: tw.observe_act(st["observation"], st["desired_goal"], eval_action=True).astype(f32)
    host = V.evaluate(ref, policy, n)
    dev = tw.evaluate(held_solo[0], n)
    assert dev == host, (dev, host)
    assert np.array_equal(bits(held_solo[0].acting_rows()["rows"].cpu().numpy()), bits(ref.rows))
    # an agent of the other kinds' dimensions is refused by `env`
    other = gcrl.DeviceGoalEnv("push", n, seed=1, max_steps=T, threshold=THR)
    with pytest.raises(ValueError, match="env"):
        tw.evaluate(other, n)
    with pytest.raises(ValueError, match="env"):
        tw.collect(other, 3)


# ---------------------------------------------------------------- (d) the ring filled from the scripted controller
def _scripted_host_loop(gcrl, ag, ref, steps, noise_std, seed, c0, **flags):
    rows = 0
    for c in range(c0, c0 + steps):
        st = ref.state_dict()
        z = TC._device_normals(gcrl, seed, c * ref.n * A, ref.n * A) if noise_std else None      # the device's own hash normals, as in (a)
        rows += _host_store(ag, ref, st, P.scripted_actions(ref, noise_std=noise_std, seed=seed, c=c, normals=z), **flags)
    return rows


@pytest.mark.parametrize("normalize", ["push", "sample"])
@pytest.mark.parametrize("n", [1, 3, 18])
def test_collect_scripted_is_the_host_loop(gcrl, normalize, n):
    gn = normalize == "sample"          # the raw-store form also with the goal normaliser
    kw = dict(relabel="sample") if normalize == "sample" else {}
    a, b = (_agent(gcrl, "DDPG", nenvs=n, normalize=normalize, g_normalize=gn, **kw) for _ in range(2))
    env, ref = _envs(gcrl, n, seed=12)
    a.buffer._ensure(D + G, A, G)
    before = a.collect_counts()
    rows_a = a.buffer.collect_scripted(env, STEPS)                                   # 2 T + 3 steps: two flushes of every env
    rows_b = _scripted_host_loop(gcrl, b, ref, STEPS, 0.0, 0, 0, obs_normalize=True, g_normalize=gn)
    assert rows_a == rows_b > 0 and len(a.buffer) == len(b.buffer)
    assert np.array_equal(TP._blob(a.buffer), TP._blob(b.buffer)), "ring blob"
    assert TC._same_nz(a, b), "normalisers"
    assert np.array_equal(bits(env.acting_rows()["rows"].cpu().numpy()), bits(ref.rows)) and env.stats() == ref.stats()
    assert env.stats()["successes"] == env.stats()["episodes"] == 2 * n              # the demonstrations solve their episodes
    assert a.collect_counts() == before                                              # the agent's stream and counters are not involved
    # with noise, continuing mid-episode; the counter goes on from the steps collected so far
    rows_a = a.buffer.collect_scripted(env, T, noise_std=0.2, seed=31)
    rows_b = _scripted_host_loop(gcrl, b, ref, T, 0.2, 31, STEPS, obs_normalize=True, g_normalize=gn)
    assert rows_a == rows_b > 0
    assert np.array_equal(TP._blob(a.buffer), TP._blob(b.buffer)) and TC._same_nz(a, b)
    assert np.array_equal(bits(env.acting_rows()["rows"].cpu().numpy()), bits(ref.rows)) and env.stats() == ref.stats()


def test_collect_scripted_refusals_name_their_field_and_consume_nothing(gcrl):
    from gcrl_amd.src.utils import RunningNormalizer
    err = (ValueError, gcrl._ffi.GcrlError)
    n = 3
    ag = _agent(gcrl, "DDPG", nenvs=n)
    buf = ag.buffer
    env, _ = _envs(gcrl, n, seed=2)
    assert buf.collect_scripted(env, 5) == 0
    snap = lambda: (TP._blob(buf).tobytes(), env.save_state().tobytes(), tuple(x.tobytes() for x in TC._nz_state(ag)))
    before = snap()
    mk = lambda kind="pick", k=n, **kw: gcrl.DeviceGoalEnv(kind, k, seed=2, **dict(dict(max_steps=T, threshold=THR), **kw))
    for field, other in [("env", mk(k=4)), ("kind", mk("push")), ("kind", mk("reach")), ("max_steps", mk(max_steps=T - 1)), ("threshold", mk(threshold=0.06)),
                         (" t: ", mk()), ("env", object())]:
        with pytest.raises(err, match=field):
            buf.collect_scripted(other, 3)
    with pytest.raises(err, match="steps"):
        buf.collect_scripted(env, 0)
    with pytest.raises(err, match="noise_std"):
        buf.collect_scripted(env, 3, noise_std=-0.5)
    keep = buf.obs_normalizer
    buf.obs_normalizer = RunningNormalizer(D)
    with pytest.raises(err, match="normalize"):
        buf.collect_scripted(env, 3)
    buf.obs_normalizer = keep
    for fn in (lambda ag_, g_, info=None: -np.ones(np.shape(ag_)[:-1], f32) * 0.5, her_oracle.dense_reward):
        odd = _agent(gcrl, "DDPG", nenvs=n)
        odd.buffer.compute_reward = fn
        with pytest.raises(err, match="compute_reward"):
            odd.buffer.collect_scripted(mk(), 3)
    small = gcrl.HERBuffer(2000, 50, n, threshold=THR, relabel="sample")              # a ring of other dimensions
    small.compute_reward = her_oracle.sparse_reward
    small._ensure(13 + G, 3, G)
    with pytest.raises(err, match="dims|env"):
        small.collect_scripted(mk(), 3)
    # the native entry's own checks, by status and field
    lib, h = gcrl._ffi.lib, gcrl._ffi.stream_handle()
    assert lib.gcrl_her_collect_scripted(buf.handle, mk("push").handle, None, None, 3, 0.0, 0, 0, h) == -1 and "kind" in gcrl._ffi.last_error()
    assert lib.gcrl_her_collect_scripted(buf.handle, mk(k=4).handle, None, None, 3, 0.0, 0, 0, h) == -1 and "env" in gcrl._ffi.last_error()
    assert lib.gcrl_her_collect_scripted(buf.handle, mk().handle, None, None, 3, 0.0, 0, 0, h) == -4 and " t: " in gcrl._ffi.last_error()
    assert lib.gcrl_her_collect_scripted(buf.handle, env.handle, ag.buffer.dg_normalizer.handle, None, 3, 0.0, 0, 0, h) == -1 and "nz_obs" in gcrl._ffi.last_error()
    assert snap() == before, "a refusal consumed something"
    assert buf.collect_scripted(env, T) > 0


# ---------------------------------------------------------------- (e) energy priorities of lifted objects
def test_energy_priorities_of_a_ring_filled_by_the_controller(gcrl):
    n = 8
    buf = gcrl.HERBuffer(2000, 50, n, threshold=THR, k_future=4, rng="device", seed=7, relabel="sample", prioritise="energy")
    buf.compute_reward = her_oracle.sparse_reward
    env = gcrl.DeviceGoalEnv("pick", n, seed=5, max_steps=T, threshold=THR)
    assert buf.collect_scripted(env, T) == n * T == len(buf)
    ag_rows, _ = buf.tails()
    episodes = [ag_rows[k * T:(k + 1) * T] for k in range(n)]                          # one flush launch: the envs' episodes in order
    ref = EN.RefEnergyRing(2000, G, seed=7)
    ref.flush(episodes)
    assert np.array_equal(bits(buf.get_priorities()), bits(ref.priorities()))
    # lifted objects: the potential term alone (no kinetic part) is positive for at least one episode, zero for those left on the table
    pot = [float(EN.trajectory_energy(ep, EN.config(G, kinetic=0.0))) for ep in episodes]
    lifted = [bool((ep[:, 2] > 0).any()) for ep in episodes]
    assert any(lifted) and not all(lifted)
    assert all((p > 0) == l for p, l in zip(pot, lifted)), (pot, lifted)
    assert env.stats()["successes"] == n


# ---------------------------------------------------------------- (f) the example
def test_example_runs_with_a_prior_ring_filled_on_the_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "trainer_standin.py"), "--device-env", "pick", "--cycles", "2", "--relabel", "sample",
                        "--prior-episodes", "4", "--prior-rows", "8", "--bc-weight", "1.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "prior ring: 200 rows of 4 scripted episodes, 4 solved" in r.stdout and "DDPG: success over the last 10 cycles" in r.stdout
    for kind in ("reach", "push"):                                                   # their demonstrations still come from the host: refused together
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "trainer_standin.py"), "--device-env", kind, "--cycles", "1",
                            "--prior-episodes", "4", "--prior-rows", "8"], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "not combined here" in r.stderr
