"""GPU (-m gpu): the device-row acting entries and the collect loop (agent.observe_act_dev, agent.process_step_dev, agent.collect;
csrc/agent.hip, csrc/her_ring.hip gcrl_her_process_step_dev) held bit for bit to the host entries they restate:

  (a) observe_act_dev == float32(observe_act) for the four agent kinds, explore and eval, with and without each normaliser, at row
      counts on both sides of the host entry's inline form (n * S <= 640 and n * A <= 96: n = 32 here) and at batch_size;
  (b) process_step_dev leaves ring, staging area, normalisers and counters as process_step does (the ring's save blob), both
      normalize modes, with and without the goal normaliser, n past the inline form's 896 floats, across a flush, with a host
      dones array that ends one env early; the pack kernel's blocks are the blocks the host entry uploads (tests/test_gpu_dev_env.py
      holds the pack kernel to the layout itself);
  (c) collect(env, 2 T + 3) == the host loop observe_act -> numpy ref env -> process_step under the same noise: ring blob,
      normalisers, env state, stats, counters and a following update_many, tuple for tuple;
  (d) a second collect call of K steps issues 3 K + flushes launches, no copy, no synchronisation;
  (e) refusals by field name with nothing consumed, and a bitwise resume.

The Gaussian values of the exploration stream come from the device's own gcrl_hash_normal_fill on both sides (its transcendental
functions differ by ulps from numpy's, tests/test_device_rng.py); the stream's counters and keys are the definition's
(tests/dev_env_ref.py).  No case provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import make_config

import dev_env_ref as E
import test_gpu_her_prior as TP
import test_gpu_her_relabel as T0
import test_gpu_her_strategy as TS

pytestmark = pytest.mark.gpu

f32 = np.float32
B, H, L, T, THR = 64, 32, 3, 50, 0.05
D, G, A = 7, 3, 3
bits = T0.bits
CLS = dict(DDPG="DDPG", TD3="TD3Agent", SAC="SACAgent", TQC="TQCAgent")


def _agent(gcrl, kind, seed=5, nenvs=3, state_dim=D + G, rng="engine", relabel="push", normalize="push", g_normalize=False, **kw):
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    cfg = make_config(kind, hidden_dim=H, layer_count=L, batch_size=B, max_len=2000, k_future=4, **TS.KINDS[kind])
    if normalize == "sample":
        kw.update(normalize="sample", obs_normalize=True, g_normalize=g_normalize)
    ag = getattr(gcrl, CLS[kind])(state_dim, A, cfg, None, nenvs=nenvs, gradient_step=4, rng=rng, seed=seed, relabel=relabel, **kw)
    ag.buffer.obs_normalizer = DeviceRunningNormalizer(state_dim - G)
    ag.buffer.dg_normalizer = DeviceRunningNormalizer(G)
    ag.buffer.compute_reward = her_oracle.sparse_reward
    return ag


def _warm_normalizers(ag, seed=0):
    gen = np.random.default_rng(seed)
    ag.buffer.obs_normalizer.update(gen.normal(0.1, 0.3, (40, ag.buffer.obs_normalizer.size)).astype(f32))
    ag.buffer.dg_normalizer.update(gen.normal(-0.05, 0.2, (40, G)).astype(f32))


def _nz_state(ag):
    out = []
    for nz in (ag.buffer.obs_normalizer, ag.buffer.dg_normalizer):
        m, v, c = nz._state()
        out += [m.view(np.uint64).copy(), v.view(np.uint64).copy(), np.float64(c).view(np.uint64)]
    return out


def _same_nz(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_nz_state(a), _nz_state(b)))


def _device_normals(gcrl, seed, ctr0, n):
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    gcrl._ffi.check(gcrl._ffi.lib.gcrl_hash_normal_fill(C.c_uint64(seed & (2**64 - 1)), C.c_uint64(ctr0), n, out.data_ptr(), gcrl._ffi.stream_handle()))
    return out.cpu().numpy()


# ---------------------------------------------------------------- (a) observe_act_dev against the host entry
@pytest.mark.parametrize("kind", ["DDPG", "TD3", "SAC", "TQC"])
def test_observe_act_dev_is_the_float32_rounding_of_observe_act(gcrl, kind):
    ag = _agent(gcrl, kind, nenvs=B)
    _warm_normalizers(ag)
    gen = np.random.default_rng(3)
    inline_max = min(640 // (D + G), 96 // A)
    assert inline_max == 32 and inline_max + 1 <= B
    for n in (1, 4, 5, inline_max, inline_max + 1, B):
        obs = gen.normal(0, 0.3, (n, D)).astype(f32); dg = gen.normal(0, 0.2, (n, G)).astype(f32)
        noise = gen.normal(0, 0.3, (n, A))
        for on, gn in ((True, False), (False, False), (True, True), (False, True)):
            for explore in (True, False):
                mode = (2 if ag._sac else 1) if explore else (2 if ag._sac else ag._ACT_MODE_EVAL)
                ag._act_noise = lambda n_, ev, noise=noise, mode=mode, explore=explore: (noise.copy() if explore else None, mode)
                want = ag.observe_act(obs, dg, eval_action=not explore, obs_normalize=on, g_normalize=gn).astype(f32)
                got = ag.observe_act_dev(torch.from_numpy(obs).cuda(), torch.from_numpy(dg).cuda(), eval_action=not explore,
                                         noise=torch.from_numpy(noise).cuda() if explore else None, obs_normalize=on, g_normalize=gn)
                assert got.dtype == torch.float32 and got.is_cuda
                assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (kind, n, on, gn, explore)
    # packed rows read in place, and the device exploration stream when no noise is given: vector step c of the stream, c advancing
    rows = torch.from_numpy(np.concatenate([obs, dg], 1)).cuda()
    sd, ns, _, c0 = ag._collect_stream()
    z = _device_normals(gcrl, sd, c0 * B * A, B * A).astype(np.float64).reshape(B, A) * ns
    got = ag.observe_act_dev(rows, obs_dim=D)
    assert ag._collect_stream()[3] == c0 + 1
    want = ag.observe_act_dev(rows, noise=torch.from_numpy(z).cuda(), obs_dim=D)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))
    counts = ag.collect_counts()
    assert counts["copies"] == 0 and counts["syncs"] == 0
    with pytest.raises(ValueError, match="n:"):
        ag.observe_act_dev(torch.zeros((B + 1, D + G), device="cuda"), obs_dim=D)
    with pytest.raises(ValueError, match="noise"):
        ag.observe_act_dev(rows, noise=torch.zeros((B, A), device="cuda"), obs_dim=D)


# ---------------------------------------------------------------- (b) process_step_dev against process_step
def _random_step(gen, n):
    mk = lambda w: gen.normal(0, 0.3, (n, w)).astype(f32)
    st = dict(observation=mk(D), desired_goal=mk(G), achieved_goal=mk(G))
    nx = dict(observation=mk(D), desired_goal=st["desired_goal"].copy(), achieved_goal=mk(G))
    return st, mk(A), nx, -(gen.random(n) < 0.7).astype(f32)


@pytest.mark.parametrize("normalize", ["push", "sample"])
@pytest.mark.parametrize("g_normalize", [False, True])
@pytest.mark.parametrize("n", [1, 3, 18])
def test_process_step_dev_leaves_what_process_step_leaves(gcrl, normalize, g_normalize, n):
    assert n != 18 or n * (2 * D + 2 * G + 32) > 896        # past the inline form of the host entry
    kw = dict(relabel="sample") if normalize == "sample" else {}
    host, dev = (_agent(gcrl, "DDPG", nenvs=n, normalize=normalize, g_normalize=g_normalize, **kw) for _ in range(2))
    gen = np.random.default_rng(n)
    cu = lambda d: {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    total = [0, 0]
    for step in range(T + 2):                                  # across a flush
        st, act, nx, rew = _random_step(gen, n)
        dones = np.zeros(n, bool)
        if step == 20 and n > 1:
            dones[1] = True                                    # one env ends early: from here on the staged counts differ
        total[0] += host.process_step(st, act, nx, rew, dones, obs_normalize=True, g_normalize=g_normalize)
        total[1] += dev.process_step_dev(cu(st), torch.from_numpy(act).cuda(), cu(nx), torch.from_numpy(rew).cuda(),
                                         dones if step % 2 == 0 or dones.any() else None, obs_normalize=True, g_normalize=g_normalize)
        if step in (0, 20, T - 1, T + 1):
            assert np.array_equal(TP._blob(host.buffer), TP._blob(dev.buffer)), (step, "ring blob")
            assert _same_nz(host, dev), (step, "normalisers")
    assert total[0] == total[1] > 0 and len(host.buffer) == len(dev.buffer)
    # a declared step count that is not the ring's: refused by the field's name, nothing staged
    from gcrl_amd import _ffi
    before = TP._blob(dev.buffer)
    raw = torch.zeros(n * (2 * D + 4 * G), device="cuda"); pay = torch.zeros((n, 32), device="cuda")
    wrong = np.full(n, 49, np.int32)
    rc = _ffi.lib.gcrl_her_process_step_dev(dev.buffer.handle, None, 0, None, 0, raw.data_ptr(), pay.data_ptr(), D, wrong.ctypes.data, None, 0, n,
                                            _ffi.stream_handle())
    assert rc == -4 and b" t: " in _ffi.lib.gcrl_last_error()
    assert np.array_equal(TP._blob(dev.buffer), before)


# ---------------------------------------------------------------- (c) collect against the host loop
def _host_loop(gcrl, ag, ref, steps, explore, c0, on=True, gn=False):
    """observe_act -> numpy ref env -> process_step, the noise of vector step c taken from the device stream's definition"""
    sd, ns, eps, _ = ag._collect_stream()
    n, rows = ref.n, 0
    for c in range(c0, c0 + steps):
        st = ref.state_dict()
        if explore and eps > 0 and E.epsilon_uniform(sd, c) < eps:
            z = _device_normals(gcrl, sd ^ E.EPS_STREAM, c * n * A, n * A).reshape(n, A)
            ag._act_noise = lambda n_, ev, z=z: (np.clip(z, -1, 1).astype(np.float64), None)
        elif explore:
            z = _device_normals(gcrl, sd, c * n * A, n * A).reshape(n, A).astype(np.float64) * ns
            ag._act_noise = lambda n_, ev, z=z: (z, 2 if ag._sac else 1)
        else:
            ag._act_noise = lambda n_, ev: (None, 2 if ag._sac else ag._ACT_MODE_EVAL)
        act = ag.observe_act(st["observation"], st["desired_goal"], eval_action=not explore, obs_normalize=on, g_normalize=gn).astype(f32)
        raw, pay = ref.step(act)
        _, nobs, _, ndg, _, nag = ref.split(raw)
        nx = dict(observation=nobs, desired_goal=ndg, achieved_goal=nag)
        rows += ag.process_step(st, act, nx, pay[:, 1].copy(), np.zeros(n, bool), obs_normalize=on, g_normalize=gn)
    return rows


def _pick_seed(steps):
    """a seed whose first `steps` epsilon uniforms fall on both sides of 0.2"""
    for seed in range(5, 50):
        u = np.array([E.epsilon_uniform(seed, c) for c in range(steps)])
        if 5 <= (u < 0.2).sum() <= steps - 5:
            return seed
    raise AssertionError("no seed")


def _compare(a, b, env, ref, what):
    assert np.array_equal(TP._blob(a.buffer), TP._blob(b.buffer)), (what, "ring blob")
    assert _same_nz(a, b), (what, "normalisers")
    assert np.array_equal(bits(env.acting_rows()["rows"].cpu().numpy()), bits(ref.rows)), (what, "env rows")
    assert env.stats() == ref.stats(), what
    assert a.buffer.relabel_counter == b.buffer.relabel_counter and T0._mt_state(a.buffer) == T0._mt_state(b.buffer), what
    assert np.array_equal(T0._state(a), T0._state(b)), (what, "agent state")


@pytest.mark.parametrize("kind", ["DDPG", "TD3", "SAC", "TQC"])
@pytest.mark.parametrize("relabel,rng", [("push", "engine"), ("sample", "device")])
def test_collect_is_the_host_loop(gcrl, kind, relabel, rng):
    steps, n = 2 * T + 3, 3
    seed = _pick_seed(steps)
    env_kind = "push" if kind in ("TD3", "TQC") else "reach"
    S = E.OBS_DIM[env_kind] + G
    a, b = (_agent(gcrl, kind, seed=seed, state_dim=S, relabel=relabel, rng=rng) for _ in range(2))
    env, ref = gcrl.DeviceGoalEnv(env_kind, n, seed=9, max_steps=T, threshold=THR), E.RefEnv(env_kind, n, seed=9, max_steps=T, threshold=THR)
    if kind == "DDPG":
        u = np.array([E.epsilon_uniform(a._collect_stream()[0], c) for c in range(steps)])
        assert (u < 0.2).any() and (u >= 0.2).any()
    rows_a = a.collect(env, steps)
    rows_b = _host_loop(gcrl, b, ref, steps, True, 0)
    assert rows_a == rows_b > 0
    _compare(a, b, env, ref, "explore")
    ta, tb = a.update_many(1, 4), b.update_many(1, 4)
    x, y = T0._tuples(ta), T0._tuples(tb)
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (x, y)
    # once more after the parameter write (the weight-copy rebuild), in eval mode and then exploring again
    assert a.collect(env, 4, explore=False) == _host_loop(gcrl, b, ref, 4, False, steps)
    _compare(a, b, env, ref, "eval after update")
    c1 = a._collect_stream()[3]
    assert c1 == steps + 4
    assert a.collect(env, T) == _host_loop(gcrl, b, ref, T, True, c1)
    _compare(a, b, env, ref, "explore after update")


# ---------------------------------------------------------------- (d) counts
@pytest.mark.parametrize("kind", ["DDPG", "SAC"])
def test_a_second_collect_call_is_three_launches_a_step_plus_flushes(gcrl, kind):
    from gcrl_amd._ffi import lib
    ag = _agent(gcrl, kind, nenvs=5)
    env = gcrl.DeviceGoalEnv("reach", 5, seed=1, max_steps=T, threshold=THR)
    ag.collect(env, 7)                       # a first call: allocation, the first step's noise fill, the weight copies
    c0, f0 = ag.collect_counts(), int(lib.gcrl_her_flush_calls(ag.buffer.handle))
    K = T + 5                                # crosses the horizon once: the five envs flush together
    ag.collect(env, K)
    c1, f1 = ag.collect_counts(), int(lib.gcrl_her_flush_calls(ag.buffer.handle))
    assert f1 - f0 >= 1
    assert c1["calls"] - c0["calls"] == 1 and c1["steps"] - c0["steps"] == K
    assert c1["launches"] - c0["launches"] == 3 * K + (f1 - f0)
    assert c1["copies"] == 0 and c1["syncs"] == 0


# ---------------------------------------------------------------- (e) refusals and resume
def _snap(ag, env):
    return (ag._collect_stream(), ag.buffer.relabel_counter if ag.buffer.handle else None, T0._mt_state(ag.buffer),
            TP._blob(ag.buffer).tobytes() if ag.buffer.handle else None, T0._state(ag).tobytes(), env.save_state().tobytes(),
            tuple(_x.tobytes() for _x in _nz_state(ag)), ag.collect_counts()["steps"])


def test_refusals_name_their_field_and_consume_nothing(gcrl):
    from gcrl_amd.src.utils import RunningNormalizer
    err = gcrl._ffi.GcrlError
    dev, twin = (_agent(gcrl, "DDPG", nenvs=3) for _ in range(2))
    env, tenv = (gcrl.DeviceGoalEnv("reach", 3, seed=2, max_steps=T, threshold=THR) for _ in range(2))
    assert dev.collect(env, 5) == twin.collect(tenv, 5)
    before = _snap(dev, env)
    mk = lambda kind="reach", n=3, **kw: gcrl.DeviceGoalEnv(kind, n, seed=2, **dict(dict(max_steps=T, threshold=THR), **kw))
    cases = [("env", mk(n=4)), ("env", mk("push")), ("max_steps", mk(max_steps=T - 1)), ("threshold", mk(threshold=0.06))]
    for field, other in cases:
        with pytest.raises((ValueError, err), match=field):
            dev.collect(other, 3)
    with pytest.raises(ValueError, match="steps"):
        dev.collect(env, 0)
    with pytest.raises(ValueError, match="env"):
        dev.collect(object(), 3)
    big = _agent(gcrl, "DDPG", nenvs=B + 1)
    with pytest.raises(ValueError, match="env"):                     # more envs than batch_size
        big.collect(mk(n=B + 1), 1)
    # an env that is not where the ring's staging area is
    moved = mk()
    with pytest.raises(err, match=" t: "):
        dev.collect(moved, 3)
    # normaliser flags that ask for a device normaliser that is not there
    keep = dev.buffer.dg_normalizer
    dev.buffer.dg_normalizer = RunningNormalizer(G)
    with pytest.raises(err, match="normalize"):
        dev.collect(env, 3, g_normalize=True)
    dev.buffer.dg_normalizer = keep
    # a ring with a host-callback reward, a dense one
    for fn in (lambda ag_, g_, info=None: -np.ones(np.shape(ag_)[:-1], f32) * 0.5, her_oracle.dense_reward):
        odd = _agent(gcrl, "DDPG", nenvs=3)
        odd.buffer.compute_reward = fn
        with pytest.raises((ValueError, err), match="compute_reward"):
            odd.collect(mk(), 3)
    # population members and agents under a gradient exchange
    pop = gcrl.DDPGPopulation(D + G, A, [make_config("DDPG", hidden_dim=H, layer_count=L, batch_size=B, max_len=500, k_future=4) for _ in range(2)],
                              nenvs=3, gradient_step=4, rng="engine", seeds=[1, 2])
    with pytest.raises(err, match="collect"):
        pop.members[0].collect(mk(), 3)
    dpa = _agent(gcrl, "DDPG", nenvs=3)
    dpa._dp_driven = True                                            # what DataParallelUpdater marks its agent with
    with pytest.raises(err, match="collect"):
        dpa.collect(mk(), 3)
    assert _snap(dev, env) == before, "a refusal consumed something"
    assert dev.collect(env, T) == twin.collect(tenv, T)
    assert _snap(dev, env) == _snap(twin, tenv)


def test_resume_mid_episode_is_bitwise(gcrl, tmp_path):
    a = _agent(gcrl, "TD3", nenvs=3, relabel="sample", rng="device")
    a.set_collect_stream(seed=1234)                      # a key of its own: the resume has to carry it
    env = gcrl.DeviceGoalEnv("reach", 3, seed=4, max_steps=T, threshold=THR)
    a.collect(env, T + 17)
    a.update_many(1, 2)
    a.save_state(str(tmp_path / "st"))
    blob = env.save_state()
    b = _agent(gcrl, "TD3", nenvs=3, relabel="sample", rng="device")
    b.buffer._ensure(D + G, A, G)
    benv = gcrl.DeviceGoalEnv("reach", 3, seed=123, max_steps=T, threshold=THR)
    b.load_state(str(tmp_path / "st"))
    benv.load_state(blob)
    assert b._collect_stream() == a._collect_stream() and a._collect_stream()[0] == 1234 and a._collect_stream()[3] == T + 17
    assert a.collect(env, T) == b.collect(benv, T)
    assert np.array_equal(env.save_state(), benv.save_state()) and _same_nz(a, b)
    for u, v in zip(a.buffer.rows() + a.buffer.tails(), b.buffer.rows() + b.buffer.tails()):
        assert np.array_equal(bits(u), bits(v))
    x, y = T0._tuples(a.update_many(3, 4)), T0._tuples(b.update_many(3, 4))
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert np.array_equal(T0._state(a), T0._state(b))
