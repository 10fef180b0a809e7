"""GPU (-m gpu): n-step returns on a sample-mode HER ring (HERBuffer(relabel="sample", n_step=N, gamma=g); csrc/her_relabel.hip) held
bit for bit to the numpy definition tests/her_nstep_ref.py: both gathers, n_step=1 against the keyword left out, the four agents
and a population on top of them (each member with its own gamma), resume and refusals.  Helpers and shapes are those of
tests/test_gpu_her_relabel.py."""
import random

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import make_config

import her_nstep_ref as NS
import her_relabel_ref as R
import test_gpu_her_relabel as T
from test_gpu_her_relabel import PICK, REACH, RINGS, SIZES, THR, _np, bits

pytestmark = pytest.mark.gpu


def _buffer(gcrl, cap, dims, k=4, rng="engine", seed=7, dense=False, nenvs=2, **kw):
    buf = gcrl.HERBuffer(cap, 50, nenvs, threshold=THR, k_future=k, rng=rng, seed=seed, relabel="sample", **kw)
    buf.compute_reward = her_oracle.dense_reward if dense else her_oracle.sparse_reward
    return buf


def _fill(buf, dims, episodes, seed):
    """episodes of 50 rows, each ending with done = 1"""
    gen = np.random.default_rng(seed)
    for e in range(episodes):
        ep = T._episode(gen, 50, dims, True)
        buf.push_episode(e % 2, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])


# ---------------------------------------------------------------- 1. gathers
KINDS = ("cut_by_episode_end", "rem0", "crosses_physical_end", "goal_inside_window", "original_window_ends_on_done")


def _row_kind(kind, snap, N, j, f):
    d, rem, head, cap = snap[4], snap[6], snap[7], snap[8]
    p = (head + j) % cap
    rm = int(rem[p])
    m = min(N, rm + 1)
    if kind == "cut_by_episode_end":
        return m < N
    if kind == "rem0":
        return rm == 0
    if kind == "crosses_physical_end":
        return p + m - 1 >= cap
    if kind == "goal_inside_window":
        return 0 < f < m
    return f == 0 and m > 1 and d[(p + m - 1) % cap] == 1.0


def _given(snap, length, n, ctr, seed, k, N, gen):
    """caller-given indices built from the snapshot: row t asks for one of KINDS in turn (the next one when no row of the ring can be
    of that kind at this counter value), so that every kind the ring can hold occurs"""
    rem, head, cap = snap[6], snap[7], snap[8]
    out = np.empty(n, np.uint32)
    for t in range(n):
        c = ctr + t
        fs = {}
        order = gen.permutation(length)
        pick = int(order[0])
        for turn in range(len(KINDS)):
            kind = KINDS[(c + turn) % len(KINDS)]
            hit = None
            for j in order:
                rm = int(rem[(head + int(j)) % cap])
                if rm not in fs:
                    fs[rm] = R.decide(seed, k, c, rm)
                if _row_kind(kind, snap, N, int(j), fs[rm]):
                    hit = int(j)
                    break
            if hit is not None:
                pick = hit
                break
        out[t] = pick
    return out


_COMBOS = [(False, 0.98), (True, 0.5), (True, 0.98), (False, 0.5)]       # (dense, gamma)
GATHER_CASES = [(ring, N, k) + _COMBOS[i % 4] for i, (ring, N, k) in enumerate((ring, N, k) for ring in RINGS for N in (2, 3, 8) for k in (0, 4))]


@pytest.mark.parametrize("ring,N,k,dense,gamma", GATHER_CASES, ids=[f"{c[0]}-n{c[1]}-k{c[2]}-{'dense' if c[3] else 'sparse'}-g{c[4]}" for c in GATHER_CASES])
def test_gathers_bitwise_the_restatement(gcrl, ring, N, k, dense, gamma):
    dims, cap, episodes = RINGS[ring]
    S, A, G = dims
    kind = R.DENSE if dense else R.SPARSE
    seed = 2000 + 10 * N + k
    gen = np.random.default_rng(5)
    for mode in ("engine", "device", "given"):
        buf = _buffer(gcrl, cap, dims, k=k, rng="device" if mode == "device" else "engine", seed=seed, dense=dense, n_step=N, gamma=gamma)
        _fill(buf, dims, episodes, 40)
        assert len(buf) == min(cap, 50 * episodes) and buf.n_step == N
        snap = T._snapshot(buf)
        live = [(snap[7] + j) % cap for j in range(len(buf))]
        assert (snap[4][live] == 1.0).sum() >= 2 and all(snap[6][p] == 0 for p in live if snap[4][p] == 1.0)      # episodes that end with done = 1
        py, draws, ctr = random.Random(seed), 0, 0
        seen = {kd: 0 for kd in KINDS}
        for n in SIZES:
            for form in ("public", "engine", "engine_head"):
                B, M = (n, 1) if n <= len(buf) else (1, n)
                if mode == "given":
                    idx = _given(snap, len(buf), n, ctr, seed, k, N, gen)
                else:
                    idx = T._indices(mode, py, seed, draws, len(buf), B, M, gen)
                draws += M
                arg = idx if mode == "given" else None
                want = NS.gather(*snap[:7], snap[7], cap, idx, ctr, seed, k, kind, THR, N, gamma)
                if form == "public":
                    out = buf.sample(B, M, indices=arg, return_indices=mode != "given")
                    if mode != "given":
                        assert np.array_equal(out[5], idx), (mode, n, "the ring drew other indices than the oracle")
                    got = dict(s=_np(out[0]), a=_np(out[1]), r=_np(out[2]).ravel(), ns=_np(out[3]), d=_np(out[4]).ravel())
                    for key in ("s", "a", "r", "ns", "d"):
                        assert np.array_equal(bits(got[key]), bits(want[key])), (mode, n, form, key)
                else:
                    side = torch.arange(48, dtype=torch.uint8, device="cuda") if form == "engine_head" else None
                    out = buf.gather_update(B, M, indices=arg, spa=True, side=side)
                    sa, nsa, spa = T._engine_form(want, dims)
                    assert np.array_equal(bits(_np(out[0])), bits(sa)), (mode, n, form, "sa")
                    assert np.array_equal(bits(_np(out[1])), bits(nsa)), (mode, n, form, "nsa")     # zero columns beyond S4 included
                    g_spa = _np(out[2])
                    assert np.array_equal(bits(g_spa[:, :spa.shape[1]]), bits(spa)) and np.isnan(g_spa[:, spa.shape[1]:]).all(), (mode, n, form, "spa")
                    assert np.array_equal(bits(_np(out[3])), bits(want["r"])), (mode, n, form, "r")
                    assert np.array_equal(bits(_np(out[4])), bits(want["d"])), (mode, n, form, "d")
                    if side is not None:
                        assert torch.equal(out[5], side), "side copy"
                ctr += n
                assert buf.relabel_counter == ctr, (mode, n, form)
                if mode == "given":
                    for t, j in enumerate(idx):
                        for kd in KINDS:
                            seen[kd] += _row_kind(kd, snap, N, int(j), int(want["f"][t]))
        if mode == "given":
            can_cross = any(p + min(N, int(snap[6][p]) + 1) - 1 >= cap for p in live)
            assert can_cross == (ring != "cap300_wrapped")               # (that ring's wrap falls between two episodes)
            for kd in KINDS:
                need = (kd != "goal_inside_window" or k > 0) and (kd != "crosses_physical_end" or can_cross)
                assert (seen[kd] > 0) == need, (kd, seen)


# ---------------------------------------------------------------- 2. n_step = 1 is the keyword left out
def _agent(gcrl, kind, seed, **kw):
    extra = {"TD3": dict(ac_update_freq=2, policy_noise=0.2, noise_clamp=0.5), "SAC": dict(ac_update_freq=2), "TQC": dict(ac_update_freq=2)}.get(kind, {})
    cfg = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150, k_future=4, **extra)
    cls = {"DDPG": gcrl.DDPG, "TD3": gcrl.TD3Agent, "SAC": gcrl.SACAgent, "TQC": gcrl.TQCAgent}[kind]
    return cls(REACH[0], REACH[1], cfg, None, nenvs=2, gradient_step=6, rng="engine", seed=seed, relabel="sample", **kw)


def test_n_step_1_is_the_keyword_left_out(gcrl):
    a, b = _buffer(gcrl, 60, REACH, seed=3), _buffer(gcrl, 60, REACH, seed=3, n_step=1)
    for buf in (a, b):
        _fill(buf, REACH, 2, 40)
    for n in (17, 48):
        for x, y in zip(a.sample(n, 1), b.sample(n, 1)):
            assert np.array_equal(bits(_np(x)), bits(_np(y))), n
        for x, y in zip(a.gather_update(n, spa=True), b.gather_update(n, spa=True)):
            assert np.array_equal(_np(x).view(np.uint32), _np(y).view(np.uint32)), n
    assert a.relabel_counter == b.relabel_counter == 2 * (17 + 48)
    one, two = _agent(gcrl, "DDPG", 33), _agent(gcrl, "DDPG", 33, n_step=1)
    for x in (one, two):
        T._fill_agent(x, 51)
        T._perturb(x, 1)
    u = T._tuples([one.update(s) for s in range(1, 4)] + one.update_many(4, 6))
    v = T._tuples([two.update(s) for s in range(1, 4)] + two.update_many(4, 6))
    assert np.array_equal(u.view(np.uint64), v.view(np.uint64)), (u, v)
    assert np.array_equal(T._state(one), T._state(two))
    assert one.buffer.relabel_counter == two.buffer.relabel_counter == 9 * 64


# ---------------------------------------------------------------- 3. engine
@pytest.mark.parametrize("kind", ["TD3", "SAC", "TQC"])
def test_engine_equals_twin_fed_the_restated_batches(gcrl, kind):
    B, seed, N = 64, 31, 3
    ag, twin, many = (_agent(gcrl, kind, seed, n_step=N) for _ in range(3))
    for x in (ag, many):
        T._fill_agent(x, 50)                                    # 200 rows through a ring of 150: wrapped
    for x in (ag, twin, many):
        T._perturb(x, 0)
    assert ag.buffer.n_step == N and len(ag.buffer) == 150 and T._head(ag.buffer) == 50
    snap = T._snapshot(ag.buffer)
    thr = ag.buffer._reward_cfg[1]
    py = random.Random(seed)
    got, want, cut = [], [], 0
    for step in range(1, 7):
        idx = her_oracle.sample_indices(py, 150, B)
        b = NS.gather(*snap[:7], snap[7], 150, idx, (step - 1) * B, seed, 4, R.SPARSE, thr, N, ag.config.gamma)
        cut += int((b["m"] < N).sum())
        batch = tuple(torch.from_numpy(x).cuda() for x in (b["s"], b["a"], b["r"].reshape(-1, 1), b["ns"], b["d"].reshape(-1, 1)))
        got.append(ag.update(step))
        want.append(twin.update(step, batch=batch))
    assert cut > 0 and ag.buffer.relabel_counter == 6 * B
    g, w = T._tuples(got), T._tuples(want)
    assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (g, w)
    assert np.array_equal(T._state(ag), T._state(twin)), "engine state differs from the twin fed the restated batches"
    m = T._tuples(many.update_many(1, 6))
    assert np.array_equal(m.view(np.uint64), g.view(np.uint64)), (m, g)
    assert np.array_equal(T._state(many), T._state(ag)), "update_many(1, 6) is not 6 x update()"
    assert many.buffer.relabel_counter == 6 * B


def test_ddpg_row_chain_update_many_equals_update(gcrl):
    """the default DDPG path: a call's head gather and its main gather carry one gamma and continue one counter"""
    one, many, plain = _agent(gcrl, "DDPG", 33, n_step=3), _agent(gcrl, "DDPG", 33, n_step=3), _agent(gcrl, "DDPG", 33)
    for x in (one, many, plain):
        T._fill_agent(x, 51)
        T._perturb(x, 1)
    a = T._tuples([one.update(s) for s in range(1, 7)])
    b = T._tuples(many.update_many(1, 6))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (a, b)
    assert np.array_equal(T._state(one), T._state(many))
    assert one.buffer.relabel_counter == many.buffer.relabel_counter == 6 * 64
    c = T._tuples(plain.update_many(1, 6))                       # N matters: the one-step ring learns from other targets
    assert plain.buffer.relabel_counter == 6 * 64
    assert not np.array_equal(b.view(np.uint64), c.view(np.uint64))


# ---------------------------------------------------------------- 4. populations
def _pop_cfgs():
    return [make_config("DDPG", hidden_dim=64, layer_count=3, batch_size=64, max_len=150, k_future=4, actor_lr=1e-3 * (1 + 0.25 * i),
                        gamma=0.98 - 0.08 * i, tau=0.05 + 0.01 * i) for i in range(2)]


CALLS = [(1, 0), (2, 6)]
AFTER = [(8, 0), (9, 6)]


def _compare(pop, solo, calls):
    for s0, n in calls:
        got = T._run(pop, s0, n)
        want = [T._run(a, s0, n) for a in solo]                  # (a shared ring: the standalone agents in member order)
        for i in range(len(solo)):
            g_, w_ = T._tuples([got[i]] if n == 0 else got[i]), T._tuples([want[i]] if n == 0 else want[i])
            assert np.array_equal(g_.view(np.uint64), w_.view(np.uint64)), (i, s0, n)
    for i, a in enumerate(solo):
        assert np.array_equal(T._state(pop.members[i]), T._state(a)), i


@pytest.mark.parametrize("shared", [False, True], ids=["own_rings", "shared_ring"])
def test_population_members_gather_with_their_own_gamma(gcrl, shared):
    cfgs, seeds, N = _pop_cfgs(), [61, 62], 3
    D = REACH[0]
    pop = gcrl.DDPGPopulation(D, REACH[1], cfgs, 2, 6, rng="engine", seeds=seeds, shared_ring=shared, relabel="sample", n_step=N)
    solo = [gcrl.DDPG(D, REACH[1], c, None, nenvs=2, gradient_step=6, rng="engine", seed=s, relabel="sample", n_step=N) for c, s in zip(cfgs, seeds)]
    if shared:
        assert pop.buffer.n_step == N and all(m.buffer is pop.buffer for m in pop.members)
        ring = gcrl.HERBuffer(cfgs[0].max_len, cfgs[0].max_eps_len, 4, k_future=4, rng="engine", seed=seeds[0], relabel="sample", n_step=N,
                              gamma=cfgs[0].gamma)
        for a in solo:
            a.buffer = ring
        for who in (pop.members, solo):
            gen = np.random.default_rng(80)
            for ep in range(4):
                for st in her_oracle.synthetic_episode(gen, 50, REACH[0], REACH[1]):
                    who[ep % 2].push_her(ep % 4, *st)
    for i in range(2):
        for x in (pop.members[i], solo[i]):
            if not shared:
                T._fill_agent(x, 70 + i)
            T._perturb(x, i)
    _compare(pop, solo, CALLS)
    pop.explore(1, gamma=0.8)                                    # a live change of gamma holds from the next call on
    solo[1].set_hyperparameters(gamma=0.8)
    _compare(pop, solo, AFTER)
    rows = sum(max(n, 1) for _, n in CALLS + AFTER) * 64
    if shared:
        assert pop.buffer.relabel_counter == solo[0].buffer.relabel_counter == 2 * rows
    else:
        assert all(pop.members[i].buffer.relabel_counter == solo[i].buffer.relabel_counter == rows for i in range(2))
    assert pop.gather_counts()[1] == 0, pop.gather_counts()     # sample-mode gathers stay member by member


def test_engine_gathers_with_the_agents_gamma_not_the_rings(gcrl):
    """an agent whose ring was built with another gamma: its update calls discount by the agent's, as of the call — also after
    set_hyperparameters — while the ring's own sample() keeps the ring's"""
    B, seed, N = 64, 35, 3
    ag, twin = (_agent(gcrl, "TD3", seed, n_step=N) for _ in range(2))
    ag.buffer = gcrl.HERBuffer(150, 50, 2, k_future=4, rng="engine", seed=seed, relabel="sample", n_step=N, gamma=0.5)
    T._fill_agent(ag, 50)
    for x in (ag, twin):
        T._perturb(x, 0)
    snap = T._snapshot(ag.buffer)
    thr = ag.buffer._reward_cfg[1]
    py = random.Random(seed)
    got, want = [], []
    for step in range(1, 5):
        if step == 3:
            for x in (ag, twin):
                x.set_hyperparameters(gamma=0.9)
        idx = her_oracle.sample_indices(py, 150, B)
        b = NS.gather(*snap[:7], snap[7], 150, idx, (step - 1) * B, seed, 4, R.SPARSE, thr, N, 0.98 if step < 3 else 0.9)
        batch = tuple(torch.from_numpy(x).cuda() for x in (b["s"], b["a"], b["r"].reshape(-1, 1), b["ns"], b["d"].reshape(-1, 1)))
        got.append(ag.update(step))
        want.append(twin.update(step, batch=batch))
    g, w = T._tuples(got), T._tuples(want)
    assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (g, w)
    assert np.array_equal(T._state(ag), T._state(twin))
    idx = np.arange(64, dtype=np.uint32)
    own = NS.gather(*snap[:7], snap[7], 150, idx, 4 * B, seed, 4, R.SPARSE, thr, N, 0.5)
    out = ag.buffer.sample(64, indices=idx)
    assert np.array_equal(bits(_np(out[2]).ravel()), bits(own["r"])) and np.array_equal(bits(_np(out[4]).ravel()), bits(own["d"]))


# ---------------------------------------------------------------- 5. resume
def test_save_load_resume_bitwise(gcrl, tmp_path):
    a = _buffer(gcrl, 60, REACH, seed=9, n_step=3, gamma=0.98)
    _fill(a, REACH, 2, 42)
    a.sample(17, 2)
    assert a.relabel_counter == 34 and T._head(a) == 40
    meta = a.save_state(str(tmp_path / "ring.bin"))
    b = _buffer(gcrl, 60, REACH, seed=9, n_step=3, gamma=0.98)
    b.load_state(str(tmp_path / "ring.bin"), meta)
    assert b.relabel_counter == 34 and len(b) == 60 and T._head(b) == 0          # re-laid at head 0: the logical order is what counts
    from gcrl_amd._ffi import lib
    assert lib.gcrl_her_get_nstep(b.handle, None) == 3                          # configuration: the constructor's, not the blob's
    for n in (16, 17, 33):
        ga, gb = a.sample(n, 1, return_indices=True), b.sample(n, 1, return_indices=True)
        assert np.array_equal(ga[5], gb[5])
        for x, y in zip(ga[:5], gb[:5]):
            assert np.array_equal(bits(_np(x)), bits(_np(y))), n
        for x, y in zip(a.gather_update(n), b.gather_update(n)):
            if x is not None:
                assert np.array_equal(bits(_np(x)), bits(_np(y))), n
    assert a.relabel_counter == b.relabel_counter
    one = _buffer(gcrl, 60, REACH, seed=9)                       # n_step is not state: a one-step ring loads the same blob
    one.load_state(str(tmp_path / "ring.bin"), meta)
    assert len(one) == 60 and one.relabel_counter == 34


# ---------------------------------------------------------------- 6. refusals
def test_refusals_name_n_step(gcrl):
    import ctypes as C
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import GcrlError, lib
    with pytest.raises(GcrlError, match="n_step"):
        gcrl.HERBuffer(100, 50, 2, relabel="push", n_step=3, gamma=0.98)
    with pytest.raises(GcrlError, match="n_step"):
        gcrl.HERBuffer(100, 50, 2, n_step=2, gamma=0.98)         # (the default mode is "push")
    with pytest.raises(GcrlError, match="n_step"):
        gcrl.HERBuffer(100, 50, 2, relabel="sample", n_step=3)   # no gamma
    for bad in (0, 9, -1, 2.5):
        with pytest.raises(GcrlError, match="n_step"):
            gcrl.HERBuffer(100, 50, 2, relabel="sample", n_step=bad, gamma=0.98)
    for kind, cls in (("DDPG", gcrl.DDPG), ("TD3", gcrl.TD3Agent), ("SAC", gcrl.SACAgent), ("TQC", gcrl.TQCAgent)):
        cfg = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150)
        with pytest.raises(GcrlError, match="n_step"):
            cls(REACH[0], REACH[1], cfg, None, nenvs=2, gradient_step=6, rng="engine", seed=1, n_step=3)                     # relabel="push"
        for bt in ("REPLAY", "PER"):
            cfg_b = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150, buffer_type=bt)
            with pytest.raises(GcrlError, match="n_step"):
                cls(REACH[0], REACH[1], cfg_b, None, nenvs=2, gradient_step=6, rng="engine", seed=1, n_step=3)
    for Pop in (gcrl.DDPGPopulation, gcrl.TD3Population, gcrl.SACPopulation, gcrl.TQCPopulation):
        kind = Pop.AGENT.KIND_NAME
        cfgs = [make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150) for _ in range(2)]
        for kw in (dict(), dict(shared_ring=True)):
            with pytest.raises(GcrlError, match="n_step"):
                Pop(REACH[0], REACH[1], cfgs, 2, 6, rng="engine", seeds=[1, 2], n_step=3, **kw)                              # relabel="push"
    # the native entries
    cfg = _ffi.HerConfig(state_dim=10, action_dim=3, goal_dim=3, capacity=100, nenvs=2, k_future=4, flush_len=50, reward_kind=0,
                         reward_threshold=0.05, device=0, rng_mode=0, seed=1)
    for mode, values in ((1, (0, 9)), (0, (0, 9, 2))):
        h = lib.gcrl_her_create_relabel(C.byref(cfg), None, mode)
        assert h
        try:
            for v in values:
                assert lib.gcrl_her_set_nstep(h, v, 0.98) != 0 and b"n_step" in lib.gcrl_last_error(), (mode, v)
            assert lib.gcrl_her_get_nstep(h, None) == 1
            assert lib.gcrl_her_set_nstep(h, 1, 0.5) == 0       # N = 1 is every ring's default
            if mode == 1:
                g = C.c_double(0.0)
                assert lib.gcrl_her_set_nstep(h, 8, 0.9) == 0 and lib.gcrl_her_get_nstep(h, C.byref(g)) == 8 and g.value == 0.9
        finally:
            lib.gcrl_her_destroy(h)
