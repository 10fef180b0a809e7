"""GPU (-m gpu): sample-time HER relabelling (HERBuffer(relabel="sample"); csrc/her_relabel.hip) held bit for bit to its numpy
definition tests/her_relabel_ref.py: the flush that stores an episode's rows once with their tails, both relabelling gathers
(the public sample's five dense outputs and the update engine's sa | nsa | spa | r | d), the engine and a population on top of
them, state and refusals."""
import random

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import make_config

import her_relabel_ref as R
import test_her_relabel_ref as host

pytestmark = pytest.mark.gpu

REACH, PICK, WIDE = (10, 3, 3), (23, 4, 3), (30, 4, 3)       # (S, A, G); WIDE: a record of more than 64 floats
THR = 0.05


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _np(t):
    return t.detach().cpu().numpy()


def _episode(gen, T, dims, done_last):
    S, A, G = dims
    st = her_oracle.synthetic_episode(gen, T, S, A, G)
    s = np.stack([x[0] for x in st]); a = np.stack([x[1] for x in st]); ns = np.stack([x[2] for x in st])
    r = np.array([x[3] for x in st], np.float32); dg = np.stack([x[5] for x in st]); ag = np.stack([x[6] for x in st])
    d = np.zeros(T, np.float32)
    d[-1] = float(done_last)
    return s, a, ns, r, d, dg, ag


def _head(buf):
    from gcrl_amd._ffi import lib
    return int(lib.gcrl_her_head(buf.handle))


def _mt_state(buf):
    from gcrl_amd._ffi import check, lib
    import ctypes as C
    st = (C.c_uint32 * 625)()
    check(lib.gcrl_mt_get_state(buf.rng.handle, st))
    return list(st)


def _buffer(gcrl, cap, dims, k=4, rng="engine", seed=7, dense=False, nenvs=4):
    buf = gcrl.HERBuffer(cap, 50, nenvs, threshold=THR, k_future=k, rng=rng, seed=seed, relabel="sample")
    buf.compute_reward = her_oracle.dense_reward if dense else her_oracle.sparse_reward
    return buf


# ---------------------------------------------------------------- 1. flush
class Expect:
    """what a sample-mode ring holds: the pushed originals in flush order, each with its tail"""

    def __init__(self):
        self.rows = []

    def flush(self, ep):
        s, a, ns, r, d, dg, ag = ep
        T = len(r)
        for i in range(T):
            self.rows.append((s[i], a[i], ns[i], r[i], d[i], ag[i], T - 1 - i))

    def check(self, buf):
        assert len(buf) == len(self.rows), (len(buf), len(self.rows))
        got = buf.rows()
        for j, key in enumerate("s a ns r d".split()):
            want = np.stack([np.asarray(x[j], np.float32) for x in self.rows])
            assert np.array_equal(bits(got[j]), bits(want)), key
        ag, rem = buf.tails()
        assert np.array_equal(bits(ag), bits(np.stack([x[5] for x in self.rows]))), "tail ag"
        assert np.array_equal(rem, np.array([x[6] for x in self.rows], np.float32)), "tail remaining"


@pytest.mark.parametrize("dims", [REACH, PICK], ids=["reach_rs48", "pickplace_rs64"])
def test_flush_all_push_paths(gcrl, dims):
    S, A, G = dims
    buf = _buffer(gcrl, 1000, dims)
    want = Expect()
    gen = np.random.default_rng(11)
    TS = [(1, True), (2, True), (12, True), (50, False)]          # T = 50 flushes at the staging length, the others by `done`
    mt0 = _mt_state(buf)
    # push: one transition per call, single-episode flushes
    for env, (T, done) in enumerate(TS):
        ep = _episode(gen, T, dims, done)
        s, a, ns, r, d, dg, ag = ep
        for t in range(T):
            st = torch.from_numpy(s[t]).cuda() if t % 2 else s[t]
            buf.push(env, st, a[t], ns[t], r[t], bool(d[t]), dg[t], ag[t])
        want.flush(ep)
    want.check(buf)
    # push_episode
    for env, (T, done) in enumerate(TS):
        ep = _episode(gen, T, dims, done)
        buf.push_episode(env, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
        want.flush(ep)
    want.check(buf)
    # push_batch: four envs step together; episodes that end on the same step flush in ONE launch, in env order
    plan = [[2, 1, 50], [2, 12, 50], [12, 50], [12, 50]]           # per env: its episodes' lengths, back to back
    eps = [[_episode(gen, T, dims, T != 50) for T in ts] for ts in plan]
    cur = [[0, 0] for _ in plan]                                   # per env: (episode, step)
    while any(c[0] < len(eps[e]) for e, c in enumerate(cur)):
        live = [e for e, c in enumerate(cur) if c[0] < len(eps[e])]
        env0, n = live[0], len(live)
        assert live == list(range(env0, env0 + n))
        row = [(eps[e][cur[e][0]], cur[e][1]) for e in live]
        states = torch.from_numpy(np.stack([ep[0][t] for ep, t in row])).cuda()
        nexts = torch.from_numpy(np.stack([ep[2][t] for ep, t in row])).cuda()
        buf.push_batch(states, np.stack([ep[1][t] for ep, t in row]), nexts, np.array([ep[3][t] for ep, t in row], np.float32),
                       np.array([ep[4][t] > 0 for ep, t in row]), np.stack([ep[6][t] for ep, t in row]), env0=env0)
        for e, (ep, t) in zip(live, row):
            if t + 1 == len(ep[3]):
                want.flush(ep)
                cur[e] = [cur[e][0] + 1, 0]
            else:
                cur[e][1] = t + 1
    want.check(buf)
    assert len(buf) == 2 * 65 + sum(sum(ts) for ts in plan)
    assert _mt_state(buf) == mt0, "a flush consumed the MT stream"
    assert buf.relabel_counter == 0


def test_push_batch_flushes_several_episodes_in_one_launch(gcrl):
    """the multi-episode launch itself: 4 envs end together (T = 2), with a ring that wraps inside the launch"""
    buf = _buffer(gcrl, 13, REACH)
    want = Expect()
    gen = np.random.default_rng(12)
    for rnd in range(2):
        eps = [_episode(gen, 2, REACH, True) for _ in range(4)]
        for t in range(2):
            buf.push_batch(torch.from_numpy(np.stack([e[0][t] for e in eps])).cuda(), np.stack([e[1][t] for e in eps]),
                           torch.from_numpy(np.stack([e[2][t] for e in eps])).cuda(), np.array([e[3][t] for e in eps], np.float32),
                           np.array([t == 1] * 4), np.stack([e[6][t] for e in eps]))
        for e in eps:
            want.flush(e)
    want.rows = want.rows[-13:]
    want.check(buf)
    assert _head(buf) == 16 - 13


# ---------------------------------------------------------------- 2. + 3. gathers
def _fill(buf, dims, episodes, seed):
    gen = np.random.default_rng(seed)
    for e in range(episodes):
        ep = _episode(gen, 50, dims, False)
        buf.push_episode(e % 2, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])


def _snapshot(buf):
    """the ring by physical slot, for the restatement"""
    cap, head = buf.max_mem_len, _head(buf)
    s, a, ns, r, d = buf.rows()
    ag, rem = buf.tails()
    return tuple(R.physical(x, head, cap) for x in (s, a, ns, r, d, ag, rem)) + (head, cap)


def _engine_form(want, dims):
    """the restated batch as the update engine's matrices: sa = [s | a | 0], nsa = [ns | 0], the columns spa receives"""
    S, A, _ = dims
    n, ldx, S4 = want["s"].shape[0], (S + A + 3) // 4 * 4, (S + 3) // 4 * 4
    sa = np.zeros((n, ldx), np.float32); nsa = np.zeros((n, ldx), np.float32)
    sa[:, :S] = want["s"]; sa[:, S:S + A] = want["a"]
    nsa[:, :S] = want["ns"]
    return sa, nsa, sa[:, :S4]


RINGS = {"cap60_evicted_crossing": (REACH, 60, 2), "cap300_wrapped": (PICK, 300, 7), "wide_record": (WIDE, 120, 3)}
SIZES = (1, 15, 16, 17, 67)


def _indices(mode, py, seed, draws, length, B, M, gen):
    """the logical indices of the next M batches of B, as the ring draws them — or caller-given ones"""
    if mode == "given":
        return gen.integers(0, length, B * M).astype(np.uint32)
    if mode == "engine":
        return np.array([j for _ in range(M) for j in her_oracle.sample_indices(py, length, B)], np.uint32)
    return np.array([her_oracle.feistel_index(seed, draws + m, length, t) for m in range(M) for t in range(B)], np.uint32)


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("k", [0, 1, 4, 8])
@pytest.mark.parametrize("ring", list(RINGS))
def test_gathers_bitwise_the_restatement(gcrl, ring, k, dense):
    dims, cap, episodes = RINGS[ring]
    S, A, G = dims
    kind = R.DENSE if dense else R.SPARSE
    seed = 1000 + k
    gen = np.random.default_rng(5)
    for mode in ("engine", "device", "given"):
        buf = _buffer(gcrl, cap, dims, k=k, rng="device" if mode == "device" else "engine", seed=seed, dense=dense, nenvs=2)
        _fill(buf, dims, episodes, 40)
        assert len(buf) == min(cap, 50 * episodes)
        snap = _snapshot(buf)
        rem_live = snap[6][[(snap[7] + j) % cap for j in range(len(buf))]]
        if ring == "cap60_evicted_crossing":
            assert snap[7] == 40 and rem_live[0] == 9 and rem_live[10] == 49     # the first episode lost its 40 oldest rows;
            # the second lies at slots 50 .. 59, 0 .. 39: its future slots cross the physical end
        py, draws, ctr = random.Random(seed), 0, 0
        relabelled = 0
        for n in SIZES:
            for form in ("public", "engine", "engine_head"):
                B, M = (n, 1) if n <= len(buf) else (1, n)       # a batch is drawn without replacement: more rows than the ring holds come as M batches of one
                idx = _indices(mode, py, seed, draws, len(buf), B, M, gen)
                draws += M
                arg = idx if mode == "given" else None
                want = R.gather(*snap[:7], snap[7], cap, idx, ctr, seed, k, kind, THR)
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
                    sa, nsa, spa = _engine_form(want, dims)
                    assert np.array_equal(bits(_np(out[0])), bits(sa)), (mode, n, form, "sa")
                    assert np.array_equal(bits(_np(out[1])), bits(nsa)), (mode, n, form, "nsa")     # zero columns beyond S4 included
                    g_spa = _np(out[2])
                    assert np.array_equal(bits(g_spa[:, :spa.shape[1]]), bits(spa)) and np.isnan(g_spa[:, spa.shape[1]:]).all(), (mode, n, form, "spa")
                    assert np.array_equal(bits(_np(out[3])), bits(want["r"])), (mode, n, form, "r")
                    assert np.array_equal(bits(_np(out[4])), bits(want["d"])), (mode, n, form, "d")
                    if side is not None:
                        assert torch.equal(out[5], side), "side copy"
                    got = dict(s=_np(out[0])[:, :S], a=_np(out[0])[:, S:S + A], r=_np(out[3]), ns=_np(out[1])[:, :S], d=_np(out[4]))
                ctr += n
                assert buf.relabel_counter == ctr, (mode, n, form)
                relabelled += _properties(got, want, snap, idx, dims, kind, k)
        if k == 0:
            assert relabelled == 0
        else:
            assert relabelled > 0


def _properties(got, want, snap, idx, dims, kind, k):
    """3.: what a relabelled row must be, read off the DEVICE's outputs and the ring alone; -> number of relabelled rows"""
    S, A, G = dims
    s, a, ns, r, d, ag, rem, head, cap = snap
    count = 0
    for t, j in enumerate(idx):
        p = (head + int(j)) % cap
        if np.array_equal(bits(got["s"][t]), bits(s[p])) and np.array_equal(bits(got["ns"][t]), bits(ns[p])) and \
                bits(got["r"][t:t + 1])[0] == bits(r[p:p + 1])[0] and got["d"][t] == d[p]:
            continue                                             # the stored row (a relabelled one carries another goal: the achieved goals walk)
        count += 1
        assert np.array_equal(bits(got["s"][t, :S - G]), bits(s[p, :S - G])) and np.array_equal(bits(got["a"][t]), bits(a[p]))
        assert np.array_equal(bits(got["ns"][t, :S - G]), bits(ns[p, :S - G]))
        goal = got["s"][t, S - G:]
        assert np.array_equal(bits(goal), bits(got["ns"][t, S - G:]))
        later = [(p + f) % cap for f in range(1, int(rem[p]) + 1)]              # the rows of its episode after it
        hits = [q for q in later if np.array_equal(bits(ag[q]), bits(goal))]
        assert hits, (t, "the goal is no later row's achieved goal")
        assert got["d"][t] == 0.0
        assert any(bits(np.array([R.reward(ag[p], ag[q], kind, THR)]))[0] == bits(got["r"][t:t + 1])[0] for q in hits)
    assert count == int((want["f"] > 0).sum())
    return count


def test_share_of_relabelled_rows_is_the_host_count(gcrl):
    """4 096 gathered rows that all have a later row, seed and k of the host test: the device relabels exactly as many"""
    buf = _buffer(gcrl, 300, PICK, k=host.SHARE_K, seed=host.SHARE_SEED, nenvs=2)
    _fill(buf, PICK, 6, 41)
    _, rem = buf.tails()
    ok = np.flatnonzero(rem > 0)
    idx = ok[np.random.default_rng(6).integers(0, ok.size, host.SHARE_N)].astype(np.uint32)
    s, _, _, _, d = buf.sample(1, host.SHARE_N, indices=idx)
    stored = buf.rows()[0]
    changed = int((bits(_np(s)) != bits(stored[idx])).any(axis=1).sum())     # (a random walk: no later goal equals the desired goal)
    assert changed == host.share_count(), (changed, host.share_count())
    sa = buf.gather_update(1, host.SHARE_N, indices=idx)[0]
    assert buf.relabel_counter == 2 * host.SHARE_N
    want = R.relabel_count(host.SHARE_SEED, host.SHARE_K, host.SHARE_N, host.SHARE_N)
    assert int((bits(_np(sa)[:, :PICK[0]]) != bits(stored[idx])).any(axis=1).sum()) == want


# ---------------------------------------------------------------- 4. engine
def _perturb(ag, i):
    gen = np.random.default_rng(200 + i)
    nets = [ag.actor] + (list(ag.critics) if hasattr(ag, "critics") else [ag.critic])
    for v in nets:
        v.set_flat((v.flat() + 0.05 * gen.standard_normal(v.numel())).astype(np.float32))
    ag.update_target_network()


def _state(ag):
    from gcrl_amd._ffi import check, lib
    n = int(lib.gcrl_agent_state_size(ag._h))
    blob = np.empty(n, np.uint8)
    check(lib.gcrl_agent_save_state(ag._h, blob.ctypes.data, n))
    return blob


def _tuples(ts):
    w = max(len(t) for t in ts)
    return np.array([[float(len(t))] + [float(x) for x in t] + [0.0] * (w - len(t)) for t in ts], np.float64)


def _fill_agent(ag, seed, episodes=4):
    gen = np.random.default_rng(seed)
    for ep in range(episodes):
        for st in her_oracle.synthetic_episode(gen, 50, REACH[0], REACH[1]):
            ag.push_her(ep % 2, *st)


def _agent(gcrl, kind, seed, relabel, **kw):
    cfg = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150, k_future=4, **kw)
    cls = {"DDPG": gcrl.DDPG, "TD3": gcrl.TD3Agent, "SAC": gcrl.SACAgent}[kind]
    return cls(REACH[0], REACH[1], cfg, None, nenvs=2, gradient_step=6, rng="engine", seed=seed, relabel=relabel)


@pytest.mark.parametrize("kind", ["TD3", "SAC"])
def test_engine_equals_twin_fed_the_restated_batches(gcrl, kind):
    B, seed = 64, 31
    extra = dict(ac_update_freq=2, policy_noise=0.2, noise_clamp=0.5) if kind == "TD3" else dict(ac_update_freq=2)
    ag, twin, many = (_agent(gcrl, kind, seed, "sample", **extra) for _ in range(3))
    for x in (ag, many):
        _fill_agent(x, 50)                                      # 200 rows through a ring of 150: wrapped
    for x in (ag, twin, many):
        _perturb(x, 0)
    assert ag.buffer.relabel == "sample" and len(ag.buffer) == 150 and _head(ag.buffer) == 50
    snap = _snapshot(ag.buffer)
    thr = ag.buffer._reward_cfg[1]
    py = random.Random(seed)
    got, want = [], []
    for step in range(1, 7):
        idx = her_oracle.sample_indices(py, 150, B)
        b = R.gather(*snap[:7], snap[7], 150, idx, (step - 1) * B, seed, 4, R.SPARSE, thr)
        batch = tuple(torch.from_numpy(x).cuda() for x in (b["s"], b["a"], b["r"].reshape(-1, 1), b["ns"], b["d"].reshape(-1, 1)))
        got.append(ag.update(step))
        want.append(twin.update(step, batch=batch))
    assert ag.buffer.relabel_counter == 6 * B
    g, w = _tuples(got), _tuples(want)
    assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (g, w)
    assert np.array_equal(_state(ag), _state(twin)), "engine state differs from the twin fed the restated batches"
    m = _tuples(many.update_many(1, 6))
    assert np.array_equal(m.view(np.uint64), g.view(np.uint64)), (m, g)
    assert np.array_equal(_state(many), _state(ag)), "update_many(1, 6) is not 6 x update()"
    assert many.buffer.relabel_counter == 6 * B


def test_ddpg_row_chain_update_many_equals_update(gcrl):
    """the default DDPG path: a call's head gather and its main gather continue one counter"""
    one, many = (_agent(gcrl, "DDPG", 33, "sample") for _ in range(2))
    for x in (one, many):
        _fill_agent(x, 51)
        _perturb(x, 1)
    a = _tuples([one.update(s) for s in range(1, 7)])
    b = _tuples(many.update_many(1, 6))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (a, b)
    assert np.array_equal(_state(one), _state(many))
    assert one.buffer.relabel_counter == many.buffer.relabel_counter == 6 * 64
    push = _agent(gcrl, "DDPG", 33, "push")                      # the mode matters: the default ring learns from other batches
    _fill_agent(push, 51)
    _perturb(push, 1)
    c = _tuples(push.update_many(1, 6))
    assert not np.array_equal(b.view(np.uint64), c.view(np.uint64))


# ---------------------------------------------------------------- 5. population
def _pop_cfgs():
    return [make_config("DDPG", hidden_dim=64, layer_count=3, batch_size=64, max_len=150, k_future=4, actor_lr=1e-3 * (1 + 0.25 * i),
                        gamma=0.98 - 0.01 * i, tau=0.05 + 0.01 * i) for i in range(2)]


CALLS = [(1, 0), (2, 0), (3, 6), (9, 6)]


def _run(x, s0, n):
    return x.update(s0) if n == 0 else x.update_many(s0, n)


def test_population_own_rings(gcrl):
    cfgs, seeds = _pop_cfgs(), [61, 62]
    D = REACH[0]
    pop = gcrl.DDPGPopulation(D, REACH[1], cfgs, 2, 6, rng="engine", seeds=seeds, relabel="sample")
    pop.merge_gather = True
    solo = [gcrl.DDPG(D, REACH[1], c, None, nenvs=2, gradient_step=6, rng="engine", seed=s, relabel="sample") for c, s in zip(cfgs, seeds)]
    for i in range(2):
        for x in (pop.members[i], solo[i]):
            _fill_agent(x, 70 + i)
            _perturb(x, i)
    for s0, n in CALLS:
        got = _run(pop, s0, n)
        for i, a in enumerate(solo):
            w = _run(a, s0, n)
            g_, w_ = _tuples([got[i]] if n == 0 else got[i]), _tuples([w] if n == 0 else w)
            assert np.array_equal(g_.view(np.uint64), w_.view(np.uint64)), (i, s0, n)
    for i in range(2):
        assert np.array_equal(_state(pop.members[i]), _state(solo[i])), i
        assert pop.members[i].buffer.relabel_counter == solo[i].buffer.relabel_counter == 14 * 64
    calls, merged, alone = pop.gather_counts()
    assert merged == 0 and calls == len(CALLS) and alone == 2 * len(CALLS), (calls, merged, alone)


def test_population_shared_ring(gcrl):
    cfgs, seeds = _pop_cfgs(), [63, 64]
    D = REACH[0]
    pop = gcrl.DDPGPopulation(D, REACH[1], cfgs, 2, 6, rng="engine", seeds=seeds, shared_ring=True, relabel="sample")
    pop.merge_gather = True
    assert pop.buffer.relabel == "sample" and all(m.buffer is pop.buffer for m in pop.members)
    solo = [gcrl.DDPG(D, REACH[1], c, None, nenvs=2, gradient_step=6, rng="engine", seed=s, relabel="sample") for c, s in zip(cfgs, seeds)]
    ring = gcrl.HERBuffer(cfgs[0].max_len, cfgs[0].max_eps_len, 4, k_future=4, rng="engine", seed=seeds[0], relabel="sample")
    for a in solo:
        a.buffer = ring
    for who in (pop.members, solo):
        gen = np.random.default_rng(80)
        for ep in range(4):
            for st in her_oracle.synthetic_episode(gen, 50, REACH[0], REACH[1]):
                who[ep % 2].push_her(ep % 4, *st)
    for i in range(2):
        _perturb(pop.members[i], i)
        _perturb(solo[i], i)
    for s0, n in CALLS:
        got = _run(pop, s0, n)
        want = [_run(a, s0, n) for a in solo]                    # standalone agents that share the ring, called in member order
        for i in range(2):
            g_, w_ = _tuples([got[i]] if n == 0 else got[i]), _tuples([want[i]] if n == 0 else want[i])
            assert np.array_equal(g_.view(np.uint64), w_.view(np.uint64)), (i, s0, n)
    for i in range(2):
        assert np.array_equal(_state(pop.members[i]), _state(solo[i])), i
    assert pop.buffer.relabel_counter == ring.relabel_counter == 2 * 14 * 64
    assert pop.gather_counts()[1] == 0, pop.gather_counts()


# ---------------------------------------------------------------- 6. state and refusals
def test_save_load_resume_bitwise(gcrl, tmp_path):
    a = _buffer(gcrl, 60, REACH, seed=9, nenvs=2)
    _fill(a, REACH, 2, 42)
    gen = np.random.default_rng(43)
    ep = _episode(gen, 7, REACH, False)
    for t in range(7):                                            # a partial episode stays staged across the save
        a.push(1, ep[0][t], ep[1][t], ep[2][t], ep[3][t], False, ep[5][t], ep[6][t])
    a.sample(17, 2)
    assert a.relabel_counter == 34 and _head(a) == 40
    meta = a.save_state(str(tmp_path / "ring.bin"))
    assert meta["relabel"] == "sample"
    b = _buffer(gcrl, 60, REACH, seed=9, nenvs=2)
    b.load_state(str(tmp_path / "ring.bin"), meta)
    assert b.relabel_counter == 34 and len(b) == 60 and _head(b) == 0          # re-laid at head 0: the logical order is what counts
    for x, y in zip(a.tails() + a.rows(), b.tails() + b.rows()):
        assert np.array_equal(bits(x), bits(y))
    for n in (16, 17, 33):
        if n == 17:                                               # the staged episode continues identically on both sides
            for buf in (a, b):
                for t in range(7, 50):
                    e2 = _episode(np.random.default_rng(44), 50, REACH, False)
                    buf.push(1, e2[0][t], e2[1][t], e2[2][t], e2[3][t], False, e2[5][t], e2[6][t])
        ga, gb = a.sample(n, 1, return_indices=True), b.sample(n, 1, return_indices=True)
        assert np.array_equal(ga[5], gb[5])
        for x, y in zip(ga[:5], gb[:5]):
            assert np.array_equal(bits(_np(x)), bits(_np(y))), n
        ua, ub = a.gather_update(n), b.gather_update(n)
        for x, y in zip(ua, ub):
            if x is not None:
                assert np.array_equal(bits(_np(x)), bits(_np(y))), n
    assert a.relabel_counter == b.relabel_counter


def test_refusals_name_their_field(gcrl, tmp_path):
    from gcrl_amd._ffi import GcrlError, lib
    # compute_reward that is neither built-in
    buf = gcrl.HERBuffer(100, 50, 2, rng="engine", seed=1, relabel="sample")
    buf.compute_reward = lambda ag, g, info: -np.abs(np.asarray(ag) - np.asarray(g)).sum() ** 2
    ep = _episode(np.random.default_rng(1), 3, REACH, True)
    with pytest.raises(GcrlError, match="compute_reward"):
        buf.push_episode(0, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
    import ctypes as C
    from gcrl_amd import _ffi
    cfg = _ffi.HerConfig(state_dim=10, action_dim=3, goal_dim=3, capacity=100, nenvs=2, k_future=4, flush_len=50, reward_kind=2,
                         reward_threshold=0.05, device=0, rng_mode=0, seed=1)
    assert not lib.gcrl_her_create_relabel(C.byref(cfg), None, 1)
    assert b"compute_reward" in lib.gcrl_last_error()
    # a priority tree on a sample-mode ring
    s = _buffer(gcrl, 100, REACH, nenvs=2)
    _fill(s, REACH, 1, 3)
    with pytest.raises(GcrlError, match="relabel"):
        _ffi.check(lib.gcrl_per_attach(s.handle, 0.6, 1e-6))
    # load_state across modes, both ways (the native entry refuses as well)
    p = gcrl.HERBuffer(100, 50, 2, rng="engine", seed=1, relabel="push")
    p.compute_reward = her_oracle.sparse_reward
    p.push_episode(0, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
    meta_s, meta_p = s.save_state(str(tmp_path / "s.bin")), p.save_state(str(tmp_path / "p.bin"))
    with pytest.raises(GcrlError, match="relabel"):
        p.load_state(str(tmp_path / "s.bin"), meta_s)
    with pytest.raises(GcrlError, match="relabel"):
        s.load_state(str(tmp_path / "p.bin"), meta_p)
    blob = np.fromfile(str(tmp_path / "p.bin"), dtype=np.uint8)
    with pytest.raises(GcrlError, match="relabel"):
        _ffi.check(lib.gcrl_her_load_state(s.handle, blob.ctypes.data, blob.size))
    with pytest.raises(GcrlError, match="relabel"):
        p.tails()
    # exploit(copy_ring=True) between rings of different modes
    cfgs = _pop_cfgs()
    pop = gcrl.DDPGPopulation(REACH[0], REACH[1], cfgs, 2, 6, rng="engine", seeds=[5, 6])
    pop.members[1].buffer = gcrl.HERBuffer(cfgs[1].max_len, 50, 2, k_future=4, rng="engine", seed=6, relabel="sample")
    for m in pop.members:
        _fill_agent(m, 90, episodes=1)
    with pytest.raises(GcrlError, match="relabel"):
        pop.exploit([(0, 1)], copy_ring=True)
    with pytest.raises(ValueError, match="relabel"):
        gcrl.HERBuffer(100, 50, 2, relabel="final")


def test_push_mode_rings_keep_the_golden_bytes(gcrl):
    """relabel="push" spelled out is the ring of before: the reference's stored rows, bit for bit"""
    import test_gpu_parity as par
    g = par.load_golden("her_rows.npz")
    for name in par.CASES:
        cap, k = (int(x) for x in g[f"{name}_cap_k"])
        random.seed(1898)
        buf = gcrl.HERBuffer(cap, 50, 2, k_future=k, rng="python", relabel="push")
        buf.compute_reward = her_oracle.sparse_reward
        par.push_case(g, name, buf, "episode")
        for key, arr in zip("s a ns r d".split(), buf.rows()):
            assert np.array_equal(bits(arr), bits(g[f"{name}_rows_{key}"])), (name, key)
        assert buf.relabel_counter == 0
