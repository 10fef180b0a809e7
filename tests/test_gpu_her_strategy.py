"""GPU (-m gpu): the `final` and `episode` goal-selection strategies of a sample-mode HER ring (HERBuffer(relabel="sample",
goal_strategy=...); csrc/her_relabel.hip) held bit for bit to the numpy definition tests/her_strategy_ref.py: the flush that
stamps `elapsed`, both gathers one-step and with n-step windows, `future` against the keyword left out, the four agents and a
population on top of them, resume and refusals.  Helpers and shapes are those of tests/test_gpu_her_relabel.py."""
import random

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import make_config

import her_relabel_ref as R
import her_strategy_ref as GS
import test_gpu_her_relabel as T
from test_gpu_her_relabel import PICK, REACH, SIZES, THR, _np, bits

pytestmark = pytest.mark.gpu

OUT = ("s", "a", "r", "ns", "d")


def _buffer(gcrl, cap, dims, strategy, k=4, rng="engine", seed=7, dense=False, nenvs=2, **kw):
    if strategy is not None:
        kw["goal_strategy"] = strategy
    buf = gcrl.HERBuffer(cap, 50, nenvs, threshold=THR, k_future=k, rng=rng, seed=seed, relabel="sample", **kw)
    buf.compute_reward = her_oracle.dense_reward if dense else her_oracle.sparse_reward
    return buf


def _fill(buf, dims, lengths, seed):
    """whole episodes of the given lengths; one of 50 rows flushes at the staging length, a shorter one ends with done = 1"""
    gen = np.random.default_rng(seed)
    for e, n in enumerate(lengths):
        ep = T._episode(gen, n, dims, n != 50)
        buf.push_episode(e % 2, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])


def _snapshot(buf):
    """the ring by physical slot, for the restatement: her_relabel's seven arrays, elapsed (None without the word), head, cap"""
    snap = T._snapshot(buf)
    el = R.physical(buf.elapsed(), snap[7], snap[8]) if buf.goal_strategy == "episode" else None
    return snap[:7] + (el,) + snap[7:]


# ---------------------------------------------------------------- 1. flush
@pytest.mark.parametrize("cap", [120, 300])
def test_flush_stamps_elapsed(gcrl, cap):
    epi, fut = _buffer(gcrl, cap, REACH, "episode", nenvs=4), _buffer(gcrl, cap, REACH, None, nenvs=4)
    gen = np.random.default_rng(11)
    want = []
    eps = [T._episode(gen, n, REACH, n != 50) for n in (50, 13, 1) + (50,) * (cap // 50 + 1)]
    for e, ep in enumerate(eps):
        s, a, ns, r, d, dg, ag = ep
        for buf in (epi, fut):
            if len(r) == 13:                                         # an episode ended by `done` at t = 12, pushed row by row
                for t in range(13):
                    buf.push(e % 4, s[t], a[t], ns[t], r[t], bool(d[t]), dg[t], ag[t])
            elif e % 2:
                buf.push_episode(e % 4, s, a, ns, r, d, ag)
            else:                                                    # a vector-env step per row, one env
                for t in range(len(r)):
                    buf.push_batch(torch.from_numpy(s[t:t + 1]).cuda(), a[t:t + 1], torch.from_numpy(ns[t:t + 1]).cuda(), r[t:t + 1],
                                   d[t:t + 1] > 0, ag[t:t + 1], env0=e % 4)
        want += list(range(len(r)))
    total = len(want)
    assert total > cap and len(epi) == len(fut) == cap and T._head(epi) == T._head(fut) == total % cap != 0
    assert np.array_equal(epi.elapsed(), np.array(want[-cap:], np.float32))
    for x, y in zip(epi.rows() + epi.tails(), fut.rows() + fut.tails()):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(epi.elapsed(3, 5), np.array(want[-cap:][3:8], np.float32))
    assert epi.relabel_counter == 0
    from gcrl_amd._ffi import GcrlError, lib
    assert lib.gcrl_her_goal_strategy(epi.handle) == 2 and lib.gcrl_her_goal_strategy(fut.handle) == 0
    with pytest.raises(GcrlError, match="goal_strategy"):
        fut.elapsed()
    el = np.empty(1, np.float32)
    assert lib.gcrl_her_read_elapsed(fut.handle, 0, 1, el.ctypes.data) != 0 and b"goal_strategy" in lib.gcrl_last_error()


# ---------------------------------------------------------------- 2. + 3. gathers
# capacity, episode lengths: 114 rows in a ring of 300; 214 rows through 114 slots (head 100: two whole episodes evicted, the oldest
# live row starts one); 164 rows through 120 slots (head 44: the oldest episode keeps its last 6 rows, drawn at j < elapsed)
RINGS = {"partly_filled": (300, [50, 13, 1, 50]), "wrapped": (114, [50, 50, 13, 1, 50, 50]), "wrapped_oldest_cut": (120, [50, 50, 13, 1, 50])}


def _run_gathers(gcrl, strategy, dims, ring, N, k, dense, gamma):
    cap, lengths = RINGS[ring]
    S, A, G = dims
    kind = R.DENSE if dense else R.SPARSE
    seed = 3000 + 10 * N + k
    gen = np.random.default_rng(5)
    kw = dict(n_step=N, gamma=gamma) if N > 1 else {}
    for mode in ("engine", "device", "given"):
        buf = _buffer(gcrl, cap, dims, strategy, k=k, rng="device" if mode == "device" else "engine", seed=seed, dense=dense, **kw)
        _fill(buf, dims, lengths, 40)
        length = min(cap, sum(lengths))
        assert len(buf) == length and T._head(buf) == (sum(lengths) % cap if sum(lengths) > cap else 0)
        snap = _snapshot(buf)
        head = snap[8]
        assert (ring == "partly_filled") == (head == 0)
        py, draws, ctr = random.Random(seed), 0, 0
        seen = dict(back=0, fwd=0, cut=0, hit=0)
        for n in SIZES:
            for form in ("public", "engine", "engine_head"):
                B, M = (n, 1) if n <= length else (1, n)
                idx = T._indices(mode, py, seed, draws, length, B, M, gen)
                if mode == "given":
                    idx[0] = ctr % 6                                 # one of the oldest rows: on the cut ring j < elapsed
                draws += M
                arg = idx if mode == "given" else None
                want = GS.gather(*snap[:8], head, cap, idx, ctr, seed, k, kind, THR, strategy, N, gamma)
                if form == "public":
                    out = buf.sample(B, M, indices=arg, return_indices=mode != "given")
                    if mode != "given":
                        assert np.array_equal(out[5], idx), (mode, n, "the ring drew other indices than the oracle")
                    got = dict(s=_np(out[0]), a=_np(out[1]), r=_np(out[2]).ravel(), ns=_np(out[3]), d=_np(out[4]).ravel())
                    for key in OUT:
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
                ctr += n                                             # the relabel counter is carried from launch to launch
                assert buf.relabel_counter == ctr, (mode, n, form)
                seen["back"] += int((want["o"] < 0).sum()); seen["fwd"] += int((want["o"] > 0).sum())
                seen["hit"] += int((want["o"] != 0).sum())
                if strategy == "episode":
                    seen["cut"] += int((idx < snap[7][(head + idx.astype(np.int64)) % cap]).sum())
                else:
                    hit = want["o"] != 0
                    assert (snap[6][want["g"][hit]] == 0).all()      # final: the goal row is an episode's last
        assert (seen["hit"] > 0) == (k > 0), seen
        if strategy == "episode" and k > 0:
            assert seen["back"] > 0 and seen["fwd"] > 0, seen
            if mode == "given":
                assert (seen["cut"] > 0) == (ring == "wrapped_oldest_cut"), seen
        if strategy == "final":
            assert seen["back"] == 0


@pytest.mark.parametrize("ring", list(RINGS))
@pytest.mark.parametrize("dims", [REACH, PICK], ids=["reach", "pickplace"])
@pytest.mark.parametrize("strategy", ["final", "episode"])
def test_gathers_bitwise_the_restatement(gcrl, strategy, dims, ring):
    _run_gathers(gcrl, strategy, dims, ring, 1, 4, dense=dims is PICK, gamma=0.0)


_COMBOS = [(REACH, False, 0.98, 4), (PICK, True, 0.5, 4), (REACH, True, 0.98, 1), (PICK, False, 0.5, 0)]    # (dims, dense, gamma, k)
NSTEP_CASES = [(s, N, ring) + _COMBOS[i % 4] for i, (s, N, ring) in enumerate((s, N, ring) for s in ("final", "episode") for N in (2, 3, 8) for ring in RINGS)]


@pytest.mark.parametrize("strategy,N,ring,dims,dense,gamma,k", NSTEP_CASES,
                         ids=[f"{c[0]}-n{c[1]}-{c[2]}-S{c[3][0]}-{'dense' if c[4] else 'sparse'}-g{c[5]}-k{c[6]}" for c in NSTEP_CASES])
def test_nstep_gathers_bitwise_the_restatement(gcrl, strategy, N, ring, dims, dense, gamma, k):
    _run_gathers(gcrl, strategy, dims, ring, N, k, dense, gamma)


TIGHT = (4, 4, 1)     # RW + G + 1 = 16: a `final` ring's record ends with `remaining`, no pad behind it (an `episode` ring's has 32 floats)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("strategy", ["final", "episode"])
def test_gathers_on_a_record_without_pad(gcrl, strategy, N):
    """the first round of loads stops at the record's end, the ring's last slot included"""
    buf = _buffer(gcrl, 114, TIGHT, strategy)
    _fill(buf, TIGHT, [50], 40)
    from gcrl_amd._ffi import lib
    before = lib.gcrl_her_state_size(buf.handle)
    _fill(buf, TIGHT, [13], 41)                                      # 13 more records in the blob: the record width
    assert (lib.gcrl_her_state_size(buf.handle) - before) // (13 * 4) == (16 if strategy == "final" else 32)
    _run_gathers(gcrl, strategy, TIGHT, "wrapped", N, 4, dense=False, gamma=0.98)


# ---------------------------------------------------------------- 4. future is the keyword left out
def test_future_is_the_keyword_left_out(gcrl, tmp_path):
    from gcrl_amd._ffi import lib
    a, b = _buffer(gcrl, 120, PICK, None, seed=3), _buffer(gcrl, 120, PICK, "future", seed=3)
    for buf in (a, b):
        _fill(buf, PICK, RINGS["wrapped_oldest_cut"][1], 40)
    assert lib.gcrl_her_state_size(a.handle) == lib.gcrl_her_state_size(b.handle)       # the record width
    for n in (17, 67):
        for x, y in zip(a.sample(n, 1), b.sample(n, 1)):
            assert np.array_equal(bits(_np(x)), bits(_np(y))), n
        side = torch.arange(48, dtype=torch.uint8, device="cuda")
        for x, y in zip(a.gather_update(n, spa=True, side=side), b.gather_update(n, spa=True, side=side)):
            assert np.array_equal(_np(x).view(np.uint8), _np(y).view(np.uint8)), n
    assert a.relabel_counter == b.relabel_counter == 2 * (17 + 67)
    ma, mb = a.save_state(str(tmp_path / "a.bin")), b.save_state(str(tmp_path / "b.bin"))
    assert ma["goal_strategy"] == mb["goal_strategy"] == "future"
    blob_a, blob_b = (tmp_path / "a.bin").read_bytes(), (tmp_path / "b.bin").read_bytes()
    assert blob_a == blob_b and int.from_bytes(blob_a[4:8], "little") == 2               # the blob version of before
    c = _buffer(gcrl, 120, PICK, None, seed=3, n_step=3, gamma=0.98)
    d = _buffer(gcrl, 120, PICK, "future", seed=3, n_step=3, gamma=0.98)
    for buf in (c, d):
        _fill(buf, PICK, RINGS["wrapped_oldest_cut"][1], 40)
    for x, y in zip(c.sample(67, 1) + c.gather_update(33), d.sample(67, 1) + d.gather_update(33)):
        if x is not None:
            assert np.array_equal(bits(_np(x)), bits(_np(y)))


# ---------------------------------------------------------------- 5. agents
KINDS = {"DDPG": {}, "TD3": dict(ac_update_freq=2, policy_noise=0.2, noise_clamp=0.5), "SAC": dict(ac_update_freq=2), "TQC": dict(ac_update_freq=2)}


def _agent(gcrl, kind, seed, **kw):
    cfg = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150, k_future=4, **KINDS[kind])
    cls = {"DDPG": gcrl.DDPG, "TD3": gcrl.TD3Agent, "SAC": gcrl.SACAgent, "TQC": gcrl.TQCAgent}[kind]
    return cls(REACH[0], REACH[1], cfg, None, nenvs=2, gradient_step=6, rng="engine", seed=seed, relabel="sample", **kw)


def _three_calls(x):
    """three update calls, one of them update_many: steps 1 .. 6"""
    return [x.update(1), x.update(2)] + x.update_many(3, 4)


@pytest.mark.parametrize("kind", ["TD3", "SAC", "TQC"])
def test_engine_equals_twin_fed_the_restated_batches(gcrl, kind):
    B, seed, N = 64, 31, 3
    ag, twin = (_agent(gcrl, kind, seed, goal_strategy="episode", n_step=N) for _ in range(2))
    T._fill_agent(ag, 50)                                       # 200 rows through a ring of 150: wrapped, the oldest episode whole
    for x in (ag, twin):
        T._perturb(x, 0)
    assert ag.goal_strategy == ag.buffer.goal_strategy == "episode" and len(ag.buffer) == 150 and T._head(ag.buffer) == 50
    snap = _snapshot(ag.buffer)
    thr = ag.buffer._reward_cfg[1]
    py = random.Random(seed)
    want, back = [], 0
    for step in range(1, 7):
        idx = her_oracle.sample_indices(py, 150, B)
        b = GS.gather(*snap[:8], snap[8], 150, idx, (step - 1) * B, seed, 4, R.SPARSE, thr, "episode", N, ag.config.gamma)
        back += int((b["o"] < 0).sum())
        batch = tuple(torch.from_numpy(x).cuda() for x in (b["s"], b["a"], b["r"].reshape(-1, 1), b["ns"], b["d"].reshape(-1, 1)))
        want.append(twin.update(step, batch=batch))
    got = _three_calls(ag)
    assert back > 0 and ag.buffer.relabel_counter == 6 * B
    g, w = T._tuples(got), T._tuples(want)
    assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (g, w)
    assert np.array_equal(T._state(ag), T._state(twin)), "engine state differs from the twin fed the restated batches"


@pytest.mark.parametrize("kw", [dict(goal_strategy="episode", n_step=3), dict(goal_strategy="final", prioritise="energy")], ids=["episode_n3", "final_energy"])
def test_ddpg_row_chain_three_calls_equal_six_updates(gcrl, kw):
    """the default DDPG path: a call's head gather and its main gather select goals by the ring's strategy and continue one counter"""
    other = dict(kw, goal_strategy="future")
    one, calls, plain = _agent(gcrl, "DDPG", 33, **kw), _agent(gcrl, "DDPG", 33, **kw), _agent(gcrl, "DDPG", 33, **other)
    for x in (one, calls, plain):
        T._fill_agent(x, 51)
        T._perturb(x, 1)
    a = T._tuples([one.update(s) for s in range(1, 7)])
    b = T._tuples(_three_calls(calls))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (a, b)
    assert np.array_equal(T._state(one), T._state(calls))
    assert one.buffer.relabel_counter == calls.buffer.relabel_counter == 6 * 64
    c = T._tuples(_three_calls(plain))                           # the strategy matters: a `future` ring learns from other goals
    assert plain.buffer.relabel_counter == 6 * 64
    assert not np.array_equal(b.view(np.uint64), c.view(np.uint64))
    # the batches the engine saw are the ring's own gathers: the next one, drawn by the same stream, is the restatement's
    if "prioritise" not in kw:
        snap = _snapshot(one.buffer)
        idx = np.arange(64, dtype=np.uint32)
        want = GS.gather(*snap[:8], snap[8], 150, idx, 6 * 64, 33, 4, R.SPARSE, one.buffer._reward_cfg[1], kw["goal_strategy"], 3, one.config.gamma)
        out = one.buffer.gather_update(64, indices=idx)
        sa, nsa, _ = T._engine_form(want, REACH)
        assert np.array_equal(bits(_np(out[0])), bits(sa)) and np.array_equal(bits(_np(out[1])), bits(nsa))
        assert np.array_equal(bits(_np(out[3])), bits(want["r"])) and np.array_equal(bits(_np(out[4])), bits(want["d"]))


# ---------------------------------------------------------------- 6. populations
def _pop_cfgs():
    return [make_config("DDPG", hidden_dim=64, layer_count=3, batch_size=64, max_len=150, k_future=4, actor_lr=1e-3 * (1 + 0.25 * i),
                        gamma=0.98 - 0.08 * i, tau=0.05 + 0.01 * i) for i in range(2)]


@pytest.mark.parametrize("shared", [False, True], ids=["own_rings", "shared_ring"])
def test_population_members_are_standalone_agents(gcrl, shared):
    cfgs, seeds, N = _pop_cfgs(), [61, 62], 3
    D = REACH[0]
    kw = dict(relabel="sample", n_step=N, goal_strategy="episode")
    pop = gcrl.DDPGPopulation(D, REACH[1], cfgs, 2, 6, rng="engine", seeds=seeds, shared_ring=shared, **kw)
    solo = [gcrl.DDPG(D, REACH[1], c, None, nenvs=2, gradient_step=6, rng="engine", seed=s, **kw) for c, s in zip(cfgs, seeds)]
    assert pop.goal_strategy == "episode" and all(m.buffer.goal_strategy == "episode" for m in pop.members)
    if shared:
        assert all(m.buffer is pop.buffer for m in pop.members)
        ring = gcrl.HERBuffer(cfgs[0].max_len, cfgs[0].max_eps_len, 4, k_future=4, rng="engine", seed=seeds[0], relabel="sample", n_step=N,
                              gamma=cfgs[0].gamma, goal_strategy="episode")
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
    calls = [(1, 0), (2, 6)]
    for s0, n in calls:
        got = T._run(pop, s0, n)
        want = [T._run(a, s0, n) for a in solo]                  # (a shared ring: the standalone agents in member order)
        for i in range(2):
            g_, w_ = T._tuples([got[i]] if n == 0 else got[i]), T._tuples([want[i]] if n == 0 else want[i])
            assert np.array_equal(g_.view(np.uint64), w_.view(np.uint64)), (i, s0, n)
    for i, a in enumerate(solo):
        assert np.array_equal(T._state(pop.members[i]), T._state(a)), i
    rows = 7 * 64
    if shared:
        assert pop.buffer.relabel_counter == solo[0].buffer.relabel_counter == 2 * rows
    else:
        assert all(pop.members[i].buffer.relabel_counter == solo[i].buffer.relabel_counter == rows for i in range(2))
    assert pop.gather_counts()[1] == 0, pop.gather_counts()     # sample-mode gathers stay member by member


def test_exploit_between_differing_strategies_is_refused(gcrl):
    from gcrl_amd._ffi import GcrlError
    cfgs = _pop_cfgs()
    pop = gcrl.DDPGPopulation(REACH[0], REACH[1], cfgs, 2, 6, rng="engine", seeds=[5, 6], relabel="sample", goal_strategy="episode")
    pop.members[1].buffer = gcrl.HERBuffer(cfgs[1].max_len, cfgs[1].max_eps_len, 2, k_future=4, rng="engine", seed=6, relabel="sample",
                                           goal_strategy="final")
    for m in pop.members:
        T._fill_agent(m, 70, episodes=1)
    with pytest.raises(GcrlError, match="goal_strategy"):
        pop.exploit([(0, 1)], copy_ring=True)
    pop.members[1].buffer.goal_strategy = "episode"             # past the Python check: the engine's own refusal
    with pytest.raises(GcrlError, match="gcrl_pop_clone: goal_strategy"):
        pop.exploit([(0, 1)], copy_ring=True)
    pop.members[1].buffer.goal_strategy = "final"
    pop.exploit([(0, 1)])                                        # without the ring: nothing to refuse


# ---------------------------------------------------------------- 7. state
def test_save_load_resume_bitwise(gcrl, tmp_path):
    a = _buffer(gcrl, 120, REACH, "episode", seed=9, n_step=3, gamma=0.98)
    _fill(a, REACH, RINGS["wrapped_oldest_cut"][1], 42)
    a.sample(17, 2)
    assert a.relabel_counter == 34 and T._head(a) == 44
    path = str(tmp_path / "ring.bin")
    meta = a.save_state(path)
    assert meta["goal_strategy"] == "episode" and int.from_bytes(open(path, "rb").read()[4:8], "little") == 3
    b = _buffer(gcrl, 120, REACH, "episode", seed=9, n_step=3, gamma=0.98)
    b.load_state(path, meta)
    assert b.relabel_counter == 34 and len(b) == 120 and T._head(b) == 0         # re-laid at head 0: the logical order is what counts
    assert np.array_equal(a.elapsed(), b.elapsed())
    gen = np.random.default_rng(43)
    for rnd in range(2):
        for n in (16, 17, 33):
            ga, gb = a.sample(n, 1, return_indices=True), b.sample(n, 1, return_indices=True)
            assert np.array_equal(ga[5], gb[5])
            for x, y in zip(ga[:5], gb[:5]):
                assert np.array_equal(bits(_np(x)), bits(_np(y))), (rnd, n)
            for x, y in zip(a.gather_update(n), b.gather_update(n)):
                if x is not None:
                    assert np.array_equal(bits(_np(x)), bits(_np(y))), (rnd, n)
        ep = T._episode(gen, 13, REACH, True)                    # the next flush: the two rings' heads differ, their logical rows do not
        for buf in (a, b):
            buf.push_episode(0, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
        for x, y in zip(a.rows() + a.tails() + (a.elapsed(),), b.rows() + b.tails() + (b.elapsed(),)):
            assert np.array_equal(bits(x), bits(y))
    assert a.relabel_counter == b.relabel_counter
    from gcrl_amd._ffi import GcrlError
    for other in ("future", "final"):
        c = _buffer(gcrl, 120, REACH, other, seed=9, n_step=3, gamma=0.98)
        with pytest.raises(GcrlError, match="goal_strategy"):
            c.load_state(path, meta)
        assert c.handle is None                                  # refused before any device work
        with pytest.raises(GcrlError, match="gcrl_her_load_state: goal_strategy"):
            c.load_state(path, dict(meta, goal_strategy=other))  # the blob itself carries the strategy
    f = _buffer(gcrl, 120, REACH, "final", seed=9)
    _fill(f, REACH, [50], 42)
    mf = f.save_state(str(tmp_path / "final.bin"))
    with pytest.raises(GcrlError, match="gcrl_her_load_state: goal_strategy"):
        _buffer(gcrl, 120, REACH, None, seed=9).load_state(str(tmp_path / "final.bin"), dict(mf, goal_strategy="future"))


def test_native_create_refusals_name_goal_strategy(gcrl):
    import ctypes as C
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import lib
    cfg = _ffi.HerConfig(state_dim=10, action_dim=3, goal_dim=3, capacity=100, nenvs=2, k_future=4, flush_len=50, reward_kind=0,
                         reward_threshold=0.05, device=0, rng_mode=0, seed=1)
    for mode, strategy in ((1, 3), (1, -1), (0, 1), (0, 2)):
        assert not lib.gcrl_her_create_goal(C.byref(cfg), None, mode, strategy)
        assert b"goal_strategy" in lib.gcrl_last_error(), (mode, strategy)
    h = lib.gcrl_her_create_goal(C.byref(cfg), None, 0, 0)
    assert h and lib.gcrl_her_goal_strategy(h) == 0 and lib.gcrl_her_relabel_mode(h) == 0
    lib.gcrl_her_destroy(h)
