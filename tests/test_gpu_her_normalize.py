"""GPU (-m gpu): sample-time normalisation of a HER ring (HERBuffer(normalize="sample"); csrc/her_norm.hip).  The in-place pass is held
bit for bit to the existing entry gcrl_normalizer_normalize at the edges of its tiling, the gathers of every family and form to the
numpy definition tests/her_normalize_ref.py, an agent on a raw ring to a twin fed pre-normalised rows while the statistics stand
still, the raw-store process_step to the existing one's statistics, populations to standalone agents; drift, the reward in metres,
resume in a fresh process and the native refusals.  Helpers and shapes are those of tests/test_gpu_her_relabel.py."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import make_config
from oracle.normalizer_oracle import RunningNormalizerOracle

import her_normalize_ref as NR
import her_relabel_ref as R
import test_gpu_her_relabel as T
import test_gpu_her_strategy as TS
from test_gpu_her_relabel import PICK, REACH, THR, _np, bits

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIMES = ("created", "loaded", "rows64")          # float64 statistics; float32 statistics (after load); float64 rows


def _pair(size, regime="created", seed=0, clip=5.0, zero=None):
    """a device normaliser and its oracle twin holding the same statistics"""
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    gen = np.random.default_rng(seed)
    mean, var = gen.standard_normal(size) * 0.3, gen.uniform(0.02, 1.5, size)
    if zero is not None:
        var[zero], mean[zero] = 0.0, float(F32(mean[zero]))             # (a float32 row can sit exactly at this mean)
    if regime == "loaded":
        mean, var = mean.astype(F32), var.astype(F32)
    z = DeviceRunningNormalizer(size, clip_range=clip)
    z.set_state(mean, var, 100.0, clip, float32=regime == "loaded")
    z.rows_dtype(np.float64 if regime == "rows64" else np.float32)
    o = RunningNormalizerOracle(size, clip)
    o.mean, o.var, o.count = mean.copy(), var.copy(), 100.0
    return z, o


def _twin_of(z):
    """an oracle holding what the device normaliser holds now"""
    o = RunningNormalizerOracle(z.size, z.clip_range)
    o.mean, o.var, o.count = z.mean, z.var, z.count
    return o


# ---------------------------------------------------------------- 1. the pass against gcrl_normalizer_normalize
SHAPES = {"reach": (7, 3, 3), "pickplace": (20, 3, 4), "aligned": (9, 3, 4), "widest": (128, 8, 4)}     # (D, G, A): S and S + A not / both multiples of 4
NS = (1, 15, 64, 65, 200)                                               # 200 = 3 workgroups of 64 rows and a partial one


def _existing(z, x, regime):
    """gcrl_normalizer_normalize of float32-valued rows, rounded to float32 as the entry returns them"""
    return np.asarray(z.normalize(x.astype(np.float64 if regime == "rows64" else F32)), F32)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pass_equals_the_existing_entry_bitwise(gcrl, shape, regime):
    from gcrl_amd._ffi import check, lib
    D, G, A = SHAPES[shape]
    S = D + G
    ldx = (S + A + 3) // 4 * 4
    gen = np.random.default_rng(D)
    zo, _ = _pair(D, regime, 1, zero=D // 2)
    zg, _ = _pair(G, regime, 2, clip=2.0, zero=0)
    for n in NS:
        for flags in ((True, False), (True, True), (False, True)):
            for with_spa in (False, True):
                for quad in (True, False):                              # the 16-byte kernel; the element kernel (odd stride, as sample()'s outputs)
                    ld = ldx if quad else S + 1
                    host = [(gen.standard_normal((n, ld)) * 4).astype(F32) for _ in range(3 if with_spa else 2)]     # beyond +-clip too
                    host[0][0, D // 2] = zo.mean[D // 2]                # a value AT the mean of the var = 0 column: exactly 0
                    for h in host:                                      # padding / action columns: patterns no arithmetic would keep
                        h[:, S:] = np.array([np.nan, -0.0, 1e-42, np.inf], F32)[np.arange(ld - S) % 4]
                    dev = [torch.from_numpy(h).cuda() for h in host]
                    assert all(d.data_ptr() % 16 == 0 for d in dev)
                    ptr = [d.data_ptr() for d in dev] + [None] * (3 - len(dev))
                    check(lib.gcrl_normalizer_normalize_states(zo.handle if flags[0] else None, zg.handle if flags[1] else None, D, S, n,
                                                               ptr[0], ld, ptr[1], ld, ptr[2], ld, None))
                    torch.cuda.synchronize()
                    for h, d in zip(host, dev):
                        want = h.copy()
                        if flags[0]:
                            want[:, :D] = _existing(zo, h[:, :D], regime)
                        if flags[1]:
                            want[:, D:S] = _existing(zg, h[:, D:S], regime)
                        assert np.array_equal(bits(_np(d)), bits(want)), (n, flags, with_spa, quad)
                    if flags == (True, True):
                        assert (np.abs(_np(dev[0])[:, D:S]) <= 2.0).all() and (n < 64 or (np.abs(_np(dev[0])[:, :D]) == 5.0).any())
                        assert _np(dev[0])[0, D // 2] == 0.0


# ---------------------------------------------------------------- 2. every gather family and both forms against the definition
def _buffer(gcrl, cap, dims, seed=7, relabel="sample", nenvs=2, flags=(True, True), regime="created", dense=False, **kw):
    buf = gcrl.HERBuffer(cap, 50, nenvs, threshold=THR, k_future=4, rng="engine", seed=seed, relabel=relabel, normalize="sample",
                         obs_normalize=flags[0], g_normalize=flags[1], **kw)
    buf.compute_reward = her_oracle.dense_reward if dense else her_oracle.sparse_reward
    S, _, G = dims
    zo, oo = _pair(S - G, regime, 11)
    zg, og = _pair(G, regime, 12, clip=3.0)
    buf.obs_normalizer, buf.dg_normalizer = zo, zg
    return buf, (oo if flags[0] else None), (og if flags[1] else None)


def _fill(buf, dims, lengths, seed):
    gen = np.random.default_rng(seed)
    for e, n in enumerate(lengths):
        ep = T._episode(gen, n, dims, n != 50)
        buf.push_episode(e % 2, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])


FAMILIES = [("future", 1, None), ("future", 3, None), ("final", 1, None), ("episode", 3, None), ("episode", 1, None), ("final", 3, None),
            ("future", 1, "energy"), ("episode", 3, "energy")]


@pytest.mark.parametrize("strategy,N,prio", FAMILIES, ids=[f"{s}-n{n}-{p or 'uniform'}" for s, n, p in FAMILIES])
@pytest.mark.parametrize("dims", [REACH, PICK], ids=["reach", "pickplace"])
def test_gathers_bitwise_the_definition(gcrl, dims, strategy, N, prio):
    cap, seed, gamma = 60, 3100 + N, 0.98
    kw = dict(goal_strategy=strategy)
    if N > 1:
        kw.update(n_step=N, gamma=gamma)
    if prio:
        kw.update(prioritise=prio)
    regime = REGIMES[(N + len(strategy)) % 3]
    flags = [(True, True), (True, False), (False, True)][(N + dims[0]) % 3]
    buf, oo, og = _buffer(gcrl, cap, dims, seed=seed, flags=flags, regime=regime, dense=dims is PICK, **kw)
    _fill(buf, dims, [50, 13, 50], 40)                                  # 113 rows through 60 slots: wrapped, head 53
    assert len(buf) == cap and T._head(buf) == 53
    from gcrl_amd._ffi import lib
    assert lib.gcrl_her_normalize_mode(buf.handle) == 1
    snap = TS._snapshot(buf)
    D, kind = dims[0] - dims[2], (R.DENSE if dims is PICK else R.SPARSE)
    r64 = regime == "rows64"
    gen = np.random.default_rng(5)
    ctr = 0
    for n in (1, 17, 67):
        for form in ("public", "engine", "engine_head"):
            B, M = (n, 1) if n <= cap else (1, n)
            if prio:                                                    # the tree draws: the same rows again from the same counter
                c0 = buf.prio_counter
                idx = buf.sample(B, M, return_indices=True)[5]
                buf.prio_counter, buf.relabel_counter, arg = c0, ctr, None
            else:
                idx = arg = gen.integers(0, cap, n).astype(np.uint32)
            want = NR.gather(*snap[:8], snap[8], cap, idx, ctr, seed, 4, kind, THR, D, oo, og, r64, r64, strategy=strategy, n_step=N, gamma=gamma)
            if form == "public":
                out = buf.sample(B, M, indices=arg)
                got = dict(s=_np(out[0]), a=_np(out[1]), r=_np(out[2]).ravel(), ns=_np(out[3]), d=_np(out[4]).ravel())
                for key in ("s", "a", "r", "ns", "d"):
                    assert np.array_equal(bits(got[key]), bits(want[key])), (n, form, key)
            else:
                side = torch.arange(48, dtype=torch.uint8, device="cuda") if form == "engine_head" else None
                out = buf.gather_update(B, M, indices=arg, spa=True, side=side)
                sa, nsa, spa = NR.engine_matrices(want, dims[1], spa=True)
                assert np.array_equal(bits(_np(out[0])), bits(sa)), (n, form, "sa")
                assert np.array_equal(bits(_np(out[1])), bits(nsa)), (n, form, "nsa")
                assert np.array_equal(bits(_np(out[2])), bits(spa)), (n, form, "spa")             # NaN where the gather writes nothing
                assert np.array_equal(bits(_np(out[3])), bits(want["r"])) and np.array_equal(bits(_np(out[4])), bits(want["d"])), (n, form)
                if side is not None:
                    assert torch.equal(out[5], side)
            ctr += n
            assert buf.relabel_counter == ctr
            assert (want["o"] != 0).any() or n == 1
            assert not np.array_equal(bits(want["s"]), bits(want["raw_s"]))


def test_push_mode_ring_gathers_normalised_rows(gcrl):
    """relabel="push": the flush relabels raw rows (rewards of raw achieved goals), her_gather_update_kernel's batch is normalised"""
    buf, oo, og = _buffer(gcrl, 300, REACH, relabel="push", flags=(True, False))
    plain = gcrl.HERBuffer(300, 50, 2, threshold=THR, k_future=4, rng="engine", seed=7)
    plain.compute_reward = her_oracle.sparse_reward
    for b in (buf, plain):
        _fill(b, REACH, [50, 50], 40)
    s, a, ns, r, d = buf.rows()
    for x, y in zip(buf.rows(), plain.rows()):
        assert np.array_equal(bits(x), bits(y))                         # stored as given: raw
    idx = np.random.default_rng(6).integers(0, len(buf), 67).astype(np.uint32)
    want = dict(s=NR.normalize_states(s[idx], 7, oo, og), a=a[idx], ns=NR.normalize_states(ns[idx], 7, oo, og), r=r[idx], d=d[idx])
    out = buf.gather_update(67, indices=idx, spa=True)
    for k, key in enumerate(("s", "ns", "s")):                          # (what this gather leaves behind ns and s in nsa / spa is not defined: the
        assert np.array_equal(bits(_np(out[k])[:, :10]), bits(want[key])), k    #  pass keeps such columns' bits, test_pass_equals_the_existing_entry_bitwise)
    assert np.array_equal(bits(_np(out[0])[:, 10:13]), bits(a[idx])) and not _np(out[0])[:, 13:].any()
    assert np.array_equal(bits(_np(out[3])), bits(r[idx])) and np.array_equal(bits(_np(out[4])), bits(d[idx]))
    out = buf.sample(67, indices=idx)
    assert np.array_equal(bits(_np(out[0])), bits(want["s"])) and np.array_equal(bits(_np(out[3])), bits(want["ns"]))
    assert np.array_equal(bits(_np(out[1])), bits(a[idx]))


# ---------------------------------------------------------------- 3. frozen statistics: a raw ring equals a ring of pre-normalised rows
KINDS = TS.KINDS


def _agent(gcrl, kind, seed, relabel="sample", normalize="sample", **kw):
    cfg = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150, k_future=4, **KINDS[kind])
    cls = {"DDPG": gcrl.DDPG, "TD3": gcrl.TD3Agent, "SAC": gcrl.SACAgent, "TQC": gcrl.TQCAgent}[kind]
    return cls(REACH[0], REACH[1], cfg, None, nenvs=2, gradient_step=6, rng="engine", seed=seed, relabel=relabel, normalize=normalize, **kw)


def _fill_agent(ag, seed, z=None, episodes=4):
    """four episodes pushed raw — or, given `z`, with their observation columns normalised by it beforehand"""
    gen = np.random.default_rng(seed)
    for ep in range(episodes):
        for s, a, ns, r, d, dg, g in her_oracle.synthetic_episode(gen, 50, REACH[0], REACH[1]):
            if z is not None:
                s, ns = s.copy(), ns.copy()
                s[:7], ns[:7] = np.asarray(z.normalize(s[:7]), F32), np.asarray(z.normalize(ns[:7]), F32)
            ag.push_her(ep % 2, s, a, ns, r, d, dg, g)


@pytest.mark.parametrize("kind,relabel", [("DDPG", "sample"), ("SAC", "sample"), ("DDPG", "push")])
def test_frozen_statistics_equal_a_twin_fed_prenormalised_rows(gcrl, kind, relabel):
    raw, pre = _agent(gcrl, kind, 33, relabel), _agent(gcrl, kind, 33, relabel, normalize="push")
    z, _ = _pair(7, "created", 21)
    z2, _ = _pair(7, "created", 21)
    raw.buffer.obs_normalizer = z
    _fill_agent(raw, 51)
    _fill_agent(pre, 51, z2)
    for x in (raw, pre):
        T._perturb(x, 1)
    assert raw.buffer.normalize == "sample" and pre.buffer.normalize == "push" and len(raw.buffer) == len(pre.buffer)
    assert not np.array_equal(bits(raw.buffer.rows()[0]), bits(pre.buffer.rows()[0]))
    a, b = T._tuples(TS._three_calls(raw)), T._tuples(TS._three_calls(pre))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (a, b)
    assert np.array_equal(T._state(raw), T._state(pre)), "weights differ"
    if relabel == "sample":
        assert raw.buffer.relabel_counter == pre.buffer.relabel_counter == 6 * 64


# ---------------------------------------------------------------- 4. + 6. the raw-store process_step, and drift
def _steps(gen, n, D, G, A, count, t0=0):
    """`count` vector-env steps of n envs as the trainer hands them over: float64 observations, float32 goals"""
    out = []
    obs, ag = gen.standard_normal((n, D)), gen.uniform(-0.15, 0.15, (n, G)).astype(F32)
    dg = gen.uniform(-0.15, 0.15, (n, G)).astype(F32)
    for t in range(count):
        nobs, nag = gen.standard_normal((n, D)).astype(F32).astype(np.float64), (ag + gen.normal(0, 0.02, (n, G))).astype(F32)
        obs = obs.astype(F32).astype(np.float64)
        st = dict(observation=obs, desired_goal=dg, achieved_goal=ag)
        nx = dict(observation=nobs, desired_goal=dg, achieved_goal=nag)
        act = gen.uniform(-1, 1, (n, A)).astype(F32)
        rew = np.array([her_oracle.sparse_reward(nag[i], dg[i]) for i in range(n)], np.float64)
        out.append((st, act, nx, rew, np.zeros(n, bool)))
        obs, ag = nobs, nag
    return out


def _stats(z):
    return np.concatenate([z.mean.astype(np.float64), z.var.astype(np.float64), [z.count]]).view(np.uint64)


def _with_device_normalisers(ag):
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    ag.buffer.obs_normalizer, ag.buffer.dg_normalizer = DeviceRunningNormalizer(7), DeviceRunningNormalizer(3)
    ag.buffer.compute_reward = her_oracle.sparse_reward
    return ag


def _agent_n(gcrl, nenvs, normalize, gn, relabel="sample"):
    cfg = make_config("DDPG", hidden_dim=64, layer_count=3, batch_size=64, max_len=4000, k_future=4)
    return _with_device_normalisers(gcrl.DDPG(REACH[0], REACH[1], cfg, None, nenvs=nenvs, gradient_step=6, rng="engine", seed=5, relabel=relabel,
                                              normalize=normalize, g_normalize=gn))


@pytest.mark.parametrize("gn", [False, True], ids=["obs", "obs_goal"])
@pytest.mark.parametrize("nenvs", [2, 32], ids=["inline", "staged"])        # 104 floats inside the kernel arguments; 1 664 through the pinned slot
def test_raw_store_process_step(gcrl, nenvs, gn):
    a, b = _agent_n(gcrl, nenvs, "push", gn), _agent_n(gcrl, nenvs, "sample", gn)
    steps = _steps(np.random.default_rng(9), nenvs, 7, 3, 3, 50)
    for i, (st, act, nx, rew, dn) in enumerate(steps):
        ra, rb = a.process_step(st, act, nx, rew, dn, g_normalize=gn), b.process_step(st, act, nx, rew, dn, g_normalize=gn)
        assert ra == rb == (50 * nenvs if i == 49 else 0)
        if i in (0, 1, 49):
            assert np.array_equal(_stats(a.buffer.obs_normalizer), _stats(b.buffer.obs_normalizer)), i
            assert np.array_equal(_stats(a.buffer.dg_normalizer), _stats(b.buffer.dg_normalizer)), i
    assert (a.buffer.dg_normalizer.count > 1) == gn
    s, ac, ns, r, d = b.buffer.rows()
    ag_tail, rem = b.buffer.tails()
    for e in range(nenvs):                                              # the flush appends env after env, 50 rows each, as they came
        rows = slice(50 * e, 50 * e + 50)
        want_s = np.stack([np.concatenate([st["observation"][e], st["desired_goal"][e]]).astype(F32) for st, *_ in steps])
        want_ns = np.stack([np.concatenate([nx["observation"][e], nx["desired_goal"][e]]).astype(F32) for _, _, nx, *_ in steps])
        assert np.array_equal(bits(s[rows]), bits(want_s)) and np.array_equal(bits(ns[rows]), bits(want_ns)), e
        assert np.array_equal(bits(ac[rows]), bits(np.stack([x[1][e] for x in steps]))) and np.array_equal(r[rows], np.array([x[3][e] for x in steps], F32))
        assert np.array_equal(bits(ag_tail[rows]), bits(np.stack([x[2]["achieved_goal"][e] for x in steps]))) and rem[rows][0] == 49
    assert not np.array_equal(bits(a.buffer.rows()[0]), bits(s))        # the existing form stored them normalised


def test_raw_store_process_step_population(gcrl):
    cfgs = [make_config("DDPG", hidden_dim=64, layer_count=3, batch_size=64, max_len=400, k_future=4) for _ in range(2)]
    pops = [gcrl.DDPGPopulation(REACH[0], REACH[1], cfgs, 2, 6, rng="engine", seeds=[5, 6], relabel="sample", normalize=nm, g_normalize=True)
            for nm in ("push", "sample")]
    for p in pops:
        p.MERGE_ACTING_FROM = 2                                         # (the class default sends fewer than 4 DDPG members one by one)
        for m in p.members:
            _with_device_normalisers(m)
    gen = np.random.default_rng(10)
    per = [_steps(gen, 2, 7, 3, 3, 50) for _ in range(2)]
    for i in range(50):
        args = [[per[m][i][k] for m in range(2)] for k in range(5)]
        got = [p.process_step(*args, g_normalize=True) for p in pops]
        assert got[0] == got[1]
    assert pops[1].acting_counts()[2:4] == pops[0].acting_counts()[2:4] == (50, 50)      # one launch per call, as without the keyword
    for m in range(2):
        x, y = pops[0].members[m].buffer, pops[1].members[m].buffer
        assert np.array_equal(_stats(x.obs_normalizer), _stats(y.obs_normalizer)) and np.array_equal(_stats(x.dg_normalizer), _stats(y.dg_normalizer))
        s, ac, ns, r, d = y.rows()
        want_s = np.stack([np.concatenate([per[m][i][0]["observation"][0], per[m][i][0]["desired_goal"][0]]).astype(F32) for i in range(50)])
        assert np.array_equal(bits(s[:50]), bits(want_s)) and len(y) == 100
        assert np.array_equal(bits(y.tails()[0][:50]), bits(np.stack([per[m][i][2]["achieved_goal"][0] for i in range(50)])))


@pytest.mark.parametrize("relabel", ["sample", "push"])
def test_drift_a_later_gather_uses_the_later_statistics(gcrl, relabel):
    ag = _agent_n(gcrl, 2, "sample", True, relabel)
    steps = _steps(np.random.default_rng(12), 2, 7, 3, 3, 60)
    for st, act, nx, rew, dn in steps[:50]:
        ag.process_step(st, act, nx, rew, dn, g_normalize=True)
    buf = ag.buffer
    rows0 = buf.rows() + (buf.tails() if relabel == "sample" else ())
    idx = np.random.default_rng(13).integers(0, len(buf), 67).astype(np.uint32)

    def expect():
        oo, og = _twin_of(buf.obs_normalizer), _twin_of(buf.dg_normalizer)
        if relabel == "sample":
            snap = TS._snapshot(buf)
            return NR.gather(*snap[:8], snap[8], buf.max_mem_len, idx, 0, 5, 4, R.SPARSE, buf._reward_cfg[1], 7, oo, og, True, False)
        s, a, ns, r, d = buf.rows()
        return dict(s=NR.normalize_states(s[idx], 7, oo, og, True, False), ns=NR.normalize_states(ns[idx], 7, oo, og, True, False), a=a[idx], r=r[idx], d=d[idx])

    def gather():
        if relabel == "sample":
            buf.relabel_counter = 0
        out = buf.sample(67, indices=idx)
        return dict(s=_np(out[0]), a=_np(out[1]), r=_np(out[2]).ravel(), ns=_np(out[3]), d=_np(out[4]).ravel())

    first, want1 = gather(), expect()
    for st, act, nx, rew, dn in steps[50:]:                              # staged only: the statistics move, the ring does not
        assert ag.process_step(st, act, nx, rew, dn, g_normalize=True) == 0
    second, want2 = gather(), expect()
    for key in ("s", "a", "r", "ns", "d"):
        assert np.array_equal(bits(first[key]), bits(want1[key])) and np.array_equal(bits(second[key]), bits(want2[key])), key
    assert not np.array_equal(bits(first["s"]), bits(second["s"])) and np.array_equal(bits(first["r"]), bits(second["r"]))
    for x, y in zip(rows0, buf.rows() + (buf.tails() if relabel == "sample" else ())):
        assert np.array_equal(bits(x), bits(y))                         # stored rows: bitwise unchanged ..
    if relabel == "sample":                                             # .. and raw (a push-mode flush interleaves its relabelled copies)
        assert np.array_equal(bits(rows0[0][:50]), bits(np.stack([np.concatenate([st["observation"][0], st["desired_goal"][0]]).astype(F32)
                                                                  for st, *_ in steps[:50]])))


# ---------------------------------------------------------------- 5. the relabelled reward is decided in metres
@pytest.mark.parametrize("case", ["tight", "wide"])
def test_relabelled_reward_under_g_normalize_is_of_raw_goals(gcrl, case):
    """tight: achieved goals within 0.03 of each other under a goal normaliser of std 0.01 — every relabelled row is a success at the
    threshold 0.05 although its normalised distance is 0.06 .. 3.  wide: goals 0.4 apart under std 10 — every one a failure although
    the normalised distance of neighbours is 0.04."""
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    buf = gcrl.HERBuffer(100, 50, 2, threshold=THR, k_future=4, rng="engine", seed=3, relabel="sample", normalize="sample", g_normalize=True)
    buf.compute_reward = her_oracle.sparse_reward
    std = 0.01 if case == "tight" else 10.0
    zo, zg = DeviceRunningNormalizer(7), DeviceRunningNormalizer(3)
    zg.set_state(np.zeros(3), np.full(3, std * std), 100.0)
    buf.obs_normalizer, buf.dg_normalizer = zo, zg
    gen = np.random.default_rng(4)
    s, a, ns, r, d, dg, ag = T._episode(gen, 50, REACH, False)
    step = 0.0006 if case == "tight" else 0.4
    ag = (np.arange(50, dtype=F32)[:, None] * np.array([step, 0, 0], F32)).astype(F32)
    r[:] = -1.0
    buf.push_episode(0, s, a, ns, r, d, ag)
    idx = np.tile(np.arange(49, dtype=np.uint32), 4)
    out = buf.sample(49, 4, indices=idx)
    snap = TS._snapshot(buf)
    want = NR.gather(*snap[:8], snap[8], 100, idx, 0, 3, 4, R.SPARSE, THR, 7, _twin_of(zo), _twin_of(zg))
    hit = want["o"] != 0
    assert hit.sum() > 100 and np.array_equal(bits(_np(out[2]).ravel()), bits(want["r"]))
    got_r = _np(out[2]).ravel()[hit]
    normalised = np.linalg.norm((ag[want["g"][hit]] - ag[idx[hit]]) / F32(std), axis=1)
    if case == "tight":
        assert (got_r == 0.0).all() and (normalised > THR).all()
    else:
        assert (got_r == -1.0).all() and (normalised <= THR).any()
    assert np.array_equal(bits(_np(out[0])[hit][:, 7:]), bits(NR.apply(_twin_of(zg), ag[want["g"][hit]])))       # the goal columns: normalised


# ---------------------------------------------------------------- 7. populations
@pytest.mark.parametrize("merge", [True, False], ids=["merged", "member_by_member"])
@pytest.mark.parametrize("shared", [False, True], ids=["own_rings", "shared_ring"])
def test_population_members_are_standalone_agents(gcrl, shared, merge):
    cfgs, seeds = TS._pop_cfgs(), [61, 62]
    D, A = REACH[0], REACH[1]
    kw = dict(relabel="push", normalize="sample")

    def build(**k):
        pop = gcrl.DDPGPopulation(D, A, cfgs, 2, 6, rng="engine", seeds=seeds, shared_ring=shared, **k)
        pop.merge_gather = merge
        return pop

    pop, plain = build(**kw), build(relabel="push")
    solo = [gcrl.DDPG(D, A, c, None, nenvs=2, gradient_step=6, rng="engine", seed=s, **kw) for c, s in zip(cfgs, seeds)]
    if shared:
        ring = gcrl.HERBuffer(cfgs[0].max_len, cfgs[0].max_eps_len, 4, k_future=4, rng="engine", seed=seeds[0], relabel="push", normalize="sample")
        for a in solo:
            a.buffer = ring
        for who in (pop.members, solo, plain.members):
            who[0].buffer.obs_normalizer = _pair(7, "created", 40)[0]
            gen = np.random.default_rng(80)
            for ep in range(4):
                for st in her_oracle.synthetic_episode(gen, 50, D, A):
                    who[ep % 2].push_her(ep % 4, *st)
    for i in range(2):
        for x in (pop.members[i], solo[i], plain.members[i]):
            if not shared:
                x.buffer.obs_normalizer = _pair(7, "created", 40 + i)[0]
                T._fill_agent(x, 70 + i)
            T._perturb(x, i)
    for s0, n in [(1, 0), (2, 6)]:
        got, base = T._run(pop, s0, n), T._run(plain, s0, n)
        want = [T._run(a, s0, n) for a in solo]
        for i in range(2):
            g_, w_ = T._tuples([got[i]] if n == 0 else got[i]), T._tuples([want[i]] if n == 0 else want[i])
            assert np.array_equal(g_.view(np.uint64), w_.view(np.uint64)), (i, s0, n)
            b_ = T._tuples([base[i]] if n == 0 else base[i])
            assert not np.array_equal(g_.view(np.uint64), b_.view(np.uint64))            # the keyword matters
    for i, a in enumerate(solo):
        assert np.array_equal(T._state(pop.members[i]), T._state(a)), i
    assert pop.gather_counts() == plain.gather_counts() and (pop.gather_counts()[1] > 0) == merge, pop.gather_counts()


# ---------------------------------------------------------------- 8. state: resumed in a fresh process
CHILD = """
import sys, json, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import gcrl_amd
import test_gpu_her_normalize as me, test_gpu_her_relabel as T
ag = me._agent(gcrl_amd, "DDPG", 33, n_step=3, goal_strategy="episode")
me._with_device_normalisers(ag)
ag.load_state({path!r})
out = T._tuples(ag.update_many(4, 3))
np.save({out!r}, np.concatenate([out.ravel().view(np.uint64), T._state(ag).astype(np.uint64)]))
"""


def test_save_load_resume_in_a_fresh_process(gcrl, tmp_path):
    ag = _with_device_normalisers(_agent(gcrl, "DDPG", 33, n_step=3, goal_strategy="episode"))
    for st, act, nx, rew, dn in _steps(np.random.default_rng(14), 2, 7, 3, 3, 110):
        ag.process_step(st, act, nx, rew, dn)
    T._perturb(ag, 1)
    ag.update_many(1, 3)
    path = str(tmp_path / "state")
    ag.save_state(path)
    meta = json.load(open(os.path.join(path, "meta.json")))["ring"]
    assert meta["normalize"] == "sample" and meta["obs_normalize"] is True and meta["g_normalize"] is False
    assert int.from_bytes(open(os.path.join(path, "ring.bin"), "rb").read()[4:8], "little") == 0x103      # version 3, rows raw
    out = str(tmp_path / "child.npy")
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path, out=out)
    subprocess.run([sys.executable, "-s", "-c", code], check=True, timeout=300)
    mine = T._tuples(ag.update_many(4, 3))
    want = np.concatenate([mine.ravel().view(np.uint64), T._state(ag).astype(np.uint64)])
    assert np.array_equal(np.load(out), want), "the resumed agent went another way"
    from gcrl_amd._ffi import GcrlError
    other = _with_device_normalisers(_agent(gcrl, "DDPG", 33, normalize="push", n_step=3, goal_strategy="episode"))
    with pytest.raises(GcrlError, match="load_state: normalize"):
        other.buffer.load_state(os.path.join(path, "ring.bin"), meta)
    with pytest.raises(GcrlError, match="gcrl_her_load_state: normalize"):
        other.buffer.load_state(os.path.join(path, "ring.bin"), dict(meta, normalize="push"))      # the blob itself says raw
    flags = _with_device_normalisers(_agent(gcrl, "DDPG", 33, n_step=3, goal_strategy="episode", g_normalize=True))
    with pytest.raises(GcrlError, match="normalize.*g_normalize"):
        flags.buffer.load_state(os.path.join(path, "ring.bin"), meta)


# ---------------------------------------------------------------- 9. refusals
def test_python_call_refusals_name_the_flag(gcrl):
    from gcrl_amd._ffi import GcrlError
    from gcrl_amd.src.utils import RunningNormalizer
    ag = _agent(gcrl, "DDPG", 33)
    st, act, nx, rew, dn = _steps(np.random.default_rng(15), 2, 7, 3, 3, 1)[0]
    with pytest.raises(GcrlError, match="process_step: normalize"):
        ag.process_step(st, act, nx, rew, dn)                           # no device normaliser assigned
    with pytest.raises(GcrlError, match="obs_normalizer: normalize"):
        ag.buffer.obs_normalizer = RunningNormalizer(7)
    _with_device_normalisers(ag)
    with pytest.raises(GcrlError, match="process_step: g_normalize"):
        ag.process_step(st, act, nx, rew, dn, g_normalize=True)
    with pytest.raises(GcrlError, match="process_step: obs_normalize"):
        ag.process_step(st, act, nx, rew, dn, obs_normalize=False)
    with pytest.raises(GcrlError, match="observe_act: g_normalize"):
        ag.observe_act(st["observation"], st["desired_goal"], g_normalize=True)
    assert ag.buffer.handle is None                                     # every one before any device work
    assert ag.process_step(st, act, nx, rew, dn) == 0 and np.asarray(ag.observe_act(st["observation"], st["desired_goal"])).shape == (2, 3)
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    with pytest.raises(ValueError, match="gcrl_her_set_normalize: normalize"):
        ag.buffer.obs_normalizer = DeviceRunningNormalizer(8)          # another size than obs_dim: the native refusal, the binding kept
    assert ag.buffer.obs_normalizer.size == 7
    pop = gcrl.DDPGPopulation(REACH[0], REACH[1], TS._pop_cfgs(), 2, 6, rng="engine", seeds=[5, 6], normalize="sample")
    for m in pop.members:
        _with_device_normalisers(m)
    with pytest.raises(GcrlError, match="process_step: g_normalize"):
        pop.process_step([st, st], [act, act], [nx, nx], [rew, rew], [dn, dn], g_normalize=True)
    with pytest.raises(GcrlError, match="observe_act: obs_normalize"):
        pop.observe_act([st["observation"]] * 2, [st["desired_goal"]] * 2, obs_normalize=False)


def test_native_refusals_name_normalize_and_consume_nothing(gcrl):
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import GcrlError, lib
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    z7, z8, z3 = DeviceRunningNormalizer(7), DeviceRunningNormalizer(8), DeviceRunningNormalizer(3)

    def refused(rc, state=False):
        assert rc == (-4 if state else -1) and b"normalize" in lib.gcrl_last_error(), (rc, lib.gcrl_last_error())

    cfg = _ffi.HerConfig(state_dim=10, action_dim=3, goal_dim=3, capacity=100, nenvs=2, k_future=4, flush_len=50, reward_kind=0,
                         reward_threshold=0.05, device=0, rng_mode=0, seed=1)
    h = lib.gcrl_her_create_relabel(C.byref(cfg), None, 1)
    refused(lib.gcrl_her_set_normalize(h, z8.handle, None, 7))          # a normaliser of another size
    refused(lib.gcrl_her_set_normalize(h, z7.handle, z7.handle, 7))
    refused(lib.gcrl_her_set_normalize(h, None, None, 8))               # obs_dim + goal_dim != state_dim
    refused(lib.gcrl_her_set_normalize(h, None, None, 200))
    refused(lib.gcrl_her_require_normalize(h, 1, 0), state=True)        # not a raw ring
    assert lib.gcrl_her_normalize_mode(h) == 0
    _ffi.check(lib.gcrl_her_set_normalize(h, z7.handle, z3.handle, 7))
    assert lib.gcrl_her_normalize_mode(h) == 1
    s = np.zeros(10, F32)
    refused(int(lib.gcrl_her_append(h, s.ctypes.data, 0, s.ctypes.data, 0.0, s.ctypes.data, 0, 0, None)))      # lone rows: the REPLAY buffers' entry
    lib.gcrl_her_destroy(h)
    # rings that hold rows pushed in the other mode: a HER ring, a REPLAY ring, a PER ring with its tree
    push = gcrl.HERBuffer(100, 50, 2, threshold=THR, k_future=4, rng="engine", seed=1)
    push.compute_reward = her_oracle.sparse_reward
    _fill(push, REACH, [50], 40)
    refused(lib.gcrl_her_set_normalize(push.handle, z7.handle, None, 7))
    from gcrl_amd.src.buffer import PERBuffer, ReplayBuffer
    rep = ReplayBuffer(100, rng="engine", seed=1)
    per = PERBuffer(100, 0.6, draw="device", rng="engine", seed=1)
    for b in (rep, per):
        b.push(torch.zeros(10).cuda(), np.zeros(3, F32), 0.0, torch.zeros(10).cuda(), False)
        refused(lib.gcrl_her_set_normalize(b.handle, None, None, 9))
        assert lib.gcrl_her_normalize_mode(b.handle) == 0

    # a raw ring whose needed normaliser is not bound refuses to gather: nothing is consumed
    ag, twin = _agent(gcrl, "DDPG", 37, prioritise="energy"), _agent(gcrl, "DDPG", 37, prioritise="energy")
    for x in (ag, twin):
        x.buffer.obs_normalizer = _pair(7, "created", 50)[0]
        _fill_agent(x, 52)
        T._perturb(x, 2)
    keep = ag.buffer.obs_normalizer
    ag.buffer.obs_normalizer = None

    def consumed(x):
        return (x.buffer.relabel_counter, x.buffer.prio_counter, T._mt_state(x.buffer))

    before = consumed(ag)
    for call in (lambda: ag.update(1), lambda: ag.update_many(1, 3), lambda: ag.buffer.sample(8), lambda: ag.buffer.gather_update(8),
                 lambda: ag.buffer.sample(8, indices=np.arange(8))):
        with pytest.raises(GcrlError, match="normalize"):
            call()
    assert b"normalize" in lib.gcrl_last_error() and consumed(ag) == before == (0, 0, before[2])
    ag.buffer.obs_normalizer = keep

    def ticket_of_next_update(x, step):
        t = C.c_int64(-1)
        x.set_train()
        _ffi.check(lib.gcrl_agent_update(x._h, x.buffer.handle, step, None, C.byref(t), _ffi.stream_handle()))
        return int(t.value)

    # an agent under a gradient exchange
    xh = _ffi.check_ptr(lib.gcrl_agent_xchg_create(ag._h, 0, 1), "gcrl_agent_xchg_create")
    try:
        _ffi.check(lib.gcrl_agent_set_exchange(ag._h, xh))
        with pytest.raises(GcrlError, match="update: normalize"):
            ag.update(1)
        with pytest.raises(GcrlError, match="update: normalize"):
            ag.update_many(1, 3)
        assert consumed(ag) == before
    finally:
        _ffi.check(lib.gcrl_agent_set_exchange(ag._h, None))
        lib.gcrl_xchg_destroy(xh)
    assert ticket_of_next_update(ag, 1) == ticket_of_next_update(twin, 1), "a refused call consumed a ticket"
    x, y = T._tuples(ag.update_many(2, 3)), T._tuples(twin.update_many(2, 3))
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)) and np.array_equal(T._state(ag), T._state(twin))

    # gcrl_pop_clone between rings of differing modes
    cfgs = TS._pop_cfgs()
    pop = gcrl.DDPGPopulation(REACH[0], REACH[1], cfgs, 2, 6, rng="engine", seeds=[5, 6], relabel="sample", normalize="sample")
    pop.members[1].buffer = gcrl.HERBuffer(cfgs[1].max_len, cfgs[1].max_eps_len, 2, k_future=4, rng="engine", seed=6, relabel="sample")
    pop.members[0].buffer.obs_normalizer = _pair(7, "created", 51)[0]
    for m in pop.members:
        T._fill_agent(m, 70, episodes=1)
    with pytest.raises(GcrlError, match="normalize"):
        pop.exploit([(0, 1)], copy_ring=True)
    pop.members[1].buffer.normalize = "sample"                          # past the Python check: the engine's own refusal
    with pytest.raises(GcrlError, match="gcrl_pop_clone: normalize"):
        pop.exploit([(0, 1)], copy_ring=True)
    pop.members[1].buffer.normalize = "push"
    pop.exploit([(0, 1)])                                               # without the ring: nothing to refuse
