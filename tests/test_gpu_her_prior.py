"""GPU (-m gpu): prior-data replay (prior_buffer= / prior_rows=; csrc/her_prior.hip) held bit for bit to its numpy definition
tests/her_prior_ref.py: the two-ring gather on its own, the batches an agent trains on (read back slot by slot) against a twin
without the keywords and a twin prior ring, the call forms, the four agent kinds, populations, state and the device-side refusals."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import make_config

import her_prior_ref as PR
import test_gpu_her_normalize as TN
import test_gpu_her_relabel as T
import test_gpu_her_strategy as TS
from test_gpu_her_relabel import REACH, THR, _np, bits

pytestmark = pytest.mark.gpu

B = 64
GAMMA = 0.98
WIDE70 = (70, 4, 3)                                   # a record of more than 64 floats
PRIORS = {"plain": {}, "nstep3": dict(n_step=3, gamma=GAMMA), "final": dict(goal_strategy="final")}


def _ring(gcrl, cap, dims, relabel="sample", rng="device", seed=7, **kw):
    buf = gcrl.HERBuffer(cap, 50, 2, threshold=THR, k_future=4, rng=rng, seed=seed, relabel=relabel, **kw)
    buf.compute_reward = her_oracle.sparse_reward
    return buf


def _prior(gcrl, dims=REACH, seed=11, episodes=3, fill_seed=300, cap=120, relabel="sample", **kw):
    """a prior ring of `episodes` scripted episodes through a ring of `cap` rows (3 x 50 through 120: wrapped, oldest rows evicted)"""
    buf = _ring(gcrl, cap, dims, relabel, "device", seed, **kw)
    T._fill(buf, dims, episodes, fill_seed)
    return buf


def _blob(buf):
    """the ring's whole state: rows, staged episodes, draws_done, the relabel counter"""
    from gcrl_amd._ffi import check, lib
    n = int(lib.gcrl_her_state_size(buf.handle))
    out = np.empty(n, np.uint8)
    check(lib.gcrl_her_save_state(buf.handle, out.ctypes.data, n))
    return out


def _same(x, y, what=""):
    assert np.array_equal(bits(x), bits(y)), what


# ---------------------------------------------------------------- 1. the two-ring gather against the restatement
def _check_mixed(main, twin, prior, ptwin, dims, Bd, M, spa=False):
    S = dims[0]
    got = main.gather_update_mixed(prior, Bd, B, M, spa=spa)
    want = PR.mix(tuple(None if x is None else _np(x) for x in twin.gather_update(B, M, spa=spa)),
                  tuple(None if x is None else _np(x) for x in ptwin.gather_update(Bd, M, spa=spa)), B, Bd, M, S)
    for k, name in enumerate("sa nsa spa r d".split()):
        if got[k] is not None:
            _same(_np(got[k]), want[k], (name, Bd, M))
    if spa:
        S4 = (S + 3) // 4 * 4
        assert np.isnan(_np(got[2])[:, S4:]).all() and not np.isnan(_np(got[2])[:, :S4]).any()
    assert prior.relabel_counter == ptwin.relabel_counter and main.relabel_counter == twin.relabel_counter
    return got


@pytest.mark.parametrize("prior_kind", list(PRIORS))
@pytest.mark.parametrize("main_mode", ["push", "sample"])
def test_gather_update_mixed_bitwise_the_restatement(gcrl, main_mode, prior_kind):
    main, twin = (_ring(gcrl, 300, REACH, main_mode, "engine", 5) for _ in range(2))
    for x in (main, twin):
        T._fill(x, REACH, 2 if main_mode == "push" else 7, 40)
    prior, ptwin = (_prior(gcrl, **PRIORS[prior_kind]) for _ in range(2))
    c0 = prior.relabel_counter
    rows = 0
    for Bd in (1, 20, 48, 63):                       # 20: a partial last wave in the prior gather and an unaligned r / d tail
        for M in (1, 3):
            _check_mixed(main, twin, prior, ptwin, REACH, Bd, M, spa=(Bd == 20 and M == 3))
            rows += Bd * M
    assert prior.relabel_counter == c0 + rows
    assert np.array_equal(_blob(prior), _blob(ptwin)) and np.array_equal(_blob(main), _blob(twin))
    assert T._mt_state(main) == T._mt_state(twin)


def test_gather_update_mixed_wide_record(gcrl):
    main, twin = (_ring(gcrl, 150, WIDE70, "sample", "device", 5) for _ in range(2))
    for x in (main, twin):
        T._fill(x, WIDE70, 3, 41)
    prior, ptwin = (_prior(gcrl, WIDE70) for _ in range(2))
    _check_mixed(main, twin, prior, ptwin, WIDE70, 20, 3, spa=True)
    _check_mixed(main, twin, prior, ptwin, WIDE70, 20, 1)


# ---------------------------------------------------------------- 2. the batches an agent trains on
def _agent(gcrl, kind, seed, rng="engine", relabel="sample", **kw):
    cfg = make_config(kind, hidden_dim=64, layer_count=3, batch_size=B, max_len=150, k_future=4, gamma=GAMMA, **TS.KINDS[kind])
    cls = {"DDPG": gcrl.DDPG, "TD3": gcrl.TD3Agent, "SAC": gcrl.SACAgent, "TQC": gcrl.TQCAgent}[kind]
    return cls(REACH[0], REACH[1], cfg, None, nenvs=2, gradient_step=6, rng=rng, seed=seed, relabel=relabel, **kw)


class PyRandom:
    """rng="python" rings consume the global `random` stream: each agent of a comparison runs on its own copy of it"""

    def __init__(self, seed):
        self.state = random.Random(seed).getstate()

    def run(self, fn):
        random.setstate(self.state)
        out = fn()
        self.state = random.getstate()
        return out


def _check_slots(ag, twin, ptwin, Bd, nb, what):
    """after a call of nb batches: every batch slot of `ag` against the keyword-less twin's slot and the twin prior ring's gather"""
    S = REACH[0]
    want = tuple(None if x is None else _np(x) for x in ptwin.gather_update(Bd, nb))
    for j in range(nb):
        g, w = ag.read_batch(j), twin.read_batch(j)
        h, t, pj = slice(0, B - Bd), slice(B - Bd, B), slice(j * Bd, (j + 1) * Bd)
        _same(g[0][h], w[0][h], (what, j, "sa head"))
        _same(g[1][h, :S], w[1][h, :S], (what, j, "nsa head"))
        _same(g[2][h], w[2][h], (what, j, "r head"))
        _same(g[3][h], w[3][h], (what, j, "d head"))
        _same(g[0][t], want[0][pj], (what, j, "sa tail"))
        _same(g[1][t, :S], want[1][pj, :S], (what, j, "nsa tail"))
        _same(g[2][t], want[3][pj], (what, j, "r tail"))
        _same(g[3][t], want[4][pj], (what, j, "d tail"))
        assert not np.array_equal(bits(g[0][t]), bits(w[0][t])), (what, j, "the tail rows are the main ring's")


def _run_calls(gcrl, ag, twin, ptwin, Bd, calls=T.CALLS, py=None):
    per_call = []
    for s0, n in calls:
        c0 = sum(ag.prior_counts())
        if py is None:
            T._run(ag, s0, n); T._run(twin, s0, n)
        else:
            py[0].run(lambda: T._run(ag, s0, n)); py[1].run(lambda: T._run(twin, s0, n))
        per_call.append(sum(ag.prior_counts()) - c0)
        _check_slots(ag, twin, ptwin, Bd, max(n, 1), (s0, n))
        assert ag.prior_buffer.relabel_counter == ptwin.relabel_counter
        assert np.array_equal(_blob(ag.buffer), _blob(twin.buffer)), "the main ring's counters moved differently from the twin's"
        assert ag.buffer.relabel_counter == twin.buffer.relabel_counter
    assert all(2 <= c <= 4 for c in per_call), per_call
    assert twin.prior_counts() == (0, 0)
    assert np.array_equal(_blob(ag.prior_buffer), _blob(ptwin))
    return per_call


@pytest.mark.parametrize("rng", ["python", "engine", "device"])
def test_agent_batches_head_from_main_tail_from_prior(gcrl, rng):
    Bd = 20
    prior, ptwin = _prior(gcrl), _prior(gcrl)
    py = (PyRandom(77), PyRandom(77)) if rng == "python" else None
    ag, twin = _agent(gcrl, "DDPG", 33, rng, prior_buffer=prior, prior_rows=Bd), _agent(gcrl, "DDPG", 33, rng)
    for i, x in enumerate((ag, twin)):
        (py[i].run if py else (lambda f: f()))(lambda: T._fill_agent(x, 51))
        T._perturb(x, 1)
    per_call = _run_calls(gcrl, ag, twin, ptwin, Bd, py=py)
    if rng == "engine":
        assert T._mt_state(ag.buffer) == T._mt_state(twin.buffer)
        assert per_call[0] == 2 and per_call[2] == 4, per_call     # update(): one gather part; update_many(3, 6): head + deferred rest
    if rng == "python":
        assert py[0].state == py[1].state
    if rng == "device":
        assert per_call == [2, 2, 2, 2], per_call                   # no host draw: nothing is deferred
    assert prior.relabel_counter == 14 * Bd


@pytest.mark.parametrize("case", ["nstep3_ring_gamma_differs", "push_mode"])
def test_agent_with_other_kinds_of_prior_ring(gcrl, case):
    """an n-step prior ring is discounted by the AGENT's gamma, whatever its own; a push-mode prior ring is gathered as it is"""
    Bd = 20
    if case == "push_mode":
        prior, ptwin = (_prior(gcrl, relabel="push", episodes=1, cap=200) for _ in range(2))     # 250 stored rows through 200
        assert len(prior) == 200 and prior.relabel == "push"
    else:
        prior, ptwin = _prior(gcrl, n_step=3, gamma=0.9), _prior(gcrl, n_step=3, gamma=GAMMA)
        a9, a98 = _prior(gcrl, n_step=3, gamma=0.9).gather_update(Bd, 2), _prior(gcrl, n_step=3, gamma=GAMMA).gather_update(Bd, 2)
        assert not np.array_equal(bits(_np(a9[3])), bits(_np(a98[3]))), "the discount does not show in these windows"
    ag, twin = _agent(gcrl, "DDPG", 47, prior_buffer=prior, prior_rows=Bd), _agent(gcrl, "DDPG", 47)
    for x in (ag, twin):
        T._fill_agent(x, 51)
        T._perturb(x, 1)
    _run_calls(gcrl, ag, twin, ptwin, Bd, calls=[(1, 0), (2, 6)])      # the twin prior ring's own gamma is the agent's


# ---------------------------------------------------------------- 3. call forms
def _with_prior(gcrl, kind, seed, Bd=20, rng="engine", **kw):
    ag = _agent(gcrl, kind, seed, rng, prior_buffer=_prior(gcrl), prior_rows=Bd, **kw)
    T._fill_agent(ag, 51)
    T._perturb(ag, 1)
    return ag


def _equal_agents(a, b, ta, tb, what):
    x, y = T._tuples(ta), T._tuples(tb)
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (what, x, y)
    assert np.array_equal(T._state(a), T._state(b)), what
    assert np.array_equal(_blob(a.buffer), _blob(b.buffer)) and np.array_equal(_blob(a.prior_buffer), _blob(b.prior_buffer)), what


def test_update_many_equals_updates_and_head_batches_do_not_matter(gcrl, monkeypatch):
    one, many = _with_prior(gcrl, "DDPG", 35), _with_prior(gcrl, "DDPG", 35)
    t1 = [one.update(s) for s in range(1, 10)]
    tm = many.update_many(1, 9)                                   # gradient_step = 6: chunks of 6 and 3, each with a deferred rest
    _equal_agents(one, many, t1, tm, "update_many(1, 9) is not 9 x update()")
    heads = []
    for hb in ("1", "4"):
        monkeypatch.setenv("GCRL_HEAD_BATCHES", hb)
        heads.append(_with_prior(gcrl, "DDPG", 35))
    monkeypatch.delenv("GCRL_HEAD_BATCHES")
    th = [x.update_many(1, 9) for x in heads]
    _equal_agents(heads[0], heads[1], th[0], th[1], "GCRL_HEAD_BATCHES 1 against 4")
    _equal_agents(heads[0], many, th[0], tm, "GCRL_HEAD_BATCHES 1 against the default")
    plain = _agent(gcrl, "DDPG", 35)                                # the keywords matter: other batches, other numbers
    T._fill_agent(plain, 51)
    T._perturb(plain, 1)
    tp = T._tuples(plain.update_many(1, 9))
    assert not np.array_equal(tp.view(np.uint64), T._tuples(tm).view(np.uint64))


# ---------------------------------------------------------------- 4. TD3, SAC, TQC
@pytest.mark.parametrize("kind", ["TD3", "SAC", "TQC"])
def test_other_agent_kinds(gcrl, kind):
    Bd = 48
    ag, ones = _with_prior(gcrl, kind, 37, Bd), _with_prior(gcrl, kind, 37, Bd)
    twin, ptwin = _agent(gcrl, kind, 37), _prior(gcrl)
    T._fill_agent(twin, 51)
    T._perturb(twin, 1)
    tuples = []
    for s0, n in [(1, 0), (2, 6)]:
        got = T._run(ag, s0, n)
        T._run(twin, s0, n)
        tuples += [got] if n == 0 else got
        _check_slots(ag, twin, ptwin, Bd, max(n, 1), (kind, s0, n))
    assert np.isfinite(T._tuples(tuples)).all()
    assert sum(ag.prior_counts()) <= 2 + 4
    _equal_agents(ag, ones, tuples, [ones.update(s) for s in range(1, 8)], f"{kind}: update_many is not update x n")


# ---------------------------------------------------------------- 5. energy draw, sample-time normalisation on the main ring
def test_main_ring_with_energy_draw(gcrl):
    Bd = 20
    ptwin = _prior(gcrl)
    ag, twin = _with_prior(gcrl, "DDPG", 39, Bd, prioritise="energy"), _agent(gcrl, "DDPG", 39, prioritise="energy")
    T._fill_agent(twin, 51)
    T._perturb(twin, 1)
    _run_calls(gcrl, ag, twin, ptwin, Bd, calls=[(1, 0), (2, 6)])
    assert ag.buffer.prio_counter == twin.buffer.prio_counter == 7 * B      # the tree still draws B rows per batch


def test_sample_time_normalisation_on_both_rings(gcrl):
    Bd = 20
    kw = dict(normalize="sample", obs_normalize=True, g_normalize=True)
    prior, ptwin = _prior(gcrl, **kw), _prior(gcrl, **kw)
    ag, twin = _agent(gcrl, "DDPG", 41, prior_buffer=prior, prior_rows=Bd, **kw), _agent(gcrl, "DDPG", 41, **kw)
    for x in (ag.buffer, twin.buffer, ptwin):                      # equal statistics, separate objects; `prior` gets the agent's
        x.obs_normalizer, x.dg_normalizer = TN._pair(7, "created", 21)[0], TN._pair(3, "created", 22)[0]
    for x in (ag, twin):
        T._fill_agent(x, 51)
        T._perturb(x, 1)
    _run_calls(gcrl, ag, twin, ptwin, Bd, calls=[(1, 0), (2, 6)])
    assert prior.obs_normalizer is ag.buffer.obs_normalizer and prior.dg_normalizer is ag.buffer.dg_normalizer


# ---------------------------------------------------------------- 6. populations
@pytest.mark.parametrize("shared", [False, True], ids=["own_prior_rings", "shared_prior_ring"])
@pytest.mark.parametrize("kind", ["DDPG", "TD3"])
def test_population_members_are_standalone_agents(gcrl, kind, shared):
    Bd = 20
    extra = TS.KINDS[kind]
    cfgs = [make_config(kind, hidden_dim=64, layer_count=3, batch_size=B, max_len=300, k_future=4, actor_lr=1e-3 * (1 + 0.25 * i),
                        gamma=0.98 - 0.01 * i, tau=0.05 + 0.01 * i, **extra) for i in range(2)]
    seeds = [61, 62]
    D, A = REACH[0], REACH[1]
    pcls, acls = (gcrl.DDPGPopulation, gcrl.DDPG) if kind == "DDPG" else (gcrl.TD3Population, gcrl.TD3Agent)

    def priors():
        return _prior(gcrl) if shared else [_prior(gcrl, seed=11 + i, fill_seed=300 + i) for i in range(2)]

    pp, sp = priors(), priors()
    pop = pcls(D, A, cfgs, 2, 6, rng="engine", seeds=seeds, relabel="push", prior_buffer=pp, prior_rows=Bd)
    pop.merge_gather = True
    solo = [acls(D, A, c, None, nenvs=2, gradient_step=6, rng="engine", seed=s, relabel="push",
                 prior_buffer=sp if shared else sp[i], prior_rows=Bd) for i, (c, s) in enumerate(zip(cfgs, seeds))]
    plain = pcls(D, A, cfgs, 2, 6, rng="engine", seeds=seeds, relabel="push")
    plain.merge_gather = True
    for i in range(2):
        for x in (pop.members[i], solo[i], plain.members[i]):
            T._fill_agent(x, 70 + i, episodes=1)
            T._perturb(x, i)
    for s0, n in T.CALLS:
        got, base = T._run(pop, s0, n), T._run(plain, s0, n)
        want = [T._run(a, s0, n) for a in solo]                    # standalone agents, called in member order
        for i in range(2):
            g_, w_ = T._tuples([got[i]] if n == 0 else got[i]), T._tuples([want[i]] if n == 0 else want[i])
            assert np.array_equal(g_.view(np.uint64), w_.view(np.uint64)), (i, s0, n)
            b_ = T._tuples([base[i]] if n == 0 else base[i])
            assert not np.array_equal(g_.view(np.uint64), b_.view(np.uint64))
    for i, a in enumerate(solo):
        assert np.array_equal(T._state(pop.members[i]), T._state(a)), i
        assert np.array_equal(_blob(pop.members[i].buffer), _blob(a.buffer)), i
        assert np.array_equal(_blob(pop.members[i].prior_buffer), _blob(a.prior_buffer)), i
        assert pop.members[i].prior_counts() == (len(T.CALLS), len(T.CALLS))     # a population defers nothing: one part per call
    calls, merged, alone = pop.gather_counts()
    assert (calls, merged, alone) == plain.gather_counts() and merged > 0 and alone == 0, (calls, merged, alone)   # the main gathers still merge
    if shared:
        assert pp.relabel_counter == 2 * 14 * Bd
        with pytest.raises(gcrl._ffi.GcrlError, match="prior_buffer"):
            pop.save_state("/nonexistent/never_written")
    pop.exploit([(0, 1)], copy_ring=True)                            # prior rings are left alone
    assert pop.members[1].prior_buffer is (pp if shared else pp[1])


def test_population_shared_prior_ring_under_sample_time_normalisation(gcrl):
    """a prior ring normalises with the normalisers bound to it: members that share one must share their normalisers — refused
    otherwise, before anything is consumed; with one pair for all, every member is bitwise its standalone agent"""
    Bd = 20
    kw = dict(relabel="push", normalize="sample")
    cfgs = [make_config("DDPG", hidden_dim=64, layer_count=3, batch_size=B, max_len=300, k_future=4, actor_lr=1e-3 * (1 + 0.25 * i),
                        gamma=0.98 - 0.01 * i, tau=0.05 + 0.01 * i) for i in range(2)]
    seeds, D, A = [61, 62], REACH[0], REACH[1]
    pp, sp = _prior(gcrl, normalize="sample"), _prior(gcrl, normalize="sample")
    pop = gcrl.DDPGPopulation(D, A, cfgs, 2, 6, rng="engine", seeds=seeds, prior_buffer=pp, prior_rows=Bd, **kw)
    pop.merge_gather = True
    zs = TN._pair(7, "created", 40)[0]
    solo = [gcrl.DDPG(D, A, c, None, nenvs=2, gradient_step=6, rng="engine", seed=s, prior_buffer=sp, prior_rows=Bd, **kw)
            for c, s in zip(cfgs, seeds)]
    for i in range(2):
        pop.members[i].buffer.obs_normalizer = TN._pair(7, "created", 40 + i)[0]      # each member its own statistics
        solo[i].buffer.obs_normalizer = zs
        for x in (pop.members[i], solo[i]):
            T._fill_agent(x, 70 + i, episodes=1)
            T._perturb(x, i)
    state = lambda: ([_blob(m.buffer).tobytes() for m in pop.members], _blob(pp).tobytes(), [m.prior_counts() for m in pop.members],
                     [T._state(m).tobytes() for m in pop.members])
    before = state()
    for call in (lambda: pop.update(1), lambda: pop.update_many(1, 6)):
        with pytest.raises(gcrl._ffi.GcrlError, match="DDPGPopulation: prior_buffer.*normalisers"):
            call()
    assert state() == before and pp.obs_normalizer is None, "a refused call bound or consumed something"
    pop.members[1].buffer.obs_normalizer = pop.members[0].buffer.obs_normalizer          # one pair for all members (seed 40, as `zs`)
    for s0, n in [(1, 0), (2, 6)]:
        got = T._run(pop, s0, n)
        want = [T._run(a, s0, n) for a in solo]
        for i in range(2):
            g_, w_ = T._tuples([got[i]] if n == 0 else got[i]), T._tuples([want[i]] if n == 0 else want[i])
            assert np.array_equal(g_.view(np.uint64), w_.view(np.uint64)), (i, s0, n)
    for i, a in enumerate(solo):
        assert np.array_equal(T._state(pop.members[i]), T._state(a)), i
    assert np.array_equal(_blob(pp), _blob(sp)) and pp.obs_normalizer is pop.members[0].buffer.obs_normalizer
    assert pp.relabel_counter == 2 * 7 * Bd


# ---------------------------------------------------------------- 7. state
def test_save_load_resume_bitwise(gcrl, tmp_path):
    Bd = 20
    a = _with_prior(gcrl, "DDPG", 43, Bd)
    a.update(1)
    a.update_many(2, 6)
    a.save_state(str(tmp_path / "st"))
    b = _agent(gcrl, "DDPG", 43, prior_buffer=_ring(gcrl, 120, REACH, "sample", "device", 11), prior_rows=Bd)
    b.load_state(str(tmp_path / "st"))
    assert b.prior_buffer.relabel_counter == a.prior_buffer.relabel_counter == 7 * Bd and len(b.prior_buffer) == len(a.prior_buffer)
    ta, tb = a.update_many(8, 9), b.update_many(8, 9)
    x, y = T._tuples(ta), T._tuples(tb)
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (x, y)
    assert np.array_equal(T._state(a), T._state(b))
    assert a.prior_buffer.relabel_counter == b.prior_buffer.relabel_counter == 16 * Bd      # (the blobs differ in the load's epoch word)
    for u, v in zip(a.prior_buffer.tails() + a.prior_buffer.rows(), b.prior_buffer.tails() + b.prior_buffer.rows()):
        _same(u, v)
    ga, gb = a.prior_buffer.gather_update(17, 2), b.prior_buffer.gather_update(17, 2)            # the draw counter resumed too
    for k, cols in ((0, 16), (1, REACH[0]), (3, None), (4, None)):
        _same(_np(ga[k])[:, :cols] if cols else _np(ga[k]), _np(gb[k])[:, :cols] if cols else _np(gb[k]), k)
    err = gcrl._ffi.GcrlError
    keep = T._state(b)
    with pytest.raises(err, match="load_state: prior_buffer"):      # with against without a prior ring, both ways
        _agent(gcrl, "DDPG", 43).load_state(str(tmp_path / "st"))
    plain = _agent(gcrl, "DDPG", 43)
    T._fill_agent(plain, 51)
    plain.save_state(str(tmp_path / "plain"))
    with pytest.raises(err, match="load_state: prior_buffer"):
        b.load_state(str(tmp_path / "plain"))
    other = _agent(gcrl, "DDPG", 43, prior_buffer=_ring(gcrl, 120, REACH, "sample", "device", 11), prior_rows=Bd + 1)
    with pytest.raises(err, match="load_state: prior_rows"):        # across different prior_rows
        other.load_state(str(tmp_path / "st"))
    assert np.array_equal(T._state(b), keep), "a refused load overwrote the agent"


# ---------------------------------------------------------------- 8. device-side refusals consume nothing
def test_device_side_refusals_consume_nothing(gcrl):
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import GcrlError, NotEnoughSamples, lib
    Bd = 20
    good = _prior(gcrl)
    ag, twin = _agent(gcrl, "DDPG", 45, prior_buffer=good, prior_rows=Bd), _with_prior(gcrl, "DDPG", 45, Bd)
    T._fill_agent(ag, 51)
    T._perturb(ag, 1)
    tick0 = int(ag.update(1)[0]._ticket)
    twin.update(1)
    prior0 = _blob(good)

    def consumed():
        return (_blob(ag.buffer).tobytes(), T._mt_state(ag.buffer), ag.prior_counts())

    before = consumed()
    # a prior ring shorter than prior_rows: the Python layer, and the engine's own check behind it
    short = _ring(gcrl, 120, REACH, "sample", "device", 11)
    ep = T._episode(np.random.default_rng(1), 10, REACH, True)
    short.push_episode(0, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
    assert len(short) == 10
    ag.prior_buffer = short
    for call in (lambda: ag.update(2), lambda: ag.update_many(2, 6)):
        with pytest.raises(NotEnoughSamples, match="prior_buffer"):
            call()
    _ffi.check(lib.gcrl_agent_set_prior(ag._h, short.handle, Bd))
    t = C.c_int64(-1)
    assert lib.gcrl_agent_update(ag._h, ag.buffer.handle, 2, None, C.byref(t), _ffi.stream_handle()) == _ffi.GCRL_ERR_NOT_ENOUGH
    assert b"prior_buffer" in lib.gcrl_last_error() and b"Not enough in buffer" in lib.gcrl_last_error()
    tickets = (C.c_int64 * 6)(); lens = (C.c_int32 * 6)()
    assert lib.gcrl_agent_update_n(ag._h, ag.buffer.handle, 2, 6, tickets, lens, _ffi.stream_handle()) == _ffi.GCRL_ERR_NOT_ENOUGH
    assert consumed() == before and short.relabel_counter == 0
    # other dims
    wrong = _prior(gcrl, T.PICK)
    ag.prior_buffer = wrong
    with pytest.raises((ValueError, GcrlError), match="prior_buffer"):
        ag.update(2)
    with pytest.raises((ValueError, GcrlError), match="prior_buffer"):
        ag.update_many(2, 6)
    assert lib.gcrl_agent_set_prior(ag._h, good.handle, 0) == -1 and b"prior_rows" in lib.gcrl_last_error()
    assert lib.gcrl_agent_set_prior(ag._h, good.handle, B) == -1 and b"prior_rows" in lib.gcrl_last_error()
    assert lib.gcrl_agent_set_prior(ag._h, ag.buffer.handle, Bd) == -1 and b"prior_buffer" in lib.gcrl_last_error()   # rng="engine", and its own ring
    assert consumed() == before and wrong.relabel_counter == 0
    # the goal width alone differs: the engine's check against the ring the call gathers from
    wrong_g = _prior(gcrl, (10, 3, 2))
    ag.prior_buffer = wrong_g
    for call in (lambda: ag.update(2), lambda: ag.update_many(2, 6), lambda: ag.buffer.gather_update_mixed(wrong_g, Bd, B)):
        with pytest.raises(GcrlError, match="prior_buffer.*G=2"):
            call()
    assert consumed() == before and wrong_g.relabel_counter == 0
    # an agent under a gradient exchange (world 1)
    ag.prior_buffer = good
    ag._prior_bound = None                                           # (the engine was handed `short` directly above)
    xh = _ffi.check_ptr(lib.gcrl_agent_xchg_create(ag._h, 0, 1), "gcrl_agent_xchg_create")
    try:
        _ffi.check(lib.gcrl_agent_set_exchange(ag._h, xh))
        with pytest.raises(GcrlError, match="update: prior_buffer"):
            ag.update(2)
        with pytest.raises(GcrlError, match="update: prior_buffer"):
            ag.update_many(2, 6)
        assert consumed() == before and np.array_equal(_blob(good), prior0)
    finally:
        _ffi.check(lib.gcrl_agent_set_exchange(ag._h, None))
        lib.gcrl_xchg_destroy(xh)
    # the two-ring gather holds the prior ring to the same rules
    with pytest.raises(NotEnoughSamples, match="prior_buffer"):
        ag.buffer.gather_update_mixed(short, Bd, B)
    with pytest.raises((ValueError, GcrlError), match="prior_buffer"):
        ag.buffer.gather_update_mixed(wrong, Bd, B)
    assert consumed() == before and np.array_equal(_blob(good), prior0)
    # ... and the agent goes on bit for bit like a twin that was never refused
    ta, tb = [ag.update(2)] + ag.update_many(3, 6), [twin.update(2)] + twin.update_many(3, 6)
    assert int(ta[0][0]._ticket) == tick0 + 1 == int(tb[0][0]._ticket), "a refused call consumed a ticket"
    _equal_agents(ag, twin, ta, tb, "after the refusals")


# ---------------------------------------------------------------- 9. the caller's side
def test_trainer_standin_with_a_prior_ring(gcrl):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import trainer_standin
    for kw in (dict(), dict(fused=True, normalize="sample", relabel="sample")):
        out = trainer_standin.train("DDPG", cycles=4, seed=0, verbose=False, prior_episodes=12, prior_rows=64, **kw)
        assert out["gradient_steps"] == 4 * 40 and np.isfinite(out["success_per_cycle"]).all(), kw
    with pytest.raises(SystemExit, match="go together"):
        trainer_standin.train("DDPG", cycles=1, seed=0, verbose=False, prior_rows=64)
