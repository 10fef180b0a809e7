"""GPU (-m gpu): the replay side of a population's update call (csrc/her_ring.hip her_gather_update_pop_kernel, csrc/agent_pop.inc
gcrl_pop_update_n; src/population.py merge_gather / gather_counts / shared_ring).

One gather launch for all members: every member's indices are drawn first, in member order, then ONE launch of the gather kernel's
population form copies every member's rows out of its own ring — or out of the ring all members share.  The gather is a copy, so
given the same indices the launch is bit for bit the members' own launches, and a member stays bit for bit a standalone agent:
metric tuples and gcrl_agent_save_state blobs are compared by np.array_equal on their bit views, as tests/test_gpu_population.py
compares them.  The shapes reach every branch of the kernel: both launch forms (head: indices read from the pinned block, control
block as a side copy; main: both uploaded first), a wrapped ring, a partial last wave, two column passes, a null index pointer with
per-member index generators, and `spa` written on the layer-per-launch schedule (TQC)."""
import random

import numpy as np
import pytest

from oracle import her_oracle
from oracle.agent_oracle import make_config

import test_gpu_population as tp
import test_gpu_population_acting as tpa
import test_gpu_population_sac as tps
import test_gpu_population_td3 as tp3
import test_gpu_population_tqc as tpq

pytestmark = pytest.mark.gpu

S, A = 10, 3
# member 1's ring holds 600 rows and is filled with more (four episodes of ~246 rows): wrapped, head != 0
MAX_LENS = (4000, 600, 3000)


def _cfgs(P, B=64, H=64):
    out = tp._cfgs(P, H, B)
    for i, c in enumerate(out):
        c.max_len = MAX_LENS[i % len(MAX_LENS)]
    return out


def _fill(ag, i, s=S, a=A):
    gen = np.random.default_rng(100 + i)          # each member its own episodes
    for ep in range(4):
        for st in her_oracle.synthetic_episode(gen, 50, s, a):
            ag.push_her(ep % 2, *st)
    _perturb(ag, i)


def _perturb(ag, i):
    gen = np.random.default_rng(200 + i)
    for v in (ag.actor, ag.critic):
        v.set_flat((v.flat() + 0.05 * gen.standard_normal(v.numel())).astype(np.float32))
    ag.update_target_network()


def _head(buf):
    from gcrl_amd._ffi import lib
    return int(lib.gcrl_her_head(buf.handle))


def _pair(gcrl, cfgs, seeds, rng="engine", gstep=8, s=S, a=A, merge=True):
    pop = gcrl.DDPGPopulation(s, a, cfgs, 2, gstep, rng=rng, seeds=seeds)
    pop.merge_gather = merge
    assert pop.merge_gather is merge
    solo = [gcrl.DDPG(s, a, c, None, nenvs=2, gradient_step=gstep, rng=rng, seed=sd) for c, sd in zip(cfgs, seeds)]
    for i in range(len(cfgs)):
        _fill(pop.members[i], i, s, a)
        _fill(solo[i], i, s, a)
    return pop, solo


def _run(ag_or_pop, calls):
    """calls of (step0, n): n == 0 is `update(step0)`, otherwise `update_many(step0, n)`; -> per call the result"""
    return [ag_or_pop.update(s0) if n == 0 else ag_or_pop.update_many(s0, n) for s0, n in calls]


def _compare(pop, solo, calls):
    got = _run(pop, calls)
    want = [_run(a, calls) for a in solo]
    for c, (s0, n) in enumerate(calls):
        for i in range(len(solo)):
            g = tp._tuples([got[c][i]] if n == 0 else got[c][i])
            w = tp._tuples([want[i][c]] if n == 0 else want[i][c])
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (i, s0, n, g, w)
    for i, (m, a) in enumerate(zip(pop.members, solo)):
        assert np.array_equal(tp._state(m), tp._state(a)), f"member {i}: engine state differs from the standalone agent"


# update(step) three times: the head form (64 indices read from each member's pinned block, its control block as a side copy);
# update_many with n = 8 twice: the members' uploads, then the main form
CALLS = [(1, 0), (2, 0), (3, 0), (4, 8), (12, 8)]


def test_own_rings_both_launch_forms(gcrl):
    pop, solo = _pair(gcrl, _cfgs(3), [21, 22, 23])
    lens = [len(m.buffer) for m in pop.members]
    assert lens[1] == 600 and _head(pop.members[1].buffer) != 0, (lens, _head(pop.members[1].buffer))     # wrapped
    assert lens[0] > 600 and lens[2] > 600
    _compare(pop, solo, CALLS)
    assert pop.gather_counts() == (len(CALLS), len(CALLS), 0), pop.gather_counts()   # one population gather per chunk, none alone


def test_partial_last_wave(gcrl):
    """batch 72: the smallest batch above 64 that is no multiple of 16 — the row chain admits any batch size (agent.hip: its row
    blocks are 4 rows); n = 1 and n = 3 give 72 and 216 rows per member, both = 8 mod 16: the launch's last wave is partial and
    stores straight from its load lanes"""
    pop, solo = _pair(gcrl, _cfgs(3, B=72), [31, 32, 33])
    _compare(pop, solo, [(1, 0), (2, 3), (5, 0), (6, 3)])
    assert pop.gather_counts() == (4, 4, 0), pop.gather_counts()


def test_two_column_passes(gcrl):
    """S 40 / A 4: a record's [s | a] and [ns] groups are 44 + 40 = 84 floats > 64, so every wave takes a second column pass"""
    pop, solo = _pair(gcrl, _cfgs(2), [41, 42], s=40, a=4)
    _compare(pop, solo, [(1, 0), (2, 8), (10, 0)])
    assert pop.gather_counts() == (3, 3, 0), pop.gather_counts()


def test_device_rng(gcrl):
    """rng="device": no index array at all — each member's entry carries its own ring's IdxGen and a null index pointer"""
    pop, solo = _pair(gcrl, _cfgs(3), [51, 52, 53], rng="device")
    _compare(pop, solo, CALLS)
    assert pop.gather_counts() == (len(CALLS), len(CALLS), 0), pop.gather_counts()


def _capture(monkeypatch, mod):
    """the kind's own bitwise case (its twins run the forms pop.forms() reports), on a population that merges its gathers"""
    made = []
    orig = mod._pop

    def wrap(*a, **k):
        p = orig(*a, **k)
        p.merge_gather = True
        made.append(p)
        return p
    monkeypatch.setattr(mod, "_pop", wrap)
    return made


def test_tqc(gcrl, monkeypatch, tmp_path):
    """the layer-per-launch schedule: the gather also writes `spa`"""
    made = _capture(monkeypatch, tpq)
    tpq._bitwise_case(gcrl, (2, 64, 64, 5, 2), 61, tmp=tmp_path)
    calls, merged, alone = made[0].gather_counts()
    assert calls == len(tpq.CALLS) and merged == calls and alone == 0, (calls, merged, alone)


def test_sac(gcrl, monkeypatch, tmp_path):
    made = _capture(monkeypatch, tps)
    tps._bitwise_case(gcrl, 10, 3, 64, 64, 2, 8, 71, tps.CALLS_SMALL, tmp=tmp_path)
    calls, merged, alone = made[0].gather_counts()
    assert calls == len(tps.CALLS_SMALL) and merged == calls and alone == 0, (calls, merged, alone)


def test_td3(gcrl):
    pop, solo = tp3._pair(gcrl, 10, 3, tp3._cfgs(2, 64, 64), 8, [81, 82])
    pop.merge_gather = True
    tp3._run_and_compare(pop, solo, tp3.CALLS_SMALL)
    assert pop.gather_counts() == (3, 3, 0), pop.gather_counts()


def test_switch(gcrl):
    """merge_gather off: the same trajectory, bit for bit, from the members' own gather launches"""
    on, _ = _pair(gcrl, _cfgs(3), [91, 92, 93])
    off = gcrl.DDPGPopulation(S, A, _cfgs(3), 2, 8, rng="engine", seeds=[91, 92, 93])
    assert off.merge_gather is (3 >= off.MERGE_GATHER_FROM)
    off.merge_gather = False
    for i, m in enumerate(off.members):
        _fill(m, i)
    g_on, g_off = _run(on, CALLS), _run(off, CALLS)
    for c, (s0, n) in enumerate(CALLS):
        for i in range(3):
            a = tp._tuples([g_on[c][i]] if n == 0 else g_on[c][i])
            b = tp._tuples([g_off[c][i]] if n == 0 else g_off[c][i])
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (i, s0, n)
    for i in range(3):
        assert np.array_equal(tp._state(on.members[i]), tp._state(off.members[i])), i
    assert on.gather_counts() == (len(CALLS), len(CALLS), 0), on.gather_counts()
    assert off.gather_counts() == (len(CALLS), 0, 3 * len(CALLS)), off.gather_counts()
    assert on.launch_counts() == off.launch_counts()      # gathers are not recorded positions


# ---------------------------------------------------------------- one ring for all members
def _shared_pair(gcrl, rng, seeds, nenvs=2, merge=True):
    """a population with shared_ring against standalone agents assigned one HERBuffer; both rings filled with the same episodes
    from identically seeded host generators"""
    from gcrl_amd.src.buffer import HERBuffer
    P = len(seeds)
    cfgs = tp._cfgs(P, 64, 64)
    random.seed(777)
    pop = gcrl.DDPGPopulation(S, A, cfgs, nenvs, 8, rng=rng, seeds=seeds, shared_ring=True)
    pop.merge_gather = merge
    assert all(m.buffer is pop.buffer for m in pop.members) and pop.buffer.nenvs == nenvs * P
    gen = np.random.default_rng(5)
    for ep in range(6):
        for st in her_oracle.synthetic_episode(gen, 50, S, A):
            pop.members[ep % P].push_her(ep % (nenvs * P), *st)
    st_pop = random.getstate()
    random.seed(777)
    solo = [gcrl.DDPG(S, A, c, None, nenvs=nenvs, gradient_step=8, rng=rng, seed=sd) for c, sd in zip(cfgs, seeds)]
    ring = HERBuffer(cfgs[0].max_len, cfgs[0].max_eps_len, nenvs * P, k_future=cfgs[0].k_future, rng=rng, seed=seeds[0])
    for a in solo:
        a.buffer = ring
    gen = np.random.default_rng(5)
    for ep in range(6):
        for st in her_oracle.synthetic_episode(gen, 50, S, A):
            solo[ep % P].push_her(ep % (nenvs * P), *st)
    assert random.getstate() == st_pop
    for i in range(P):
        _perturb(pop.members[i], i)
        _perturb(solo[i], i)
    return pop, solo, ring


@pytest.mark.parametrize("rng", ["python", "engine", "device"])
def test_shared_ring_update(gcrl, rng):
    """members sharing a ring draw from its index stream in member order (device mode: the ring's draw counter advances per
    member) and are bit for bit standalone agents that share the ring and are called in member order"""
    pop, solo, ring = _shared_pair(gcrl, rng, [101, 102, 103])
    assert len(pop.buffer) == len(ring) >= 64
    for g, w in zip(pop.buffer.rows(), ring.rows()):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    random.seed(99)
    got = _run(pop, CALLS)
    st_pop = random.getstate()
    random.seed(99)
    want = [[a.update(s0) if n == 0 else a.update_many(s0, n) for a in solo] for s0, n in CALLS]     # per call, in member order
    assert random.getstate() == st_pop
    for c, (s0, n) in enumerate(CALLS):
        for i in range(3):
            g = tp._tuples([got[c][i]] if n == 0 else got[c][i])
            w = tp._tuples([want[c][i]] if n == 0 else want[c][i])
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (rng, i, s0, n, g, w)
    for i in range(3):
        assert np.array_equal(tp._state(pop.members[i]), tp._state(solo[i])), (rng, i)
    # the members did not all learn from the same batches
    assert not np.array_equal(tp._tuples(got[-1][0]).view(np.uint64), tp._tuples(got[-1][1]).view(np.uint64))
    assert pop.gather_counts() == (len(CALLS), len(CALLS), 0), pop.gather_counts()


def test_shared_ring_push(gcrl):
    """pop.process_step with a shared ring: member by member, member i's envs in episode slots i * nenvs ...; the ring and the
    shared normalisers end bit for bit where the standalone agents' process_step(env0 = i * nenvs) in member order leaves them"""
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    sh, n, P = tpa.CFG1, tpa.NENVS, 3
    pop, solo, ring = _shared_pair(gcrl, "engine", [111, 112, 113], nenvs=n)
    for buf in (pop.buffer, ring):
        buf.obs_normalizer = DeviceRunningNormalizer(sh["D"])
        buf.dg_normalizer = DeviceRunningNormalizer(sh["G"])
    proc0 = pop.acting_counts()[2]
    for step in range(60):
        rows = [tpa._rows(step, i, sh, n) for i in range(P)]
        gen = np.random.default_rng(9000 + step)
        acts = [gen.uniform(-1, 1, (n, sh["A"])).astype(np.float32) for _ in range(P)]
        states, nxts, rews = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
        dn = [np.asarray(tpa._dones(step + 7 * i), bool) for i in range(P)]      # episodes ending, at other steps for each member
        got, want = tpa._both(8000 + step, lambda: pop.process_step(states, acts, nxts, rews, dn),
                              lambda: [a.process_step(s, ac, nx, r, d, env0=i * n)
                                       for i, (a, s, ac, nx, r, d) in enumerate(zip(solo, states, acts, nxts, rews, dn))])
        assert got == want, (step, got, want)
    assert pop.acting_counts()[2] == proc0          # the merged staging launch was never taken
    assert len(pop.buffer) == len(ring) and _head(pop.buffer) == _head(ring)
    assert len(ring) == pop.buffer.max_mem_len and _head(ring) != 0      # the ring wrapped
    for g, w in zip(pop.buffer.rows(), ring.rows()):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), "ring rows differ"
    for name in ("obs_normalizer", "dg_normalizer"):
        g, w = tpa._nz_state(getattr(pop.buffer, name)), tpa._nz_state(getattr(ring, name))
        assert np.array_equal(g[0], w[0]) and g[1] == w[1], name
    assert np.array_equal(tpa._mt_state(pop.members[0]), tpa._mt_state(solo[0]))
