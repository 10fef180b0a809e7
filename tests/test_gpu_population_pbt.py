"""GPU (-m gpu): population-based training on a live population (src/population.py exploit / explore / replace; include/gcrl.h
gcrl_pop_clone — pop_clone_kernel, csrc/pop_clone.hip —, gcrl_agent_set_hparams, gcrl_pop_replace), held to BITWISE equality with the
paths the tree already had: the host save_state / load_state round trip, and a freshly constructed agent / population.

Shapes are the smallest the population tests use (H 64 — a multiple of 16 for the slab forms —, L 2, B 64, S 10, A 4), P = 3 so that
one member is a bystander, and each ring holds 700 rows and has wrapped once (984 rows pushed), so a ring clone copies two pieces."""
import os

import numpy as np
import pytest

from oracle import her_oracle
from oracle.agent_oracle import make_config

pytestmark = pytest.mark.gpu

S, A, D, G, H, L, B, GSTEP, P = 10, 4, 7, 3, 64, 2, 64, 8, 3
RING = 700
KINDS = ["DDPG", "TD3", "SAC", "TQC"]
SEEDS = [11, 12, 13]


def _classes(gcrl, kind):
    return {"DDPG": (gcrl.DDPGPopulation, gcrl.DDPG), "TD3": (gcrl.TD3Population, gcrl.TD3Agent),
            "SAC": (gcrl.SACPopulation, gcrl.SACAgent), "TQC": (gcrl.TQCPopulation, gcrl.TQCAgent)}[kind]


def _cfg(kind, i):
    """members that differ in learning rates and their schedules, gamma, tau, grad_clip (member 1: none) and alpha_lr; the actor of
    TD3 / SAC / TQC steps every second step, so six steps hold actor steps and critic-only steps"""
    kw = dict(hidden_dim=H, layer_count=L, batch_size=B, max_len=RING, ac_update_freq=1 if kind == "DDPG" else 2,
              actor_lr=1e-3 * (1 + 0.25 * i), actor_lr_min=2e-4, ac_scheduler_steps=30 + i,
              critic_lr=1e-3 * (1 + 0.5 * i), critic_lr_min=3e-4, cr_scheduler_steps=25 + 2 * i,
              gamma=0.98 - 0.01 * i, tau=0.05 + 0.01 * i, grad_clip=None if i == 1 else 1.0 + i)
    if kind in ("SAC", "TQC"):
        kw.update(alpha_lr=3e-4 * (1 + i), alpha_min_steps=2)
    if kind == "TQC":
        kw.update(num_critics=3, top_quantiles_to_drop=1)
    return make_config(kind, **kw)


def _fill_ring(ag, i, episodes=4):
    gen = np.random.default_rng(300 + i)          # each member its own episodes; 4 x 246 rows: the 700-row ring wraps once
    for ep in range(episodes):
        for st in her_oracle.synthetic_episode(gen, 50, S, A):
            ag.push_her(ep % 2, *st)


def _scramble(ag, i):
    gen = np.random.default_rng(400 + i)
    for v in [ag.actor] + list(ag.critics):
        v.set_flat((v.flat() + 0.05 * gen.standard_normal(v.numel())).astype(np.float32))
    ag.update_target_network()


def _pop(gcrl, kind, cfgs=None, seeds=SEEDS, scramble=True):
    cls, _ = _classes(gcrl, kind)
    pop = cls(S, A, cfgs or [_cfg(kind, i) for i in range(P)], 2, GSTEP, rng="engine", seeds=list(seeds))
    for i, m in enumerate(pop.members):
        _fill_ring(m, i)
        if scramble:
            _scramble(m, i)
    return pop


def _state(ag):
    from gcrl_amd._ffi import check, lib
    n = int(lib.gcrl_agent_state_size(ag._h))
    blob = np.empty(n, np.uint8)
    check(lib.gcrl_agent_save_state(ag._h, blob.ctypes.data, n))
    return blob


def _host_round_trip(pop, s, d):
    """the parent's only way: member s's blob to host memory and back into member d, plus what load_state sets on the Python side"""
    from gcrl_amd._ffi import check, lib
    blob = _state(pop.members[s])
    check(lib.gcrl_agent_load_state(pop.members[d]._h, blob.ctypes.data, blob.size))
    a, b = pop.members[s], pop.members[d]
    b.beta, b.actor.num_batches_tracked = a.beta, int(a.actor.num_batches_tracked)
    b._metric_cache.clear()


def _vals(ts):
    w = max(len(t) for t in ts)
    return np.array([[float(x) for x in t] + [0.0] * (w - len(t)) for t in ts], np.float64), [len(t) for t in ts]


def _same(got, want, what):
    (g, gl), (w, wl) = _vals(got), _vals(want)
    assert gl == wl, (what, gl, wl)
    assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, g, w)


def _same_pops(a, b, step0, n, members=range(P)):
    ga, gb = a.update_many(step0, n), b.update_many(step0, n)
    for i in members:
        _same(ga[i], gb[i], ("member", i, "step0", step0))
        assert np.array_equal(_state(a.members[i]), _state(b.members[i])), f"member {i}: engine state differs"
        assert int(a.members[i].actor.num_batches_tracked) == int(b.members[i].actor.num_batches_tracked), i


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pairs", [[(0, 2)], [(0, 1), (0, 2)]], ids=["one_pair", "one_source_two_destinations"])
def test_clone_equals_host_round_trip(gcrl, kind, pairs):
    pop, twin = _pop(gcrl, kind), _pop(gcrl, kind)
    _same_pops(pop, twin, 1, 6)
    bystanders = [i for i in range(P) if i not in [d for _, d in pairs]]
    before = {i: _state(pop.members[i]) for i in bystanders}
    merged0 = pop.launch_counts()
    pop.exploit(pairs)
    assert pop.launch_counts() == merged0            # (the clone is no update launch position)
    for s, d in pairs:
        _host_round_trip(twin, s, d)
    for s, d in pairs:
        got, want = _state(pop.members[d]), _state(twin.members[d])
        assert np.array_equal(got, want), f"{kind}: member {d} after the clone differs from the host round trip in {int((got != want).sum())} bytes"
        assert np.array_equal(got, _state(pop.members[s]))        # (the blob holds state only: the destination's config stays its own)
        assert pop.members[d].config.gamma == _cfg(kind, d).gamma
    for i in bystanders:
        assert np.array_equal(_state(pop.members[i]), before[i]), f"member {i} was touched"
    _same_pops(pop, twin, 7, 6)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("merged", [True, False], ids=["population_launch", "members_own_entry"])
def test_acting_after_a_clone(gcrl, kind, merged):
    pop = _pop(gcrl, kind)
    pop.MERGE_ACTING_FROM = 2 if merged else 17
    pop.update_many(1, 6)
    gen = np.random.default_rng(5)
    obs, dg = gen.standard_normal((8, D)).astype(np.float32), gen.uniform(-0.2, 0.2, (8, G)).astype(np.float32)

    def act():
        return pop.observe_act([obs] * P, [dg] * P, eval_action=True, obs_normalize=False, g_normalize=False)

    calls0 = pop.acting_counts()[0]
    a = act()                                        # (the [in][out] acting copies are clean from here on)
    assert not np.array_equal(a[0], a[2]) and not np.array_equal(a[0], a[1])
    pop.exploit([(0, 2)])
    b = act()
    assert (pop.acting_counts()[0] - calls0 == 2) == merged
    assert np.array_equal(b[0].view(np.uint64), a[0].view(np.uint64)) and np.array_equal(b[1].view(np.uint64), a[1].view(np.uint64))
    assert np.array_equal(b[2].view(np.uint64), b[0].view(np.uint64)), "member 2 does not act as member 0 after the clone"


@pytest.mark.parametrize("kind", KINDS)
def test_ring_clone_equals_file_round_trip(gcrl, kind, tmp_path):
    pop, twin = _pop(gcrl, kind), _pop(gcrl, kind)
    half = her_oracle.synthetic_episode(np.random.default_rng(77), 50, S, A)
    for p in (pop, twin):
        p.update_many(1, 6)
        for st in half[:25]:                          # half an episode staged in member 0's env 1 before the clone
            p.members[0].push_her(1, *st)
    assert len(pop.members[0].buffer) == RING and len(pop.members[2].buffer) == RING
    pop.exploit([(0, 2)], copy_ring=True)
    twin.members[0].save_state(str(tmp_path / "m0"))
    twin.members[2].load_state(str(tmp_path / "m0"))
    assert np.array_equal(_state(pop.members[2]), _state(twin.members[2]))
    for p in (pop, twin):
        done = [st[:4] + (i == 24,) + st[5:] for i, st in enumerate(half[25:])]
        for st in done:                               # ... finished after it, in the destination: the episode flushes there
            p.members[2].push_her(1, *st)
    assert len(pop.members[2].buffer) == len(twin.members[2].buffer) == RING
    for g, w in zip(pop.members[2].buffer.rows(), twin.members[2].buffer.rows()):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), "ring rows differ from the file round trip"
    for g, w in zip(pop.members[1].buffer.rows(), twin.members[1].buffer.rows()):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    for _ in range(2):
        for g, w in zip(pop.members[2].buffer.sample(B), twin.members[2].buffer.sample(B)):
            assert np.array_equal(g.cpu().numpy().view(np.uint32), w.cpu().numpy().view(np.uint32)), "sampled batch differs"
    _same_pops(pop, twin, 7, 6)


NEW = dict(actor_lr=7e-4, actor_lr_min=1e-4, ac_scheduler_steps=7, critic_lr=1.3e-3, critic_lr_min=5e-4, cr_scheduler_steps=9,
           gamma=0.95, tau=0.02, grad_clip=0.5)


def _header(blob):
    """(t_actor, t_critic, t_alpha, lr_actor, lr_critic) of an engine state blob: the header's three int64 counters at byte 64 and the
    two float64 rates after them (csrc/agent.hip AgentStateHeader: 2 uint32, 8 int32, 3 int64 before them)"""
    return tuple(int(x) for x in blob[64:88].view(np.int64)) + tuple(float(x) for x in blob[88:104].view(np.float64))


@pytest.mark.parametrize("kind", KINDS)
def test_set_hparams_rates_are_the_new_schedule_at_the_kept_positions(gcrl, kind):
    """Independent of load_state (which would hand the rates over): an agent CONSTRUCTED with the new schedule and stepped as many actor
    and critic steps on its own holds, bit for bit, the rates member 1 holds after `explore` — and they are neither the old schedule's
    rates nor the new base rates.  11 steps: past the new schedules' lengths (7 and 9), so the recursion has turned; for TD3 / SAC / TQC
    the actor has stepped 5 times and the critics 11, so swapped positions would show."""
    new = dict(NEW, **(dict(alpha_lr=9e-4) if kind in ("SAC", "TQC") else {}))
    pop = _pop(gcrl, kind)
    pop.update_many(1, 8)
    pop.update_many(9, 3)
    old = _header(_state(pop.members[1]))
    others = {i: _state(pop.members[i]) for i in (0, 2)}
    pop.explore(1, **new)
    got = _header(_state(pop.members[1]))
    cfg = _cfg(kind, 1)
    for k, v in new.items():
        setattr(cfg, k, v)
    _, agent_cls = _classes(gcrl, kind)
    solo = agent_cls(S, A, cfg, None, nenvs=2, gradient_step=GSTEP, rng="engine", seed=5)
    _fill_ring(solo, 1)
    solo.update_many(1, 8)
    solo.update_many(9, 3)
    want = _header(_state(solo))
    assert got[:3] == old[:3] == want[:3] and got[1] == 11 and got[0] == (11 if kind == "DDPG" else 5), (got, old, want)
    assert np.float64(got[3]).view(np.uint64) == np.float64(want[3]).view(np.uint64), ("actor rate", got[3], want[3])
    assert np.float64(got[4]).view(np.uint64) == np.float64(want[4]).view(np.uint64), ("critic rate", got[4], want[4])
    assert got[3] not in (old[3], new["actor_lr"]) and got[4] not in (old[4], new["critic_lr"]), (got, old)
    for i in (0, 2):
        assert np.array_equal(_state(pop.members[i]), others[i]), i


@pytest.mark.parametrize("kind", KINDS)
def test_set_hparams_equals_a_constructed_agent(gcrl, kind, tmp_path):
    new = dict(NEW, **(dict(alpha_lr=9e-4) if kind in ("SAC", "TQC") else {}))
    pop, twin = _pop(gcrl, kind), _pop(gcrl, kind)
    _same_pops(pop, twin, 1, 5)
    forms = pop.forms()
    pop.explore(1, **new)
    assert pop.forms() == forms
    assert pop.members[1].config.gamma == 0.95 and twin.members[1].config.gamma != 0.95 and pop.members[0].config.gamma == 0.98
    # a standalone agent CONSTRUCTED with the new values, given member 1's state (engine blob, ring, index stream) by load_state
    cfg = _cfg(kind, 1)
    for k, v in new.items():
        setattr(cfg, k, v)
    _, agent_cls = _classes(gcrl, kind)
    solo = agent_cls(S, A, cfg, None, nenvs=2, gradient_step=GSTEP, rng="engine", seed=SEEDS[1])
    pop.members[1].save_state(str(tmp_path / "m1"))
    solo.load_state(str(tmp_path / "m1"))
    assert np.array_equal(_state(solo), _state(pop.members[1]))
    got, ref = pop.update_many(6, 5), twin.update_many(6, 5)
    _same(got[1], solo.update_many(6, 5), "member 1 against the constructed agent")
    assert np.array_equal(_state(pop.members[1]), _state(solo)), "member 1's state differs from the constructed agent's"
    assert not np.array_equal(_state(pop.members[1]), _state(twin.members[1]))          # (the new values did something)
    for i in (0, 2):
        _same(got[i], ref[i], ("bystander", i))
        assert np.array_equal(_state(pop.members[i]), _state(twin.members[i])), i


@pytest.mark.parametrize("kind", KINDS)
def test_replace_equals_a_fresh_member(gcrl, kind):
    new_cfg, new_seed = _cfg(kind, 2), 99
    new_cfg.actor_lr, new_cfg.gamma = 4e-4, 0.9
    pop = _pop(gcrl, kind)
    pop.update_many(1, 5)
    forms = pop.forms()
    others = {i: _state(pop.members[i]) for i in (0, 2)}
    ring = pop.members[1].buffer
    pop.replace(1, new_cfg, new_seed)
    assert pop.members[1].buffer is ring and len(ring) == 0 and pop.forms() == forms
    fresh = _pop(gcrl, kind, cfgs=[_cfg(kind, 0), new_cfg, _cfg(kind, 2)], seeds=[SEEDS[0], new_seed, SEEDS[2]], scramble=False)
    got, want = _state(pop.members[1]), _state(fresh.members[1])
    assert np.array_equal(got, want), f"{kind}: the replaced member differs from a fresh one in {int((got != want).sum())} bytes"
    for i in (0, 2):
        assert np.array_equal(_state(pop.members[i]), others[i]), f"member {i} was touched"
    _fill_ring(pop.members[1], 1)
    for g, w in zip(pop.members[1].buffer.rows(), fresh.members[1].buffer.rows()):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    (m1, a1), (f1, g1) = pop.launch_counts(), fresh.launch_counts()
    _same(pop.update_many(6, 5)[1], fresh.update_many(6, 5)[1], "replaced member against the fresh one")
    assert np.array_equal(_state(pop.members[1]), _state(fresh.members[1]))
    (m2, a2), (f2, g2) = pop.launch_counts(), fresh.launch_counts()
    assert (m2 - m1, a2 - a1) == (f2 - f1, g2 - g1) and m2 > m1, "launch positions per step differ from a fresh population's"
    assert pop.forms() == fresh.forms() == forms


def test_population_state_round_trip(gcrl, tmp_path):
    pop, other = _pop(gcrl, "TD3"), _pop(gcrl, "TD3", seeds=[21, 22, 23])
    pop.update_many(1, 5)
    pop.save_state(str(tmp_path / "pop"))
    assert sorted(os.listdir(tmp_path / "pop")) == ["member_00", "member_01", "member_02", "population.json"]
    other.load_state(str(tmp_path / "pop"))
    _same_pops(pop, other, 6, 5)
    with pytest.raises(gcrl._ffi.GcrlError, match="kind"):
        _pop(gcrl, "DDPG").load_state(str(tmp_path / "pop"))


def test_native_refusals_name_the_argument(gcrl):
    import ctypes as C
    from gcrl_amd import _ffi
    pop = _pop(gcrl, "DDPG")
    before = [_state(m) for m in pop.members]

    def clone(src, dst, what=1, rings=None, n=None):
        s, d = (C.c_int32 * len(src))(*src), (C.c_int32 * len(dst))(*dst)
        rc = _ffi.lib.gcrl_pop_clone(pop._pop.h, rings, s, d, len(src) if n is None else n, what, None)
        return rc, _ffi.last_error()

    for args, field in [(([0], [3]), "dst:"), (([-1], [1]), "src:"), (([0, 1], [1, 2]), "dst: member 1 is both"), (([0, 1], [2, 2]), "dst: member 2 is a destination twice"),
                        (([0], [1], 4), "what:"), (([0], [1], 0), "what:"), (([0], [1], 2), "rings:")]:
        rc, msg = clone(*args)
        assert rc == _ffi.GCRL_ERR_ARG and "gcrl_pop_clone: " + field in msg, (args, rc, msg)
    for n in (0, 17):
        rc, msg = clone([0] * 17, [1] * 17, n=n)
        assert rc == _ffi.GCRL_ERR_ARG and "gcrl_pop_clone: pairs:" in msg, msg
    small = gcrl.HERBuffer(300, 50, 2, rng="engine", seed=1)
    small._ensure(S, A, G)
    rings = (C.c_void_p * P)(pop.members[0].buffer.handle, pop.members[1].buffer.handle, small.handle)
    rc, msg = clone([0], [2], 3, rings)
    assert rc == _ffi.GCRL_ERR_ARG and "gcrl_pop_clone: capacity:" in msg, msg
    cfg = pop.members[1].config
    h = _ffi.HParams(actor_lr=-1.0, actor_lr_min=0.0, critic_lr=1e-3, critic_lr_min=0.0, ac_scheduler_steps=1, cr_scheduler_steps=1,
                     gamma=cfg.gamma, tau=cfg.tau, grad_clip=1.0)
    assert _ffi.lib.gcrl_agent_set_hparams(pop.members[1]._h, C.byref(h)) == _ffi.GCRL_ERR_ARG and "actor_lr:" in _ffi.last_error()
    from gcrl_amd.src.agent import KIND, native_config
    bad = native_config(KIND["DDPG"], S, A, _cfg("DDPG", 1), GSTEP, num_critics=1, seed=5)
    bad.hidden_dim = 128
    assert _ffi.lib.gcrl_pop_replace(pop._pop.h, 1, C.byref(bad)) == _ffi.GCRL_ERR_ARG and "gcrl_pop_replace: hidden_dim:" in _ffi.last_error()
    assert _ffi.lib.gcrl_pop_replace(pop._pop.h, 3, C.byref(bad)) == _ffi.GCRL_ERR_ARG and "gcrl_pop_replace: i:" in _ffi.last_error()
    for m, b in zip(pop.members, before):
        assert np.array_equal(_state(m), b)
