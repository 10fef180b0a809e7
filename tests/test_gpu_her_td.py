"""GPU (-m gpu): TD-error prioritised replay on a sample-mode HER ring (HERBuffer(relabel="sample", prioritise="td_error");
csrc/her_td.hip) held to its numpy definition tests/her_td_ref.py: the leaves a flush seeds and the nodes above them, the update and
the p_max word, the draw, the four agents on top of it, state and refusals.

Bounds.  Adds, compares, fmaxf and the hash are held bit for bit; with alpha == 1 so is every leaf (one fp32 add).  With another
alpha a leaf is one fp32 add and one powf: 1e-6 relative against the fp64 evaluation from the device's own fp32 inputs, the bound of
tests/test_gpu_per_device.py.  p_max is then held bit for bit to the restated reduction of the device's own new leaves.

No case provokes a fault: the garbage inputs (indices >= cap, NaN, inf, poisoned neighbours) are chosen so that every address stays
inside its allocation by the kernels' own guards."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import make_config

import her_normalize_ref as NZ
import her_relabel_ref as RR
import her_td_ref as T
import per_tree_ref as R
import test_gpu_her_relabel as T0
import test_gpu_her_strategy as TS

pytestmark = pytest.mark.gpu

REACH, THR = T0.REACH, T0.THR
F32 = np.float32
bits, _np, _head, _episode = T0.bits, T0._np, T0._head, T0._episode
REL = 1e-6
SEED = 7


def _same(a, b):
    """bit for bit, NaN words aside (a NaN's payload is not the arithmetic's to fix)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _buffer(gcrl, cap, alpha=0.6, nenvs=8, seed=SEED, prioritise="td_error", **kw):
    td = dict(alpha=alpha, eps=1e-6) if prioritise == "td_error" else None
    buf = gcrl.HERBuffer(cap, 50, nenvs, threshold=THR, k_future=4, rng="engine", seed=seed, relabel="sample", prioritise=prioritise, td=td, **kw)
    buf.compute_reward = her_oracle.sparse_reward
    return buf


def _launches(buf):
    from gcrl_amd._ffi import lib
    return int(lib.gcrl_per_launches(buf.handle))


def _levels_or_empty(buf, cap):
    if buf.handle is None:
        return [np.zeros(p, F32) for _, p in R.level_sizes(cap)], T.P_MAX_INIT, 0, 0
    return buf.tree_levels(), buf.p_max, _head(buf), len(buf)


def _check_flush(buf, cap, push, total):
    """`push()` is ONE flush launch of `total` rows: afterwards every level is the restated seed on the device's previous levels"""
    prev, pm, head, length = _levels_or_empty(buf, cap)
    n0 = _launches(buf) if buf.handle is not None else 0
    push()
    assert _launches(buf) - n0 == 1, "one seed launch per flush launch"
    head, length, _ = T.book_append(head, length, cap, total)
    assert (head, length) == (_head(buf), len(buf))
    want = [x.copy() for x in prev]
    segs = T.seed(want, head, length, cap, total, pm)
    got = buf.tree_levels()
    for k, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), f"level {k} after a flush of {total} rows"
    R.check_invariant(got)
    assert bits(buf.p_max) == bits(pm), "a flush changed p_max"
    return segs


def _push_episode(buf, gen, T_rows, env=0):
    ep = _episode(gen, T_rows, REACH, T_rows != 50)
    buf.push_episode(env, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])


def _push_eight(buf, gen):
    """eight envs end together after three steps: eight episodes in one flush launch"""
    eps = [_episode(gen, 3, REACH, True) for _ in range(8)]
    for t in range(3):
        buf.push_batch(torch.from_numpy(np.stack([e[0][t] for e in eps])).cuda(), np.stack([e[1][t] for e in eps]),
                       torch.from_numpy(np.stack([e[2][t] for e in eps])).cuda(), np.array([e[3][t] for e in eps], F32),
                       np.array([t == 2] * 8), np.stack([e[6][t] for e in eps]))


# ---------------------------------------------------------------- 1. seed
@pytest.mark.parametrize("cap", [40, 60, 150])
def test_every_flush_seeds_p_max_and_recomputes_the_ancestors(gcrl, cap):
    buf = _buffer(gcrl, cap, alpha=1.0)
    gen = np.random.default_rng(cap)
    _check_flush(buf, cap, lambda: _push_episode(buf, gen, 50), 50)            # cap 40: a ring smaller than the flush (skip = 10)
    assert np.all(buf.get_priorities() == 1.0)
    buf.update_priorities(torch.tensor([0, 7, 3], dtype=torch.int32).cuda(), torch.tensor([0.5, -6.0, 2.0]).cuda())
    pm = F32(6.0) + F32(1e-6)
    assert bits(buf.p_max) == bits(pm)
    segs = _check_flush(buf, cap, lambda: _push_eight(buf, gen), 24)            # cap 60: evicting and crossing the ring's end
    if cap == 60:
        assert len(segs) == 2
    lv = buf.tree_levels()[0]
    for a, b in segs:
        assert np.all(bits(lv[a:b]) == bits(pm)), "new rows do not carry the raised p_max"
    _check_flush(buf, cap, lambda: _push_episode(buf, gen, 3, env=1), 3)
    _check_flush(buf, cap, lambda: _push_episode(buf, gen, 50), 50)
    assert len(buf.tree_levels()) == (1 if cap <= 64 else 2)


# ---------------------------------------------------------------- 2. update
def _filled(gcrl, cap, alpha, seed=SEED, rows=None):
    buf = _buffer(gcrl, cap, alpha=alpha, nenvs=2, seed=seed)
    gen = np.random.default_rng(100 + cap)
    rows = cap + 50 if rows is None else rows
    for e in range((rows + 49) // 50):
        _push_episode(buf, gen, 50, env=e % 2)
    return buf


def _update_poisoned(buf, idx, td):
    """the update reads idx[B] and td[B] and nothing beside them: both live inside larger tensors whose other words would show"""
    B = idx.size
    big_i = torch.full((B + 16,), -1, dtype=torch.int32).cuda()                # 0xFFFFFFFF: skipped if read as an index ...
    big_t = torch.full((B + 16,), 1e30, dtype=torch.float32).cuda()            # ... and a td that would own p_max
    big_i[8:8 + B] = torch.from_numpy(idx.astype(np.int64).astype(np.uint32).view(np.int32)).cuda()
    big_t[8:8 + B] = torch.from_numpy(td).cuda()
    buf.update_priorities(big_i[8:8 + B], big_t[8:8 + B])
    assert bool((big_i[:8] == -1).all()) and bool((big_i[8 + B:] == -1).all()) and bool((big_t[:8] == 1e30).all()) and bool((big_t[8 + B:] == 1e30).all())


def _check_update(buf, cap, alpha, idx, td):
    prev, pm, head = buf.tree_levels(), buf.p_max, _head(buf)
    n0 = _launches(buf)
    _update_poisoned(buf, idx, td)
    assert _launches(buf) - n0 == 1
    got = buf.tree_levels()
    want = [x.copy() for x in prev]
    want_pm = T.update(want, head, cap, idx, td, 1e-6, alpha, pm, device_leaves=got[0])
    for k, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), f"level {k} after an update of {idx.size} rows"
    assert bits(buf.p_max) == bits(want_pm) and want_pm >= pm and np.isfinite(buf.p_max)
    u = idx.astype(np.int64) & 0xFFFFFFFF
    keep = R.last_occurrence(u) & (u < cap)
    slots = (head + u[keep]) % cap
    new, ref32 = got[0][slots], T.new_values(td[keep], 1e-6, alpha)
    if alpha == 1.0:
        assert _same(new, ref32)
    fin = np.isfinite(ref32)
    want64 = R.priority64(td[keep][fin], 1e-6, alpha)
    assert np.all(np.abs(new[fin].astype(np.float64) - want64) <= REL * want64)
    assert _same(new[~fin], ref32[~fin])                                        # NaN and inf reach their leaves as the PER update writes them
    untouched = np.ones(got[0].size, bool)
    untouched[slots] = False
    assert np.array_equal(bits(got[0][untouched]), bits(prev[0][untouched]))
    return want_pm


@pytest.mark.parametrize("alpha", [1.0, 0.6])
def test_update_writes_the_leaves_raises_p_max_and_recomputes_the_ancestors(gcrl, alpha):
    cap = 4160
    buf = _filled(gcrl, cap, alpha)
    assert len(buf) == cap and _head(buf) == 90 and len(buf.tree_levels()) == 3
    gen = np.random.default_rng(3)
    _check_update(buf, cap, alpha, np.array([4000]), np.array([3.5], F32))                                        # B = 1
    idx = gen.integers(0, cap, 64)
    idx[32:] = idx[:32]                                                          # every index twice; the winners carry the larger |td|
    td = np.concatenate([gen.uniform(0.1, 1.0, 32), gen.uniform(2.0, 9.0, 32)]).astype(F32) * gen.choice([-1, 1], 64).astype(F32)
    _check_update(buf, cap, alpha, idx, td)
    edges = [0, 63, 64, 4095, 4159]                                              # leaves in different level-1 blocks and at their edges;
    idx = np.concatenate([edges, gen.permutation(np.setdiff1d(np.arange(cap), edges))[:295]])   # more rows than one pass of the ancestor stage's waves
    td = (gen.standard_normal(300) * 12).astype(F32)
    td[7] = F32(-0.0)
    pm = _check_update(buf, cap, alpha, idx, td)
    # an index >= cap between valid ones: skipped, and its td — the batch's largest — never reaches p_max
    idx = np.array([5, cap, 9, 2 ** 31 - 1, 2 ** 32 - 1, 11], np.int64)
    td = np.array([0.25, 1e6, 0.5, 1e6, 1e6, 0.125], F32)
    assert bits(_check_update(buf, cap, alpha, idx, td)) == bits(pm)
    # the next flush seeds the raised p_max
    _push_episode(buf, np.random.default_rng(4), 50)
    lv = buf.tree_levels()[0]
    assert np.all(bits(buf.get_priorities()[-50:]) == bits(pm)) and bits(lv.max()) == bits(pm)
    # NaN and inf in td: written to their leaves, never into p_max (last: the sums above them are NaN from here on)
    idx = np.array([20, 21, 22, 23], np.int64)
    td = np.array([np.nan, np.inf, -np.inf, 1.5], F32)
    assert bits(_check_update(buf, cap, alpha, idx, td)) == bits(pm)


def test_an_overwritten_occurrence_still_raises_p_max(gcrl):
    """the rule takes m over ALL rows of the batch: the first occurrence of a duplicated index holds the batch's largest |td|, a later
    one wins the leaf — alpha == 1, so p_max is bit for bit |td| + eps of the overwritten row while the leaf holds the later value"""
    cap = 150
    buf = _filled(gcrl, cap, 1.0)
    head = _head(buf)
    for B, dup_at, later_at in ((8, 0, 5), (64, 3, 63), (300, 17, 299)):
        gen = np.random.default_rng(B)
        idx = gen.permutation(cap)[:B] if B <= cap else np.concatenate([gen.permutation(cap), gen.permutation(cap)])[:B]
        idx = idx.astype(np.int64)
        idx[later_at] = idx[dup_at]
        td = gen.uniform(0.1, 1.0, B).astype(F32)
        big = F32(40.0 + B)
        td[dup_at] = -big                                                         # the batch maximum, on the occurrence that loses its leaf
        pm0 = buf.p_max
        assert big + F32(1e-6) > pm0
        pm = _check_update(buf, cap, 1.0, idx, td)
        assert bits(pm) == bits(big + F32(1e-6)) and bits(buf.p_max) == bits(big + F32(1e-6))
        leaf = buf.tree_levels()[0][(head + idx[dup_at]) % cap]
        assert bits(leaf) == bits(td[later_at] + F32(1e-6)) and leaf < 2.0
        assert bits(buf.tree_levels()[0].max()) != bits(buf.p_max), "p_max is no leaf of the tree here: only the overwritten row carried it"


# ---------------------------------------------------------------- 3. draw
@pytest.mark.parametrize("cap", [60, 150, 4160])
def test_draw_is_the_restated_descent_and_the_weights_formula(gcrl, cap):
    buf = _filled(gcrl, cap, 0.6)
    twin = T0._buffer(gcrl, cap, REACH, seed=SEED, nenvs=2)                     # the same rows, no tree
    gen = np.random.default_rng(100 + cap)
    for e in range((cap + 99) // 50):
        ep = _episode(gen, 50, REACH, False)
        twin.push_episode(e % 2, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
    gen = np.random.default_rng(cap)
    for o in range(0, cap, 256):                                                 # leaves over three decades
        n = min(256, cap - o)
        buf.update_priorities(torch.arange(o, o + n, dtype=torch.int32).cuda(),
                              torch.from_numpy(np.exp(gen.uniform(np.log(1e-3), np.log(30.0), n)).astype(F32)).cuda())
    levels, head = buf.tree_levels(), _head(buf)
    R.check_invariant(levels)
    total = R.reduce64(levels[-1])[0]
    from gcrl_amd import _ffi
    for B, counter, beta in ((1, 0, 0.4), (64, 12345, 0.7), (72, 2 ** 33 + 1, 1.0)):
        want_idx, want_p = R.draw(levels, SEED, counter, B, head, cap)
        want_w = R.weights64(want_p, total, cap, beta)
        assert np.array_equal(bits(levels[0][(head + want_idx.astype(np.int64)) % cap]), bits(want_p)) and np.all(want_p > 0)
        buf.draw_counter = counter                                               # the draw on its own (with replacement: B may exceed the rows)
        idx, w = torch.empty(B, dtype=torch.int32).cuda(), torch.empty(B, dtype=torch.float32).cuda()
        _ffi.check(_ffi.lib.gcrl_per_draw(buf.handle, B, beta, idx.data_ptr(), w.data_ptr(), _ffi.stream_handle()))
        assert np.array_equal(_np(idx).view(np.uint32), want_idx), (cap, B)
        w = _np(w)
        assert float(w.max()) == 1.0 and np.all(np.abs(w.astype(np.float64) - want_w) <= REL * want_w)
        if B > cap:
            continue
        buf.draw_counter = counter                                               # sample(): the same draw, gathered
        c0 = buf.relabel_counter
        out = buf.sample(B, return_indices=True, beta=beta)
        assert len(out) == 7 and buf.draw_counter == counter + 1 and buf.relabel_counter == c0 + B
        assert np.array_equal(out[5], want_idx) and out[6].shape == (B,) and np.array_equal(bits(_np(out[6])), bits(w))
        twin.relabel_counter = c0                                                # the ring's own relabelling gather of those rows
        ref = twin.sample(B, indices=want_idx)
        for x, y in zip(out[:5], ref):
            assert np.array_equal(bits(_np(x)), bits(_np(y)))
    two = buf.sample(16, 2, return_indices=True, beta=0.5)                       # two batches: two draws, weights normalised per batch
    assert buf.draw_counter == 2 ** 33 + 4 and two[5].shape == (32,) and float(two[6][:16].max()) == float(two[6][16:].max()) == 1.0


# ---------------------------------------------------------------- 4. agents
KINDS = TS.KINDS
CLS = {"DDPG": "DDPG", "TD3": "TD3Agent", "SAC": "SACAgent", "TQC": "TQCAgent"}


def _agent(gcrl, kind, seed=31, **kw):
    cfg = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150, k_future=4, alpha=0.6, beta=0.4, beta_end=50, **KINDS[kind])
    return getattr(gcrl, CLS[kind])(REACH[0], REACH[1], cfg, None, nenvs=2, gradient_step=6, rng="engine", seed=seed, relabel="sample", **kw)


def _fill_agent(ag, seed, episodes=4):
    gen = np.random.default_rng(seed)
    for ep in range(episodes):
        for st in her_oracle.synthetic_episode(gen, 50, REACH[0], REACH[1]):
            ag.push_her(ep % 2, *st)


def _ready(ag, seed=50):
    _fill_agent(ag, seed)                                                        # 200 rows through a ring of 150: wrapped, head = 50
    T0._perturb(ag, 0)
    return ag


def _scalars(ag, outs):
    """the tuples of update calls without td_error (an array here, a mean on a twin)"""
    rows = []
    for t in outs:
        k = ag.TD_INDEX[len(t)]
        rows.append([float(len(t))] + [float(x) for i, x in enumerate(t) if i != k] + [0.0] * (9 - len(t)))
    return np.array(rows, np.float64).view(np.uint64)


def _get(ag, name, n):
    from gcrl_amd._ffi import check, lib
    v = np.empty(n, F32)
    check(lib.gcrl_agent_get(ag._h, name, v.ctypes.data, n))
    return v


@pytest.mark.parametrize("kind", ["DDPG", "TD3", "SAC", "TQC"])
def test_agent_step_equals_a_twin_fed_the_drawn_indices_and_weights(gcrl, kind):
    from gcrl_amd import _ffi
    lib = _ffi.lib
    dev, twin = _ready(_agent(gcrl, kind, prioritise="td_error")), _ready(_agent(gcrl, kind, pipeline=0))
    assert dev.buffer.prioritise == "td_error" and dev.td == dict(alpha=float(F32(0.6)), eps=float(F32(1e-6))) and lib.gcrl_her_prio_mode(dev.buffer.handle) == 2
    assert len(dev.buffer) == 150 and _head(dev.buffer) == 50 and np.array_equal(T0._state(dev), T0._state(twin))
    mt0 = T0._mt_state(dev.buffer)
    for step in (1, 2):
        levels, pm = dev.buffer.tree_levels(), dev.buffer.p_max
        n0 = _launches(dev.buffer)
        info = dev.update(step)
        assert _launches(dev.buffer) - n0 == 3                                   # draw, weights, update
        idx, w = dev.drawn_indices(1)[0], _get(dev, b"w_in", 64)
        want_idx, want_p = R.draw(levels, 31, step - 1, 64, 50, 150)
        assert np.array_equal(idx, want_idx) and float(w.max()) == 1.0 and np.all(w > 0)
        want_w = R.weights64(want_p, R.reduce64(levels[-1])[0], 150, 0.4 if step == 1 else 0.4 + 0.6 / 50)
        assert np.all(np.abs(w.astype(np.float64) - want_w) <= REL * want_w)
        twin.set_train()
        inputs = _ffi.UpdateInputs()
        inputs.idx_host, inputs.weights_host = idx.ctypes.data, w.ctypes.data
        ticket = C.c_int64(-1)
        n = _ffi.check(lib.gcrl_agent_update(twin._h, twin.buffer.handle, step, C.byref(inputs), C.byref(ticket), _ffi.stream_handle()))
        assert n == len(info)
        assert np.array_equal(_scalars(dev, [info]), _scalars(dev, [twin._tuple(ticket.value, n)]))
        assert np.array_equal(T0._state(dev), T0._state(twin)), "engine state differs from the twin fed the drawn indices and weights"
        td = np.asarray(info[dev.TD_INDEX[n]])
        assert td.shape == (64, 1) and np.array_equal(bits(td[:, 0]), bits(_get(dev, b"td_abs", 64))) and np.array_equal(bits(td[:, 0]), bits(_get(twin, b"td_abs", 64)))
        # the tree followed on the device: the restated update of this step's td on the previous levels, p_max included
        got = dev.buffer.tree_levels()
        want_pm = T.update(levels, 50, 150, idx, td[:, 0], 1e-6, 0.6, pm, device_leaves=got[0])
        for g, x in zip(got, levels):
            assert _same(g, x)
        keep = R.last_occurrence(idx)
        want = R.priority64(td[keep, 0], 1e-6, 0.6)
        assert np.all(np.abs(got[0][(50 + idx[keep].astype(np.int64)) % 150].astype(np.float64) - want) <= REL * want)
        all64 = R.priority64(td[:, 0], 1e-6, 0.6).max()
        assert dev.buffer.p_max >= pm and abs(float(dev.buffer.p_max) - max(float(pm), all64)) <= REL * max(float(pm), all64)
        if keep.all() or np.argmax(np.abs(td[:, 0])) in np.flatnonzero(keep):     # (the largest |td| won its leaf: the device's own value)
            assert bits(dev.buffer.p_max) == bits(want_pm)
    assert dev.buffer.relabel_counter == twin.buffer.relabel_counter == 128 and dev.buffer.draw_counter == 2
    assert T0._mt_state(dev.buffer) == mt0, "an update call consumed the MT stream"


def test_update_many_is_one_call_equal_to_single_updates_and_new_rows_enter_at_p_max(gcrl):
    many, single = (_ready(_agent(gcrl, "TD3", prioritise="td_error")) for _ in range(2))
    outs = many.update_many(1, 5)
    assert len(outs) == 5 and many.beta == pytest.approx(0.4 + (5 / 50) * 0.6)
    idx_many = many.drawn_indices(5)
    idx_single, outs_single = [], []
    for i in range(5):
        o = single.update(1 + i)
        idx_single.append(single.drawn_indices(1)[0])
        outs_single.append(o)
    assert np.array_equal(idx_many, np.stack(idx_single))
    assert np.array_equal(_scalars(many, outs), _scalars(single, outs_single))
    assert np.array_equal(T0._state(many), T0._state(single))
    for a, b in zip(many.buffer.tree_levels(), single.buffer.tree_levels()):
        assert np.array_equal(bits(a), bits(b))
    assert bits(many.buffer.p_max) == bits(single.buffer.p_max) and many.buffer.draw_counter == single.buffer.draw_counter == 5
    assert many.buffer.relabel_counter == single.buffer.relabel_counter == 5 * 64 and many.beta == single.beta
    td = np.asarray(outs[4][many.TD_INDEX[len(outs[4])]])
    assert td.shape == (64, 1) and np.array_equal(bits(td), bits(np.asarray(outs_single[4][single.TD_INDEX[len(outs_single[4])]])))
    # pushes between calls: the new rows carry p_max — the largest leaf of the tree — and are drawn
    pm = many.buffer.p_max
    gen = np.random.default_rng(77)
    for st in her_oracle.synthetic_episode(gen, 50, REACH[0], REACH[1]):
        many.push_her(0, *st)
    pr = many.buffer.get_priorities()
    assert np.all(bits(pr[-50:]) == bits(pm)) and bits(pr.max()) == bits(pm) and bits(many.buffer.p_max) == bits(pm)
    many.update_many(6, 2)
    drawn = many.drawn_indices(2)
    assert (drawn >= 100).sum() >= 2 * 64 * 50 // 150 // 2, "the new rows are drawn less than half as often as uniformly"


def _ref_batch(ag, idx, counter, nz_obs=None, **rule):
    snap = TS._snapshot(ag.buffer)
    return NZ.gather(*snap[:8], snap[8], snap[9], idx, counter, 31, 4, RR.SPARSE, ag.buffer._reward_cfg[1], 7, nz_obs, None, **rule)


@pytest.mark.parametrize("case", ["n_step", "episode", "normalize"])
def test_a_drawn_batch_is_the_rings_own_gather_of_the_drawn_rows(gcrl, case):
    """n_step=3, goal_strategy="episode" and normalize="sample": the batch of a step is the reference gather on the drawn indices at
    the ring's relabel counter"""
    import test_gpu_her_normalize as TN
    kw = dict(n_step=dict(n_step=3), episode=dict(goal_strategy="episode"), normalize=dict(normalize="sample"))[case]
    ag = _agent(gcrl, "DDPG", prioritise="td_error", **kw)
    oracle = None
    if case == "normalize":
        z, oracle = TN._pair(7, "created", 21)
        ag.buffer.obs_normalizer = z
    _ready(ag)
    for step in (1, 2):
        levels = ag.buffer.tree_levels()
        snap_ctr = ag.buffer.relabel_counter
        assert snap_ctr == (step - 1) * 64
        ag.update(step)
        idx = ag.drawn_indices(1)[0]
        assert np.array_equal(idx, R.draw(levels, 31, step - 1, 64, 50, 150)[0])
        rule = dict(n_step=dict(n_step=3, gamma=ag.config.gamma), episode=dict(strategy="episode"), normalize={})[case]
        want = _ref_batch(ag, idx, snap_ctr, oracle, **rule)
        sa, nsa, r, d = ag.read_batch(0)
        S, A = REACH[0], REACH[1]
        assert np.array_equal(bits(sa[:, :S]), bits(want["s"])) and np.array_equal(bits(sa[:, S:S + A]), bits(want["a"]))
        assert np.array_equal(bits(nsa[:, :S]), bits(want["ns"])) and np.array_equal(bits(r), bits(want["r"])) and np.array_equal(bits(d), bits(want["d"]))
        assert (want["o"] != 0).any() and (want["o"] == 0).any()                 # relabelled and original rows in one batch


# ---------------------------------------------------------------- 5. resume
def test_agent_resume_is_bitwise(gcrl, tmp_path):
    ref, first = (_ready(_agent(gcrl, "TD3", prioritise="td_error")) for _ in range(2))
    ref_outs = ref.update_many(1, 3) + ref.update_many(4, 3)
    first.update_many(1, 3)
    first.save_state(str(tmp_path / "ck"))
    meta = json.load(open(tmp_path / "ck" / "meta.json"))["ring"]
    assert meta["prioritise"] == "td_error" and len(meta["prio_leaves"]) == 150 and meta["td_draw_counter"] == 3 and meta["prio_head"] == 50
    assert meta["td_pmax"] == int(bits(first.buffer.p_max)[0]) and meta["td"] == first.td
    resumed = _agent(gcrl, "TD3", prioritise="td_error")
    resumed.load_state(str(tmp_path / "ck"))
    assert resumed.buffer.draw_counter == 3 and _head(resumed.buffer) == 50 and resumed.beta == first.beta
    assert bits(resumed.buffer.p_max) == bits(first.buffer.p_max) and resumed.buffer.relabel_counter == 3 * 64
    for a, b in zip(resumed.buffer.tree_levels(), first.buffer.tree_levels()):
        assert np.array_equal(bits(a), bits(b))
    outs = resumed.update_many(4, 3)
    assert np.array_equal(_scalars(ref, ref_outs[3:]), _scalars(resumed, outs))
    assert np.array_equal(ref.drawn_indices(3), resumed.drawn_indices(3))
    assert np.array_equal(T0._state(ref), T0._state(resumed))
    for a, b in zip(resumed.buffer.tree_levels(), ref.buffer.tree_levels()):
        assert np.array_equal(bits(a), bits(b))
    assert bits(resumed.buffer.p_max) == bits(ref.buffer.p_max)
    # loading across settings is refused by the field's name before anything is overwritten
    from gcrl_amd._ffi import GcrlError
    for other in (_agent(gcrl, "TD3"), _agent(gcrl, "TD3", prioritise="energy"), _agent(gcrl, "TD3", prioritise="td_error", td=dict(alpha=0.5)),
                  _agent(gcrl, "TD3", prioritise="td_error", td=dict(eps=1e-5))):
        before = T0._state(other)
        with pytest.raises(GcrlError, match="prioritise"):
            other.load_state(str(tmp_path / "ck"))
        assert np.array_equal(T0._state(other), before)
    plain = _ready(_agent(gcrl, "TD3"))
    plain.save_state(str(tmp_path / "plain"))
    before = T0._state(resumed)
    with pytest.raises(GcrlError, match="prioritise"):
        resumed.load_state(str(tmp_path / "plain"))
    assert np.array_equal(T0._state(resumed), before)


# ---------------------------------------------------------------- 6. refusals
def test_native_refusals_name_prioritise_and_the_pinned_ones_stay(gcrl):
    from gcrl_amd import _ffi
    lib, err = _ffi.lib, _ffi.last_error
    gen = np.random.default_rng(1)
    push = gcrl.HERBuffer(2000, 50, 2, threshold=THR, rng="engine", seed=1)
    push.compute_reward = her_oracle.sparse_reward
    _push_episode(push, gen, 50)
    assert lib.gcrl_her_td_attach(push.handle, 0.6, 1e-6) < 0 and "prioritise" in err() and lib.gcrl_per_attached(push.handle) == 0
    plain = T0._buffer(gcrl, 150, REACH, nenvs=2)
    _push_episode(plain, gen, 50)
    for alpha, eps in ((-0.1, 1e-6), (float("nan"), 1e-6), (float("inf"), 1e-6), (0.6, 0.0), (0.6, -1.0), (0.6, float("nan")), (0.6, float("inf"))):
        assert lib.gcrl_her_td_attach(plain.handle, alpha, eps) < 0 and "prioritise" in err(), (alpha, eps)
    assert lib.gcrl_per_attached(plain.handle) == 0 and lib.gcrl_her_prio_mode(plain.handle) == 0
    _ffi.check(lib.gcrl_her_td_attach(plain.handle, 0.6, 1e-6))                  # after rows exist: p_max's initial value everywhere
    assert lib.gcrl_her_prio_mode(plain.handle) == 2
    lv = [np.empty(int(lib.gcrl_per_level_size(plain.handle, k)), F32) for k in range(int(lib.gcrl_per_levels(plain.handle)))]
    for k, a in enumerate(lv):
        _ffi.check(lib.gcrl_per_read_level(plain.handle, k, a.ctypes.data, a.size))
    assert np.all(lv[0][:50] == 1.0) and not lv[0][50:].any()
    R.check_invariant(lv)
    assert lib.gcrl_her_td_attach(plain.handle, 0.6, 1e-6) < 0 and "prioritise" in err()          # a second tree
    ecfg = _ffi.EnergyConfig(potential=9.81, kinetic=312.5, axis=2, clip=0.5, alpha=1.0, eps=1e-3)
    assert lib.gcrl_her_prio_attach(plain.handle, C.byref(ecfg)) < 0 and "prioritise" in err()
    assert lib.gcrl_per_attach(plain.handle, 0.6, 1e-6) < 0 and "relabel" in err()                 # pinned: stays refused, naming relabel
    energy = _buffer(gcrl, 150, prioritise="energy", nenvs=2)
    _push_episode(energy, gen, 50)
    assert lib.gcrl_her_td_attach(energy.handle, 0.6, 1e-6) < 0 and "prioritise" in err()
    with pytest.raises(_ffi.GcrlError, match="prioritise"):                      # the new write path is the TD tree's: an energy tree's leaves stay the flush's
        energy.set_priorities(np.ones(50, F32))
    out = C.c_float(0)
    assert lib.gcrl_her_td_get_pmax(energy.handle, C.byref(out)) < 0 and "prioritise" in err()
    assert lib.gcrl_her_td_set_pmax(plain.handle, float("nan")) < 0 and lib.gcrl_her_td_set_pmax(plain.handle, 0.0) < 0
    _ffi.check(lib.gcrl_her_td_get_pmax(plain.handle, C.byref(out)))
    assert out.value == 1.0


def test_python_and_engine_refusals_consume_nothing(gcrl):
    from gcrl_amd import _ffi
    from gcrl_amd.src.dp import DataParallelUpdater
    err = _ffi.GcrlError
    lib = _ffi.lib
    S, A = REACH[0], REACH[1]
    with pytest.raises(err, match="prioritise"):
        gcrl.TD3Agent(S, A, make_config("TD3", batch_size=64), None, nenvs=2, gradient_step=4, relabel="push", prioritise="td_error")
    with pytest.raises(err, match="prioritise"):
        gcrl.TD3Agent(S, A, make_config("TD3", batch_size=64, buffer_type="PER", max_len=500), None, nenvs=2, gradient_step=4, prioritise="td_error")
    with pytest.raises(err, match="prioritise"):
        gcrl.TD3Agent(S, A, make_config("TD3", batch_size=64, buffer_type="PER", max_len=500), None, nenvs=2, gradient_step=4, per_draw="device",
                      prioritise="td_error")
    with pytest.raises(err, match="prioritise"):
        gcrl.TQCAgent(S, A, make_config("TQC", batch_size=64, max_len=500), None, nenvs=2, gradient_step=4, relabel="sample", n_quantiles=25,
                      prioritise="td_error")
    prior = gcrl.HERBuffer(500, 50, 2, threshold=THR, rng="device", seed=3, relabel="sample")
    prior.compute_reward = her_oracle.sparse_reward
    _push_episode(prior, np.random.default_rng(2), 50)
    for kw in (dict(prior_buffer=prior, prior_rows=8), dict(prior_buffer=prior, prior_rows=8, bc_weight=1.0)):
        with pytest.raises(err, match="prioritise"):
            _agent(gcrl, "TD3", prioritise="td_error", **kw)
    for bad in ("td", "tde"):
        with pytest.raises(err, match="prioritise"):
            _agent(gcrl, "TD3", prioritise=bad)
    with pytest.raises(err, match="prioritise"):
        gcrl.DDPGPopulation(S, A, [make_config("DDPG", batch_size=64)] * 2, nenvs=1, gradient_step=4, prioritise="td_error")
    dev, twin = (_ready(_agent(gcrl, "TD3", prioritise="td_error")) for _ in range(2))
    with pytest.raises(err, match="prioritise"):
        DataParallelUpdater(dev)
    # the engine: a prior ring bound behind Python's back is refused before a ticket, slot, draw or relabel counter is consumed
    dev.update(1); twin.update(1)
    before = (dev.buffer.draw_counter, dev.buffer.relabel_counter, dev.beta, _launches(dev.buffer), T0._state(dev).tobytes())
    _ffi.check(lib.gcrl_agent_set_prior(dev._h, prior.handle, 8))
    for call in (lambda: dev.update(2), lambda: dev.update_many(2, 3)):
        with pytest.raises(err, match="prioritise"):
            call()
    _ffi.check(lib.gcrl_agent_set_prior(dev._h, None, 0))
    # entries that do not run the per-step loop refuse the ring
    t = C.c_int64(-1)
    assert lib.gcrl_agent_update_phase(dev._h, dev.buffer.handle, 2, 0, None, 1.0, C.byref(t), _ffi.stream_handle()) < 0
    assert "prioritise" in _ffi.last_error() and "td_error" in _ffi.last_error()
    # the buffer's gather without indices would be a uniform draw passing for a prioritised one: refused, nothing consumed
    mt0 = T0._mt_state(dev.buffer)
    with pytest.raises(err, match="prioritise"):
        dev.buffer.gather_update(16)
    out = [torch.empty((16, n), dtype=torch.float32).cuda() for n in (S, A, 1, S, 1)]
    assert lib.gcrl_her_sample(dev.buffer.handle, 16, 1, None, out[0].data_ptr(), S, out[1].data_ptr(), A, out[2].data_ptr(), out[3].data_ptr(), S,
                               out[4].data_ptr(), None, _ffi.stream_handle()) < 0 and "prioritise" in _ffi.last_error()
    assert T0._mt_state(dev.buffer) == mt0
    dev.buffer.gather_update(16, indices=np.arange(16))                          # (given indices: served, one relabel row each)
    dev.buffer.relabel_counter -= 16
    assert before == (dev.buffer.draw_counter, dev.buffer.relabel_counter, dev.beta, _launches(dev.buffer), T0._state(dev).tobytes())
    a, b = dev.update_many(2, 3), twin.update_many(2, 3)
    assert np.array_equal(_scalars(dev, a), _scalars(twin, b)) and np.array_equal(T0._state(dev), T0._state(twin))
    assert np.array_equal(dev.drawn_indices(3), twin.drawn_indices(3)) and bits(dev.buffer.p_max) == bits(twin.buffer.p_max)


def _snap(ag):
    return (ag.buffer.draw_counter, ag.buffer.relabel_counter, ag.beta, _launches(ag.buffer), bits(ag.buffer.p_max).tobytes(),
            T0._mt_state(ag.buffer), T0._state(ag).tobytes())


def test_engine_refusals_name_prioritise_and_consume_nothing(gcrl):
    """what the update engine refuses on a ring with a TD-error tree — a gradient exchange, the behaviour-cloning term, a population
    entry, a clone of the ring — each set up behind Python's back, each named `prioritise`, each before a ticket, slot, draw or relabel
    counter is consumed: afterwards the agent goes on bit for bit like a twin that was never refused, ticket numbers included"""
    from gcrl_amd import _ffi
    lib, err = _ffi.lib, _ffi.GcrlError
    dev, twin = (_ready(_agent(gcrl, "DDPG", prioritise="td_error")) for _ in range(2))
    a0, b0 = dev.update(1), twin.update(1)
    assert a0[0]._ticket == b0[0]._ticket and np.array_equal(T0._state(dev), T0._state(twin))
    before = _snap(dev)
    calls = (lambda: dev.update(2), lambda: dev.update_many(2, 3))
    # a gradient exchange (world 1: one process)
    xh = _ffi.check_ptr(lib.gcrl_agent_xchg_create(dev._h, 0, 1), "gcrl_agent_xchg_create")
    try:
        _ffi.check(lib.gcrl_agent_set_exchange(dev._h, xh))
        for call in calls:
            with pytest.raises(err, match="prioritise"):
                call()
    finally:
        _ffi.check(lib.gcrl_agent_set_exchange(dev._h, None))
        lib.gcrl_xchg_destroy(xh)
    assert _snap(dev) == before, "a call refused under a gradient exchange consumed something"
    # the behaviour-cloning term
    _ffi.check(lib.gcrl_agent_set_bc(dev._h, 1.0, 1, 8))
    try:
        for call in calls:
            with pytest.raises(err, match="prioritise"):
                call()
    finally:
        _ffi.check(lib.gcrl_agent_set_bc(dev._h, 0.0, 0, 0))
    assert _snap(dev) == before, "a call refused for bc_weight consumed something"
    # a population member's ring, through the population's update and clone entries
    cfgs = [make_config("DDPG", hidden_dim=64, layer_count=3, batch_size=64, max_len=150, k_future=4) for _ in range(2)]
    pop = gcrl.DDPGPopulation(REACH[0], REACH[1], cfgs, 2, 6, rng="engine", seeds=[5, 6], relabel="sample")
    pop.members[1].buffer = _buffer(gcrl, 150, nenvs=2, seed=6)
    for m in pop.members:
        T0._fill_agent(m, 90, episodes=2)
    ring = pop.members[1].buffer
    ring_before = (ring.draw_counter, ring.relabel_counter, _launches(ring), bits(ring.p_max).tobytes(), T0._mt_state(ring),
                   pop.members[0].buffer.relabel_counter, T0._mt_state(pop.members[0].buffer), [T0._state(m).tobytes() for m in pop.members])
    with pytest.raises(err, match="prioritise"):
        pop.update_many(1, 2)
    with pytest.raises(err, match="prioritise"):
        pop.exploit([(0, 1)], copy_ring=True)
    with pytest.raises(err, match="prioritise"):
        pop.exploit([(1, 0)], copy_ring=True)
    assert ring_before == (ring.draw_counter, ring.relabel_counter, _launches(ring), bits(ring.p_max).tobytes(), T0._mt_state(ring),
                           pop.members[0].buffer.relabel_counter, T0._mt_state(pop.members[0].buffer), [T0._state(m).tobytes() for m in pop.members])
    # never refused: the twin and the agent go on alike, ticket for ticket
    a, b = dev.update(2), twin.update(2)
    assert a[0]._ticket == b[0]._ticket == a0[0]._ticket + 1, "a refused call consumed a ticket"
    a, b = [a] + dev.update_many(3, 3), [b] + twin.update_many(3, 3)
    assert np.array_equal(_scalars(dev, a), _scalars(twin, b)) and np.array_equal(T0._state(dev), T0._state(twin))
    assert np.array_equal(dev.drawn_indices(3), twin.drawn_indices(3)) and _snap(dev) == _snap(twin)


def test_prioritise_none_is_the_keyword_left_out(gcrl):
    from gcrl_amd._ffi import lib
    a, b = _ready(_agent(gcrl, "DDPG", prioritise=None, td=None)), _ready(_agent(gcrl, "DDPG"))
    x, y = T0._tuples(a.update_many(1, 3)), T0._tuples(b.update_many(1, 3))
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)) and np.array_equal(T0._state(a), T0._state(b))
    for ag in (a, b):
        assert lib.gcrl_per_attached(ag.buffer.handle) == 0 and lib.gcrl_per_launches(ag.buffer.handle) == -1 and lib.gcrl_her_prio_mode(ag.buffer.handle) == 0
    assert a.rowchain_form() == b.rowchain_form() != 0 and a.buffer.relabel_counter == b.buffer.relabel_counter
    with pytest.raises(gcrl._ffi.GcrlError, match="prioritise"):
        a.buffer.p_max
    with pytest.raises(gcrl._ffi.GcrlError, match="prioritise"):
        a.buffer.sample(16, beta=0.5)
