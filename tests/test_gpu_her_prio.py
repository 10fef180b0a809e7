"""GPU (-m gpu): the energy-prioritised replay draw of a sample-mode HER ring (HERBuffer(relabel="sample", prioritise="energy");
csrc/her_prio.hip) held to its numpy definition tests/her_energy_ref.py: the leaves a flush writes and the nodes above them, the
draw through the public sample and the engine's gather, the four agents on top of it, state and refusals.  Bit for bit where the
arithmetic is adds, multiplies, a divide and compares (alpha == 1); within 1e-6 relative of the fp64 evaluation where a powf enters."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import make_config

import her_energy_ref as E
import her_nstep_ref as NS
import her_relabel_ref as R
import per_tree_ref as PT
import test_gpu_her_relabel as T0
import test_her_energy_ref as host

pytestmark = pytest.mark.gpu

REACH, PICK, WIDE, THR = T0.REACH, T0.PICK, T0.WIDE, T0.THR
RINGS = dict(T0.RINGS, cap4160_three_levels=(REACH, host.CAP3, 84))
SIZES = T0.SIZES
bits, _np, _head, _episode = T0.bits, T0._np, T0._head, T0._episode


def _buffer(gcrl, cap, dims, k=4, rng="engine", seed=7, nenvs=4, prioritise="energy", energy=None, **kw):
    buf = gcrl.HERBuffer(cap, 50, nenvs, threshold=THR, k_future=k, rng=rng, seed=seed, relabel="sample", prioritise=prioritise,
                         energy=energy, **kw)
    buf.compute_reward = her_oracle.sparse_reward
    return buf


def _push(buf, ref, ep, env=0):
    buf.push_episode(env, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
    ref.flush([ep[6]])


def _check_tree(buf, ref, exact=True):
    """leaves against the restatement, nodes against per_tree_ref.build of the device's own leaves, never-filled slots 0"""
    levels = buf.tree_levels()
    leaves = levels[0]
    assert leaves.size == ref.leaves.size and (ref.head, ref.len) == (_head(buf), len(buf))
    if exact:
        assert np.array_equal(bits(leaves), bits(ref.leaves)), np.flatnonzero(bits(leaves) != bits(ref.leaves))[:8]
    else:
        filled = ref.leaves > 0
        assert not leaves[~filled].any()
        assert (np.abs(leaves[filled].astype(np.float64) / ref.leaves[filled] - 1.0) <= 1e-6).all()
    live = np.zeros(leaves.size, bool)
    live[(ref.head + np.arange(ref.len)) % ref.cap] = True
    assert not leaves[~live].any() and (leaves[live] > 0).all()
    built = PT.build(leaves)
    assert len(built) == len(levels)
    for k, (g, w) in enumerate(zip(levels, built)):
        assert np.array_equal(bits(g), bits(w)), f"level {k} is not the reduction of the device's own leaves"
    assert np.array_equal(bits(buf.get_priorities()), bits(leaves[(ref.head + np.arange(ref.len)) % ref.cap]))


# ---------------------------------------------------------------- 1. leaves and nodes
@pytest.mark.parametrize("alpha", [1.0, 0.6])
@pytest.mark.parametrize("ring", list(RINGS))
def test_leaves_and_nodes_after_every_push(gcrl, ring, alpha):
    dims, cap, episodes = RINGS[ring]
    buf = _buffer(gcrl, cap, dims, nenvs=2, energy=dict(alpha=alpha))
    ref = E.RefEnergyRing(cap, dims[2], seed=7, leaf_fn=E.leaf if alpha == 1.0 else E.leaf64, alpha=alpha)
    gen = np.random.default_rng(40)
    lengths = [1, 2, 50] + [50] * (episodes - 1)
    for i, T in enumerate(lengths):
        _push(buf, ref, _episode(gen, T, dims, T != 50), env=i % 2)
        _check_tree(buf, ref, exact=alpha == 1.0)
    assert len(buf.tree_levels()) == {60: 1, 120: 2, 300: 2, host.CAP3: 3}[cap]
    assert len(buf) == min(cap, sum(lengths)) and (sum(lengths) <= cap or _head(buf) != 0)
    assert buf.prio_counter == 0 and buf.relabel_counter == 0


def test_push_batch_several_episodes_share_one_flush_launch(gcrl):
    """4 envs end together (T = 2), twice, on a ring of 13 slots that wraps inside the second launch; then an episode longer than
    the ring: the flush skips its first rows and every written row still gets p_ep / T of the FULL episode"""
    from gcrl_amd._ffi import lib
    buf = _buffer(gcrl, 13, REACH)
    ref = E.RefEnergyRing(13, 3, seed=7)
    gen = np.random.default_rng(12)
    for rnd in range(2):
        eps = [_episode(gen, 2, REACH, True) for _ in range(4)]
        n0 = int(lib.gcrl_per_launches(buf.handle)) if rnd else 0
        for t in range(2):
            buf.push_batch(torch.from_numpy(np.stack([e[0][t] for e in eps])).cuda(), np.stack([e[1][t] for e in eps]),
                           torch.from_numpy(np.stack([e[2][t] for e in eps])).cuda(), np.array([e[3][t] for e in eps], np.float32),
                           np.array([t == 1] * 4), np.stack([e[6][t] for e in eps]))
        ref.flush([e[6] for e in eps])
        assert int(lib.gcrl_per_launches(buf.handle)) - n0 == 1, "one energy launch per flush launch"
        _check_tree(buf, ref)
    assert _head(buf) == 3
    _push(buf, ref, _episode(gen, 50, REACH, False))
    _check_tree(buf, ref)
    assert len(set(bits(buf.get_priorities()).tolist())) == 1       # 13 rows of one episode


def test_hand_made_goals(gcrl):
    buf = _buffer(gcrl, 200, REACH, nenvs=2)
    ref = E.RefEnergyRing(200, 3, seed=7)
    gen = np.random.default_rng(13)
    want = []
    for name in ("stationary", "clip", "nan", "inf"):
        ep = list(_episode(gen, 20, REACH, True))
        ag = np.repeat(ep[6][:1], 20, axis=0)
        if name == "clip":
            ag[7:, 2] += np.float32(10.0)
        elif name == "nan":
            ag[5, 1] = np.nan
        elif name == "inf":
            ag[3, 2], ag[9, 0] = np.inf, -np.inf
        ep[6] = ag
        _push(buf, ref, ep)
        want.append(E.leaf(ag, ref.cfg))
    _check_tree(buf, ref)
    got = buf.get_priorities()[::20]
    assert np.array_equal(bits(got), bits(np.array(want, np.float32)))
    eps, clip = ref.cfg["eps"], ref.cfg["clip"]
    assert bits(got[0]) == bits(np.float32(eps / np.float32(20))) and bits(got[1]) == bits(np.float32(np.float32(clip + eps) / np.float32(20)))
    assert np.isfinite(got).all() and (got > 0).all()


# ---------------------------------------------------------------- 2. draws
def _filled(gcrl, ring, seed, k=4, **kw):
    dims, cap, episodes = RINGS[ring]
    buf = _buffer(gcrl, cap, dims, k=k, seed=seed, nenvs=2, **kw)
    gen = np.random.default_rng(40)
    for e in range(episodes):
        ep = list(_episode(gen, 50, dims, False))
        if e % 3 == 2:
            ep[6] = np.repeat(ep[6][:1], 50, axis=0)                 # an object nobody moved
        buf.push_episode(e % 2, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
    return buf


@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("ring", list(RINGS))
def test_draws_and_gathers_bitwise_the_restatement(gcrl, ring, n_step):
    dims, cap, _ = RINGS[ring]
    S, A, G = dims
    seed, k, gamma = 1004, 4, 0.98
    buf = _filled(gcrl, ring, seed, k=k, **(dict(n_step=n_step, gamma=gamma) if n_step > 1 else {}))
    mt0 = T0._mt_state(buf)
    snap = T0._snapshot(buf)
    head, levels = snap[7], buf.tree_levels()
    assert len({float(x) for x in levels[0][levels[0] > 0]}) >= 2                # not a uniform draw
    pc = rc = 0
    for n in SIZES:
        for form in ("public", "engine", "engine_head"):
            B, M = (n, 1) if n <= len(buf) else (1, n)
            idx = E.draw(levels, seed, pc, n, head, cap)
            assert (idx < len(buf)).all() and (levels[0][(head + idx.astype(np.int64)) % cap] > 0).all()
            if n_step > 1:
                want = NS.gather(*snap[:7], head, cap, idx, rc, seed, k, R.SPARSE, THR, n_step, gamma)
            else:
                want = R.gather(*snap[:7], head, cap, idx, rc, seed, k, R.SPARSE, THR)
            if form == "public":
                out = buf.sample(B, M, return_indices=True)
                assert np.array_equal(out[5], idx), (n, "the tree drew other indices than the restated descent")
                got = dict(s=_np(out[0]), a=_np(out[1]), r=_np(out[2]).ravel(), ns=_np(out[3]), d=_np(out[4]).ravel())
                for key in ("s", "a", "r", "ns", "d"):
                    assert np.array_equal(bits(got[key]), bits(want[key])), (n, form, key)
            else:
                side = torch.arange(48, dtype=torch.uint8, device="cuda") if form == "engine_head" else None
                out = buf.gather_update(B, M, spa=True, side=side)
                sa, nsa, spa = T0._engine_form(want, dims)
                assert np.array_equal(bits(_np(out[0])), bits(sa)), (n, form, "sa")
                assert np.array_equal(bits(_np(out[1])), bits(nsa)), (n, form, "nsa")
                assert np.array_equal(bits(_np(out[2])[:, :spa.shape[1]]), bits(spa)), (n, form, "spa")
                assert np.array_equal(bits(_np(out[3])), bits(want["r"])) and np.array_equal(bits(_np(out[4])), bits(want["d"])), (n, form)
                if side is not None:
                    assert torch.equal(out[5], side), "side copy"
            pc += n
            rc += n
            assert buf.prio_counter == pc and buf.relabel_counter == rc, (n, form)
    assert T0._mt_state(buf) == mt0, "a tree draw consumed the MT stream"
    # indices= bypasses the draw
    given = np.random.default_rng(5).integers(0, len(buf), 17).astype(np.uint32)
    out = buf.sample(17, 1, indices=given)
    gather = NS.gather(*snap[:7], head, cap, given, rc, seed, k, R.SPARSE, THR, n_step, gamma) if n_step > 1 else \
        R.gather(*snap[:7], head, cap, given, rc, seed, k, R.SPARSE, THR)
    assert np.array_equal(bits(_np(out[0])), bits(gather["s"]))
    assert buf.prio_counter == pc and buf.relabel_counter == rc + 17


def test_sample_B_M_equals_M_samples_of_B(gcrl):
    a, b = (_filled(gcrl, "cap300_wrapped", 21) for _ in range(2))
    one = a.sample(17, 5, return_indices=True)
    parts = [b.sample(17, 1, return_indices=True) for _ in range(5)]
    assert np.array_equal(one[5], np.concatenate([p[5] for p in parts]))
    for j in range(5):
        assert np.array_equal(bits(_np(one[j])), bits(np.concatenate([_np(p[j]) for p in parts]))), j
    assert a.prio_counter == b.prio_counter == 85


def test_draw_frequencies_on_the_three_level_ring(gcrl):
    """the host test's ring and seed through the device: 2^18 rows in one launch, bit for bit the restated descent (so its
    frequencies are the host test's); no never-filled and no zero slot is drawn"""
    from gcrl_amd._ffi import check, lib
    gen = np.random.default_rng(6)
    buf = _buffer(gcrl, host.CAP3, REACH, seed=host.SEED, nenvs=2)
    ref = E.RefEnergyRing(host.CAP3, 3, seed=host.SEED)
    for e in range(84):
        ep = list(_episode(gen, 50, REACH, False))
        ep[6] = host.walk(gen, 50, still=gen.random() < 0.3)
        _push(buf, ref, ep, env=e % 2)
    _check_tree(buf, ref)
    n = 1 << 18
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    buf.prio_counter = (1 << 20) - 1000                               # the launch crosses a multiple of 2^20
    check(lib.gcrl_her_prio_draw(buf.handle, n, idx.data_ptr(), None))
    check(lib.gcrl_stream_synchronize(lib.gcrl_her_stream(buf.handle)))
    got = idx.cpu().numpy().astype(np.uint32)
    assert buf.prio_counter == (1 << 20) - 1000 + n
    levels = ref.levels()
    want = np.concatenate([E.draw(levels, host.SEED, (1 << 20) - 1000 + c0, 1 << 16, ref.head, ref.cap) for c0 in range(0, n, 1 << 16)])
    assert np.array_equal(got, want)
    assert (ref.leaves[(ref.head + got.astype(np.int64)) % ref.cap] > 0).all()


# ---------------------------------------------------------------- 3. agents
KINDS = {"DDPG": {}, "TD3": dict(ac_update_freq=2, policy_noise=0.2, noise_clamp=0.5), "SAC": dict(ac_update_freq=2), "TQC": dict(ac_update_freq=2)}


def _agent(gcrl, kind, seed, max_len=150, **kw):
    cfg = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=max_len, k_future=4, **KINDS[kind])
    cls = {"DDPG": gcrl.DDPG, "TD3": gcrl.TD3Agent, "SAC": gcrl.SACAgent, "TQC": gcrl.TQCAgent}[kind]
    return cls(REACH[0], REACH[1], cfg, None, nenvs=2, gradient_step=6, rng="engine", seed=seed, relabel="sample", **kw)


def _fill_agent(ag, seed, episodes=4):
    gen = np.random.default_rng(seed)
    for ep in range(episodes):
        still = ep == 1
        for st in her_oracle.synthetic_episode(gen, 50, REACH[0], REACH[1]):
            st = list(st)
            if still:
                st[6] = np.zeros_like(st[6]) + np.float32(0.5)
            ag.push_her(ep % 2, *st)


def _update_given(ag, step, idx):
    """one update of an agent WITHOUT the keyword on caller-given row indices: the engine's own launch forms, other rows"""
    from gcrl_amd import _ffi
    idx = np.ascontiguousarray(idx, np.uint32)
    ag.set_train()
    inputs = _ffi.UpdateInputs()
    inputs.idx_host = idx.ctypes.data
    ticket = C.c_int64(-1)
    n = _ffi.check(_ffi.lib.gcrl_agent_update(ag._h, ag.buffer.handle, int(step), C.byref(inputs), C.byref(ticket), _ffi.stream_handle()))
    ag.beta_scheduler(step)
    if ag._sac:
        ag.actor.num_batches_tracked += 1 + (1 if n == 9 else 0)
    return ag._tuple(ticket.value, n)


@pytest.mark.parametrize("kind,n_step", [("DDPG", 1), ("TD3", 3), ("SAC", 1), ("TQC", 1)])
def test_agents_equal_twin_fed_the_restated_batches(gcrl, kind, n_step):
    B, seed, steps = 64, 31, 3
    kw = dict(n_step=n_step) if n_step > 1 else {}
    ag, many = (_agent(gcrl, kind, seed, prioritise="energy", **kw) for _ in range(2))
    twin, given = (_agent(gcrl, kind, seed, **kw) for _ in range(2))
    for x in (ag, many, twin, given):
        _fill_agent(x, 50)                                           # 200 rows through a ring of 150: wrapped
        T0._perturb(x, 0)
    assert ag.buffer.prioritise == "energy" and twin.buffer.prioritise is None and len(ag.buffer) == 150 and _head(ag.buffer) == 50
    forms = (ag.rowchain_form(), ag.meetings())
    assert forms == (twin.rowchain_form(), twin.meetings())
    if kind == "DDPG":
        assert forms[0] != 0, "the DDPG case does not run the fused row-chain launches"
    snap = T0._snapshot(ag.buffer)
    levels, thr, gamma = ag.buffer.tree_levels(), ag.buffer._reward_cfg[1], ag.config.gamma
    assert len({float(x) for x in levels[0][levels[0] > 0]}) >= 2                # not a uniform draw
    mt0 = T0._mt_state(ag.buffer)
    got, want, want_idx = [], [], []
    for step in range(1, steps + 1):
        idx = E.draw(levels, seed, (step - 1) * B, B, snap[7], 150)
        if n_step > 1:
            b = NS.gather(*snap[:7], snap[7], 150, idx, (step - 1) * B, seed, 4, R.SPARSE, thr, n_step, gamma)
        else:
            b = R.gather(*snap[:7], snap[7], 150, idx, (step - 1) * B, seed, 4, R.SPARSE, thr)
        batch = tuple(torch.from_numpy(x).cuda() for x in (b["s"], b["a"], b["r"].reshape(-1, 1), b["ns"], b["d"].reshape(-1, 1)))
        got.append(ag.update(step))
        want_idx.append(_update_given(given, step, idx))
        if kind != "DDPG":                                           # (DDPG's injected batch takes the layer-per-launch schedule: other launch forms)
            want.append(twin.update(step, batch=batch))
    assert T0._mt_state(ag.buffer) == mt0, "an update call consumed the MT stream"
    assert (ag.rowchain_form(), ag.meetings()) == (given.rowchain_form(), given.meetings()) == forms, "the keyword changed a launch form"
    assert ag.buffer.prio_counter == ag.buffer.relabel_counter == steps * B
    g, w = T0._tuples(got), T0._tuples(want_idx)
    assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (g, w)
    assert np.array_equal(T0._state(ag), T0._state(given)), "engine state differs from the twin fed the restated indices"
    if kind != "DDPG":
        w = T0._tuples(want)
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (g, w)
        assert np.array_equal(T0._state(ag), T0._state(twin)), "engine state differs from the twin fed the restated batches"
    m = T0._tuples(many.update_many(1, steps))
    assert np.array_equal(m.view(np.uint64), g.view(np.uint64)), (m, g)
    assert np.array_equal(T0._state(many), T0._state(ag)), f"update_many(1, {steps}) is not {steps} x update()"
    assert many.buffer.prio_counter == steps * B and T0._mt_state(many.buffer) == mt0
    assert (many.rowchain_form(), many.meetings()) == forms
    if kind == "DDPG":                                               # the keyword matters: a uniform draw learns from other batches
        u = T0._tuples(twin.update_many(1, steps))
        assert not np.array_equal(u.view(np.uint64), m.view(np.uint64))


# ---------------------------------------------------------------- 4. resume
def test_buffer_resume_bitwise(gcrl, tmp_path):
    a = _filled(gcrl, "cap300_wrapped", 9)
    a.sample(17, 2)
    assert a.prio_counter == 34 and _head(a) == 50 and len(a) == 300
    meta = a.save_state(str(tmp_path / "ring.bin"))
    assert meta["prioritise"] == "energy" and len(meta["prio_leaves"]) == 300
    import json
    meta = json.loads(json.dumps(meta))
    b = _buffer(gcrl, 300, PICK, seed=9, nenvs=2)
    b.load_state(str(tmp_path / "ring.bin"), meta)
    assert b.prio_counter == 34 and b.relabel_counter == 34 and _head(b) == 50
    for x, y in zip(a.tree_levels(), b.tree_levels()):
        assert np.array_equal(bits(x), bits(y))
    gen_a, gen_b = np.random.default_rng(44), np.random.default_rng(44)
    for n in (16, 17, 33):
        if n == 17:                                                  # a flush after the resume lands on the same slots
            for buf, gen in ((a, gen_a), (b, gen_b)):
                ep = _episode(gen, 50, PICK, False)
                buf.push_episode(0, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
        ga, gb = a.sample(n, 1, return_indices=True), b.sample(n, 1, return_indices=True)
        assert np.array_equal(ga[5], gb[5])
        for x, y in zip(ga[:5], gb[:5]):
            assert np.array_equal(bits(_np(x)), bits(_np(y))), n
    for x, y in zip(a.tree_levels(), b.tree_levels()):
        assert np.array_equal(bits(x), bits(y))
    from gcrl_amd._ffi import GcrlError
    plain = _buffer(gcrl, 300, PICK, seed=9, nenvs=2, prioritise=None)
    with pytest.raises(GcrlError, match="prioritise"):
        plain.load_state(str(tmp_path / "ring.bin"), meta)
    plain = T0._buffer(gcrl, 300, PICK, seed=9, nenvs=2)
    T0._fill(plain, PICK, 1, 3)
    with pytest.raises(GcrlError, match="prioritise"):
        b.load_state(str(tmp_path / "p.bin"), plain.save_state(str(tmp_path / "p.bin")))
    other = _buffer(gcrl, 300, PICK, seed=9, nenvs=2, energy=dict(clip=0.25))
    with pytest.raises(GcrlError, match="prioritise"):
        other.load_state(str(tmp_path / "ring.bin"), meta)


def test_agent_resume_bitwise(gcrl, tmp_path):
    a, b = _agent(gcrl, "DDPG", 33, prioritise="energy"), _agent(gcrl, "DDPG", 33, prioritise="energy")
    _fill_agent(a, 51)
    T0._perturb(a, 1)
    a.update_many(1, 2)
    a.save_state(str(tmp_path / "ck"))
    b.load_state(str(tmp_path / "ck"))
    assert b.buffer.prio_counter == a.buffer.prio_counter == 128 and _head(b.buffer) == _head(a.buffer) == 50
    x, y = T0._tuples(a.update_many(3, 3)), T0._tuples(b.update_many(3, 3))
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert np.array_equal(T0._state(a), T0._state(b))
    plain = _agent(gcrl, "DDPG", 33)
    from gcrl_amd._ffi import GcrlError
    with pytest.raises(GcrlError, match="prioritise"):
        plain.load_state(str(tmp_path / "ck"))


# ---------------------------------------------------------------- 5. refusals
def test_refusals_name_their_field(gcrl):
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import GcrlError, lib
    H = lambda **kw: gcrl.HERBuffer(100, 50, 2, rng="engine", seed=1, **kw)
    with pytest.raises(GcrlError, match="prioritise"):
        H(relabel="push", prioritise="energy")
    with pytest.raises(GcrlError, match="prioritise"):
        H(relabel="sample", prioritise="td")
    with pytest.raises(GcrlError, match="prioritise"):
        H(relabel="sample", energy=dict(clip=1.0))
    for key, bad in (("clip", 0.0), ("clip", -1.0), ("eps", 0.0), ("alpha", -0.5), ("potential", float("nan")), ("kinetic", float("inf")),
                     ("eps", float("nan")), ("axis", 1.5), ("height", 2)):
        with pytest.raises(GcrlError, match=f"energy: .*{key}"):
            H(relabel="sample", prioritise="energy", energy={key: bad})
    buf = H(relabel="sample", prioritise="energy", energy=dict(axis=3))
    buf.compute_reward = her_oracle.sparse_reward
    ep = _episode(np.random.default_rng(1), 3, REACH, True)
    with pytest.raises(GcrlError, match="energy: axis"):
        buf.push_episode(0, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
    assert buf.handle is None                                        # refused before any device work
    for kind, cls in (("DDPG", gcrl.DDPG), ("TD3", gcrl.TD3Agent), ("SAC", gcrl.SACAgent), ("TQC", gcrl.TQCAgent)):
        A = lambda cfg, **kw: cls(REACH[0], REACH[1], cfg, None, nenvs=2, gradient_step=6, rng="engine", seed=1, **kw)
        her = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150)
        with pytest.raises(GcrlError, match="prioritise"):
            A(her, prioritise="energy")                              # relabel="push"
        with pytest.raises(GcrlError, match="prioritise"):
            A(her, relabel="sample", prioritise="tde")
        with pytest.raises(GcrlError, match="energy: clip"):
            A(her, relabel="sample", prioritise="energy", energy=dict(clip=0))
        for bt in ("REPLAY", "PER"):
            other = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150, buffer_type=bt)
            with pytest.raises(GcrlError, match="prioritise"):
                A(other, prioritise="energy")
        per = make_config(kind, hidden_dim=64, layer_count=3, batch_size=64, max_len=150, buffer_type="PER")
        with pytest.raises(GcrlError, match="prioritise: .*per_draw"):
            A(per, per_draw="device", prioritise="energy")
    for Pop in (gcrl.DDPGPopulation, gcrl.TD3Population, gcrl.SACPopulation, gcrl.TQCPopulation):
        cfgs = [make_config(Pop.AGENT.KIND_NAME, hidden_dim=64, layer_count=3, batch_size=64, max_len=150) for _ in range(2)]
        for kw in (dict(), dict(shared_ring=True)):
            with pytest.raises(GcrlError, match="prioritise"):
                Pop(REACH[0], REACH[1], cfgs, 2, 6, rng="engine", seeds=[5, 6], relabel="sample", prioritise="energy", **kw)
    # the native entries
    s = _filled(gcrl, "cap60_evicted_crossing", 3)
    with pytest.raises(GcrlError, match="relabel"):
        _ffi.check(lib.gcrl_per_attach(s.handle, 0.6, 1e-6))
    ecfg = _ffi.EnergyConfig(potential=9.81, kinetic=312.5, axis=2, clip=0.5, alpha=1.0, eps=1e-3)
    with pytest.raises(GcrlError, match="prioritise"):
        _ffi.check(lib.gcrl_her_prio_attach(s.handle, C.byref(ecfg)))            # a second tree
    assert lib.gcrl_her_prio_mode(s.handle) == 1
    idx = torch.empty(8, dtype=torch.int32, device="cuda")
    w = torch.empty(8, dtype=torch.float32, device="cuda")
    with pytest.raises(GcrlError, match="prioritise"):
        _ffi.check(lib.gcrl_per_draw(s.handle, 8, 0.4, idx.data_ptr(), w.data_ptr(), None))
    with pytest.raises(GcrlError, match="prioritise"):
        _ffi.check(lib.gcrl_per_update(s.handle, idx.data_ptr(), w.data_ptr(), 8, None))
    p = H(relabel="push")
    p.compute_reward = her_oracle.sparse_reward
    p.push_episode(0, ep[0], ep[1], ep[2], ep[3], ep[4], ep[6])
    with pytest.raises(GcrlError, match="prioritise"):
        _ffi.check(lib.gcrl_her_prio_attach(p.handle, C.byref(ecfg)))            # a push-mode ring
    assert lib.gcrl_her_prio_mode(p.handle) == 0 and lib.gcrl_her_get_prio_counter(p.handle) == 0
    with pytest.raises(GcrlError, match="prioritise"):
        _ffi.check(lib.gcrl_her_prio_draw(p.handle, 8, idx.data_ptr(), None))
    with pytest.raises(GcrlError, match="prioritise"):
        p.get_priorities()
    # a stale tree: the ring reloaded, its leaves not yet set
    plain = T0._buffer(gcrl, 60, REACH, seed=3, nenvs=2)
    late = T0._buffer(gcrl, 60, REACH, seed=3, nenvs=2)
    for b_ in (plain, late):
        T0._fill(b_, REACH, 2, 40)
    _ffi.check(lib.gcrl_her_prio_attach(late.handle, C.byref(ecfg)))             # after rows exist: the floor leaf everywhere
    leaves = np.empty(int(lib.gcrl_per_level_size(late.handle, 0)), np.float32)
    _ffi.check(lib.gcrl_per_read_level(late.handle, 0, leaves.ctypes.data, leaves.size))
    assert np.array_equal(bits(leaves[:60]), bits(np.full(60, 1e-3, np.float32))) and not leaves[60:].any()
    late.sample(8)                                                               # ... and can be drawn
    n = int(lib.gcrl_her_state_size(plain.handle))
    blob = np.empty(n, np.uint8)
    _ffi.check(lib.gcrl_her_save_state(plain.handle, blob.ctypes.data, n))
    _ffi.check(lib.gcrl_her_load_state(late.handle, blob.ctypes.data, n))
    with pytest.raises(GcrlError, match="prioritise"):
        _ffi.check(lib.gcrl_her_prio_draw(late.handle, 8, idx.data_ptr(), None))
    with pytest.raises(GcrlError, match="prioritise"):
        late.sample(8)
    # a population member's ring, and a population entry
    cfgs = [make_config("DDPG", hidden_dim=64, layer_count=3, batch_size=64, max_len=150, k_future=4) for _ in range(2)]
    pop = gcrl.DDPGPopulation(REACH[0], REACH[1], cfgs, 2, 6, rng="engine", seeds=[5, 6], relabel="sample")
    pop.members[1].buffer = gcrl.HERBuffer(150, 50, 2, k_future=4, rng="engine", seed=6, relabel="sample", prioritise="energy")
    for m in pop.members:
        T0._fill_agent(m, 90, episodes=2)
    with pytest.raises(GcrlError, match="prioritise"):
        pop.update_many(1, 2)
    with pytest.raises(GcrlError, match="prioritise"):
        pop.exploit([(0, 1)], copy_ring=True)


def test_agent_under_a_gradient_exchange_is_refused_before_anything_is_consumed(gcrl):
    """an in-engine exchange (world 1: one process) attached to an agent whose ring has the tree: update and update_many are refused
    naming `prioritise`, and neither a ticket nor a row of the draw stream is consumed — detached again, the agent goes on bit for
    bit like a twin that was never refused"""
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import GcrlError, lib
    ag, twin = _agent(gcrl, "DDPG", 37, prioritise="energy"), _agent(gcrl, "DDPG", 37, prioritise="energy")
    for x in (ag, twin):
        _fill_agent(x, 52)
        T0._perturb(x, 2)
    a0 = T0._tuples([ag.update(1)])
    b0 = T0._tuples([twin.update(1)])
    assert np.array_equal(a0.view(np.uint64), b0.view(np.uint64)) and ag.buffer.prio_counter == 64

    def ticket_of_next_update(x, step):
        t = C.c_int64(-1)
        x.set_train()
        _ffi.check(lib.gcrl_agent_update(x._h, x.buffer.handle, step, None, C.byref(t), _ffi.stream_handle()))
        return int(t.value)

    xh = _ffi.check_ptr(lib.gcrl_agent_xchg_create(ag._h, 0, 1), "gcrl_agent_xchg_create")
    try:
        _ffi.check(lib.gcrl_agent_set_exchange(ag._h, xh))
        mt0 = T0._mt_state(ag.buffer)
        with pytest.raises(GcrlError, match="prioritise"):
            ag.update(2)
        with pytest.raises(GcrlError, match="prioritise"):
            ag.update_many(2, 3)
        assert ag.buffer.prio_counter == 64 and ag.buffer.relabel_counter == 64 and T0._mt_state(ag.buffer) == mt0
    finally:
        _ffi.check(lib.gcrl_agent_set_exchange(ag._h, None))
        lib.gcrl_xchg_destroy(xh)
    assert ticket_of_next_update(ag, 2) == ticket_of_next_update(twin, 2), "a refused call consumed a ticket"
    assert ag.buffer.prio_counter == twin.buffer.prio_counter == 128
    x, y = T0._tuples(ag.update_many(3, 3)), T0._tuples(twin.update_many(3, 3))
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)) and np.array_equal(T0._state(ag), T0._state(twin))


def test_a_negative_axis_resumes_into_a_buffer_built_alike(gcrl, tmp_path):
    """every negative axis is the one setting "no potential term": saved as -1 and accepted by a buffer built with the same arguments"""
    kw = dict(energy=dict(axis=-3))
    a = _buffer(gcrl, 60, REACH, seed=3, nenvs=2, **kw)
    ref = E.RefEnergyRing(60, 3, seed=3, axis=-1)
    gen = np.random.default_rng(8)
    for _ in range(2):
        _push(a, ref, _episode(gen, 50, REACH, False))
    _check_tree(a, ref)
    meta = a.save_state(str(tmp_path / "ring.bin"))
    assert meta["energy"]["axis"] == -1
    b = _buffer(gcrl, 60, REACH, seed=3, nenvs=2, **kw)
    b.load_state(str(tmp_path / "ring.bin"), meta)
    assert np.array_equal(a.sample(17, 1, return_indices=True)[5], b.sample(17, 1, return_indices=True)[5])


# ---------------------------------------------------------------- 6. prioritise=None is the keyword left out
def test_prioritise_none_is_the_keyword_left_out(gcrl):
    from gcrl_amd._ffi import lib
    a, b = T0._buffer(gcrl, 60, REACH, seed=3, nenvs=2), _buffer(gcrl, 60, REACH, seed=3, nenvs=2, prioritise=None)
    for buf in (a, b):
        T0._fill(buf, REACH, 2, 40)
        assert lib.gcrl_per_attached(buf.handle) == 0 and lib.gcrl_per_launches(buf.handle) == -1 and lib.gcrl_her_prio_mode(buf.handle) == 0
    for n in (16, 17):
        ga, gb = a.sample(n, 1, return_indices=True), b.sample(n, 1, return_indices=True)
        assert np.array_equal(ga[5], gb[5])
        for x, y in zip(ga[:5], gb[:5]):
            assert np.array_equal(bits(_np(x)), bits(_np(y)))
    assert a.prio_counter == b.prio_counter == 0 and T0._mt_state(a) == T0._mt_state(b)
    x, y = _agent(gcrl, "DDPG", 33), _agent(gcrl, "DDPG", 33, prioritise=None)
    for ag in (x, y):
        _fill_agent(ag, 51)
        T0._perturb(ag, 1)
    assert (x.rowchain_form(), x.meetings()) == (y.rowchain_form(), y.meetings())
    u, v = T0._tuples(x.update_many(1, 3)), T0._tuples(y.update_many(1, 3))
    assert np.array_equal(u.view(np.uint64), v.view(np.uint64)) and np.array_equal(T0._state(x), T0._state(y))
    assert lib.gcrl_per_attached(y.buffer.handle) == 0
