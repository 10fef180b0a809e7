"""GPU (-m gpu): Q-filtered behaviour cloning on the prior rows of a batch (bc_weight= / q_filter=; csrc/her_bc.hip) held to its
numpy definition tests/her_bc_ref.py: the kernel alone bit for bit, the engine's wiring on DDPG and TD3 against torch autograd of the
full loss and a twin without the term, the call forms, the path through the rings, the refusals and the saved state."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.agent_oracle import make_config

import her_bc_ref as BC
import test_gpu_her_prior as TP
import test_gpu_her_relabel as T
from test_gpu_her_relabel import REACH, bits

pytestmark = pytest.mark.gpu

F32 = np.float32
S, A = REACH[0], REACH[1]
RTOL, ATOL = 1e-5, 1e-6          # tests/test_gpu_parity.py: fp32 gradients, vec_close
TD3_KW = dict(ac_update_freq=2, policy_noise=0.2, noise_clamp=0.5)


def vec_close(got, want, rtol=RTOL, atol=ATOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want))) <= atol + rtol * float(np.max(np.abs(want)))


def _get(ag, name, n=None):
    from gcrl_amd._ffi import check, lib
    n = int(lib.gcrl_agent_numel(ag._h, name.encode())) if n is None else n
    out = np.empty(n, F32)
    check(lib.gcrl_agent_get(ag._h, name.encode(), out.ctypes.data, n))
    return out


def _set(ag, name, arr):
    from gcrl_amd._ffi import check, lib
    arr = np.ascontiguousarray(arr, F32)
    check(lib.gcrl_agent_set(ag._h, name.encode(), arr.ctypes.data, arr.size))


def _bc_state(ag):
    from gcrl_amd._ffi import check, lib
    w, f, r, n = C.c_double(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    check(lib.gcrl_agent_get_bc(ag._h, C.byref(w), C.byref(f), C.byref(r), C.byref(n)))
    return float(w.value), int(f.value), int(r.value), int(n.value)


# ---------------------------------------------------------------- 1. the kernel alone against the restatement, bit for bit
SHAPES = [(1, 1, 1, 4), (8, 3, 4, 4), (8, 7, 4, 4), (8, 8, 16, 16), (257, 200, 3, 4), (64, 1, 4, 8),
          (700, 650, 2, 4)]      # the last: more demonstration rows than the workgroup's 256 threads


@pytest.mark.parametrize("q_filter", [True, False], ids=["filter", "nofilter"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_Bd%d_A%d_Apad%d" % s)
def test_standalone_entry_bitwise_the_restatement(gcrl, shape, q_filter):
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import lib
    B, Bd, A_, Apad = shape
    gen = np.random.default_rng(B * 1000 + Bd * 10 + A_)
    col0, slots, slot, W = 5, 3, 1, 0.7
    ldx = (col0 + A_ + 3) // 4 * 4
    spa = np.full((slots, B, ldx), np.nan, F32)                   # the neighbouring slots are poison
    sa = np.full((slots, B, ldx), np.nan, F32)
    spa[slot], sa[slot] = gen.standard_normal((B, ldx)), gen.standard_normal((B, ldx))
    pi = np.tanh(gen.standard_normal((B, A_))).astype(F32)
    act = np.tanh(gen.standard_normal((B, A_))).astype(F32)
    spa[slot, :, col0:col0 + A_], sa[slot, :, col0:col0 + A_] = pi, act
    q_pi, q_a = gen.standard_normal(B).astype(F32), gen.standard_normal(B).astype(F32)
    dact = gen.standard_normal((B, Apad)).astype(F32)
    dact[:, A_:] = np.nan                                          # poison behind A within Apad
    r0 = B - Bd
    if Bd == 1:
        q_a[r0] = q_pi[r0] + F32(1.0)                              # the one demonstration row is accepted
    else:
        q_a[r0] = q_pi[r0]                                         # a tie: a rejected row, with a -0.0 gradient word
        dact[r0, 0] = F32(-0.0)
        q_a[r0 + 1] = np.nan                                       # a NaN
        q_a[r0 + 2] = q_pi[r0 + 2] + F32(0.25)                     # an accepted row with a -0.0 word
        dact[r0 + 2, 0] = F32(-0.0)
        if Bd >= 4:
            q_pi[r0 + 3] = np.nan
        if Bd >= 5:
            q_a[r0 + 4] = q_pi[r0 + 4] - F32(0.5)                  # another rejected row
    if r0 > 0:
        dact[0, 0] = F32(-0.0)                                     # a head row's
        q_a[0] = q_pi[0] + F32(9.0)                                # head rows never take part, whatever their q
    mask0 = np.full(B, 7.0, F32)
    met0 = np.arange(100, 132).astype(F32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_spa, d_sa, d_qpi, d_qa, d_dact, d_mask, d_met = (dev(x) for x in (spa, sa, q_pi, q_a, dact, mask0, met0))
    rc = lib.gcrl_bc_qfilter_f32(d_spa.data_ptr(), d_sa.data_ptr(), ldx, col0, slots, slot, d_qpi.data_ptr(),
                                 d_qa.data_ptr() if q_filter else None, B, Bd, A_, W, d_dact.data_ptr(), Apad, d_mask.data_ptr(),
                                 d_met.data_ptr(), _ffi.stream_handle())
    _ffi.check(rc)
    torch.cuda.synchronize()
    want_mask = BC.mask_of(q_a, q_pi, B, Bd, q_filter)
    want_dact, want_loss, want_pass = BC.step(pi, act, dact, want_mask, W, Bd)
    got_mask, got_dact, got_met = d_mask.cpu().numpy(), d_dact.cpu().numpy(), d_met.cpu().numpy()
    assert np.array_equal(bits(got_mask[r0:]), bits(want_mask[r0:])) and (got_mask[:r0] == 7.0).all()
    if q_filter and Bd >= 3:
        assert want_mask[r0] == 0 and want_mask[r0 + 1] == 0 and want_mask[r0 + 2] == 1
        assert np.signbit(got_dact[r0, 0]) and got_dact[r0, 0] == 0, "a rejected row's -0.0 was added to"
    assert np.array_equal(bits(got_dact), bits(want_dact))
    assert np.array_equal(bits(got_dact[:, A_:]), bits(dact[:, A_:])) and np.array_equal(bits(got_dact[:r0]), bits(dact[:r0]))
    assert int(bits(got_met[22])[0]) == int(bits(want_loss)[0]) and int(bits(got_met[23])[0]) == int(bits(want_pass)[0]), (got_met[22:24], want_loss, want_pass)
    keep = [i for i in range(32) if i not in (22, 23)]
    assert np.array_equal(got_met[keep], met0[keep])
    assert want_mask[r0:].sum() >= 1 and np.isfinite(got_met[22]) and got_met[22] > 0
    for t, h in ((d_spa, spa), (d_sa, sa), (d_qpi, q_pi), (d_qa, q_a)):      # inputs are read only
        assert np.array_equal(bits(t.cpu().numpy()), bits(h))


def test_standalone_entry_refuses_bad_arguments(gcrl):
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import lib
    x = torch.zeros(8 * 8, device="cuda")
    call = lambda **k: lib.gcrl_bc_qfilter_f32(*[{**dict(spa=x.data_ptr(), sa=x.data_ptr(), ldx=8, col0=4, slots=1, slot=0, q_pi=x.data_ptr(),
                                                         q_a=None, B=8, Bd=3, A=4, w=1.0, dact=x.data_ptr(), ld=4, mask=None, met=x.data_ptr(),
                                                         st=_ffi.stream_handle()), **k}[n]
                                                 for n in "spa sa ldx col0 slots slot q_pi q_a B Bd A w dact ld mask met st".split()])
    assert call() == 0
    for bad in (dict(Bd=0), dict(Bd=9), dict(A=17), dict(A=0), dict(col0=5), dict(ld=3), dict(slot=1), dict(w=0.0), dict(w=float("nan")),
                dict(w=-1.0), dict(dact=None)):
        assert call(**bad) == -1 and b"gcrl_bc_qfilter_f32" in lib.gcrl_last_error(), bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. engine wiring
def _small(gcrl, kind, seed, **kw):
    """REACH dims, H = 32, L = 3, B = 8, the layer-per-launch schedule"""
    cfg = make_config(kind, hidden_dim=32, layer_count=3, batch_size=8, max_len=150, k_future=4, grad_clip=None, **(TD3_KW if kind == "TD3" else {}))
    cls = {"DDPG": gcrl.DDPG, "TD3": gcrl.TD3Agent}[kind]
    ag = cls(S, A, cfg, None, nenvs=2, gradient_step=1, rng="engine", seed=seed, pipeline=0, **kw)
    T._perturb(ag, seed)
    return ag


def _batch(seed, B=8):
    gen = np.random.default_rng(900 + seed)
    f = lambda *shape: torch.from_numpy(gen.standard_normal(shape).astype(F32)).cuda()
    return (f(B, S), torch.tanh(f(B, A)), -torch.rand(B, generator=torch.Generator().manual_seed(seed)).cuda(), f(B, S),
            torch.zeros(B).cuda())


def _mlp64(flat, dims, x, out_tanh):
    """Linear + LeakyReLU per hidden layer, Linear (+ tanh): torch's parameter order, float64"""
    off, params = 0, []
    for k, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        w = torch.tensor(flat[off:off + i * o].reshape(o, i), dtype=torch.float64, requires_grad=True); off += i * o
        b = torch.tensor(flat[off:off + o], dtype=torch.float64, requires_grad=True); off += o
        params += [w, b]
        x = x @ w.T + b
        if k < len(dims) - 2:
            x = torch.nn.functional.leaky_relu(x, 0.01)
    assert off == flat.size
    return (torch.tanh(x) if out_tanh else x), params


CRITIC_VECS = ["grad:critic_{}", "critic_{}", "target_critic_{}", "adam_m:critic_{}", "adam_v:critic_{}"]


@pytest.mark.parametrize("kind", ["DDPG", "TD3"])
def test_engine_wiring_against_autograd_and_a_twin(gcrl, kind):
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import lib
    B, Bd, W, H = 8, 3, 0.9, 32
    nc = 1 if kind == "DDPG" else 2
    for seed in range(1, 17):           # the first seed whose filter both accepts and rejects a demonstration row
        ag, batch = _small(gcrl, kind, seed), _batch(seed)
        _ffi.check(lib.gcrl_agent_set_bc(ag._h, W, 1, Bd))
        assert _bc_state(ag) == (W, 1, Bd, 0)
        step = 1
        if kind == "TD3":               # step 1 is critic-only: no BC launch, the mask is nobody's to write
            _set(ag, "bc_mask", np.full(B, 5.0, F32))
            t0 = ag.update(1, batch=batch)
            assert len(t0) == 6 and _bc_state(ag)[3] == 0 and (_get(ag, "bc_mask") == 5.0).all()
            _set(ag, "bc_mask", np.zeros(B, F32))
            step = 2
        actor0 = ag.actor.flat().copy()
        out = ag.update(step, batch=batch)
        mask = _get(ag, "bc_mask")
        if mask[B - Bd:].min() == 0 and mask[B - Bd:].max() == 1:
            break
    assert mask[B - Bd:].min() == 0 and mask[B - Bd:].max() == 1 and not mask[:B - Bd].any(), mask
    assert len(out) == (6 if kind == "DDPG" else 8) and _bc_state(ag)[3] == 1
    # a twin without the term: everything of the critics bit for bit
    twin = _small(gcrl, kind, seed)
    for s_ in range(1, step + 1):
        tw = twin.update(s_, batch=batch)
    for c in range(nc):
        for name in CRITIC_VECS:
            assert np.array_equal(bits(_get(ag, name.format(c))), bits(_get(twin, name.format(c)))), name.format(c)
    x, y = T._tuples([out]), T._tuples([tw])
    keep = [i for i in range(x.shape[1]) if i != x.shape[1] - 1]                 # all but the actor's gradient norm
    assert np.array_equal(x[:, keep].view(np.uint64), y[:, keep].view(np.uint64)), (x, y)
    assert not np.array_equal(bits(_get(ag, "grad:actor")), bits(_get(twin, "grad:actor"))), "the term left the actor's gradient alone"
    # the mask, recomputed
    q_a, q_pi = _get(ag, "bc_q"), _get(ag, "bc_q_pi")
    assert np.array_equal(mask, BC.mask_of(q_a, q_pi, B, Bd)) and not q_a[:B - Bd].any()
    # torch autograd of the full loss from the agent's own weights, that mask held fixed
    s, a = batch[0].cpu().double(), batch[1].cpu().double()
    pi, pa = _mlp64(actor0.astype(np.float64), [S] + [H] * 3 + [A], s, True)
    q, _ = _mlp64(_get(ag, "critic_0").astype(np.float64), [S + A] + [H] * 3 + [1], torch.cat([s, pi], 1), False)
    loss = -q.mean() + W * (1.0 / Bd) * (torch.from_numpy(mask.astype(np.float64))[:, None] * (pi - a) ** 2).sum()
    loss.backward()
    want = np.concatenate([p.grad.numpy().ravel() for p in pa])
    got = _get(ag, "grad:actor")
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{kind}: grad:actor max-norm relative error {err:.3e} (scale {np.abs(want).max():.3e})")
    assert vec_close(got, want), err
    qa64, _ = _mlp64(_get(ag, "critic_0").astype(np.float64), [S + A] + [H] * 3 + [1], torch.cat([s, a], 1), False)
    assert vec_close(q_a[B - Bd:], qa64.detach().numpy().ravel()[B - Bd:]) and vec_close(q_pi, q.detach().numpy().ravel())
    # the metric words: the restatement on the read-back pi, a and mask
    ldx = (S + A + 3) // 4 * 4
    pi32 = _get(ag, "batch_spa").reshape(-1, B, ldx)[0][:, S:S + A]
    assert vec_close(pi32, pi.detach().numpy())
    _, want_loss, want_pass = BC.step(pi32, batch[1].cpu().numpy(), np.zeros((B, 4), F32), mask, W, Bd)
    assert ag.bc_weight is None
    w2 = (C.c_double * 2)()
    _ffi.check(lib.gcrl_agent_bc_metrics(ag._h, int(out[0]._ticket), w2))
    assert (w2[0], w2[1]) == (float(want_loss), float(want_pass)), (list(w2), want_loss, want_pass)
    assert w2[0] > 0 and 0 < w2[1] < 1
    assert abs(float(out[1 if kind == "DDPG" else 2]) + float(q.mean().detach())) <= 1e-5 * abs(float(q.mean().detach())) + 1e-6      # the tuple's actor loss stays -mean Q
    # off again: the next step is the twin's launch sequence
    _ffi.check(lib.gcrl_agent_set_bc(ag._h, 0.0, 1, 0))
    assert _bc_state(ag)[:3] == (0.0, 0, 0)
    ag.update(step + (1 if kind == "DDPG" else 2), batch=batch)
    assert _bc_state(ag)[3] == 1


def test_q_filter_off_accepts_every_demonstration_row(gcrl):
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import lib
    B, Bd, W = 8, 8, 2.0                                      # every row of the batch is a demonstration
    ag, batch = _small(gcrl, "DDPG", 3), _batch(3)
    _ffi.check(lib.gcrl_agent_set_bc(ag._h, W, 0, Bd))
    out = ag.update(1, batch=batch)
    assert (_get(ag, "bc_mask") == 1).all() and not _get(ag, "bc_q").any()
    ldx = (S + A + 3) // 4 * 4
    pi32 = _get(ag, "batch_spa").reshape(-1, B, ldx)[0][:, S:S + A]
    _, want_loss, want_pass = BC.step(pi32, batch[1].cpu().numpy(), np.zeros((B, 4), F32), np.ones(B, F32), W, Bd)
    w2 = (C.c_double * 2)()
    _ffi.check(lib.gcrl_agent_bc_metrics(ag._h, int(out[0]._ticket), w2))
    assert (w2[0], w2[1]) == (float(want_loss), 1.0)


# ---------------------------------------------------------------- 3. call forms, 4. through the rings
BD, WEIGHT = 3, 0.8


def _with_bc(gcrl, kind, seed, **kw):
    ag = TP._agent(gcrl, kind, seed, "engine", prior_buffer=TP._prior(gcrl), prior_rows=BD, bc_weight=WEIGHT, **kw)
    T._fill_agent(ag, 51)
    T._perturb(ag, 1)
    return ag


@pytest.mark.parametrize("kind", ["DDPG", "TD3"])
def test_update_many_equals_updates(gcrl, kind):
    one, many = _with_bc(gcrl, kind, 35), _with_bc(gcrl, kind, 35)
    assert one.bc_weight == WEIGHT and one.q_filter is True and _bc_state(one)[:3] == (WEIGHT, 1, BD)
    t1 = [one.update(s) for s in range(1, 7)]
    tm = many.update_many(1, 6)
    TP._equal_agents(one, many, t1, tm, "update_many(1, 6) is not 6 x update()")
    actor_steps = sum(len(t) == max(one.TD_INDEX) for t in t1)
    assert _bc_state(one)[3] == _bc_state(many)[3] == actor_steps == (6 if kind == "DDPG" else 3)
    m1, m2 = one.bc_metrics(), many.bc_metrics()
    assert m1 == m2 and m1[0] >= 0 and m1[1] in [float(F32(F32(k) / F32(BD))) for k in range(BD + 1)]
    for name in ("bc_mask", "bc_q", "grad:actor"):
        assert np.array_equal(bits(_get(one, name)), bits(_get(many, name))), name
    plain = TP._with_prior(gcrl, kind, 35, BD, pipeline=0)           # the term matters
    tp = T._tuples(plain.update_many(1, 6))
    assert not np.array_equal(tp.view(np.uint64), T._tuples(tm).view(np.uint64))


def test_through_the_rings_equals_a_twin_fed_the_same_batches(gcrl):
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import lib
    ag = _with_bc(gcrl, "DDPG", 37)
    twin = TP._agent(gcrl, "DDPG", 37, "engine", pipeline=0)
    T._perturb(twin, 1)
    _ffi.check(lib.gcrl_agent_set_bc(twin._h, WEIGHT, 1, BD))
    ta, tb = [], []
    for step in range(1, 5):
        ta.append(ag.update(step))
        sa, nsa, r, d = ag.read_batch(0)
        batch = tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (sa[:, :S], sa[:, S:S + A], r, nsa[:, :S], d))
        tb.append(twin.update(step, batch=batch))
    x, y = T._tuples(ta), T._tuples(tb)
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (x, y)
    assert np.array_equal(T._state(ag), T._state(twin))
    for name in ("bc_mask", "bc_q", "bc_q_pi", "grad:actor"):
        assert np.array_equal(bits(_get(ag, name)), bits(_get(twin, name))), name
    assert ag.bc_metrics() == tuple(_bc_words(twin, tb[-1]))


def _bc_words(ag, tup):
    from gcrl_amd import _ffi
    w2 = (C.c_double * 2)()
    _ffi.check(_ffi.lib.gcrl_agent_bc_metrics(ag._h, int(tup[0]._ticket), w2))
    return list(w2)


# ---------------------------------------------------------------- 5. refusals and state
def test_refusals_name_bc_weight_and_consume_nothing(gcrl):
    from gcrl_amd import _ffi
    from gcrl_amd._ffi import GcrlError, lib
    ag, twin = _with_bc(gcrl, "DDPG", 45), _with_bc(gcrl, "DDPG", 45)
    tick0 = int(ag.update(1)[0]._ticket)
    twin.update(1)

    def consumed():
        return (TP._blob(ag.buffer).tobytes(), TP._blob(ag.prior_buffer).tobytes(), T._mt_state(ag.buffer), ag.prior_counts(), _bc_state(ag))

    before = consumed()
    refused = lambda rc: rc < 0 and b"bc_weight" in lib.gcrl_last_error()
    # the setter: weights, rows, agent kinds, schedules
    for w, rows in ((-1.0, BD), (float("nan"), BD), (float("inf"), BD), (1.0, 0), (1.0, TP.B + 1)):
        assert refused(lib.gcrl_agent_set_bc(ag._h, w, 1, rows)), (w, rows)
    chain = TP._agent(gcrl, "DDPG", 45)                                   # the default schedule: row chain, pipelined
    assert refused(lib.gcrl_agent_set_bc(chain._h, 1.0, 1, BD))
    for kind in ("SAC", "TQC"):
        other = TP._agent(gcrl, kind, 45)
        assert refused(lib.gcrl_agent_set_bc(other._h, 1.0, 1, BD)), kind
    pop = gcrl.DDPGPopulation(S, A, T._pop_cfgs(), 2, 6, rng="engine", seeds=[61, 62])
    assert refused(lib.gcrl_agent_set_bc(pop.members[0]._h, 1.0, 1, BD))      # a population's members run the row chain
    assert consumed() == before
    # a gradient exchange (world 1)
    xh = _ffi.check_ptr(lib.gcrl_agent_xchg_create(ag._h, 0, 1), "gcrl_agent_xchg_create")
    try:
        _ffi.check(lib.gcrl_agent_set_exchange(ag._h, xh))
        for call in (lambda: ag.update(2), lambda: ag.update_many(2, 6)):
            with pytest.raises(GcrlError, match="bc_weight"):
                call()
        assert refused(lib.gcrl_agent_set_bc(ag._h, 1.0, 1, BD))
    finally:
        _ffi.check(lib.gcrl_agent_set_exchange(ag._h, None))
        lib.gcrl_xchg_destroy(xh)
    tickets = (C.c_int64 * 6)(); lens = (C.c_int32 * 6)()
    assert refused(lib.gcrl_agent_dp_begin(ag._h, ag.buffer.handle, 2, 6, 1.0, tickets, lens, _ffi.stream_handle()))
    # importance-sampling weights
    inputs, keep = ag._inject(batch=_batch(1, TP.B))
    w32 = np.ones(TP.B, F32)
    inputs.weights_host = w32.ctypes.data
    t = C.c_int64(-1)
    assert refused(lib.gcrl_agent_update(ag._h, None, 2, C.byref(inputs), C.byref(t), _ffi.stream_handle()))
    assert consumed() == before
    # ... and the agent goes on bit for bit like a twin that was never refused
    ta, tb = [ag.update(2)] + ag.update_many(3, 6), [twin.update(2)] + twin.update_many(3, 6)
    assert int(ta[0][0]._ticket) == tick0 + 1 == int(tb[0][0]._ticket), "a refused call consumed a ticket"
    TP._equal_agents(ag, twin, ta, tb, "after the refusals")


def test_save_load_resume_bitwise_and_refused_across_settings(gcrl, tmp_path):
    a = _with_bc(gcrl, "DDPG", 43)
    a.update(1)
    a.update_many(2, 6)
    a.save_state(str(tmp_path / "st"))
    fresh = lambda **kw: TP._agent(gcrl, "DDPG", 43, prior_buffer=TP._ring(gcrl, 120, REACH, "sample", "device", 11), prior_rows=BD, **kw)
    b = fresh(bc_weight=WEIGHT)
    b.load_state(str(tmp_path / "st"))
    ta, tb = a.update_many(8, 6), b.update_many(8, 6)
    x, y = T._tuples(ta), T._tuples(tb)
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (x, y)
    assert np.array_equal(T._state(a), T._state(b)) and a.bc_metrics() == b.bc_metrics()
    err = gcrl._ffi.GcrlError
    keep = T._state(b)
    with pytest.raises(err, match="load_state: bc_weight"):
        fresh(bc_weight=WEIGHT * 2).load_state(str(tmp_path / "st"))
    with pytest.raises(err, match="load_state: bc_weight"):
        fresh().load_state(str(tmp_path / "st"))
    with pytest.raises(err, match="load_state: q_filter"):
        fresh(bc_weight=WEIGHT, q_filter=False).load_state(str(tmp_path / "st"))
    plain = TP._with_prior(gcrl, "DDPG", 43, BD)
    plain.update(1)
    plain.save_state(str(tmp_path / "plain"))
    with pytest.raises(err, match="load_state: bc_weight"):
        b.load_state(str(tmp_path / "plain"))
    assert np.array_equal(T._state(b), keep), "a refused load overwrote the agent"
