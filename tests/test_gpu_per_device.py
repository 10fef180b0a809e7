"""GPU (-m gpu): the device-resident prioritised replay (csrc/per_tree.hip; PERBuffer draw="device", agents per_draw="device") against
its CPU restatement tests/per_tree_ref.py.

Shapes: the smallest at which the structure can still go wrong — cap 96 / len 70 (two levels, a partial leaf block, an unfilled
tail), cap 96 with 130 pushes (the ring wraps), cap 4160 / len 4130 (three levels, a partial block on level 1), B in {33, 64, 256}
(33: not a multiple of the waves per workgroup).

Bounds.  Adds, compares and the hash are held bitwise.  The weights and the updated leaves involve one add / divide and one powf
in float32: relative 1e-6 against a float64 evaluation from the device's own float32 inputs (a few float32 ulp; the precedent is
tests/test_device_rng.py's 4e-6 absolute bound).  Measured on an MI355X (profiles/r15_per_device_accuracy.jsonl): weights worst
relative 2.3e-7, updated leaves worst relative 9.3e-8, 2^18 device draws worst |z| 2.9."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import per_tree_ref as R
from oracle.agent_oracle import make_config

pytestmark = pytest.mark.gpu

S, A = 10, 3
ALPHA, EPS = 0.6, 1e-6
REL = 1e-6


def _note(**kw):
    """Measured figures: printed, and appended to the file GCRL_PER_ACCURACY_OUT names when it is set."""
    print(json.dumps(kw))
    out = os.environ.get("GCRL_PER_ACCURACY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _rows(n, seed=0):
    gen = np.random.default_rng(seed)
    return (gen.standard_normal((n, S)).astype(np.float32), gen.uniform(-1, 1, (n, A)).astype(np.float32),
            gen.standard_normal((n, S)).astype(np.float32), -(gen.random(n) < 0.7).astype(np.float32), gen.random(n) < 0.05)


def _push(target, n, seed=0, first=0):
    s, a, ns, r, d = _rows(first + n, seed)
    for i in range(first, first + n):
        target.push(s[i], a[i], float(r[i]), ns[i], bool(d[i]))


def _buffer(gcrl, cap, pushes, seed=5):
    buf = gcrl.PERBuffer(cap, ALPHA, draw="device", rng="engine", seed=seed)
    _push(buf, pushes)
    return buf


def _head(gcrl, buf):
    return int(gcrl._ffi.lib.gcrl_her_head(buf.handle))


def _check_tree(gcrl, buf, cap):
    """Levels read back == the restated reduction of the device's own children, bitwise; padding and unfilled slots zero."""
    levels = buf.tree_levels()
    assert [lv.size for lv in levels] == [p for _, p in R.level_sizes(cap)]
    R.check_invariant(levels)
    filled = np.zeros(levels[0].size, bool)
    filled[(_head(gcrl, buf) + np.arange(len(buf))) % cap] = True
    assert not levels[0][~filled].any(), "a never-filled slot holds a priority"
    return levels


def _random_priorities(n, seed):
    gen = np.random.default_rng(seed)
    return np.exp(gen.uniform(np.log(1e-3), np.log(11.0), n)).astype(np.float32)


def test_levels_are_the_reduction_of_the_devices_own_children(gcrl):
    cap = 96
    buf = _buffer(gcrl, cap, 70)
    lv = _check_tree(gcrl, buf, cap)                       # after attach + pushes: 70 ones, 26 + 32 zeros
    assert len(lv) == 2 and np.all(lv[0][:70] == 1.0) and lv[1][0] == 64.0 and lv[1][1] == 6.0
    assert np.array_equal(buf.get_priorities(), np.ones(70, np.float32))
    p = _random_priorities(70, 1)
    buf.set_priorities(p)                                  # full rebuild
    lv = _check_tree(gcrl, buf, cap)
    assert np.array_equal(buf.get_priorities().view(np.uint32), p.view(np.uint32))
    _push(buf, 60, first=70)                               # 130 pushes: wraps, head = 34, the evicted rows' priorities overwritten by 1.0
    assert len(buf) == cap and _head(gcrl, buf) == 34
    lv = _check_tree(gcrl, buf, cap)
    want = np.concatenate([p[34:], np.ones(60, np.float32)])           # logical order: rows 34..69 keep theirs, 60 new rows
    assert np.array_equal(buf.get_priorities().view(np.uint32), want.view(np.uint32))
    buf.draw_counter = 7                                   # a draw on the wrapped ring: slots map back to logical indices
    got_idx, _ = buf.draw(64, 0.5)
    want_idx, _ = R.draw(lv, 5, 7, 64, 34, cap)
    assert np.array_equal(got_idx.cpu().numpy().view(np.uint32), want_idx)
    # an update with duplicate indices whose td values differ: the last occurrence wins, untouched leaves keep their bits
    before = lv[0].copy()
    idx = np.array([5, 40, 5, 95, 0, 40, 5, 17], np.int32)
    td = np.array([0.5, -2.0, 0.25, 1e-3, 0.0, 3.0, -0.125, 7.5], np.float32)
    buf.update_priorities(torch.from_numpy(idx).cuda(), torch.from_numpy(td).cuda().unsqueeze(-1))
    lv = _check_tree(gcrl, buf, cap)
    keep = R.last_occurrence(idx)
    slots = (34 + idx) % cap
    got, want = lv[0][slots[keep]].astype(np.float64), R.priority64(td[keep], EPS, ALPHA)
    rel = float(np.max(np.abs(got - want) / want))
    _note(check="updated_leaves", case="cap96_wrapped", worst_rel=rel)
    assert rel <= REL
    assert sorted(idx[keep].tolist()) == [0, 5, 17, 40, 95]
    untouched = np.ones(lv[0].size, bool)
    untouched[slots] = False
    assert np.array_equal(lv[0][untouched].view(np.uint32), before[untouched].view(np.uint32))


def test_three_level_tree_and_updates(gcrl):
    cap, n = 4160, 4130
    buf = _buffer(gcrl, cap, n)
    p = _random_priorities(n, 2)
    buf.set_priorities(p)
    lv = _check_tree(gcrl, buf, cap)
    assert len(lv) == 3 and lv[1].size == 128 and lv[2].size == 64
    gen = np.random.default_rng(3)
    worst = 0.0
    for B in (33, 64, 256):
        before = lv[0].copy()
        idx = gen.integers(0, n, B).astype(np.int32)
        idx[B // 2:] = idx[:B - B // 2]                     # every index twice, different td
        td = gen.standard_normal(B).astype(np.float32) * 3
        buf.update_priorities(torch.from_numpy(idx).cuda(), torch.from_numpy(td).cuda())
        lv = _check_tree(gcrl, buf, cap)
        keep = R.last_occurrence(idx)
        got, want = lv[0][idx[keep]].astype(np.float64), R.priority64(td[keep], EPS, ALPHA)
        worst = max(worst, float(np.max(np.abs(got - want) / want)))
        untouched = np.ones(lv[0].size, bool)
        untouched[idx] = False
        assert np.array_equal(lv[0][untouched].view(np.uint32), before[untouched].view(np.uint32))
    _note(check="updated_leaves", case="cap4160", worst_rel=worst)
    assert worst <= REL


@pytest.mark.parametrize("cap,n,batches", [(96, 70, (33, 64)), (4160, 4130, (33, 64, 256))])
def test_draw_equals_the_restated_descent_and_weights_formula(gcrl, cap, n, batches):
    worst = 0.0
    for seed, counter in ((5, 0), (77, 12345), (2 ** 40 + 9, 2 ** 33 + 1)):
        buf = _buffer(gcrl, cap, n, seed=seed)
        buf.set_priorities(_random_priorities(n, seed % 1000))
        levels = _check_tree(gcrl, buf, cap)
        total = R.reduce64(levels[-1])[0]
        for B in batches:
            buf.draw_counter = counter
            beta = 0.4 + 0.1 * (B % 7)
            idx, w = buf.draw(B, beta)
            assert buf.draw_counter == counter + 1
            idx, w = idx.cpu().numpy().view(np.uint32), w.cpu().numpy()
            want_idx, want_p = R.draw(levels, seed, counter, B, _head(gcrl, buf), cap)
            assert np.array_equal(idx, want_idx), (seed, counter, B)
            assert np.all(idx < n) and np.all(want_p > 0) and np.all(levels[0][idx] > 0)
            want_w = R.weights64(levels[0][idx], total, n, beta)
            worst = max(worst, float(np.max(np.abs(w.astype(np.float64) - want_w) / want_w)))
            assert float(w.max()) == 1.0
            # sample(): the same draw, gathered — rows are the ring's rows at those indices
            buf.draw_counter = counter
            out = buf.sample(B, beta)
            assert len(out) == 7 and out[5].shape == (B, 1) and out[5].is_cuda and out[6].is_cuda
            assert np.array_equal(out[6].cpu().numpy().view(np.uint32), want_idx)
            rows = buf.rows()
            assert np.array_equal(out[0].cpu().numpy(), rows[0][want_idx]) and np.array_equal(out[2].cpu().numpy()[:, 0], rows[3][want_idx])
    _note(check="weights", case=f"cap{cap}", worst_rel=worst)
    assert worst <= REL


@pytest.mark.parametrize("cap,n,B", [(96, 70, 64), (4160, 4130, 256)])
def test_device_draw_frequency(gcrl, cap, n, B):
    """2^18 device draws: the relative frequency of the 70 filled rows (cap 96) / the 64 heaviest rows against p_i / total within 5
    binomial standard errors; no zero slot is ever drawn."""
    buf = _buffer(gcrl, cap, n, seed=11)
    p = _random_priorities(n, 4)
    if n > 100:
        p[np.random.default_rng(9).choice(n, 9, replace=False)] = 0.0
    buf.set_priorities(p)
    levels = _check_tree(gcrl, buf, cap)
    draws = (1 << 18) // B
    got = torch.cat([buf.draw(B, 0.5)[0] for _ in range(draws)]).cpu().numpy().astype(np.int64)
    assert np.all(got < n) and np.all(levels[0][got] > 0), "a zero slot was drawn"
    prob = levels[0].astype(np.float64) / levels[0].astype(np.float64).sum()
    counts = np.bincount(got, minlength=levels[0].size)
    heavy = np.argsort(-prob)[:70 if cap == 96 else 64]
    N = draws * B
    z = (counts[heavy] - N * prob[heavy]) / np.sqrt(N * prob[heavy] * (1 - prob[heavy]))
    _note(check="frequency", case=f"cap{cap}", worst_abs_z=float(np.max(np.abs(z))))
    assert float(np.max(np.abs(z))) <= 5.0


# ------------------------------------------------------------------------------------------------ engine integration
CLS = {"DDPG": "DDPG", "TD3": "TD3Agent", "SAC": "SACAgent"}


def _agent(gcrl, kind, per_draw, gradient_step=5, cap=4160, rows=600, seed=3):
    cfg = make_config(kind, buffer_type="PER", max_len=cap, hidden_dim=64, batch_size=64, alpha=ALPHA, beta=0.4, beta_end=50, policy_noise=0.2)
    ag = getattr(gcrl, CLS[kind])(S, A, cfg, None, nenvs=1, gradient_step=gradient_step, rng="engine", seed=seed, per_draw=per_draw)
    _push(ag, rows, seed=21)
    return ag


def _names(ag):
    names = ["actor", "adam_m:actor", "adam_v:actor", "td_abs"]
    for i in range(ag.num_critics):
        names += [f"critic_{i}", f"target_critic_{i}", f"adam_m:critic_{i}", f"adam_v:critic_{i}"]
    names += ["log_alpha", "bn_running_mean", "bn_running_var"] if ag._sac else ["target_actor"]
    return names


def _state(gcrl, ag, names=None):
    out = {}
    for name in names or _names(ag):
        n = int(gcrl._ffi.lib.gcrl_agent_numel(ag._h, name.encode()))
        v = np.empty(n, np.float32)
        gcrl._ffi.check(gcrl._ffi.lib.gcrl_agent_get(ag._h, name.encode(), v.ctypes.data, n))
        out[name] = v.view(np.uint32)
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _noise(kind, step):
    g = torch.Generator().manual_seed(100 + step)
    if kind == "TD3":
        return dict(noise=torch.randn(64, A, generator=g))
    if kind == "SAC":
        return dict(eps_next=torch.randn(64, A, generator=g), eps_cur=torch.randn(64, A, generator=g))
    return {}


@pytest.mark.parametrize("kind", ["TD3", "SAC", "DDPG"])
def test_device_step_equals_a_twin_fed_the_drawn_indices_and_weights(gcrl, kind):
    """One device-mode update()'s indices and weights, read back and fed to a twin through the existing idx_host / weights_host inputs:
    parameters, targets, Adam moments and td_abs bitwise equal after the step (two steps: the second draws from updated priorities)."""
    lib, ffi = gcrl._ffi.lib, gcrl._ffi
    dev, twin = _agent(gcrl, kind, "device"), _agent(gcrl, kind, "host")
    _same(_state(gcrl, dev), _state(gcrl, twin))
    for step in (1, 2):
        kw = _noise(kind, step)
        launches = int(lib.gcrl_per_launches(dev.buffer.handle))
        info = dev.update(step, **kw)
        assert int(lib.gcrl_per_launches(dev.buffer.handle)) - launches == (4 if step == 1 else 3)   # (refresh of the pushes), draw, weights, update
        idx = dev.drawn_indices(1)[0]
        w = np.empty(64, np.float32)
        ffi.check(lib.gcrl_agent_get(dev._h, b"w_in", w.ctypes.data, 64))
        assert np.all(idx < len(dev.buffer)) and float(w.max()) == 1.0 and np.all(w > 0)
        twin.set_train()
        inputs, keep = twin._inject(None, kw.get("noise"), kw.get("eps_next"), kw.get("eps_cur"))
        inputs = inputs or ffi.UpdateInputs()
        inputs.idx_host, inputs.weights_host = idx.ctypes.data, w.ctypes.data
        ticket = C.c_int64(-1)
        n = ffi.check(lib.gcrl_agent_update(twin._h, twin.buffer.handle, step, C.byref(inputs), C.byref(ticket), ffi.stream_handle()))
        assert n == len(info)
        a, b = _state(gcrl, dev), _state(gcrl, twin)
        _same(a, b)
        td = np.asarray(info[dev.TD_INDEX[n]])                  # the lazy td_error: the reference's [B, 1] array
        assert td.shape == (64, 1) and td.dtype == np.float32 and np.array_equal(td[:, 0].view(np.uint32), a["td_abs"])
        # the priorities followed on the device: the drawn rows' leaves are the formula of this step's td_abs
        pr = dev.buffer.get_priorities()
        keepm = R.last_occurrence(idx)
        want = R.priority64(td[keepm, 0], EPS, ALPHA)
        assert float(np.max(np.abs(pr[idx[keepm]].astype(np.float64) - want) / want)) <= REL


def test_update_many_is_one_call_equal_to_single_updates(gcrl):
    many, single, again = (_agent(gcrl, "TD3", "device") for _ in range(3))
    outs = many.update_many(1, 5)
    assert len(outs) == 5 and many.beta == pytest.approx(0.4 + (5 / 50) * 0.6)
    idx_many = many.drawn_indices(5)
    idx_single, td_single, m_single = [], [], []
    for i in range(5):
        o = single.update(1 + i)
        idx_single.append(single.drawn_indices(1)[0])
        td_single.append(np.asarray(o[single.TD_INDEX[len(o)]]))
        m_single.append(float(o[0]))
    names = [n for n in _names(many)]
    _same(_state(gcrl, many, names), _state(gcrl, single, names))
    assert np.array_equal(idx_many, np.stack(idx_single))
    assert np.array_equal(many.buffer.get_priorities().view(np.uint32), single.buffer.get_priorities().view(np.uint32))
    assert many.buffer.draw_counter == single.buffer.draw_counter == 5 and many.beta == single.beta
    for i in range(5):
        td = np.asarray(outs[i][many.TD_INDEX[len(outs[i])]])
        assert td.shape == (64, 1) and np.array_equal(td.view(np.uint32), td_single[i].view(np.uint32))
        assert float(outs[i][0]) == m_single[i]
    # two runs with one seed
    again.update_many(1, 5)
    _same(_state(gcrl, many, names), _state(gcrl, again, names))
    assert np.array_equal(idx_many, again.drawn_indices(5))
    # the history buffer belongs to the last call: a late read raises instead of returning another step's values
    stale = many.update_many(6, 2)
    many.update(8)
    with pytest.raises(gcrl.buffer.TdHistoryOverwritten):
        np.asarray(stale[0][many.TD_INDEX[len(stale[0])]])


def test_resume_is_bitwise(gcrl, tmp_path):
    """save after 3 steps, load into fresh objects, continue 3 steps == the uninterrupted run; on a ring that has wrapped (head != 0), so
    the loaded rows and leaves must return to their slots."""
    def make():
        return _agent(gcrl, "TD3", "device", cap=500, rows=650)
    ref, first = make(), make()
    assert _head(gcrl, ref.buffer) == 150
    for step in range(1, 7):
        ref.update(step)
    for step in range(1, 4):
        first.update(step)
    first.save_state(str(tmp_path / "ck"))
    resumed = _agent(gcrl, "TD3", "device", cap=500, rows=0)      # (the seed keys the draw: part of the construction, not of the state)
    resumed.load_state(str(tmp_path / "ck"))
    assert resumed.buffer.draw_counter == 3 and _head(gcrl, resumed.buffer) == 150 and resumed.beta == first.beta
    for a, b in zip(resumed.buffer.tree_levels(), first.buffer.tree_levels()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    idx = []
    for step in range(4, 7):
        resumed.update(step)
        idx.append(resumed.drawn_indices(1)[0])
    _same(_state(gcrl, ref), _state(gcrl, resumed))
    assert np.array_equal(ref.buffer.get_priorities().view(np.uint32), resumed.buffer.get_priorities().view(np.uint32))
    assert np.array_equal(ref.drawn_indices(1)[0], idx[-1])


def test_refusals_and_defaults(gcrl):
    # the default stays the host-drawn parity mode
    buf = gcrl.PERBuffer(100, 0.6, rng="engine", seed=1)
    assert buf.draw_mode == "host" and hasattr(buf, "priorities")
    _push(buf, 5)
    assert list(buf.priorities) == [1.0] * 5 and not gcrl._ffi.lib.gcrl_per_attached(buf.handle)
    host = _agent(gcrl, "TD3", "host", rows=80)
    assert host.per_draw == "host" and host.buffer.draw_mode == "host"
    with pytest.raises(gcrl._ffi.GcrlError, match="draw='device'"):
        buf.tree_levels()
    # engine entries that do not draw from a tree refuse a ring that has one, naming per_draw
    dev = _agent(gcrl, "TD3", "device", rows=80)
    t = C.c_int64(-1)
    rc = gcrl._ffi.lib.gcrl_agent_update_phase(dev._h, dev.buffer.handle, 1, 0, None, 1.0, C.byref(t), gcrl._ffi.stream_handle())
    assert rc < 0 and "per_draw" in gcrl._ffi.last_error()
    # and the update entry refuses to run without a queued beta
    rc = gcrl._ffi.lib.gcrl_agent_update(dev._h, dev.buffer.handle, 1, None, C.byref(t), gcrl._ffi.stream_handle())
    assert rc < 0 and "gcrl_per_set_betas" in gcrl._ffi.last_error()
    dev.update(1)      # still usable
    with pytest.raises(gcrl._ffi.GcrlError, match="per_draw"):
        gcrl.DDPGPopulation(S, A, [make_config("DDPG", batch_size=64)] * 2, nenvs=1, gradient_step=4, per_draw="device")
    with pytest.raises(gcrl._ffi.GcrlError, match="per_draw"):
        gcrl.TQCAgent(S, A, make_config("TQC", buffer_type="PER", max_len=500, batch_size=64), None, nenvs=1, gradient_step=4, n_quantiles=25,
                      per_draw="device")
    from gcrl_amd.src.dp import DataParallelUpdater
    with pytest.raises(gcrl._ffi.GcrlError, match="per_draw"):
        DataParallelUpdater(dev)
