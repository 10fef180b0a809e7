"""GPU (-m gpu): the device-resident goal environments (gcrl_amd.DeviceGoalEnv; csrc/dev_env.hip) held bit for bit to their numpy
definition tests/dev_env_ref.py: env_reset_kernel and env_step_kernel over two full episodes plus three steps — so an automatic
reset and a mid-episode state are both covered — under actions with out-of-range, infinite and NaN components; the raw and pay
blocks of every step, the acting rows, the counters, a state saved and loaded into a fresh handle (also under agent.collect, after the
saved handle is gone), poison past N, refused loads.

No case provokes a fault: every buffer compared or poisoned is either the handle's own block (read only) or a test-owned tensor
with room past N; the kernels' own guard (env index >= N does nothing) keeps every address inside its allocation."""
import numpy as np
import pytest
import torch

import dev_env_ref as E

pytestmark = pytest.mark.gpu

f32 = np.float32
T_STEPS = 6          # horizon of the test envs: 2 T + 3 = 15 steps


def bits(x):
    return np.ascontiguousarray(np.asarray(x, f32)).view(np.uint32)


def _same(a, b):
    """bit for bit; NaN words (the stored action of a NaN component) compare as NaN"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _actions(gen, n):
    a = gen.uniform(-2.5, 2.5, (n, 3)).astype(f32)
    a[gen.random((n, 3)) < 0.08] = np.inf
    a[gen.random((n, 3)) < 0.08] = -np.inf
    a[gen.random((n, 3)) < 0.08] = np.nan
    a[gen.random((n, 3)) < 0.2] *= f32(0.2)         # and small ones: a push env needs some contact
    return a


def _env_pair(gcrl, kind, n, seed=3, thr=0.05):
    return gcrl.DeviceGoalEnv(kind, n, seed=seed, max_steps=T_STEPS, threshold=thr), E.RefEnv(kind, n, seed=seed, max_steps=T_STEPS, threshold=thr)


def _check_rows(dev, ref):
    assert _same(dev.acting_rows()["rows"].cpu().numpy(), ref.rows)


def _pay_cols(pay):
    return np.asarray(pay)[:, :9]           # t | r | d | action | next_ag: the words the step writes


@pytest.mark.parametrize("kind", ["reach", "push"])
@pytest.mark.parametrize("n", [1, 5, 65])
def test_reset_and_step_match_the_definition(gcrl, kind, n):
    dev, ref = _env_pair(gcrl, kind, n)
    assert (dev.obs_dim, dev.goal_dim, dev.ac_dim, dev.num_envs, dev.max_steps) == (ref.D, 3, 3, n, T_STEPS)
    _check_rows(dev, ref)
    gen = np.random.default_rng(100 * n + len(kind))
    touched = False
    for step in range(2 * T_STEPS + 3):
        a = _actions(gen, n)
        if kind == "push" and step % T_STEPS in (1, 2):     # drive the pusher down onto the puck so that the contact branch runs
            a = np.clip((np.concatenate([ref.q[:, :2], np.zeros((n, 1), f32)], 1) - ref.p) / f32(0.04), -1, 1).astype(f32)
        q0 = ref.q.copy()
        want_raw, want_pay = ref.step(a)
        touched = touched or bool(np.any(ref.q[:, :2] != q0[:, :2]) and kind == "push")
        dev.step(torch.from_numpy(a).cuda() if step % 2 == 0 else torch.from_numpy(a.astype(np.float64)).cuda())     # float32 and float64 actions
        raw, pay = dev.step_blocks()
        assert _same(raw.cpu().numpy(), want_raw), (kind, n, step)
        assert _same(_pay_cols(pay.cpu().numpy()), _pay_cols(want_pay)), (kind, n, step)
        _check_rows(dev, ref)
    assert dev.stats() == ref.stats() and dev.stats()["episodes"] == 2 * n
    if kind == "push" and n > 1:
        assert touched, "no step of the test moved a puck"
    # masked reset: the selected envs go on to their next episode, the others stay where they are
    mask = (np.arange(n) % 2 == 0)
    dev.reset(mask); ref.reset(mask)
    _check_rows(dev, ref)
    # state saved mid-episode into a fresh handle: the continuation is bitwise
    blob = dev.save_state()
    twin = gcrl.DeviceGoalEnv(kind, n, seed=999, max_steps=T_STEPS, threshold=0.05)
    twin.load_state(blob)
    assert twin.seed == 3 and twin.stats() == dev.stats()
    for step in range(T_STEPS + 1):
        a = torch.from_numpy(_actions(gen, n)).cuda()
        dev.step(a); twin.step(a)
        assert _same(dev.step_blocks()[0].cpu().numpy(), twin.step_blocks()[0].cpu().numpy())
        assert _same(dev.acting_rows()["rows"].cpu().numpy(), twin.acting_rows()["rows"].cpu().numpy())
    assert np.array_equal(dev.save_state(), twin.save_state())
    # full reset: back to episode 0, counters to zero
    dev.reset()
    fresh = E.RefEnv(kind, n, seed=3, max_steps=T_STEPS)
    _check_rows(dev, fresh)
    assert dev.stats() == dict(episodes=0, successes=0, reward_sum=0.0)


@pytest.mark.parametrize("n", [5, 65])
def test_collect_goes_on_bitwise_on_a_handle_loaded_from_a_blob(gcrl, n):
    """agent.collect on a standalone env saved mid-episode and loaded into a fresh handle of another seed, after the first handle was
    destroyed and a third created (which may get the first one's address): the ring blob, the normalisers and the env state are bit
    for bit those of an uninterrupted twin.  The agent knows whose noise its stream last wrote by the handle's token, never by its
    address, and the loaded record carries seed, step counts and the host mirror of t."""
    import test_gpu_collect as TC
    import test_gpu_her_prior as TP
    from gcrl_amd.src.utils import DeviceRunningNormalizer

    def agent():
        cfg = TC.make_config("DDPG", hidden_dim=TC.H, layer_count=TC.L, batch_size=128, max_len=2000, k_future=4, **TC.TS.KINDS["DDPG"])
        ag = gcrl.DDPG(TC.D + TC.G, TC.A, cfg, None, nenvs=n, gradient_step=4, rng="engine", seed=5)
        ag.buffer.obs_normalizer, ag.buffer.dg_normalizer = DeviceRunningNormalizer(TC.D), DeviceRunningNormalizer(TC.G)
        ag.buffer.compute_reward = TC.her_oracle.sparse_reward
        return ag

    mk = lambda seed: gcrl.DeviceGoalEnv("reach", n, seed=seed, max_steps=TC.T, threshold=TC.THR)
    a, b = agent(), agent()
    env, twin = mk(4), mk(4)
    assert a.collect(env, 17) == b.collect(twin, 17)
    blob = env.save_state()
    loaded = mk(99)
    loaded.load_state(blob)
    env.__del__()                                     # the handle is destroyed here, not when the collector gets to it
    third = mk(7)
    assert loaded.seed == 4 and third.seed == 7
    assert a.collect(loaded, TC.T) == b.collect(twin, TC.T) > 0      # across the horizon: every env flushes once
    assert np.array_equal(TP._blob(a.buffer), TP._blob(b.buffer)), "ring blob"
    assert TC._same_nz(a, b), "normalisers"
    assert np.array_equal(loaded.save_state(), twin.save_state()), "env state"
    assert loaded.stats() == twin.stats() and loaded.stats()["episodes"] == n


def test_a_success_is_counted_with_a_strict_threshold(gcrl):
    """reach under the proportional controller: every episode ends inside the threshold, and the device counts what the definition counts"""
    dev, ref = _env_pair(gcrl, "reach", 5, seed=11)
    for _ in range(T_STEPS * 2):
        s = ref.state_dict()
        a = np.clip((s["desired_goal"] - s["achieved_goal"]) / f32(0.04), -1, 1).astype(f32)
        ref.step(a); dev.step(torch.from_numpy(a).cuda())
    assert dev.stats() == ref.stats() and ref.stats()["successes"] > 0


def test_pack_kernel_and_poison_past_n(gcrl, lib):
    """gcrl_proc_pack on separate tensors builds the blocks the step kernel writes; words past the n envs' share of a larger buffer
    keep their poison."""
    from gcrl_amd import _ffi
    n, kind = 5, "push"
    dev, ref = _env_pair(gcrl, kind, n)
    gen = np.random.default_rng(1)
    a = _actions(gen, n)
    st0 = ref.state_dict()
    want_raw, want_pay = ref.step(a)
    obs, nobs, dg, ndg, ag, nag = ref.split(want_raw)
    D, G, A = ref.D, 3, 3
    raw_words = n * (2 * D + 4 * G)
    POISON = f32(-77.25)
    raw = torch.full((raw_words + 64,), float(POISON), device="cuda")
    pay = torch.full((n + 2, 32), float(POISON), device="cuda")
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x, f32)).cuda()
    t = [cu(x) for x in (obs, nobs, dg, ndg, ag, nag, a, want_pay[:, 1])]
    _ffi.check(lib.gcrl_proc_pack(*[x.data_ptr() for x in t], None, 0, n, D, G, A, raw.data_ptr(), pay.data_ptr(), _ffi.stream_handle()))
    raw_h, pay_h = raw.cpu().numpy(), pay.cpu().numpy()
    assert _same(raw_h[:raw_words], want_raw) and np.all(raw_h[raw_words:] == POISON)
    assert _same(pay_h[:n, :9], want_pay[:, :9]) and np.all(pay_h[:n, 9:] == POISON) and np.all(pay_h[n:] == POISON)
    assert np.array_equal(st0["achieved_goal"], ag)
    # per-env t words from a device array
    tt = torch.tensor([4, 0, 2, 2, 1], dtype=torch.int32, device="cuda")
    _ffi.check(lib.gcrl_proc_pack(*[x.data_ptr() for x in t], tt.data_ptr(), 0, n, D, G, A, raw.data_ptr(), pay.data_ptr(), _ffi.stream_handle()))
    assert np.array_equal(pay.cpu().numpy()[:n, 0].view(np.int32), [4, 0, 2, 2, 1])
    # the env's own step leaves the payload words it does not own at their initial zero
    dev.step(cu(a))
    assert np.all(dev.step_blocks()[1].cpu().numpy()[:, 9:] == 0.0)


def test_refused_loads_name_their_field_and_leave_the_handle_alone(gcrl):
    dev, _ = _env_pair(gcrl, "reach", 5)
    dev.step(torch.zeros((5, 3), device="cuda"))
    before = dev.save_state()
    others = dict(kind=gcrl.DeviceGoalEnv("push", 5, seed=3, max_steps=T_STEPS), num_envs=gcrl.DeviceGoalEnv("reach", 4, seed=3, max_steps=T_STEPS),
                  max_steps=gcrl.DeviceGoalEnv("reach", 5, seed=3, max_steps=T_STEPS + 1),
                  threshold=gcrl.DeviceGoalEnv("reach", 5, seed=3, max_steps=T_STEPS, threshold=0.06))
    for field, other in others.items():
        with pytest.raises(ValueError, match=field):
            dev.load_state(other.save_state())
        assert np.array_equal(dev.save_state(), before), field
    with pytest.raises(ValueError, match="blob"):
        dev.load_state(before[:-4])
    with pytest.raises(ValueError, match="kind"):
        gcrl.DeviceGoalEnv("slide", 2)
    with pytest.raises(gcrl._ffi.GcrlError, match="num_envs"):
        gcrl.DeviceGoalEnv("reach", 1025)
    with pytest.raises(gcrl._ffi.GcrlError, match="threshold"):
        gcrl.DeviceGoalEnv("push", 2, threshold=0.08)
    with pytest.raises(ValueError, match="actions"):
        dev.step(torch.zeros((4, 3), device="cuda"))
