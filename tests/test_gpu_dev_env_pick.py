"""GPU (-m gpu): the `pick` device environment (gcrl_amd.DeviceGoalEnv("pick"); csrc/dev_env.hip, dev_env_body.h) and its scripted
controller (csrc/dev_env_script.hip env_scripted_kernel) held bit for bit to their numpy definition tests/dev_env_pick_ref.py:
env_reset_kernel and env_step_kernel over two full episodes plus three steps under actions with out-of-range, infinite and NaN
components, with steps that grasp, carry and release the object; the raw and pay blocks of every step, the acting rows, the whole
state blob (18-float records) and the counters; masked and full resets; a state saved and loaded into a fresh handle; poison past N;
refused loads across kinds; scripted_actions() with and without noise; and a device-only episode under the controller.

No case provokes a fault: every buffer compared or poisoned is the handle's own block (read only) or a test-owned tensor with room
past N; the kernels' own guard (env index >= N does nothing) keeps every address inside its allocation."""
import struct

import numpy as np
import pytest
import torch

import dev_env_pick_ref as P
import test_gpu_dev_env as TE
import test_gpu_env_group as TG

pytestmark = pytest.mark.gpu

f32 = np.float32
T_STEPS = 6          # horizon of the test envs: 2 T + 3 = 15 steps
same, bits = TE._same, TE.bits


def _actions(gen, n):
    a = gen.uniform(-2.5, 2.5, (n, 4)).astype(f32)
    a[gen.random((n, 4)) < 0.08] = np.inf
    a[gen.random((n, 4)) < 0.08] = -np.inf
    a[gen.random((n, 4)) < 0.08] = np.nan
    a[gen.random((n, 4)) < 0.2] *= f32(0.2)
    a[np.arange(n) % 4 == 0, 0] = np.nan             # every step carries a NaN and an out-of-range component
    a[np.arange(n) % 4 == 0, 1] = 7.0
    return a


def _env_pair(gcrl, n, seed=3, thr=0.05, T=T_STEPS):
    return gcrl.DeviceGoalEnv("pick", n, seed=seed, max_steps=T, threshold=thr), P.RefPickEnv(n, seed=seed, max_steps=T, threshold=thr)


def _noisy(gcrl, ref, noise_std, seed, c):
    """the definition's noisy actions of vector step c, the hash normals taken from the device's own fill (their transcendental functions
    differ from numpy's by ulps); the counters and the arithmetic around them are the definition's"""
    z = TG._normals(gcrl, seed, c * ref.n * 4, ref.n * 4)
    return P.scripted_actions(ref, noise_std=noise_std, seed=seed, c=c, normals=z)


def _blob(ref, steps):
    """the bytes gcrl_env_save_state writes for a device env in the reference's state"""
    head = struct.pack("<IiiifIQq", 0x564E4547, P.KIND, ref.n, ref.T, float(ref.thr), 0, ref.seed, steps)
    cnt = np.stack([ref.episode, ref.episodes, ref.successes], 1).astype(np.uint64)
    parts = [ref.state_array(), ref.t.astype(np.int32), cnt, ref.reward_sum.astype(np.float64), ref.rows]
    return np.frombuffer(head + b"".join(np.ascontiguousarray(x).tobytes() for x in parts), np.uint8)


def _check(dev, ref, steps, what):
    assert same(dev.acting_rows()["rows"].cpu().numpy(), ref.rows), what
    assert np.array_equal(dev.save_state(), _blob(ref, steps)), what


@pytest.mark.parametrize("n", [1, 5, 65])
def test_reset_and_step_match_the_definition(gcrl, n):
    dev, ref = _env_pair(gcrl, n)
    assert (dev.obs_dim, dev.goal_dim, dev.ac_dim, dev.num_envs, dev.max_steps) == (20, 3, 4, n, T_STEPS)
    assert dev.save_state().size == 40 + n * (18 * 4 + 4 + 24 + 8 + 23 * 4)
    _check(dev, ref, 0, "fresh")
    gen = np.random.default_rng(100 * n + 4)
    steps = 0
    for step in range(2 * T_STEPS + 3):
        a = _actions(gen, n)
        want_raw, want_pay = ref.step(a)
        dev.step(torch.from_numpy(a).cuda() if step % 2 == 0 else torch.from_numpy(a.astype(np.float64)).cuda())     # float32 and float64 actions
        steps += 1
        raw, pay = dev.step_blocks()
        assert same(raw.cpu().numpy(), want_raw), (n, step)
        pay = pay.cpu().numpy()
        assert same(pay[:, :10], want_pay[:, :10]) and np.all(pay[:, 10:] == 0), (n, step)
        _check(dev, ref, steps, (n, step))
    assert dev.stats() == ref.stats() and dev.stats()["episodes"] == 2 * n
    # masked reset: the selected envs go on to their next episode, the others stay where they are
    mask = (np.arange(n) % 2 == 0)
    dev.reset(mask); ref.reset(mask)
    _check(dev, ref, steps, "masked reset")
    # state saved mid-episode into a fresh handle: the continuation is bitwise
    blob = dev.save_state()
    twin = gcrl.DeviceGoalEnv("pick", n, seed=999, max_steps=T_STEPS, threshold=0.05)
    twin.load_state(blob)
    assert twin.seed == 3 and twin.stats() == dev.stats()
    for step in range(T_STEPS + 1):
        a = _actions(gen, n)
        ref.step(a)
        a = torch.from_numpy(a).cuda()
        dev.step(a); twin.step(a)
        assert same(dev.step_blocks()[0].cpu().numpy(), twin.step_blocks()[0].cpu().numpy())
    assert np.array_equal(dev.save_state(), twin.save_state())
    _check(twin, ref, steps + T_STEPS + 1, "resumed")
    # full reset: back to episode 0, counters to zero
    dev.reset()
    _check(dev, P.RefPickEnv(n, seed=3, max_steps=T_STEPS), 0, "full reset")
    assert dev.stats() == dict(episodes=0, successes=0, reward_sum=0.0)


@pytest.mark.parametrize("n", [1, 5, 65])
def test_grasp_carry_and_release_match_the_definition(gcrl, n):
    """The branches random actions never reach, step by step against the definition: the controller's approach and grasp, a lift with
    the fingers closed, the release once the fingers are CLOSE apart, the fall back to the table."""
    dev, ref = _env_pair(gcrl, n, seed=6, T=30)
    seen = dict(grasp=False, lift=False, fall=False, landed=False)
    for step in range(27):
        if step < 14:
            a = P.scripted_actions(ref)
        elif step < 18:
            a = np.tile(np.array([0.25, np.nan, 1, -1], f32), (n, 1))
        else:
            a = np.tile(np.array([0, 0, 0, 3.0], f32), (n, 1))
        held0, z0 = ref.held.copy(), ref.q[:, 2].copy()
        want_raw, want_pay = ref.step(a)
        seen["grasp"] |= bool(np.any((held0 == 0) & (ref.held == 1)))
        seen["lift"] |= bool(np.any((ref.held == 1) & (ref.q[:, 2] > z0)))
        seen["fall"] |= bool(np.any((ref.held == 0) & (ref.q[:, 2] < z0)))
        seen["landed"] |= bool(np.any((ref.held == 0) & (z0 > 0) & (ref.q[:, 2] == 0)))
        dev.step(torch.from_numpy(a).cuda() if step % 2 else torch.from_numpy(a.astype(np.float64)).cuda())
        assert same(dev.step_blocks()[0].cpu().numpy(), want_raw), (n, step)
        assert same(dev.step_blocks()[1].cpu().numpy()[:, :10], want_pay[:, :10]), (n, step)
        _check(dev, ref, step + 1, (n, step))
    assert all(seen.values()), seen


def test_a_closed_fist_pushes_the_object(gcrl):
    """fingers closed on the way down: no grasp, and the object moves along the table with the gripper (the `push` branch of the rule)"""
    dev, ref = _env_pair(gcrl, 5, seed=8, T=12)
    moved = False
    for step in range(12):
        if step < 3:
            a = np.tile(np.array([0, 0, 0, -1], f32), (5, 1))
        else:
            a = np.concatenate([np.clip((ref.q - ref.p) / f32(0.04), -1, 1), -np.ones((5, 1))], 1).astype(f32)
        xy0 = ref.q[:, :2].copy()
        want_raw, _ = ref.step(a)
        moved |= bool(np.any(ref.q[:, :2] != xy0))
        dev.step(torch.from_numpy(a).cuda())
        assert same(dev.step_blocks()[0].cpu().numpy(), want_raw), step
        assert np.all(ref.held == 0)
    assert moved


@pytest.mark.parametrize("n", [1, 5, 65])
def test_scripted_actions_match_the_definition(gcrl, n):
    """env_scripted_kernel on every state of an episode and a half — approach, closing, carrying, the re-seeded episode — with and
    without noise; the output tensor has room past N that keeps its poison (the entry writes N rows and no more)."""
    dev, ref = _env_pair(gcrl, n, seed=5, T=20)
    for step in range(30):
        a = dev.scripted_actions()
        assert a.dtype == torch.float32 and tuple(a.shape) == (n, 4) and a.is_cuda
        want = P.scripted_actions(ref)
        assert np.array_equal(bits(a.cpu().numpy()), bits(want)), (n, step)
        noisy = dev.scripted_actions(noise_std=0.25, seed=77, counter=step)
        assert np.array_equal(bits(noisy.cpu().numpy()), bits(_noisy(gcrl, ref, 0.25, 77, step))), (n, step)
        use = _noisy(gcrl, ref, 0.05, 1, step) if step % 3 == 2 else want
        ref.step(use); dev.step(torch.from_numpy(use).cuda())
    assert np.any(ref.held == 1) or n == 1
    out = torch.full((n + 3, 4), -77.25, device="cuda")
    gcrl._ffi.check(gcrl._ffi.lib.gcrl_env_scripted_act(dev.handle, out.data_ptr(), 0.0, 0, 0, gcrl._ffi.stream_handle()))
    out = out.cpu().numpy()
    assert np.array_equal(bits(out[:n]), bits(P.scripted_actions(ref))) and np.all(out[n:] == f32(-77.25))
    assert dev.stats() == ref.stats()


def test_the_controller_solves_every_episode_on_the_device(gcrl):
    """scripted actions + env.step for one horizon at N = 64, nothing crossing to the host: 64 successes"""
    dev = gcrl.DeviceGoalEnv("pick", 64, seed=2, max_steps=50, threshold=0.05)
    for _ in range(50):
        dev.step(dev.scripted_actions())
    st = dev.stats()
    assert st["episodes"] == 64 and st["successes"] == 64, st


def test_poison_past_n_in_a_larger_action_tensor_is_not_read(gcrl):
    """the step reads N rows of the action tensor: rows past them may hold anything"""
    dev, ref = _env_pair(gcrl, 5)
    big = torch.full((9, 4), float("nan"), device="cuda")
    a = _actions(np.random.default_rng(2), 5)
    big[:5] = torch.from_numpy(a).cuda()
    want_raw, want_pay = ref.step(a)
    dev.step(big[:5])
    assert same(dev.step_blocks()[0].cpu().numpy(), want_raw) and same(dev.step_blocks()[1].cpu().numpy()[:, :10], want_pay[:, :10])


def test_refusals_name_their_field_and_leave_the_handle_alone(gcrl):
    dev, _ = _env_pair(gcrl, 5)
    dev.step(torch.zeros((5, 4), device="cuda"))
    before = dev.save_state()
    push = gcrl.DeviceGoalEnv("push", 5, seed=3, max_steps=T_STEPS)
    push_before = push.save_state()
    with pytest.raises(ValueError, match="kind"):
        dev.load_state(push_before)                  # a push blob into a pick env
    with pytest.raises(ValueError, match="kind"):
        push.load_state(before)                      # and the reverse
    assert np.array_equal(dev.save_state(), before) and np.array_equal(push.save_state(), push_before)
    assert push_before.size == 40 + 5 * (12 * 4 + 4 + 24 + 8 + 16 * 4)     # the other kinds' records keep their 12 floats
    for field, other in dict(num_envs=gcrl.DeviceGoalEnv("pick", 4, seed=3, max_steps=T_STEPS),
                             max_steps=gcrl.DeviceGoalEnv("pick", 5, seed=3, max_steps=T_STEPS + 1),
                             threshold=gcrl.DeviceGoalEnv("pick", 5, seed=3, max_steps=T_STEPS, threshold=0.06)).items():
        with pytest.raises(ValueError, match=field):
            dev.load_state(other.save_state())
        assert np.array_equal(dev.save_state(), before), field
    err = (ValueError, gcrl._ffi.GcrlError)
    with pytest.raises(err, match="threshold"):
        gcrl.DeviceGoalEnv("pick", 2, threshold=0.08)
    with pytest.raises(ValueError, match="actions"):
        dev.step(torch.zeros((5, 3), device="cuda"))
    for kind in ("reach", "push"):                   # their controllers are not built
        other = gcrl.DeviceGoalEnv(kind, 2)
        with pytest.raises(err, match="kind"):
            other.scripted_actions()
        out = torch.zeros((2, 4), device="cuda")
        assert gcrl._ffi.lib.gcrl_env_scripted_act(other.handle, out.data_ptr(), 0.0, 0, 0, gcrl._ffi.stream_handle()) == -1
        assert "kind" in gcrl._ffi.last_error()
    with pytest.raises(err, match="noise_std"):
        dev.scripted_actions(noise_std=-1.0)
    assert np.array_equal(dev.save_state(), before)
