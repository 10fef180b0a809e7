"""GPU (-m gpu): the `glide` device environment (gcrl_amd.DeviceGoalEnv("glide"); csrc/dev_env.hip, dev_env_body.h) and its scripted
controller (csrc/dev_env_script.hip env_scripted_kernel) held bit for bit to their numpy definition tests/dev_env_glide_ref.py:
env_reset_kernel and env_step_kernel over two full episodes plus three steps at T = 10, the first episode under the controller's
actions and the rest under actions with out-of-range, infinite and NaN components, float32 and float64 action tensors in turn; the
raw and pay blocks of every step, the acting rows, the whole state blob (15-float records) and the counters; masked and full resets;
a state saved and loaded into a fresh handle; poison past N; refused loads across kinds; scripted_actions() with and without noise.

The reference run of every N is made once, on the host, before the device is touched, and is asserted to contain a contact step, a
free glide step with a moving puck, a clamp at the far wall, a clamp in y and a horizon re-seed.  The seed of each N is the first
one whose run has the contact and the glide.  The two wall clamps come from a state the test loads into the device mid-run (the
reference's own blob with env 0's puck placed next to the corner and moving into it): from a reset no sequence of actions brings a
puck to x = 0.9 — a contact leaves it below 0.39 and a glide adds at most STEP * FRICTION / (1 - FRICTION) = 0.36 — so that clamp
guards loaded states alone, and the test reaches it the way such a state arrives.

No case provokes a fault: every buffer compared or poisoned is the handle's own block (read only) or a test-owned tensor with room
past N; the kernels' own guard (env index >= N does nothing) keeps every address inside its allocation."""
import functools
import struct

import numpy as np
import pytest
import torch

import dev_env_glide_ref as S
import test_gpu_dev_env as TE
import test_gpu_env_group as TG

pytestmark = pytest.mark.gpu

f32 = np.float32
T_STEPS = 10         # horizon of the test envs: 2 T + 3 = 23 steps
STEPS = 2 * T_STEPS + 3
INJECT = T_STEPS + 3  # before this step of the run the corner state is loaded
same, bits, _actions = TE._same, TE.bits, TE._actions


def _env_pair(gcrl, n, seed=3, thr=0.05, T=T_STEPS):
    return gcrl.DeviceGoalEnv("glide", n, seed=seed, max_steps=T, threshold=thr), S.RefGlideEnv(n, seed=seed, max_steps=T, threshold=thr)


def _noisy(gcrl, ref, noise_std, seed, c):
    """the definition's noisy actions of vector step c, the hash normals taken from the device's own fill (their transcendental functions
    differ from numpy's by ulps); the counters and the arithmetic around them are the definition's"""
    z = TG._normals(gcrl, seed, c * ref.n * 3, ref.n * 3)
    return S.scripted_actions(ref, noise_std=noise_std, seed=seed, c=c, normals=z)


def _blob(ref, steps):
    """the bytes gcrl_env_save_state writes for a device env in the reference's state"""
    head = struct.pack("<IiiifIQq", 0x564E4547, S.KIND, ref.n, ref.T, float(ref.thr), 0, ref.seed, steps)
    cnt = np.stack([ref.episode, ref.episodes, ref.successes], 1).astype(np.uint64)
    parts = [ref.state_array(), ref.t.astype(np.int32), cnt, ref.reward_sum.astype(np.float64), ref.rows]
    return np.frombuffer(head + b"".join(np.ascontiguousarray(x).tobytes() for x in parts), np.uint8)


def _check(dev, ref, steps, what):
    assert same(dev.acting_rows()["rows"].cpu().numpy(), ref.rows), what
    assert np.array_equal(dev.save_state(), _blob(ref, steps)), what


def _run(n, seed):
    """The reference's run alone: per step the actions, the blocks and the state blob it leaves, the blob loaded before step INJECT,
    what the run contained, and the reference at the end."""
    ref = S.RefGlideEnv(n, seed=seed, max_steps=T_STEPS)
    gen = np.random.default_rng(100 * n + 4)
    seen = dict(contact=False, glide=False, far=False, y=False, reseed=False)
    steps, loaded = [], None
    for step in range(STEPS):
        if step == INJECT:                                     # env 0's puck next to the far corner, moving into it; its pusher is out of contact
            ref.q[0] = [f32(0.88), f32(0.29), f32(0.0)]
            ref.vel_q[0] = [f32(0.05), f32(0.03), f32(0.0)]
            loaded = _blob(ref, step)
        a = S.scripted_actions(ref) if step < T_STEPS else _actions(gen, n)
        raw, pay = ref.step(a)
        live = ~ref.reseeded
        seen["contact"] |= bool(ref.contact.any())
        own = np.arange(n) != 0 if step >= INJECT else np.ones(n, bool)      # (not the glide the loaded state brings with it)
        seen["glide"] |= bool((~ref.contact & live & own & np.any(ref.vel_q != 0, axis=1)).any())
        seen["far"] |= bool(ref.hit_far.any()); seen["y"] |= bool(ref.hit_y.any()); seen["reseed"] |= bool(ref.reseeded.any())
        steps.append((a, raw, pay, ref.rows, _blob(ref, step + 1)))
    return steps, loaded, seen, ref


@functools.lru_cache(maxsize=None)
def _reference(n):
    for seed in range(3, 40):
        out = _run(n, seed)
        if out[2]["contact"] and out[2]["glide"]:
            return (seed,) + out
    raise AssertionError("no seed")


@pytest.mark.parametrize("n", [1, 5, 65])
def test_reset_and_step_match_the_definition(gcrl, n):
    seed, steps, loaded, seen, ref = _reference(n)
    assert all(seen.values()), (n, seed, seen)                  # from the reference alone, before anything is compared
    dev = gcrl.DeviceGoalEnv("glide", n, seed=seed, max_steps=T_STEPS, threshold=0.05)
    assert (dev.obs_dim, dev.goal_dim, dev.ac_dim, dev.num_envs, dev.max_steps) == (16, 3, 3, n, T_STEPS)
    assert dev.save_state().size == 40 + n * (15 * 4 + 4 + 24 + 8 + 19 * 4)
    _check(dev, S.RefGlideEnv(n, seed=seed, max_steps=T_STEPS), 0, "fresh")
    for step, (a, want_raw, want_pay, want_rows, want_blob) in enumerate(steps):
        if step == INJECT:
            dev.load_state(loaded)
        dev.step(torch.from_numpy(a).cuda() if step % 2 == 0 else torch.from_numpy(a.astype(np.float64)).cuda())     # float32 and float64 actions
        raw, pay = dev.step_blocks()
        assert same(raw.cpu().numpy(), want_raw), (n, step)
        pay = pay.cpu().numpy()
        assert same(pay[:, :9], want_pay[:, :9]) and np.all(pay[:, 9:] == 0), (n, step)
        assert same(dev.acting_rows()["rows"].cpu().numpy(), want_rows), (n, step)
        assert np.array_equal(dev.save_state(), want_blob), (n, step)
    assert dev.stats() == ref.stats() and dev.stats()["episodes"] == 2 * n
    ref = S.RefGlideEnv(n, seed=seed, max_steps=T_STEPS)         # a copy of the shared reference at its end, to go on from
    _load_ref(ref, steps[-1][4])
    gen = np.random.default_rng(n)
    # masked reset: the selected envs go on to their next episode, the others stay where they are
    mask = (np.arange(n) % 2 == 0)
    dev.reset(mask); ref.reset(mask)
    _check(dev, ref, STEPS, "masked reset")
    # state saved mid-episode into a fresh handle: the continuation is bitwise
    blob = dev.save_state()
    twin = gcrl.DeviceGoalEnv("glide", n, seed=999, max_steps=T_STEPS, threshold=0.05)
    twin.load_state(blob)
    assert twin.seed == seed and twin.stats() == dev.stats()
    for step in range(T_STEPS + 1):
        a = _actions(gen, n)
        ref.step(a)
        a = torch.from_numpy(a).cuda()
        dev.step(a); twin.step(a)
        assert same(dev.step_blocks()[0].cpu().numpy(), twin.step_blocks()[0].cpu().numpy())
    assert np.array_equal(dev.save_state(), twin.save_state())
    _check(twin, ref, STEPS + T_STEPS + 1, "resumed")
    # full reset: back to episode 0, counters to zero
    dev.reset()
    _check(dev, S.RefGlideEnv(n, seed=seed, max_steps=T_STEPS), 0, "full reset")
    assert dev.stats() == dict(episodes=0, successes=0, reward_sum=0.0)


def _load_ref(ref, blob):
    """the reference put into the state of a blob (the inverse of _blob)"""
    n, o = ref.n, 40
    def take(dtype, count):
        nonlocal o
        x = np.frombuffer(blob.tobytes(), dtype, count, o)
        o += x.nbytes
        return x.copy()
    st = take(f32, n * S.STATE_W).reshape(n, S.STATE_W)
    ref.p, ref.q, ref.vel, ref.goal, ref.vel_q = (st[:, k:k + 3].copy() for k in (0, 3, 6, 9, 12))
    ref.t = take(np.int32, n)
    cnt = take(np.uint64, n * 3).reshape(n, 3)
    ref.episode, ref.episodes, ref.successes = cnt[:, 0].copy(), cnt[:, 1].copy(), cnt[:, 2].copy()
    ref.reward_sum = take(np.float64, n)


@pytest.mark.parametrize("n", [1, 5, 65])
def test_scripted_actions_match_the_definition(gcrl, n):
    """env_scripted_kernel on every state of an episode and a half — rising, travelling, descending, carrying, the strike, hands off,
    the re-seeded episode — with and without noise; the output tensor has room past N that keeps its poison (the entry writes N rows
    and no more)."""
    dev, ref = _env_pair(gcrl, n, seed=5, T=30)
    seen = dict(contact=False, glide=False)
    for step in range(45):
        a = dev.scripted_actions()
        assert a.dtype == torch.float32 and tuple(a.shape) == (n, 3) and a.is_cuda
        want = S.scripted_actions(ref)
        assert np.array_equal(bits(a.cpu().numpy()), bits(want)), (n, step)
        noisy = dev.scripted_actions(noise_std=0.25, seed=77, counter=step)
        assert np.array_equal(bits(noisy.cpu().numpy()), bits(_noisy(gcrl, ref, 0.25, 77, step))), (n, step)
        use = _noisy(gcrl, ref, 0.05, 1, step) if step % 3 == 2 else want
        ref.step(use); dev.step(torch.from_numpy(use).cuda())
        seen["contact"] |= bool(ref.contact.any())
        seen["glide"] |= bool((~ref.contact & np.any(ref.vel_q != 0, axis=1)).any())
    assert all(seen.values()), seen
    out = torch.full((n + 3, 3), -77.25, device="cuda")
    gcrl._ffi.check(gcrl._ffi.lib.gcrl_env_scripted_act(dev.handle, out.data_ptr(), 0.0, 0, 0, gcrl._ffi.stream_handle()))
    out = out.cpu().numpy()
    assert np.array_equal(bits(out[:n]), bits(S.scripted_actions(ref))) and np.all(out[n:] == f32(-77.25))
    assert dev.stats() == ref.stats()
    _check(dev, ref, 45, "after the controller's steps")


def test_the_controller_solves_its_episodes_on_the_device(gcrl):
    """scripted actions + env.step for one horizon at N = 64, nothing crossing to the host: the definition's count (64 of 64 at seed 0;
    tests/test_dev_env_glide_ref.py holds the definition to at least 60)"""
    dev = gcrl.DeviceGoalEnv("glide", 64, seed=0, max_steps=50, threshold=0.05)
    for _ in range(50):
        dev.step(dev.scripted_actions())
    st = dev.stats()
    assert st["episodes"] == 64 and st["successes"] >= 60, st


def test_poison_past_n_in_a_larger_action_tensor_is_not_read(gcrl):
    """the step reads N rows of the action tensor: rows past them may hold anything"""
    dev, ref = _env_pair(gcrl, 5)
    big = torch.full((9, 3), float("nan"), device="cuda")
    a = _actions(np.random.default_rng(2), 5)
    big[:5] = torch.from_numpy(a).cuda()
    want_raw, want_pay = ref.step(a)
    dev.step(big[:5])
    assert same(dev.step_blocks()[0].cpu().numpy(), want_raw) and same(dev.step_blocks()[1].cpu().numpy()[:, :9], want_pay[:, :9])


def test_refusals_name_their_field_and_leave_the_handle_alone(gcrl):
    dev, _ = _env_pair(gcrl, 5)
    dev.step(torch.zeros((5, 3), device="cuda"))
    before = dev.save_state()
    for kind, words, rows in (("push", 12, 16), ("pick", 18, 23)):
        other = gcrl.DeviceGoalEnv(kind, 5, seed=3, max_steps=T_STEPS)
        other_before = other.save_state()
        with pytest.raises(ValueError, match="kind"):
            dev.load_state(other_before)                 # a push / pick blob into a glide env
        with pytest.raises(ValueError, match="kind"):
            other.load_state(before)                     # and the reverse
        assert np.array_equal(dev.save_state(), before) and np.array_equal(other.save_state(), other_before)
        assert other_before.size == 40 + 5 * (words * 4 + 4 + 24 + 8 + rows * 4)      # the other kinds' records keep their widths
    for field, other in dict(num_envs=gcrl.DeviceGoalEnv("glide", 4, seed=3, max_steps=T_STEPS),
                             max_steps=gcrl.DeviceGoalEnv("glide", 5, seed=3, max_steps=T_STEPS + 1),
                             threshold=gcrl.DeviceGoalEnv("glide", 5, seed=3, max_steps=T_STEPS, threshold=0.06)).items():
        with pytest.raises(ValueError, match=field):
            dev.load_state(other.save_state())
        assert np.array_equal(dev.save_state(), before), field
    err = (ValueError, gcrl._ffi.GcrlError)
    with pytest.raises(err, match="threshold"):
        gcrl.DeviceGoalEnv("glide", 2, threshold=0.08)
    with pytest.raises(ValueError, match="kind"):
        gcrl.DeviceGoalEnv("slide", 2)                   # the name stays unknown
    with pytest.raises(ValueError, match="actions"):
        dev.step(torch.zeros((5, 4), device="cuda"))
    with pytest.raises(err, match="noise_std"):
        dev.scripted_actions(noise_std=-1.0)
    assert np.array_equal(dev.save_state(), before)
