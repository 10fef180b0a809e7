"""GPU (-m gpu): gcrl_amd.DeviceGoalEnvGroup (csrc/dev_env_group.hip env_step_pop_kernel, env_reset_pop_kernel) alone, with no agent, held
bit for bit to P standalone DeviceGoalEnv twins — which tests/test_gpu_dev_env.py holds to the numpy definition — stepped with the same
actions: the step blocks, the acting rows, member_state(m), stats()[m]; a member on the epsilon step against a twin fed the clipped
normals; masked, per-member and full resets; poison past n in every member's slice, the last member's included; a state loaded into a
fresh group; refused loads.  P = 3 with n = 1, 5, 65 (65 crosses the 64-thread workgroup edge inside a member and between members)
and P = 1 with n = 5, 65 (a one-member group runs env_step_kernel / env_reset_kernel, its one member also the epsilon member); 2 T + 3 steps, float32 and float64 action tensors in turn.

No case provokes a fault: what is poisoned are the group's own padding rows and floats (inside its allocations), read back only."""
import ctypes as C

import numpy as np
import pytest
import torch

import dev_env_ref as E
import test_gpu_dev_env as TE

pytestmark = pytest.mark.gpu

f32 = np.float32
T_STEPS = TE.T_STEPS
POISON = -77.25
same = TE._same


def _normals(gcrl, seed, ctr0, n):
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    gcrl._ffi.check(gcrl._ffi.lib.gcrl_hash_normal_fill(C.c_uint64(seed & (2**64 - 1)), C.c_uint64(ctr0), n, out.data_ptr(), gcrl._ffi.stream_handle()))
    return out.cpu().numpy()


def _make(gcrl, kind, seeds, n, thr=0.05, T=T_STEPS):
    group = gcrl.DeviceGoalEnvGroup(kind, len(seeds), n, seeds, max_steps=T, threshold=thr)
    twins = [gcrl.DeviceGoalEnv(kind, n, seed=s, max_steps=T, threshold=thr) for s in seeds]
    return group, twins


def _poison(group):
    rows, data, noise, act = group.padded_blocks()
    n = group.num_envs
    rows[:, n:] = POISON
    data[:, group.raw_floats + n * 32:] = POISON
    noise[:] = POISON
    act[:] = POISON
    torch.cuda.synchronize()


def _poison_intact(group):
    rows, data, noise, act = (x.cpu().numpy() for x in group.padded_blocks())
    n = group.num_envs
    assert group.stride_n >= n + 4 and data.shape[1] >= group.raw_floats + n * 32 + 4
    return bool(np.all(rows[:, n:] == POISON) and np.all(data[:, group.raw_floats + n * 32:] == POISON) and np.all(noise == POISON)
                and np.all(act == POISON))


def _check(group, twins, what):
    raw, pay = group.step_blocks()
    rows = group.acting_rows()["rows"]
    for m, tw in enumerate(twins):
        traw, tpay = tw.step_blocks()
        assert same(raw[m].cpu().numpy(), traw.cpu().numpy()), (what, m, "raw")
        assert same(pay[m].cpu().numpy(), tpay.cpu().numpy()), (what, m, "pay")
        assert same(rows[m].cpu().numpy(), tw.acting_rows()["rows"].cpu().numpy()), (what, m, "rows")


def _check_state(group, twins, what):
    stats = group.stats()
    for m, tw in enumerate(twins):
        assert np.array_equal(group.member_state(m), tw.save_state()), (what, m, "state blob")
        assert stats[m] == tw.stats(), (what, m)


@pytest.mark.parametrize("kind", ["reach", "push"])
@pytest.mark.parametrize("seeds,n", [([3, 8, 3], 1), ([3, 8, 3], 5), ([3, 8, 3], 65), ([6], 5), ([6], 65)])
def test_group_members_are_standalone_envs(gcrl, kind, seeds, n):
    P = len(seeds)
    group, twins = _make(gcrl, kind, seeds, n)
    assert (group.members, group.num_envs, group.obs_dim, group.max_steps, group.seeds) == (P, n, twins[0].obs_dim, T_STEPS, seeds)
    _poison(group)
    rows = group.acting_rows()["rows"]
    for m, tw in enumerate(twins):
        assert same(rows[m].cpu().numpy(), tw.acting_rows()["rows"].cpu().numpy())
    gen = np.random.default_rng(100 * n + P)
    eps_member = P - 1                                         # the last member: its epsilon steps also end the grid
    for step in range(2 * T_STEPS + 3):
        a = np.stack([TE._actions(gen, n) for _ in range(P)])
        if kind == "push" and step % T_STEPS in (1, 2):        # drive the pushers onto the pucks so that the contact branch runs
            r = group.acting_rows()["rows"].cpu().numpy()
            a = np.clip((np.concatenate([r[:, :, 3:5], np.zeros((P, n, 1), f32)], 2) - r[:, :, 0:3]) / f32(0.04), -1, 1).astype(f32)
        eps = None
        if step % 5 == 2:                                      # one member takes an epsilon step: its slice of the tensor is not read
            sd, c0 = 0x1234 + step, step * n * 3
            eps = {eps_member: (sd, c0)}
            z = np.clip(_normals(gcrl, sd, c0, n * 3), -1, 1).astype(f32).reshape(n, 3)
            twins[eps_member].step(torch.from_numpy(z).cuda())
            a[eps_member] = np.nan
        dt = np.float32 if step % 2 == 0 else np.float64
        group.step(torch.from_numpy(a.astype(dt)).cuda(), eps=eps)
        for m, tw in enumerate(twins):
            if eps is None or m != eps_member:
                tw.step(torch.from_numpy(a[m].astype(dt)).cuda())
        _check(group, twins, (kind, n, step))
    _check_state(group, twins, "after the steps")
    assert all(s["episodes"] == 2 * n for s in group.stats())
    # masked reset, then every env of one member
    mask = (np.arange(P * n).reshape(P, n) % 3 == 0)
    group.reset(mask)
    for m, tw in enumerate(twins):
        tw.reset(mask[m])
    _check_state(group, twins, "masked reset")
    group.reset(members=[P - 1]); twins[P - 1].reset(np.ones(n, bool))
    _check_state(group, twins, "member reset")
    # a state saved mid-episode into a fresh group of other seeds: the continuation is bitwise
    a = torch.from_numpy(np.stack([TE._actions(gen, n) for _ in range(P)])).cuda()
    group.step(a)
    for m, tw in enumerate(twins):
        tw.step(a[m].contiguous())
    blob = group.save_state()
    fresh = gcrl.DeviceGoalEnvGroup(kind, P, n, [99] * P, max_steps=T_STEPS, threshold=0.05)
    fresh.load_state(blob)
    assert fresh.seeds == seeds and fresh.stats() == group.stats()
    for step in range(T_STEPS + 1):
        a = torch.from_numpy(np.stack([TE._actions(gen, n) for _ in range(P)])).cuda()
        group.step(a); fresh.step(a)
        for m, tw in enumerate(twins):
            tw.step(a[m].contiguous())
        _check(fresh, twins, ("resumed", step))
    assert np.array_equal(group.save_state(), fresh.save_state())
    _check_state(fresh, twins, "resumed")
    assert _poison_intact(group), "a word past a member's n envs was written"
    # full reset: every member back to episode 0, counters to zero
    group.reset()
    for tw in twins:
        tw.reset()
    _check_state(group, twins, "full reset")
    assert group.stats() == [dict(episodes=0, successes=0, reward_sum=0.0)] * P
    assert _poison_intact(group)


def test_refused_loads_name_their_field_and_leave_the_group_alone(gcrl):
    mk = lambda kind="reach", P=3, n=5, T=T_STEPS, thr=0.05: gcrl.DeviceGoalEnvGroup(kind, P, n, list(range(P)), max_steps=T, threshold=thr)
    group = mk()
    group.step(torch.zeros((3, 5, 3), device="cuda"))
    before = group.save_state()
    others = dict(members=mk(P=2), kind=mk("push"), num_envs=mk(n=4), max_steps=mk(T=T_STEPS + 1), threshold=mk(thr=0.06))
    for field, other in others.items():
        with pytest.raises(ValueError, match=field):
            group.load_state(other.save_state())
        assert np.array_equal(group.save_state(), before), field
    with pytest.raises(ValueError, match="blob"):
        group.load_state(before[:-4])
    with pytest.raises(ValueError, match="blob"):                      # a standalone env's blob is not a group's
        group.load_state(gcrl.DeviceGoalEnv("reach", 5, seed=0, max_steps=T_STEPS).save_state())
    assert np.array_equal(group.save_state(), before)
    err = gcrl._ffi.GcrlError
    with pytest.raises(ValueError, match="kind"):
        gcrl.DeviceGoalEnvGroup("slide", 2, 2, [0, 1])
    with pytest.raises(ValueError, match="seeds"):
        gcrl.DeviceGoalEnvGroup("reach", 3, 2, [0, 1])
    with pytest.raises(err, match="members"):
        gcrl.DeviceGoalEnvGroup("reach", 17, 2, list(range(17)))
    with pytest.raises(err, match="num_envs"):
        gcrl.DeviceGoalEnvGroup("reach", 2, 1025, [0, 1])
    with pytest.raises(ValueError, match="actions"):
        group.step(torch.zeros((3, 4, 3), device="cuda"))
    with pytest.raises(ValueError, match="mask"):
        group.reset(np.ones(5, bool))
    with pytest.raises(ValueError, match="members"):
        group.reset(members=[3])
