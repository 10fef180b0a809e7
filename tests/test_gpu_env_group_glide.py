"""GPU (-m gpu): gcrl_amd.DeviceGoalEnvGroup("glide") (csrc/dev_env_group.hip) alone, with no agent, held bit for bit to P standalone
DeviceGoalEnv("glide") twins — which tests/test_gpu_dev_env_glide.py holds to the numpy definition — stepped with the same actions: the
step blocks, the acting rows, member_state(m) (15-float state records), stats()[m]; a member on the epsilon step against a twin fed
the clipped normals; masked, per-member and full resets; poison past n in every member's slice of the rows, the data and the
[P][stride_n][3] noise and action blocks; a state round trip into a fresh group.  P = 3 (two members share a seed) with n = 5;
2 T + 3 steps at T = 10, float32 and float64 action tensors in turn, the first episode under the controller so that pucks are
struck and glide.

No case provokes a fault: what is poisoned are the group's own padding rows and floats (inside its allocations), read back only."""
import numpy as np
import pytest
import torch

import test_gpu_dev_env as TE
import test_gpu_env_group as TG

pytestmark = pytest.mark.gpu

f32 = np.float32
T_STEPS = 10
same = TG.same


def _scripted(twins):
    return np.stack([tw.scripted_actions().cpu().numpy() for tw in twins])


def test_group_members_are_standalone_glide_envs(gcrl):
    seeds, n = [4, 8, 4], 5
    P = len(seeds)
    group, twins = TG._make(gcrl, "glide", seeds, n, T=T_STEPS)
    assert (group.members, group.num_envs, group.obs_dim, group.ac_dim, group.max_steps, group.seeds) == (P, n, 16, 3, T_STEPS, seeds)
    rows, data, noise, act = group.padded_blocks()
    assert tuple(noise.shape) == tuple(act.shape) == (P, group.stride_n, 3) and rows.shape[2] == 19
    assert group.raw_floats == n * (2 * 16 + 4 * 3)
    TG._poison(group)
    for m, tw in enumerate(twins):
        assert same(group.acting_rows()["rows"][m].cpu().numpy(), tw.acting_rows()["rows"].cpu().numpy())
    gen = np.random.default_rng(100 * n + P)
    eps_member = P - 1
    glided = False
    for step in range(2 * T_STEPS + 3):
        a = np.stack([TE._actions(gen, n) for _ in range(P)])
        if step < T_STEPS:                                     # the first episode under the controller: travel, descend, strike, hands off
            a = _scripted(twins)
        eps = None
        if step % 5 == 2:                                      # one member takes an epsilon step: its slice of the tensor is not read
            sd, c0 = 0x1234 + step, step * n * 3
            eps = {eps_member: (sd, c0)}
            z = np.clip(TG._normals(gcrl, sd, c0, n * 3), -1, 1).astype(f32).reshape(n, 3)
            twins[eps_member].step(torch.from_numpy(z).cuda())
            a[eps_member] = np.nan
        dt = np.float32 if step % 2 == 0 else np.float64
        group.step(torch.from_numpy(a.astype(dt)).cuda(), eps=eps)
        for m, tw in enumerate(twins):
            if eps is None or m != eps_member:
                tw.step(torch.from_numpy(a[m].astype(dt)).cuda())
        TG._check(group, twins, (n, step))
        glided = glided or bool((group.acting_rows()["rows"][:, :, 12:14] != 0).any())     # the puck's velocity in the obs
    TG._check_state(group, twins, "after the steps")
    assert all(s["episodes"] == 2 * n for s in group.stats())
    assert glided, "no step of the test moved a puck"
    assert group.member_state(0).size == 40 + n * (15 * 4 + 4 + 24 + 8 + 19 * 4)
    # member-masked reset, then every env of one member
    mask = (np.arange(P * n).reshape(P, n) % 3 == 0)
    group.reset(mask)
    for m, tw in enumerate(twins):
        tw.reset(mask[m])
    TG._check_state(group, twins, "masked reset")
    group.reset(members=[P - 1]); twins[P - 1].reset(np.ones(n, bool))
    TG._check_state(group, twins, "member reset")
    # a state saved mid-episode into a fresh group of other seeds: the continuation is bitwise
    a = torch.from_numpy(np.stack([TE._actions(gen, n) for _ in range(P)])).cuda()
    group.step(a)
    for m, tw in enumerate(twins):
        tw.step(a[m].contiguous())
    fresh = gcrl.DeviceGoalEnvGroup("glide", P, n, [99] * P, max_steps=T_STEPS, threshold=0.05)
    fresh.load_state(group.save_state())
    assert fresh.seeds == seeds and fresh.stats() == group.stats()
    for step in range(3):
        a = torch.from_numpy(np.stack([TE._actions(gen, n) for _ in range(P)])).cuda()
        group.step(a); fresh.step(a)
        for m, tw in enumerate(twins):
            tw.step(a[m].contiguous())
        TG._check(fresh, twins, ("resumed", step))
    assert np.array_equal(group.save_state(), fresh.save_state())
    assert TG._poison_intact(group), "a word past a member's n envs was written"
    group.reset()
    for tw in twins:
        tw.reset()
    TG._check_state(group, twins, "full reset")
    assert group.stats() == [dict(episodes=0, successes=0, reward_sum=0.0)] * P
    assert TG._poison_intact(group)


def test_refusals_across_kinds(gcrl):
    mk = lambda kind="glide", P=2, n=3: gcrl.DeviceGoalEnvGroup(kind, P, n, list(range(P)), max_steps=T_STEPS, threshold=0.05)
    group = mk()
    group.step(torch.zeros((2, 3, 3), device="cuda"))
    before = group.save_state()
    for kind in ("push", "pick"):
        other = mk(kind)
        with pytest.raises(ValueError, match="kind"):
            group.load_state(other.save_state())
        with pytest.raises(ValueError, match="kind"):
            other.load_state(before)
    with pytest.raises(ValueError, match="actions"):
        group.step(torch.zeros((2, 3, 4), device="cuda"))
    with pytest.raises((ValueError, gcrl._ffi.GcrlError), match="threshold"):
        gcrl.DeviceGoalEnvGroup("glide", 2, 2, [0, 1], threshold=0.08)
    with pytest.raises(ValueError, match="kind"):
        gcrl.DeviceGoalEnvGroup("slide", 2, 2, [0, 1])
    assert np.array_equal(group.save_state(), before)
