"""CPU (-m "not gpu"): the evaluation rule and the group rule as tests/evaluate_ref.py states them over tests/dev_env_ref.py — what
agent.evaluate, pop.evaluate and gcrl_amd.DeviceGoalEnvGroup are held to on the GPU (tests/test_gpu_pop_collect.py,
tests/test_gpu_env_group.py).  No device entry is called here."""
import numpy as np
import pytest

import dev_env_ref as E
import evaluate_ref as V

THR = 0.05


def test_the_proportional_controller_scores_64_of_64_on_reach():
    # 12 steps of 0.04 cover the farthest spawn (0.3 per component) with room to spare
    env = E.RefEnv("reach", 8, seed=3, max_steps=12, threshold=THR)
    r = V.evaluate(env, V.proportional, 64)
    assert r["episodes"] == 64 and r["successes"] == 64 and r["success_rate"] == 1.0
    assert -64 * 12 < r["reward_sum"] < 0                 # -1 per step outside the threshold, -0 inside
    assert env.stats()["episodes"] == 64


def test_idling_scores_0_of_192_on_push():
    # the goal lies at least 2 thr from the puck and nothing moves the puck
    env = E.RefEnv("push", 6, seed=5, max_steps=4, threshold=THR)
    r = V.evaluate(env, V.idle, 192)
    assert r == dict(episodes=192, successes=0, success_rate=0.0, reward_sum=-192.0 * 4)


@pytest.mark.parametrize("episodes,ran", [(1, 4), (4, 4), (5, 8), (10, 12)])
def test_episodes_round_up_to_a_multiple_of_n(episodes, ran):
    env = E.RefEnv("reach", 4, seed=1, max_steps=3, threshold=THR)
    assert V.evaluate(env, V.idle, episodes)["episodes"] == ran
    assert np.all(env.t == 0) and np.all(env.episode == ran // 4)


def test_reset_true_scores_the_same_episodes_every_time_and_reset_false_the_difference():
    env = E.RefEnv("reach", 4, seed=9, max_steps=12, threshold=THR)
    first = V.evaluate(env, V.proportional, 8)
    again = V.evaluate(env, V.proportional, 8)
    assert first == again                                  # episodes 0 and 1 of every env, both times
    more = V.evaluate(env, V.idle, 4, reset=False)         # episode 2 of every env, on top of the counters
    assert more["episodes"] == 4 and env.stats()["episodes"] == 12
    assert more["successes"] == env.stats()["successes"] - first["successes"]
    assert more["reward_sum"] == env.stats()["reward_sum"] - first["reward_sum"]
    env.step(np.zeros((4, 3), E.f32))
    before = (env.stats(), env.t.copy(), env.p.copy())
    with pytest.raises(ValueError, match=" t: "):
        V.evaluate(env, V.idle, 4, reset=False)
    assert before[0] == env.stats() and np.array_equal(before[1], env.t) and np.array_equal(before[2], env.p)
    with pytest.raises(ValueError, match="episodes"):
        V.evaluate(env, V.idle, 0)


@pytest.mark.parametrize("kind", ["reach", "push"])
def test_member_m_of_a_group_is_a_standalone_env_of_seed_m_whatever_p_is(kind):
    seeds, n, T = [11, 4, 11], 3, 5
    gen = np.random.default_rng(0)
    acts = gen.uniform(-1.5, 1.5, (2 * T + 3, 3, n, 3)).astype(E.f32)
    big = V.RefGroup(kind, 3, n, seeds, max_steps=T, threshold=THR)
    ones = [V.RefGroup(kind, 1, n, [s], max_steps=T, threshold=THR) for s in seeds]
    alone = [E.RefEnv(kind, n, seed=s, max_steps=T, threshold=THR) for s in seeds]
    for step, a in enumerate(acts):
        out = big.step(a)
        for m in range(3):
            raw1, pay1 = ones[m].step(a[m:m + 1])[0]
            raw0, pay0 = alone[m].step(a[m])
            for x, y, z in ((out[m][0], raw1, raw0), (out[m][1], pay1, pay0)):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(x.view(np.uint32), z.view(np.uint32)), (step, m)
        if step == T + 1:                                   # a member's envs on to their next episodes, the others untouched
            big.reset(members=[1]); ones[1].reset(members=[0]); alone[1].reset(np.ones(n, bool))
    assert big.stats() == [e.stats() for e in alone] == [g.stats()[0] for g in ones]
    # members of equal seeds meet the same episodes (here under different actions): identical evaluation sets
    assert np.array_equal(big.envs[0].goal.view(np.uint32), big.envs[2].goal.view(np.uint32))
    assert not np.array_equal(big.envs[0].goal, big.envs[1].goal)


def test_the_group_kernels_use_no_scratch(tmp_path):
    """csrc/dev_env_group.hip compiled to gfx950 assembly with the Makefile's flags: .private_segment_fixed_size is 0 for both kernels,
    although they index per-member kernel arguments with a member index that differs across a wave"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "goal-conditioned-rl-framework_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)).split()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    assert "dev_env_group.hip" in re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split() and "-ffp-contract=off" in flags
    asm = tmp_path / "dev_env_group.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "dev_env_group.hip"), "-o", str(asm)], check=True, cwd=csrc)
    found = re.findall(r"\.name:\s+(\S*_kernel\S*)\n((?:(?!\.name:).)*?)\.private_segment_fixed_size:\s+(\d+)", asm.read_text(), re.S)
    sizes = {n: int(sz) for n, _, sz in found}
    for k in ("env_step_pop_kernel", "env_reset_pop_kernel"):
        assert sum(bool(re.search(r"\d" + k, n)) for n in sizes) == 1, (k, sizes)
    assert len(sizes) == 2 and all(v == 0 for v in sizes.values()), sizes
