"""Host tests (no GPU) of tests/dev_env_ref.py, the numpy definition of the two device-resident goal environments
(gcrl_amd.DeviceGoalEnv; csrc/dev_env.hip) and of the exploration stream of agent.collect: determinism, independence of an env's
episodes from N, finite states inside the box for any action bits, that `reach` and `push` can be solved and that `push` is never
solved by doing nothing, the noise and epsilon streams against oracle/device_rng_oracle.py, and that the new kernels use no scratch."""
import os
import re
import subprocess

import numpy as np
import pytest

import dev_env_ref as E
from oracle.device_rng_oracle import hash_normal, mix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
T = 50


def bits(x):
    return np.ascontiguousarray(np.asarray(x, f32)).view(np.uint32)


def nasty_actions(gen, n):
    a = gen.uniform(-3, 3, (n, 3)).astype(f32)
    a[gen.random((n, 3)) < 0.1] = np.inf
    a[gen.random((n, 3)) < 0.1] = -np.inf
    a[gen.random((n, 3)) < 0.1] = np.nan
    return a


@pytest.mark.parametrize("kind", ["reach", "push"])
def test_ref_is_deterministic(kind):
    outs = []
    for _ in range(2):
        env, gen = E.RefEnv(kind, 5, seed=7, max_steps=9), np.random.default_rng(3)
        outs.append([env.step(nasty_actions(gen, 5)) for _ in range(21)] + [(env.rows, np.zeros(1, f32))])
    for (r0, p0), (r1, p1) in zip(*outs):
        assert np.array_equal(bits(r0), bits(r1)) and np.array_equal(bits(p0), bits(p1))


@pytest.mark.parametrize("kind", ["reach", "push"])
def test_episode_j_of_an_env_does_not_depend_on_n(kind):
    """env 2 of N = 3 and of N = 8 see the same episodes 0, 1, 2 under the same actions — there is no state besides the counters."""
    gen = np.random.default_rng(11)
    acts = gen.uniform(-1, 1, (25, 3)).astype(f32)
    rows = []
    for n in (3, 8):
        env = E.RefEnv(kind, n, seed=5, max_steps=10)
        seen = []
        for a in acts:
            seen.append(env.rows[2].copy())
            env.step(np.tile(a, (n, 1)))
        rows.append(np.stack(seen))
    assert np.array_equal(bits(rows[0]), bits(rows[1]))
    # ... nor on the step at which it is reached: episode 1 after a masked reset equals episode 1 after a full first episode
    a, b = E.RefEnv(kind, 4, seed=5, max_steps=10), E.RefEnv(kind, 4, seed=5, max_steps=10)
    a.reset(mask=[1, 1, 1, 1])
    for _ in range(10):
        b.step(np.zeros((4, 3), f32))
    assert np.array_equal(bits(a.rows), bits(b.rows))


@pytest.mark.parametrize("kind", ["reach", "push"])
def test_states_stay_finite_and_inside_the_box(kind):
    env, gen = E.RefEnv(kind, 16, seed=1), np.random.default_rng(0)
    for _ in range(3 * T + 7):
        raw, pay = env.step(nasty_actions(gen, 16))
        assert np.all(np.isfinite(raw)) and np.all(np.abs(raw[: 2 * 16 * env.D]) <= 1.0)
        assert np.all(np.abs(env.p) <= E.BOX) and np.all(np.abs(env.q) <= E.BOX) and np.all(np.isfinite(env.goal))
        assert np.all(np.isfinite(pay[:, 1:3])) and np.all(np.isfinite(pay[:, 6:9]))
        assert set(np.unique(pay[:, 1])) <= {-1.0, 0.0}
    assert env.stats()["episodes"] == 3 * 16


def test_reach_proportional_controller_solves_all_64():
    env = E.RefEnv("reach", 64, seed=2)
    for _ in range(T):
        s = env.state_dict()
        env.step(np.clip((s["desired_goal"] - s["achieved_goal"]) / f32(0.04), -1, 1))
    assert env.stats() == dict(episodes=64, successes=64, reward_sum=env.stats()["reward_sum"])


def test_push_never_starts_solved_and_idling_solves_nothing():
    env = E.RefEnv("push", 64, seed=2)
    two = 2 * float(env.thr)
    for ep in range(3):
        s = env.state_dict()
        assert np.all(np.abs(s["desired_goal"][:, 0] - s["achieved_goal"][:, 0]) >= two - 1e-7)
        assert np.all(np.linalg.norm(s["desired_goal"] - s["achieved_goal"], axis=1) > float(env.thr))
        assert np.all(np.linalg.norm(env.p - env.q, axis=1) > float(E.CONTACT))      # the pusher starts outside the contact radius
        for _ in range(T):
            env.step(np.zeros((64, 3), f32))
    assert env.stats()["episodes"] == 3 * 64 and env.stats()["successes"] == 0
    assert env.stats()["reward_sum"] == -3.0 * 64 * T


def push_controller(env):
    """Go behind the puck at the spawn height, come down, then push along the line to the goal."""
    p, q, g = env.p.astype(np.float64), env.q.astype(np.float64), env.goal.astype(np.float64)
    act = np.zeros((env.n, 3))
    for i in range(env.n):
        to_goal = g[i, :2] - q[i, :2]
        dist = np.linalg.norm(to_goal)
        if dist < 1e-9:
            continue
        behind = q[i, :2] - 0.03 * to_goal / dist
        off = behind - p[i, :2]
        in_contact = np.linalg.norm(p[i] - q[i]) < float(E.CONTACT) - 1e-6
        if in_contact:
            a = to_goal / 0.04
            act[i, :2] = a / max(1.0, np.max(np.abs(a)))          # scaled, not clipped per axis: the push keeps its direction
        elif np.max(np.abs(off)) > 1e-6:
            act[i, :2] = np.clip(off / 0.04, -1, 1)
            act[i, 2] = np.clip((float(E.LIFT) - p[i, 2]) / 0.04, -1, 1)
        else:
            act[i, 2] = np.clip((0.0 - p[i, 2]) / 0.04, -1, 1)
    return act.astype(f32)


def test_push_scripted_controller_solves_all_64():
    env = E.RefEnv("push", 64, seed=2)
    for _ in range(T):
        env.step(push_controller(env))
    st = env.stats()
    assert st["episodes"] == 64 and st["successes"] == 64, st


def test_exploration_streams_restate_the_device_hash():
    seed, n = 1898, 5
    for c in (0, 1, 7):
        ctr = (c * n * 3 + np.arange(n * 3, dtype=np.uint64)).reshape(n, 3)
        z = hash_normal(seed, ctr)
        assert np.array_equal(E.explore_noise(seed, c, n, 0.1), z.astype(np.float64) * 0.1)
        assert np.array_equal(E.explore_noise(seed, c, n, 1.0).astype(f32).view(np.uint32), z.view(np.uint32))     # SAC / TQC: the eps is the hash value
        za = hash_normal(np.uint64(seed ^ E.EPS_STREAM), ctr)
        assert np.array_equal(bits(E.epsilon_actions(seed, c, n)), bits(np.clip(za, -1, 1)))
        # the epsilon uniform: the ring's multiply-high reduction of the 64-bit counter hash, 24 bits
        with np.errstate(over="ignore"):
            h = int(mix64(mix64(np.uint64(seed) ^ (np.uint64(E.EPS_STREAM) * np.uint64(0xD1342543DE82EF95))) + np.uint64(c)))
        assert E.epsilon_uniform(seed, c) == (((h >> 32) << 24) >> 32) * 2.0 ** -24
    u = np.array([E.epsilon_uniform(seed, c) for c in range(4000)])
    assert 0.0 <= u.min() and u.max() < 1.0 and abs((u < 0.2).mean() - 0.2) < 0.03
    e = E.explore_noise(seed, 3, 4096, 1.0)
    assert abs(e.mean()) < 0.03 and abs(e.std() - 1.0) < 0.03


def test_new_kernels_use_no_scratch(tmp_path):
    """dev_env.hip compiled to gfx950 assembly with the Makefile's flags: .private_segment_fixed_size is 0 for every kernel of the unit"""
    csrc = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)).split()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    assert "dev_env.hip" in re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split() and "-ffp-contract=off" in flags
    asm = tmp_path / "dev_env.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "dev_env.hip"), "-o", str(asm)], check=True, cwd=csrc)
    found = re.findall(r"\.name:\s+(\S*_kernel\S*)\n((?:(?!\.name:).)*?)\.private_segment_fixed_size:\s+(\d+)", asm.read_text(), re.S)
    sizes = {n: int(sz) for n, _, sz in found}
    for k in ("env_reset_kernel", "env_step_kernel", "proc_pack_kernel", "clipped_normal_fill_kernel", "normal_fill_kernel", "round_to_f32_kernel"):
        assert sum(bool(re.search(r"\d" + k, n)) for n in sizes) == 1, (k, sizes)     # (mangled names: the length precedes the identifier)
    assert len(sizes) == 6 and all(v == 0 for v in sizes.values()), sizes
