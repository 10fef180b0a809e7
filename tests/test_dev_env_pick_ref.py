"""Host tests (no GPU) of tests/dev_env_pick_ref.py, the numpy definition of the `pick` device environment (gcrl_amd.DeviceGoalEnv("pick");
csrc/dev_env.hip), of the exploration streams at its action width and of its scripted controller (csrc/dev_env_script.hip):
determinism, independence of an env's episodes from N, finite states inside the box above the table for any action bits, that
idling solves nothing, that open fingers never move the object, that the scripted controller in float32 solves every episode, how
a released object falls, that no episode starts near its goal, the streams against oracle/device_rng_oracle.py, and that the three
env units compile for gfx950 with no scratch."""
import os
import re
import subprocess

import numpy as np
import pytest

import dev_env_pick_ref as P
import dev_env_ref as E
from oracle.device_rng_oracle import hash_normal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
T = 50


def bits(x):
    return np.ascontiguousarray(np.asarray(x, f32)).view(np.uint32)


def nasty_actions(gen, n):
    a = gen.uniform(-3, 3, (n, 4)).astype(f32)
    a[gen.random((n, 4)) < 0.1] = np.inf
    a[gen.random((n, 4)) < 0.1] = -np.inf
    a[gen.random((n, 4)) < 0.1] = np.nan
    return a


def test_ref_is_deterministic():
    outs = []
    for _ in range(2):
        env, gen = P.RefPickEnv(5, seed=7, max_steps=9), np.random.default_rng(3)
        outs.append([env.step(nasty_actions(gen, 5)) for _ in range(21)] + [(env.rows, env.state_array())])
    for (r0, p0), (r1, p1) in zip(*outs):
        assert np.array_equal(bits(r0), bits(r1)) and np.array_equal(bits(p0), bits(p1))


def test_dimensions_and_layout():
    env = P.RefPickEnv(3, seed=1, max_steps=9)
    assert env.D == 20 and P.A == 4 and env.rows.shape == (3, 23) and env.state_array().shape == (3, 18)
    raw, pay = env.step(np.full((3, 4), 0.5, f32))
    assert raw.shape == (3 * (2 * 20 + 4 * 3),) and pay.shape == (3, 32)
    obs, nobs, dg, ndg, ag, nag = env.split(raw)
    assert np.array_equal(pay[:, 3:7], np.full((3, 4), 0.5, f32)) and np.array_equal(bits(pay[:, 7:10]), bits(nag))
    assert np.array_equal(bits(nobs[:, 3:6]), bits(nag)) and np.array_equal(bits(dg), bits(ndg)) and np.all(pay[:, 10:] == 0)
    assert np.array_equal(bits(obs[:, 15]), bits(np.full(3, P.OPEN))) and np.all(obs[:, 19] == 0) and np.all(nobs[:, 19] == f32(1) / f32(9))


def test_episode_j_of_an_env_does_not_depend_on_n():
    gen = np.random.default_rng(11)
    acts = gen.uniform(-1, 1, (25, 4)).astype(f32)
    rows = []
    for n in (3, 8):
        env = P.RefPickEnv(n, seed=5, max_steps=10)
        seen = []
        for a in acts:
            seen.append(env.rows[2].copy())
            env.step(np.tile(a, (n, 1)))
        rows.append(np.stack(seen))
    assert np.array_equal(bits(rows[0]), bits(rows[1]))
    # ... nor on the step at which it is reached: episode 1 after a masked reset equals episode 1 after a full first episode
    a, b = P.RefPickEnv(4, seed=5, max_steps=10), P.RefPickEnv(4, seed=5, max_steps=10)
    a.reset(mask=[1, 1, 1, 1])
    for _ in range(10):
        b.step(np.zeros((4, 4), f32))
    assert np.array_equal(bits(a.rows), bits(b.rows)) and np.array_equal(bits(a.state_array()), bits(b.state_array()))


@pytest.mark.parametrize("mode", ["random", "inf", "-inf", "nan"])
def test_states_stay_finite_inside_the_box_and_above_the_table(mode):
    env, gen = P.RefPickEnv(16, seed=1), np.random.default_rng(0)
    for _ in range(2 * T + 7):
        a = nasty_actions(gen, 16) if mode == "random" else np.full((16, 4), float(mode), f32)
        raw, pay = env.step(a)
        assert np.all(np.isfinite(raw)) and np.all(np.abs(raw[: 2 * 16 * env.D]) <= 1.0)
        assert np.all(np.abs(env.p) <= E.BOX) and np.all(np.abs(env.q) <= E.BOX) and np.all(np.isfinite(env.goal))
        assert np.all(env.q[:, 2] >= 0) and np.all(env.p[:, 2] >= 0) and np.all((env.w >= 0) & (env.w <= P.OPEN))
        assert np.all(np.isfinite(pay[:, 1:3])) and np.all(np.isfinite(pay[:, 7:10]))
        assert set(np.unique(pay[:, 1])) <= {-1.0, 0.0} and set(np.unique(env.held)) <= {0.0, 1.0}
    assert env.stats()["episodes"] == 2 * 16


def test_no_episode_starts_near_its_goal_and_idling_solves_none_of_192():
    env = P.RefPickEnv(64, seed=3)
    two = 2 * float(env.thr)
    high = 0
    for ep in range(3):
        s = env.state_dict()
        assert np.all(np.abs(s["desired_goal"][:, 0] - s["achieved_goal"][:, 0]) >= two - 1e-7)
        assert np.all(np.linalg.norm(s["desired_goal"] - s["achieved_goal"], axis=1) >= two - 1e-7)
        assert np.all(np.linalg.norm(env.p - env.q, axis=1) > float(E.CONTACT))      # the gripper starts outside the grasp radius
        assert np.all(s["desired_goal"][:, 2] >= 0) and np.all(s["achieved_goal"][:, 2] == 0)
        high += int((s["desired_goal"][:, 2] > float(env.thr)).sum())
        for _ in range(T):
            env.step(np.zeros((64, 4), f32))
    assert env.stats()["episodes"] == 192 and env.stats()["successes"] == 0
    assert env.stats()["reward_sum"] == -192.0 * T
    assert 0.15 * 192 < high < 0.5 * 192, high                   # goals in the air, out of reach of a push along the table


def test_open_fingers_never_move_the_object():
    env, gen = P.RefPickEnv(16, seed=4, max_steps=T), np.random.default_rng(5)
    q0 = env.q.copy()
    for _ in range(T - 1):
        a = gen.uniform(-1, 1, (16, 4)).astype(f32)
        s = env.state_dict()
        a[:8, :3] = np.clip((s["achieved_goal"][:8] - env.p[:8]) / f32(0.04), -1, 1)     # half of them go and sit on the object
        a[:, 3] = 1.0
        env.step(a)
        assert np.array_equal(bits(env.q), bits(q0)) and np.all(env.held == 0) and np.all(env.w == P.OPEN)
    assert np.all(np.linalg.norm(env.p[:8] - env.q[:8], axis=1) < 1e-6)


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_scripted_controller_in_float32_solves_64_of_64(seed):
    env = P.RefPickEnv(16, seed=seed)
    lifted = 0
    for _ in range(200):
        a = P.scripted_actions(env)
        assert a.dtype == f32 and a.shape == (16, 4) and np.all(np.abs(a) <= 1)
        env.step(a)
        lifted += int((env.q[:, 2] > 0).sum())
    st = env.stats()
    assert st["episodes"] == 64 and st["successes"] == 64, st
    assert lifted > 0                                            # some goals were in the air and the object went there


def test_a_released_object_falls_to_the_table():
    env = P.RefPickEnv(1, seed=2, max_steps=60)
    while env.held[0] == 0:
        env.step(P.scripted_actions(env))
    for _ in range(6):                                           # straight up, fingers closed
        env.step(np.array([[0, 0, 1, -1]], f32))
    assert env.held[0] == 1 and env.q[0, 2] > f32(0.2)
    zs, held = [env.q[0, 2]], []
    for _ in range(10):
        env.step(np.array([[0, 0, 0, 1]], f32))                  # open: the grasp lasts until the fingers are CLOSE apart
        zs.append(env.q[0, 2]); held.append(env.held[0])
    assert held[0] == 1 and held[-1] == 0 and sorted(held, reverse=True) == held and 1 <= sum(held) <= 2
    for z0, z1, h in zip(zs, zs[1:], held):
        assert bits(z1) == bits(z0 if h else f32(max(f32(z0 - P.FALL), f32(0))))
    assert zs[-1] == 0 and zs[0] > zs[5] > 0
    xy = env.q[0, :2].copy()
    env.step(np.array([[0, 0, 0, 1]], f32))
    assert env.q[0, 2] == 0 and np.array_equal(env.q[0, :2], xy)


def test_noisy_scripted_actions():
    env = P.RefPickEnv(5, seed=3)
    clean = P.scripted_actions(env)
    assert np.array_equal(bits(P.scripted_actions(env, noise_std=0.0, seed=9, c=4)), bits(clean))
    noisy = P.scripted_actions(env, noise_std=0.3, seed=9, c=4)
    ctr = (4 * 5 * 4 + np.arange(5 * 4, dtype=np.uint64)).reshape(5, 4)
    z = (hash_normal(9, ctr).astype(np.float64) * 0.3).astype(f32)
    assert np.array_equal(bits(noisy), bits(np.clip((clean + z).astype(f32), -1, 1)))
    assert not np.array_equal(noisy, clean) and np.all(np.abs(noisy) <= 1)


def test_exploration_streams_at_four_components_restate_the_device_hash():
    seed, n = 1898, 5
    for c in (0, 1, 7):
        ctr = (c * n * 4 + np.arange(n * 4, dtype=np.uint64)).reshape(n, 4)
        z = hash_normal(seed, ctr)
        assert np.array_equal(P.explore_noise(seed, c, n, 0.1), z.astype(np.float64) * 0.1)
        assert np.array_equal(P.explore_noise(seed, c, n, 1.0).astype(f32).view(np.uint32), z.view(np.uint32))
        za = hash_normal(np.uint64(seed ^ E.EPS_STREAM), ctr)
        assert np.array_equal(bits(P.epsilon_actions(seed, c, n)), bits(np.clip(za, -1, 1)))
    # the streams are laid out by the action width: the pick kind's are not the three-component ones
    assert not np.array_equal(P.explore_noise(seed, 1, n, 1.0)[:, :3], E.explore_noise(seed, 1, n, 1.0))


def test_env_units_compile_for_gfx950_without_scratch(tmp_path):
    """The three env units compiled to gfx950 assembly with the Makefile's flags: .private_segment_fixed_size is 0 for every kernel,
    env_scripted_kernel among them."""
    csrc = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)).split()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert "-ffp-contract=off" in flags
    sizes = {}
    for unit in ("dev_env.hip", "dev_env_group.hip", "dev_env_script.hip"):
        assert unit in srcs
        asm = tmp_path / (unit + ".s")
        subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, unit), "-o", str(asm)], check=True, cwd=csrc)
        found = re.findall(r"\.name:\s+(\S*_kernel\S*)\n((?:(?!\.name:).)*?)\.private_segment_fixed_size:\s+(\d+)", asm.read_text(), re.S)
        sizes.update({n: int(sz) for n, _, sz in found})
    for k in ("env_reset_kernel", "env_step_kernel", "env_step_pop_kernel", "env_reset_pop_kernel", "env_scripted_kernel"):
        assert sum(bool(re.search(r"\d" + k, n)) for n in sizes) == 1, (k, sizes)
    assert len(sizes) == 9 and all(v == 0 for v in sizes.values()), sizes
