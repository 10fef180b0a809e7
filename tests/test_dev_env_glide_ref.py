"""Host tests (no GPU) of tests/dev_env_glide_ref.py, the numpy definition of the `glide` device environment
(gcrl_amd.DeviceGoalEnv("glide"); csrc/dev_env.hip) and of its scripted controller (csrc/dev_env_script.hip): the kind is known to the
package while "slide" stays unknown, determinism, independence of an env's episodes from N and from the step they are reached at,
finite states inside their boxes for any action bits, that no episode starts or idles into its goal, that a puck in contact
stays short of every goal, how a free puck glides, and that the scripted controller in float32 solves its episodes.

Counts of the controller at seed 0, envs 0..63, episode 0, T = 50: 64 of 64 without noise; 25 of 64 with noise_std = 0.1 (recorded,
not asserted: a strike is one step, and noise on it moves the puck's resting place by a multiple of itself)."""
import numpy as np
import pytest

import dev_env_glide_ref as S
import dev_env_ref as E
from oracle.device_rng_oracle import hash_normal

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


def _package_kinds():
    """the package's kind table, read from its source: the module itself imports torch and loads the library"""
    import ast
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "goal-conditioned-rl-framework_amd", "src", "device_env.py")
    return ast.literal_eval(open(path).read().split("KINDS = ", 1)[1].split("\n", 1)[0])


@pytest.fixture(autouse=True)
def _the_definition_is_of_a_kind_the_package_has():
    assert _package_kinds()["glide"] == S.KIND


def test_the_package_knows_the_kind_and_still_refuses_slide():
    kinds = _package_kinds()
    assert kinds == {"reach": 0, "push": 1, "pick": 2, "glide": 3} and "slide" not in kinds


def test_ref_is_deterministic():
    outs = []
    for _ in range(2):
        env, gen = S.RefGlideEnv(5, seed=7, max_steps=9), np.random.default_rng(3)
        outs.append([env.step(nasty_actions(gen, 5)) for _ in range(21)] + [(env.rows, env.state_array())])
    for (r0, p0), (r1, p1) in zip(*outs):
        assert np.array_equal(bits(r0), bits(r1)) and np.array_equal(bits(p0), bits(p1))


def test_dimensions_and_layout():
    env = S.RefGlideEnv(3, seed=1, max_steps=9)
    assert env.D == 16 and S.A == 3 and env.rows.shape == (3, 19) and env.state_array().shape == (3, 15)
    raw, pay = env.step(np.full((3, 3), 0.5, f32))
    assert raw.shape == (3 * (2 * 16 + 4 * 3),) and pay.shape == (3, 32)
    obs, nobs, dg, ndg, ag, nag = env.split(raw)
    assert np.array_equal(pay[:, 3:6], np.full((3, 3), 0.5, f32)) and np.array_equal(bits(pay[:, 6:9]), bits(nag))
    assert np.array_equal(bits(nobs[:, 3:6]), bits(nag)) and np.array_equal(bits(dg), bits(ndg)) and np.all(pay[:, 9:] == 0)
    assert np.all(obs[:, 9:15] == 0) and np.all(obs[:, 15] == 0) and np.all(nobs[:, 15] == f32(1) / f32(9))
    assert np.array_equal(bits(nobs[:, 9:12]), bits(np.full((3, 3), f32(0.04) * f32(0.5))))
    assert np.all((dg[:, 0] >= f32(0.45)) & (dg[:, 0] <= f32(0.65))) and np.all(np.abs(dg[:, 1]) <= E.SPAWN) and np.all(dg[:, 2] == 0)


def test_episode_j_of_an_env_does_not_depend_on_n_nor_on_the_step_it_is_reached_at():
    gen = np.random.default_rng(11)
    acts = gen.uniform(-1, 1, (25, 3)).astype(f32)
    rows = []
    for n in (3, 8):
        env = S.RefGlideEnv(n, seed=5, max_steps=10)
        seen = []
        for a in acts:
            seen.append(env.rows[2].copy())
            env.step(np.tile(a, (n, 1)))
        rows.append(np.stack(seen))
    assert np.array_equal(bits(rows[0]), bits(rows[1]))
    a, b = S.RefGlideEnv(4, seed=5, max_steps=10), S.RefGlideEnv(4, seed=5, max_steps=10)
    a.reset(mask=[1, 1, 1, 1])
    for _ in range(10):
        b.step(gen.uniform(-1, 1, (4, 3)).astype(f32))
    assert np.array_equal(bits(a.rows), bits(b.rows)) and np.array_equal(bits(a.state_array()), bits(b.state_array()))


@pytest.mark.parametrize("mode", ["random", "inf", "-inf", "nan"])
def test_states_stay_finite_inside_their_boxes(mode):
    env, gen = S.RefGlideEnv(16, seed=1), np.random.default_rng(0)
    for _ in range(2 * T + 7):
        a = nasty_actions(gen, 16) if mode == "random" else np.full((16, 3), float(mode), f32)
        raw, pay = env.step(a)
        assert np.all(np.isfinite(raw)) and np.all(np.abs(raw[: 2 * 16 * env.D]) <= 1.2)
        assert np.all(np.abs(env.p) <= E.BOX) and np.all(np.isfinite(env.goal)) and np.all(np.isfinite(env.vel_q))
        assert np.all((env.q[:, 0] >= -E.BOX) & (env.q[:, 0] <= S.FAR)) and np.all(np.abs(env.q[:, 1]) <= E.BOX) and np.all(env.q[:, 2] == 0)
        assert np.all(np.isfinite(pay[:, 1:3])) and np.all(np.isfinite(pay[:, 6:9]))
        assert set(np.unique(pay[:, 1])) <= {-1.0, 0.0}
    assert env.stats()["episodes"] == 2 * 16


def test_no_episode_of_192_starts_or_idles_within_the_threshold():
    env = S.RefGlideEnv(64, seed=3)
    thr = float(env.thr)
    for ep in range(3):
        s = env.state_dict()
        assert np.all(np.linalg.norm(s["desired_goal"] - s["achieved_goal"], axis=1) > thr)
        assert np.all(s["desired_goal"][:, 0] - s["achieved_goal"][:, 0] >= 0.3 - 1e-6)      # beyond the pusher's box by at least SPAWN
        assert np.all(np.linalg.norm(env.p - env.q, axis=1) > float(E.CONTACT))               # the pusher starts out of contact
        for _ in range(T):
            env.step(np.zeros((64, 3), f32))
            assert not env.contact.any()
    assert env.stats()["episodes"] == 192 and env.stats()["successes"] == 0
    assert env.stats()["reward_sum"] == -192.0 * T


def test_a_puck_in_contact_stays_short_of_every_goal():
    """random actions, half of the envs driven onto their pucks: after every contact step q.x < 0.39, so with goal.x >= 0.45 and the
    threshold 0.05 no episode can end solved while the pusher touches the puck"""
    env, gen = S.RefGlideEnv(32, seed=4, max_steps=T), np.random.default_rng(5)
    contacts = free = 0
    for _ in range(3 * T):
        a = gen.uniform(-1.5, 1.5, (32, 3)).astype(f32)
        to_puck = np.clip((env.q[:16] - env.p[:16]) / f32(0.04), -1, 1)
        a[:16] = np.where(gen.random((16, 1)) < 0.7, to_puck + gen.normal(0, 0.3, (16, 3)), a[:16]).astype(f32)
        env.step(a)
        hit = env.contact & ~env.reseeded
        contacts += int(hit.sum())
        free += int((~env.contact & ~env.reseeded & np.any(env.vel_q != 0, axis=1)).sum())
        assert np.all(env.q[hit, 0] < f32(0.39))
    assert contacts > 100 and free > 100, (contacts, free)


def test_a_free_puck_keeps_nine_tenths_of_its_displacement_and_a_wall_stops_it():
    env = S.RefGlideEnv(1, seed=2, max_steps=60)
    env.p[0] = [f32(0.0), f32(0.0), f32(0.0)]; env.q[0] = [f32(0.03), f32(0.0), f32(0.0)]
    env.step(np.array([[1, 0.5, 0]], f32))                       # a strike: the puck takes the pusher's displacement
    assert env.contact[0] and bits(env.vel_q[0, 0]) == bits(f32(0.04)) and bits(env.vel_q[0, 1]) == bits(f32(0.02))
    for _ in range(40):
        v0, q0 = env.vel_q[0].copy(), env.q[0].copy()
        env.step(np.array([[-1, 0, 0]], f32))                    # hands off
        assert not env.contact[0]
        want = np.array([min(f32(q0[0] + f32(S.FRICTION * v0[0])), S.FAR), min(f32(q0[1] + f32(S.FRICTION * v0[1])), E.BOX), 0], f32)
        assert np.array_equal(bits(env.q[0]), bits(want)) and np.array_equal(bits(env.vel_q[0]), bits((want - q0).astype(f32)))
    # struck to (0.07, 0.02), then 0.04 * 0.9 / (1 - 0.9) = 0.36 of glide in x and half of it in y, less the 0.9^40 still to come
    assert 0.42 < env.q[0, 0] < 0.43 and 0.19 < env.q[0, 1] < 0.20
    # a faster puck runs into the far wall: that component stops, the other glides on
    env.q[0] = [f32(0.85), f32(0.0), f32(0.0)]; env.vel_q[0] = [f32(0.1), f32(0.01), f32(0.0)]
    env.step(np.zeros((1, 3), f32))
    assert env.hit_far[0] and env.q[0, 0] == S.FAR and bits(env.vel_q[0, 0]) == bits(f32(S.FAR - f32(0.85)))
    env.step(np.zeros((1, 3), f32))
    assert env.hit_far[0] and env.q[0, 0] == S.FAR and env.vel_q[0, 0] == 0 and env.vel_q[0, 1] > 0
    env.step(np.zeros((1, 3), f32))
    assert not env.hit_far[0] and env.q[0, 0] == S.FAR and env.vel_q[0, 0] == 0


def _run_controller(seed, noise_std=0.0):
    env = S.RefGlideEnv(64, seed=seed)
    worst = 0.0
    for t in range(T):
        a = S.scripted_actions(env, noise_std=noise_std, seed=5, c=t)
        assert a.dtype == f32 and a.shape == (64, 3) and np.all(np.abs(a) <= 1)
        env.step(a)
        if t == T - 2:                                            # one step before the horizon (and the re-seed) the pucks are at rest or nearly
            worst = float(np.linalg.norm(env.q - env.goal, axis=1).max())
    return env.stats(), worst


def test_scripted_controller_in_float32_solves_at_least_60_of_64():
    st, worst = _run_controller(0)
    print("glide controller, seed 0:", st, "largest distance one step before the horizon %.4f" % worst)
    assert st["episodes"] == 64 and st["successes"] >= 60, st


def test_scripted_controller_with_noise_is_recorded_not_asserted():
    st, _ = _run_controller(0, noise_std=0.1)
    print("glide controller, seed 0, noise_std 0.1:", st)
    assert st["episodes"] == 64 and 0 <= st["successes"] <= 64


def test_noisy_scripted_actions():
    env = S.RefGlideEnv(5, seed=3)
    clean = S.scripted_actions(env)
    assert np.array_equal(bits(S.scripted_actions(env, noise_std=0.0, seed=9, c=4)), bits(clean))
    noisy = S.scripted_actions(env, noise_std=0.3, seed=9, c=4)
    ctr = (4 * 5 * 3 + np.arange(5 * 3, dtype=np.uint64)).reshape(5, 3)
    z = (hash_normal(9, ctr).astype(np.float64) * 0.3).astype(f32)
    assert np.array_equal(bits(noisy), bits(np.clip((clean + z).astype(f32), -1, 1)))
    assert not np.array_equal(noisy, clean) and np.all(np.abs(noisy) <= 1)
