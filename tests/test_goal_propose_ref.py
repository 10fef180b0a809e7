"""CPU: tests/goal_propose_ref.py, the definition of practice goals, against an independent restatement and its own stated
properties — and that the fixtures the GPU tests run (tests/goal_propose_cases.py) reach the branches they are there for, so that
no GPU comparison passes vacuously."""
import numpy as np
import pytest

from oracle.her_oracle import hash_below

import dev_env_ref as E
import goal_propose_cases as K
import goal_propose_ref as R

f32 = np.float32
bits = lambda x: np.ascontiguousarray(x, f32).view(np.uint32)


def _brute_choice(entries, js, radius):
    """min-density choice by loops over entries and scalar float32 arithmetic (no broadcasting)"""
    rho2 = f32(radius) * f32(radius)
    best, best_cnt, counts = -1, None, []
    for k, j in enumerate(js):
        c = entries[j]
        cnt = 0
        for m in range(len(entries)):
            e = entries[m]
            dx, dy, dz = f32(e[0] - c[0]), f32(e[1] - c[1]), f32(e[2] - c[2])
            d2 = f32(f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz))
            if d2 < rho2:
                cnt += 1
        counts.append(cnt)
        if best_cnt is None or cnt < best_cnt:
            best, best_cnt = k, cnt
    return best, counts


@pytest.mark.parametrize("kind", ["reach", "push", "glide", "pick"])
def test_choice_is_the_brute_force_recomputation(kind):
    case = K.CASES[kind]
    seen = [0]

    def each(step, env, prop):
        entries = prop.logical()
        for rec in prop.last:
            if not rec["took"]:
                continue
            assert rec["js"] == [hash_below(K.PROP_SEED, R.CAND_STREAM, ((prop.q - 1) * case["N"] + rec["env"]) * case["candidates"] + k, prop.len)
                                 for k in range(case["candidates"])]
            if kind != "push" or rec["env"] % 9 == 0:            # (the 70-env case: every ninth env keeps the loop short)
                best, counts = _brute_choice(entries, rec["js"], case["radius"])
                assert best == rec["best"] and counts == list(rec["counts"]) and min(counts) >= 1
            assert np.array_equal(bits(env.goal[rec["env"]]), bits(entries[rec["js"][rec["best"]]]))
            assert np.array_equal(bits(env.rows[rec["env"], env.D:]), bits(env.goal[rec["env"]]))
            seen[0] += 1

    env, prop, _ = K.run_ref(kind, each)
    rolls = (3 * case["T"] + 2) // case["T"]
    assert seen[0] > 0 and prop.q == rolls and prop.roll_steps == rolls
    assert prop.appended == (3 * case["T"] + 2) * case["N"] and prop.patched == seen[0]


def test_archive_wraps_as_a_deque():
    import collections
    prop = R.RefProposer(capacity=37, candidates=3, radius=0.05, share=0.5, min_fill=6, seed=1)
    env = E.RefEnv("reach", 5, seed=2, max_steps=50, threshold=0.05)
    dq = collections.deque(maxlen=37)
    gen = np.random.default_rng(0)
    for s in range(20):
        raw, _ = prop.step_env(env, gen.uniform(-1, 1, (5, 3)).astype(f32))
        for row in env.split(raw)[5]:
            dq.append(row.copy())
        assert prop.len == len(dq) == min(37, 5 * (s + 1))
        assert np.array_equal(bits(prop.logical()), bits(np.array(dq)))
    assert prop.head == (20 * 5 - 37) % 37 and prop.q == 0 and prop.patched == 0


def test_below_min_fill_nothing_is_patched_but_q_advances():
    prop = R.RefProposer(capacity=64, candidates=4, radius=0.05, share=1.0, min_fill=13, seed=3)
    env, twin = (E.RefEnv("reach", 3, seed=4, max_steps=2, threshold=0.05) for _ in range(2))
    act = np.zeros((3, 3), f32)
    for s in range(4):                                      # L = 3, 6, 9, 12 < 13: roll-overs at s = 1 and 3
        prop.step_env(env, act); twin.step(act)
        assert np.array_equal(bits(env.goal), bits(twin.goal))
    assert prop.q == 2 and prop.roll_steps == 2 and prop.patched == 0 and prop.last == []
    prop.step_env(env, act); prop.step_env(env, act)        # L = 18 at the third roll-over
    assert prop.q == 3 and prop.patched == 3 and all(r["took"] for r in prop.last)


def test_share_one_always_takes_and_share_is_a_threshold_on_the_hash():
    for q in range(5):
        for i in range(40):
            assert R.takes(9, q, 40, i, 1.0)
            u = f32(hash_below(9, R.TAKE_STREAM, q * 40 + i, 1 << 24)) * f32(2.0 ** -24)
            assert R.takes(9, q, 40, i, 0.3) == bool(u < f32(0.3))
    frac = np.mean([R.takes(9, q, 40, i, 0.3) for q in range(50) for i in range(40)])
    assert 0.25 < frac < 0.35


def test_a_masked_reset_is_not_a_roll_over():
    prop = R.RefProposer(capacity=64, candidates=4, radius=0.05, share=1.0, min_fill=1, seed=5)
    env, twin = (E.RefEnv("reach", 5, seed=6, max_steps=4, threshold=0.05) for _ in range(2))
    gen = np.random.default_rng(1)
    mask = np.array([0, 1, 0, 1, 0], bool)
    for s in range(7):
        if s == 2:
            env.reset(mask); twin.reset(mask)
            assert np.array_equal(bits(env.goal), bits(twin.goal))       # the reset envs carry their task goals
        act = gen.uniform(-1, 1, (5, 3)).astype(f32)
        prop.step_env(env, act); twin.step(act)
        rolled = [r["env"] for r in prop.last]
        if s == 3:
            assert rolled == [0, 2, 4] and np.array_equal(bits(env.goal[mask]), bits(twin.goal[mask]))
            assert not np.array_equal(bits(env.goal[~mask]), bits(twin.goal[~mask]))
        elif s == 5:
            assert rolled == [1, 3]
        else:
            assert rolled == []
    assert prop.q == 2


def test_same_seed_same_run_other_seed_other_goals():
    a, b = K.run_ref("reach"), K.run_ref("reach")
    assert np.array_equal(bits(a[0].goal), bits(b[0].goal)) and np.array_equal(bits(a[1].arch), bits(b[1].arch))
    assert [(r["env"], r["took"], r["best"]) for r in a[2]] == [(r["env"], r["took"], r["best"]) for r in b[2]]
    case = K.CASES["reach"]
    env = K.ref_env("reach", case["N"], K.ENV_SEED, case["T"])
    prop = R.RefProposer(seed=K.PROP_SEED + 1, **K.settings(case))
    other = []
    for act in K.actions("reach", case):
        prop.step_env(env, act)
        other += prop.last
    assert [(r["took"], r["js"]) for r in other] != [(r["took"], r["js"]) for r in a[2]]


# ---------------------------------------------------------------- the GPU fixtures reach their branches
def test_gpu_fixtures_reach_their_branches():
    _, prop, dec = K.run_ref("push")
    took = [r for r in dec if r["took"]]
    assert len(took) == 3 * 70 and prop.head != 0                                      # share = 1; the archive wrapped
    tie = [r for r in took if (r["counts"] == r["counts"].min()).sum() > 1]
    assert tie, "no winner decided by the tie rule"
    assert any(r["best"] > 0 for r in took), "no winner with k > 0"
    assert max(int(r["counts"].max()) for r in took) >= 3                              # exact duplicates: pucks that never moved
    _, prop, dec = K.run_ref("reach")
    assert any(not r["took"] for r in dec) and any(r["took"] for r in dec), "share = 0.5 neither declined nor took"
    assert prop.head != 0 and prop.len == 37
    _, prop, dec = K.run_ref("glide")
    assert dec and all(r["best"] == 0 and (r["counts"] == r["counts"][0]).all() for r in dec)
    assert all(int(r["counts"][0]) == 3 * (2 * (n // 3 + 1)) for n, r in enumerate(dec))   # every count equals L
    _, prop, dec = K.run_ref("pick")
    assert prop.cap == 2 and len(dec) == 6 and all(r["took"] and r["best"] == 0 for r in dec)


def test_grid_fixture_has_distances_exactly_at_the_radius():
    tile = 1024
    rho2 = f32(K.GRID_RADIUS) * f32(K.GRID_RADIUS)
    for L in K.grid_lengths(tile):
        arch, head, n = K.grid_archive(L, tile)
        assert n == L - 1 and (head + n > K.grid_capacity(tile)) == (L >= 63)
        if n < 2:
            continue
        ent = arch[(head + np.arange(n)) % K.grid_capacity(tile)]
        d = ent[:, None, :] - ent[None, :16, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert (d2 == rho2).any() and (d2 < rho2).any() and (d2 > rho2).any()
