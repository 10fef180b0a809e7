"""Fixtures shared by tests/test_goal_propose_ref.py (CPU: the definition itself, and that these fixtures reach their branches) and
tests/test_gpu_goal_propose.py (the kernels against the definition).  Everything is generated from seeds."""
import numpy as np

import dev_env_glide_ref as SG
import dev_env_pick_ref as SP
import dev_env_ref as E
import goal_propose_ref as R

f32 = np.float32
THR = 0.05

# kind -> env shape and proposer settings; every case runs 3 T + 2 vector steps
CASES = {
    "reach": dict(N=5, T=4, capacity=37, candidates=3, radius=0.05, share=0.5, min_fill=6),     # wrap, partial wave, declining envs
    "push": dict(N=70, T=3, capacity=256, candidates=16, radius=1e-6, share=1.0, min_fill=1),   # pucks that never moved: duplicates, ties
    "glide": dict(N=3, T=2, capacity=4096, candidates=64, radius=10.0, share=1.0, min_fill=1),  # every count equals L: k = 0 wins
    "pick": dict(N=2, T=5, capacity=2, candidates=1, radius=0.05, share=1.0, min_fill=2),       # capacity = N, C = 1
}
ENV_SEED, PROP_SEED = 11, 7


def ref_env(kind, n, seed, max_steps, threshold=THR):
    if kind == "pick":
        return SP.RefPickEnv(n, seed=seed, max_steps=max_steps, threshold=threshold)
    if kind == "glide":
        return SG.RefGlideEnv(n, seed=seed, max_steps=max_steps, threshold=threshold)
    return E.RefEnv(kind, n, seed=seed, max_steps=max_steps, threshold=threshold)


def settings(case):
    return {k: case[k] for k in ("capacity", "candidates", "radius", "share", "min_fill")}


def actions(kind, case, steps=None):
    """[steps][N][A] float32: random clipped actions"""
    steps = 3 * case["T"] + 2 if steps is None else steps
    gen = np.random.default_rng(sorted(CASES).index(kind) + 100)
    A = 4 if kind == "pick" else 3
    return np.clip(gen.normal(0.0, 1.0, (steps, case["N"], A)), -1.0, 1.0).astype(f32)


def run_ref(kind, each=None):
    """The case on the numpy definition; each(step, env, prop) after every step.  Returns (env, prop, decisions): the `last` records of
    every propose, in order."""
    case = CASES[kind]
    env = ref_env(kind, case["N"], ENV_SEED, case["T"])
    prop = R.RefProposer(seed=PROP_SEED, **settings(case))
    decisions = []
    for s, act in enumerate(actions(kind, case)):
        prop.step_env(env, act)
        decisions += prop.last
        if each:
            each(s, env, prop)
    return env, prop, decisions


# ---- archive lengths around the kernel's tile: one env, entries on a grid of 1/8, radius 1/4 — squared distances are exact in float32
# and many equal rho2 = 1/16 exactly, which the strict comparison must leave out
GRID_RADIUS, GRID_C = 0.25, 16


def grid_lengths(tile):
    return [1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3]


def grid_capacity(tile):
    return 2 * tile + 16


def grid_archive(L, tile):
    """(physical archive [cap][3], head, len): len = L - 1 entries, so that the append of a one-env step makes L; from L = 63 on the
    live range wraps around the end of the allocation"""
    cap = grid_capacity(tile)
    gen = np.random.default_rng(L)
    n = L - 1
    ent = np.stack([gen.integers(0, 12, n), gen.integers(0, 3, n), np.zeros(n, np.int64)], axis=1).astype(f32) * f32(0.125)
    head = cap - 7 if L >= 63 else 0
    arch = np.zeros((cap, 3), f32)
    arch[(head + np.arange(n)) % cap] = ent
    return arch, head, n
