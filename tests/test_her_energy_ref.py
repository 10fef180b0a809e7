"""Host tests (no GPU) of tests/her_energy_ref.py, the numpy definition of the energy-prioritised replay draw of a sample-mode HER
ring (HERBuffer(relabel="sample", prioritise="energy"); csrc/her_prio.hip): properties of the episode energy, the per-row draw
counter, the frequencies the descent gives on energy-like leaves — the condition the GPU draw inherits by being bitwise this code —
and the two new kernels use no scratch memory."""
import os
import re
import subprocess

import numpy as np
import pytest

import her_energy_ref as E
import per_tree_ref as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SEED = 20261019            # the seed of the frequency test, here and on the GPU
CAP3 = 4160                # three tree levels: 4160 -> 65 -> 2, the second level's last block mostly padding


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F32)).view(np.uint32)


def walk(gen, T, G=3, still=False, step=0.01):
    """achieved goals of one episode: a random walk, or an object nobody moved"""
    start = gen.uniform(0.4, 0.8, G).astype(F32)
    if still:
        return np.repeat(start[None], T, axis=0)
    return (start + np.cumsum(step * gen.standard_normal((T, G)), axis=0)).astype(F32)


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("T", [1, 2, 50])
def test_stationary_trajectory_has_the_floor_leaf(T):
    for alpha in (1.0, 0.6):
        cfg = E.config(3, alpha=alpha)
        ag = walk(np.random.default_rng(T), T, still=True)
        assert E.trajectory_energy(ag, cfg) == 0.0
        want = cfg["eps"] if alpha == 1.0 else F32(np.power(cfg["eps"], cfg["alpha"]))
        assert bits(E.leaf(ag, cfg)) == bits(F32(want / F32(T)))
        assert abs(E.leaf64(ag, cfg) - float(cfg["eps"]) ** float(cfg["alpha"]) / T) <= 1e-12


def test_a_falling_object_gains_nothing_from_the_potential():
    T = 50
    ag = np.zeros((T, 3), F32)
    ag[:, 0], ag[:, 1] = 0.5, 0.7
    ag[:, 2] = np.linspace(0.9, 0.4, T).astype(F32)                # height only decreases, at constant speed: kin constant from step 1 on
    cfg = E.config(3)
    e = E.gains(ag, cfg)
    kin1 = F32(cfg["kinetic"] * F32(F32(ag[1, 2] - ag[0, 2]) ** 2))
    pot = (cfg["potential"] * ag[:, 2]).astype(F32)
    assert e[0] == 0 and bits(e[1]) == bits(np.fmin(np.fmax(F32(F32(pot[1] + kin1) - pot[0]), F32(0)), cfg["clip"]))   # the kinetic onset only
    no_kin = E.gains(ag, E.config(3, kinetic=0.0))
    assert not no_kin.any(), "a falling height gained potential energy"
    up = E.gains(ag[::-1].copy(), E.config(3, kinetic=0.0))
    assert (up[1:] > 0).all()                                       # ... and the same path upwards does


def test_one_jump_larger_than_clip_contributes_exactly_clip():
    T = 7
    ag = walk(np.random.default_rng(1), T, still=True)
    ag[4:, 2] += F32(10.0)                                           # 98 J in one step
    cfg = E.config(3)
    e = E.gains(ag, cfg)
    assert bits(e[4]) == bits(cfg["clip"]) and not e[:4].any()
    assert e[5] == 0.0                                               # the kinetic term falls back to 0: a loss, not counted
    assert bits(E.trajectory_energy(ag, cfg)) == bits(cfg["clip"])
    assert bits(E.episode_priority(ag, cfg)) == bits(F32(cfg["clip"] + cfg["eps"]))     # alpha == 1: one fp32 add, no powf


def test_nan_and_inf_goals_give_a_finite_bounded_energy():
    gen = np.random.default_rng(2)
    cfg = E.config(3)
    for T in (1, 2, 50, 64):
        for bad in (np.nan, np.inf, -np.inf):
            ag = walk(gen, T)
            ag[gen.integers(0, T, 5), gen.integers(0, 3, 5)] = bad
            e = E.gains(ag, cfg)
            assert np.isfinite(e).all() and (e >= 0).all() and (e <= cfg["clip"]).all()
            x = E.trajectory_energy(ag, cfg)
            assert np.isfinite(x) and 0.0 <= x <= 63 * float(cfg["clip"])
            assert np.isfinite(E.leaf(ag, cfg)) and E.leaf(ag, cfg) > 0
    ag = np.full((64, 3), np.inf, F32)
    ag[::2] = -np.inf                                                # every difference inf or nan
    assert E.trajectory_energy(ag, cfg) <= 63 * float(cfg["clip"])


def test_axis_default_and_no_potential_term():
    assert E.config(3)["axis"] == 2 and E.config(2)["axis"] == -1 and E.config(8)["axis"] == 2
    ag = walk(np.random.default_rng(3), 20, G=2)
    kin_only = E.gains(ag, E.config(2))
    assert np.array_equal(bits(kin_only), bits(E.gains(ag, E.config(2, potential=1e6))))
    assert kin_only.any()


def test_powf_priority_is_the_fp64_evaluation_within_1e6():
    gen = np.random.default_rng(4)
    cfg = E.config(3, alpha=0.6)
    for T in (1, 2, 50):
        ag = walk(gen, T)
        assert abs(float(E.episode_priority(ag, cfg)) / E.episode_priority64(ag, cfg) - 1) <= 1e-6


# ---------------------------------------------------------------- counters
def _ring(cap, episodes, seed, still_share=0.3, **energy):
    gen = np.random.default_rng(seed)
    ring = E.RefEnergyRing(cap, 3, seed=SEED, **energy)
    for _ in range(episodes):
        ring.flush([walk(gen, 50, still=gen.random() < still_share)])
    return ring


def test_one_draw_of_nB_rows_equals_n_draws_of_B():
    ring = _ring(300, 7, 5)
    levels = ring.levels()
    for c0 in (0, 12345, (1 << 20) - 100, (3 << 20) - 7, (1 << 40) + 5):
        whole = E.draw(levels, SEED, c0, 4 * 67, ring.head, ring.cap)
        parts = np.concatenate([E.draw(levels, SEED, c0 + i * 67, 67, ring.head, ring.cap) for i in range(4)])
        assert np.array_equal(whole, parts), c0
    # across a multiple of 2^20 the per-level key is (c << 3) + level, continuous in c
    c = np.uint64((1 << 20) - 1)
    for k in range(3):
        a = PT.uniform24(SEED, (c + np.uint64(1)) >> np.uint64(20), (c + np.uint64(1)) & np.uint64(0xFFFFF), k)
        with np.errstate(over="ignore"):
            h = PT.mix64(PT.mix64(np.uint64(SEED) ^ PT.K) + (((c + np.uint64(1)) << np.uint64(3)) + np.uint64(k)))
        assert a == (h >> np.uint64(40)).astype(F32) * F32(2.0 ** -24)


# ---------------------------------------------------------------- frequencies
def _draw_many(ring, n):
    levels = ring.levels()
    return np.concatenate([E.draw_slots(levels, SEED, c0, 1 << 16) for c0 in range(0, n, 1 << 16)])


@pytest.mark.parametrize("episodes", [84, 60], ids=["full_wrapped", "filled_3000_of_4160"])
def test_draw_frequencies_follow_the_episode_energies(episodes):
    n = 1 << 18
    ring = _ring(CAP3, episodes, 6)
    assert len(ring.levels()) == 3
    assert (ring.len, ring.head) == ((CAP3, 40) if episodes == 84 else (3000, 0))
    slots = _draw_many(ring, n)
    logical = (slots - ring.head) % ring.cap
    assert (logical < ring.len).all(), "a never-filled slot was drawn"
    assert (ring.leaves[slots] > 0).all(), "a zero leaf was drawn"
    ep = ring.episode_of[slots]
    live = np.unique(ring.episode_of[ring.episode_of >= 0])
    mass = np.array([ring.leaves[ring.episode_of == e].astype(np.float64).sum() for e in live])       # (an evicted head keeps its live rows' share)
    q = mass / mass.sum()
    count = np.array([(ep == e).sum() for e in live])
    big = n * q >= 100
    z = (count[big] - n * q[big]) / np.sqrt(n * q[big] * (1 - q[big]))
    print(f"episodes {episodes}: worst |z| {np.abs(z).max():.2f} over {big.sum()} episodes")
    assert big.sum() >= 0.6 * live.size and np.abs(z).max() <= 5.0
    floor = float(ring.cfg["eps"])
    zero = np.array([abs(ring.p_ep[e] - floor) < 1e-9 for e in live])
    assert 0.15 * live.size <= zero.sum() <= 0.45 * live.size
    assert count[zero].sum() >= 1, "the zero-energy episodes were never drawn"


# ---------------------------------------------------------------- no scratch in the new kernels
def test_new_kernels_use_no_scratch(tmp_path):
    """her_prio.hip compiled to gfx950 assembly with the Makefile's flags: .private_segment_fixed_size is 0 for both kernels"""
    csrc = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)).split()
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1))
    assert "her_prio.hip" in re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    asm = tmp_path / "her_prio.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "her_prio.hip"), "-o", str(asm)], check=True, cwd=csrc)
    found = re.findall(r"\.name:\s+(\S*(?:her_energy_kernel|her_prio_draw_kernel)\S*)\n((?:(?!\.name:).)*?)\.private_segment_fixed_size:\s+(\d+)", asm.read_text(), re.S)
    sizes = {n: int(sz) for n, _, sz in found}
    assert len(sizes) == 2 and sum("her_energy_kernel" in n for n in sizes) == 1, sizes
    assert all(v == 0 for v in sizes.values()), sizes
    vgprs = dict(re.findall(r"\.amdhsa_kernel\s+(\S+)\n(?:(?!\.end_amdhsa_kernel).)*?\.amdhsa_next_free_vgpr\s+(\d+)", asm.read_text(), re.S))
    print({k: int(v) for k, v in vgprs.items()})                    # the figures DESIGN 4k quotes
