"""CPU (-m "not gpu"): the definition of the device-resident prioritised draw (tests/per_tree_ref.py) is a proportional draw
that never yields a zero slot; the tree stays the reduction of its leaves under pushes, wraps and updates; the host-only C code
of the new entries is clean under the sanitizers (stand-alone program); per_draw's refusals come before any device work."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import per_tree_ref as R
from oracle.agent_oracle import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the three trees of the draw-frequency test: (capacity, filled rows); priorities span 1e-3 .. 11
FREQ_CASES = {"cap96": (96, 70), "cap4160": (4160, 4130), "cap12288": (12288, 12288)}
FREQ_SEEDS = (11, 23, 37, 41, 59, 73)     # fixed
FREQ_DRAWS, FREQ_B = 1 << 18, 256


def fixed_tree(cap: int, filled: int, head: int = 0):
    """Leaves with log-uniform priorities in [1e-3, 11] on the filled rows, a handful of exact zeros among them, 0 elsewhere."""
    gen = np.random.default_rng(cap * 7919 + filled)
    p = np.exp(gen.uniform(np.log(1e-3), np.log(11.0), filled)).astype(np.float32)
    if filled > 100:
        p[gen.choice(filled, 9, replace=False)] = 0.0   # set_priorities may store zeros: never drawn either
    padded = R.level_sizes(cap)[0][1]
    leaves = np.zeros(padded, np.float32)
    leaves[(head + np.arange(filled)) % cap] = p
    return R.build(leaves)


def frequency_check(levels, slots, n_draws: int, top: int):
    """Relative frequency of the `top` heaviest slots against p_i / total within 5 binomial standard errors."""
    leaves = levels[0].astype(np.float64)
    prob = leaves / leaves.sum()
    counts = np.bincount(slots, minlength=leaves.size)
    heavy = np.argsort(-prob)[:top]
    se = np.sqrt(n_draws * prob[heavy] * (1.0 - prob[heavy]))
    z = (counts[heavy] - n_draws * prob[heavy]) / se
    return float(np.max(np.abs(z)))


@pytest.mark.parametrize("seed", FREQ_SEEDS)
@pytest.mark.parametrize("case", sorted(FREQ_CASES))
def test_draw_frequency_is_proportional_and_skips_zero_slots(case, seed):
    cap, filled = FREQ_CASES[case]
    levels = fixed_tree(cap, filled)
    R.check_invariant(levels)
    n_batches = FREQ_DRAWS // FREQ_B
    slots = []
    for c0 in range(0, n_batches, 256):      # 2^16 descents at a time
        d = np.repeat(np.arange(c0, min(c0 + 256, n_batches), dtype=np.uint64), FREQ_B)
        b = np.tile(np.arange(FREQ_B, dtype=np.uint64), d.size // FREQ_B)
        s, p = R.descend(levels, seed, d, b)
        assert np.all(p > 0), "a zero slot was drawn"
        assert np.array_equal(p.view(np.uint32), levels[0][s].view(np.uint32))
        slots.append(s)
    slots = np.concatenate(slots)
    assert slots.size == FREQ_DRAWS and np.all(slots < cap) and np.all(levels[0][slots] > 0)
    worst = frequency_check(levels, slots, FREQ_DRAWS, 70 if cap == 96 else 64)
    print(f"{case} seed {seed}: worst |z| = {worst:.2f}")
    assert worst <= 5.0


def test_child_rule_guards():
    """The two guards of the child rule on hand-made blocks: x == P[63] (u * P[63] rounded up) takes the LAST positive child, and a
    zero child is skipped even where the scan says P > x."""
    v = np.zeros(64, np.float32)
    v[3], v[10], v[40] = 1.0, 2.0, 0.5
    P = R.scan64(v)[0]
    assert P[63] == np.float32(3.5)
    pos = v > 0
    for x, want in ((np.float32(0.0), 3), (np.float32(0.999), 3), (np.float32(1.0), 10), (np.float32(2.9999), 10), (np.float32(3.0), 40),
                    (np.float32(3.5), 40)):
        hit = pos & (P > x)
        child = int(np.argmax(hit)) if hit.any() else 63 - int(np.argmax(pos[::-1]))
        assert child == want, (x, child, want)
    # all descents of a tree whose only positive leaf is one slot end there
    leaves = np.zeros(4160, np.float32)
    leaves[4100] = 1e-3
    s, p = R.descend(R.build(leaves), 5, np.zeros(64, np.uint64), np.arange(64, dtype=np.uint64))
    assert np.all(s == 4100) and np.all(p == np.float32(1e-3))


def test_uniform_is_a_24_bit_fraction_and_keyed():
    u = R.uniform24(7, np.arange(4096, dtype=np.uint64) // 64, np.arange(4096, dtype=np.uint64) % 64, 1)
    assert u.dtype == np.float32 and np.all(u >= 0) and np.all(u < 1) and np.all((u * np.float32(2 ** 24)) % 1 == 0)
    assert 0.45 < float(u.mean()) < 0.55
    assert not np.array_equal(u, R.uniform24(8, np.arange(4096, dtype=np.uint64) // 64, np.arange(4096, dtype=np.uint64) % 64, 1))
    assert not np.array_equal(u, R.uniform24(7, np.arange(4096, dtype=np.uint64) // 64, np.arange(4096, dtype=np.uint64) % 64, 0))
    # scalar restatement of the counter formula with Python integers
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    for draw, b, lvl in ((0, 0, 0), (3, 17, 2), (123456789, 255, 1)):
        h = mix((mix(7 ^ 0x5045525F54524545) + ((((draw << 20) + b) << 3) + lvl)) & M)
        assert float(R.uniform24(7, draw, b, lvl)) == (h >> 40) / float(1 << 24)


@pytest.mark.parametrize("cap", [96, 4160])
def test_tree_invariant_under_pushes_wraps_and_updates(cap):
    """Incremental maintenance (pending-push segments, touched ancestors) == a full rebuild from the leaves, bitwise, whatever the order."""
    gen = np.random.default_rng(cap)
    t = R.RefPER(cap, alpha=0.6, seed=3)
    for it in range(60):
        op = it % 3
        if op == 0:
            t.push(int(gen.integers(1, cap // 2 + 40)))       # wraps within a few rounds; sometimes more than the rest of the ring
        elif op == 1 and t.len >= 8:
            B = int(gen.integers(1, min(t.len, 300) + 1))
            idx, p = t.draw(B)
            assert np.all(idx < t.len) and np.all(p > 0)
        elif t.len >= 8:
            B = int(gen.integers(2, 200))
            idx = gen.integers(0, t.len, B)
            idx[B // 2:] = idx[:B - B // 2]                    # duplicates with different td values
            td = gen.standard_normal(B).astype(np.float32)
            t.update(idx, td)
            keep = R.last_occurrence(idx)
            want = ((np.abs(td[keep]) + t.eps) ** t.alpha).astype(np.float32)
            assert np.array_equal(t.levels[0][(t.head + idx[keep]) % cap], want)     # the last occurrence won
        t.refresh()
        R.check_invariant(t.levels)
        full = R.build(t.levels[0])
        for a, b in zip(t.levels, full):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        filled = np.zeros(t.levels[0].size, bool)
        filled[(t.head + np.arange(t.len)) % cap] = True
        assert not t.levels[0][~filled].any() and np.all(t.levels[0][filled] > 0)
    assert t.len == cap and t.head != 0


def test_level_sizes():
    assert R.level_sizes(1_000_000) == [(1_000_000, 1_000_000), (15625, 15680), (245, 256), (4, 64)]
    assert R.level_sizes(96) == [(96, 128), (2, 64)]
    assert R.level_sizes(4160) == [(4160, 4160), (65, 128), (2, 64)]
    assert R.level_sizes(64) == [(64, 64)]


def test_host_code_is_clean_under_sanitizers(tmp_path):
    """csrc/per_host.h — level sizes, slot arithmetic, pending-push segments — as a stand-alone program (tools/per_host_check.cc, its own
    main) built with -fsanitize=address,undefined and run on the CPU; the sanitizer runtimes are linked statically."""
    exe = str(tmp_path / "per_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "per_host_check.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "per host check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_entries_are_declared_and_bound(gcrl):
    header = open(os.path.join(ROOT, "include", "gcrl.h")).read()
    for e in ("gcrl_per_attach", "gcrl_per_draw", "gcrl_per_update", "gcrl_per_get_priorities", "gcrl_per_set_priorities", "gcrl_per_read_level",
              "gcrl_per_get_draw_counter", "gcrl_per_set_draw_counter", "gcrl_per_set_betas", "gcrl_her_sample_dev"):
        assert e + "(" in header and e in gcrl._ffi.PROTOTYPES and callable(getattr(gcrl._ffi.lib, e))
    # entries on a null ring answer without touching a device
    lib = gcrl._ffi.lib
    assert lib.gcrl_per_attached(None) == 0 and lib.gcrl_per_levels(None) == 0 and lib.gcrl_per_get_draw_counter(None) == -1
    assert lib.gcrl_per_attach(None, 0.6, 1e-6) < 0 and "null ring" in gcrl._ffi.last_error()


def test_refusals_name_per_draw_before_any_device_work(gcrl):
    cfg_per = make_config("TD3", buffer_type="PER", max_len=4160, batch_size=64)
    cfg_her = make_config("TD3", buffer_type="HER", max_len=4160, batch_size=64)
    with pytest.raises(ValueError, match="per_draw"):
        gcrl.TD3Agent(10, 3, cfg_per, None, nenvs=1, gradient_step=4, per_draw="gpu")
    with pytest.raises(gcrl._ffi.GcrlError, match="per_draw.*buffer_type 'PER'"):
        gcrl.TD3Agent(10, 3, cfg_her, None, nenvs=1, gradient_step=4, per_draw="device")
    # the distributional TQC variant
    with pytest.raises(gcrl._ffi.GcrlError, match="per_draw.*distributional"):
        gcrl.TQCAgent(10, 3, make_config("TQC", buffer_type="PER", max_len=4160, batch_size=64), None, nenvs=1, gradient_step=4,
                      n_quantiles=25, per_draw="device")
    # populations
    for name in ("DDPGPopulation", "TD3Population", "SACPopulation", "TQCPopulation"):
        kind = {"DDPGPopulation": "DDPG", "TD3Population": "TD3", "SACPopulation": "SAC", "TQCPopulation": "TQC"}[name]
        with pytest.raises(gcrl._ffi.GcrlError, match=f"{name}: per_draw:"):
            getattr(gcrl, name)(10, 3, [make_config(kind, batch_size=64)] * 2, nenvs=1, gradient_step=4, per_draw="device")
    with pytest.raises(gcrl._ffi.GcrlError, match="per_draw"):
        gcrl.TD3Agent(10, 3, cfg_per, None, nenvs=1, gradient_step=4, per_draw="device", _member=lambda cfg: (None, None))
    # DataParallelUpdater: refused before any collective (no process group exists here)
    from gcrl_amd.src.dp import DataParallelUpdater
    with pytest.raises(gcrl._ffi.GcrlError, match="per_draw"):
        DataParallelUpdater(SimpleNamespace(per_draw="device"))
    with pytest.raises(ValueError, match="draw must be"):
        gcrl.PERBuffer(100, 0.6, draw="gpu")
