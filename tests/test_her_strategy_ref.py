"""Host tests (no GPU) of tests/her_strategy_ref.py, the numpy definition of the goal-selection strategies of a sample-mode HER
ring (HERBuffer(relabel="sample", goal_strategy="future" | "final" | "episode"); csrc/her_relabel.hip): `future` is the rule of
before bit for bit, `episode` is uniform over the other live rows of the episode and never leaves it, `final` picks the last row,
no tail — however dishonest — takes a slot out of the ring, the keyword's refusals come before any device work, and the
unit's kernels use no scratch memory."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import her_nstep_ref as NS
import her_relabel_ref as R
import her_strategy_ref as GS
from oracle.agent_oracle import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
OUT = ("s", "a", "r", "ns", "d")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F32)).view(np.uint32)


def make_ring(cap, episodes, dims=(6, 2, 2), seed=0, dense=False):
    """A ring of `cap` slots after flushing episodes of the given lengths, by physical slot, FIFO-evicted as the device ring is:
    global row g lies at slot g mod cap.  -> dict(s, a, ns, r, d, ag, rem, el: by slot; ep: the episode number of each slot's row;
    head, cap, len)"""
    S, A, G = dims
    gen = np.random.default_rng(seed)
    total = sum(episodes)
    q = dict(s=np.zeros((cap, S), F32), a=np.zeros((cap, A), F32), ns=np.zeros((cap, S), F32), r=np.zeros(cap, F32), d=np.zeros(cap, F32),
             ag=np.zeros((cap, G), F32), rem=np.zeros(cap, F32), el=np.zeros(cap, F32), ep=np.full(cap, -1, np.int64))
    g = 0
    for e, T in enumerate(episodes):
        goal = gen.standard_normal(G).astype(F32)
        pos = gen.standard_normal(G).astype(F32)
        for i in range(T):
            p = g % cap
            pos = (pos + 0.03 * gen.standard_normal(G)).astype(F32)
            q["s"][p] = np.concatenate([gen.standard_normal(S - G).astype(F32), goal])
            q["ns"][p] = np.concatenate([gen.standard_normal(S - G).astype(F32), goal])
            q["a"][p] = gen.standard_normal(A).astype(F32)
            q["r"][p] = -F32(gen.random()) if dense else (F32(-1.0) if gen.random() < 0.7 else F32(-0.0))
            q["d"][p] = 1.0 if i == T - 1 else 0.0
            q["ag"][p], q["rem"][p], q["el"][p], q["ep"][p] = pos, T - 1 - i, i, e
            g += 1
    q.update(head=total % cap if total > cap else 0, cap=cap, len=min(cap, total))
    return q


def ring_args(q):
    return [q[k] for k in ("s", "a", "ns", "r", "d", "ag", "rem")]


# ---------------------------------------------------------------- 1. future is the rule of before
@pytest.mark.parametrize("N", [1, 3, 8])
def test_future_equals_the_old_refs(N):
    for cap, eps, seed, dense in ((60, [50, 50], 3, True), (130, [50, 13, 50, 50], 4, False)):
        q = make_ring(cap, eps, seed=seed, dense=dense)
        assert q["head"] != 0 and q["len"] == cap                       # wrapped
        idx = np.random.default_rng(5).integers(0, q["len"], 700)
        kind = R.DENSE if dense else R.SPARSE
        for k in (0, 4):
            got = GS.gather(*ring_args(q), q["el"], q["head"], cap, idx, 11, 21, k, kind, 0.05, GS.FUTURE, N, 0.98)
            want = NS.gather(*ring_args(q), q["head"], cap, idx, 11, 21, k, kind, 0.05, N, 0.98)
            for key in OUT:
                assert np.array_equal(bits(got[key]), bits(want[key])), (N, k, key)
            assert np.array_equal(got["o"], want["f"]) and np.array_equal(got["g"], want["fut"])
            if N == 1:
                one = R.gather(*ring_args(q), q["head"], cap, idx, 11, 21, k, kind, 0.05)
                for key in OUT:
                    assert np.array_equal(bits(got[key]), bits(one[key])), (k, key)


# ---------------------------------------------------------------- 2. the distribution of `episode`
@pytest.mark.parametrize("back,rem", [(0, 49), (49, 0), (20, 29), (3, 1), (1, 1), (12, 37)])
def test_episode_offsets_are_uniform(back, rem):
    """seed 7, k = 4, counters 0 .. 2^16 - 1: every offset of [-back, rem] \\ {0} occurs, 0 only as "not relabelled"; each count
    against its binomial expectation M p, p = (k / (k + 1)) / (back + rem), and the relabelled share against k / (k + 1): |z| <= 4"""
    seed, k, M = 7, 4, 1 << 16
    o = np.array([GS.decide(seed, k, c, rem, back, GS.EPISODE) for c in range(M)])
    share = k / (k + 1)
    kept = np.array([R.hash_below(seed, R.K, 2 * c, k + 1) == 0 for c in range(M)])
    assert np.array_equal(o == 0, kept)                                  # 0 is "not relabelled" and nothing else
    vals, counts = np.unique(o[o != 0], return_counts=True)
    assert vals.tolist() == [v for v in range(-back, rem + 1) if v != 0]
    p = share / (back + rem)
    z_off = float(np.max(np.abs(counts - M * p)) / math.sqrt(M * p * (1 - p)))
    z_share = abs(int((o != 0).sum()) - M * share) / math.sqrt(M * share * (1 - share))
    print(f"(back, rem) = ({back}, {rem}): worst |z| of an offset {z_off:.2f}, of the relabelled share {z_share:.2f}")
    assert z_off <= 4.0 and z_share <= 4.0


# ---------------------------------------------------------------- 3. final
def test_final_picks_the_last_row():
    seed, k = 7, 4
    for rem in range(0, 50):
        o = np.array([GS.decide(seed, k, c, rem, 0, GS.FINAL) for c in range(256)])
        if rem == 0:
            assert (o == 0).all()                                        # an episode's last row is never relabelled
        else:
            assert set(o.tolist()) == {0, rem}
            assert np.array_equal(o != 0, [R.hash_below(seed, R.K, 2 * c, k + 1) != 0 for c in range(256)])
    q = make_ring(130, [50, 13, 50, 50], seed=8)
    idx = np.random.default_rng(9).integers(0, q["len"], 600)
    got = GS.gather(*ring_args(q), None, q["head"], 130, idx, 3, seed, k, R.SPARSE, 0.05, GS.FINAL, 3, 0.98)
    hit = np.flatnonzero(got["o"])
    assert hit.size > 300
    assert (q["rem"][got["g"][hit]] == 0).all()                          # the goal row is an episode's last one ..
    p = (q["head"] + idx[hit]) % 130
    assert np.array_equal(q["ep"][got["g"][hit]], q["ep"][p])            # .. of the row's own episode


# ---------------------------------------------------------------- 4. episode on a ring whose oldest episode is cut
def test_episode_stays_inside_the_live_part_of_its_episode():
    cap = 120
    q = make_ring(cap, [50, 50, 50], seed=10)                            # 150 rows: the first 30 of episode 0 are evicted
    assert q["head"] == 30 and q["len"] == cap
    live = {(q["head"] + j) % cap for j in range(q["len"])}
    idx = np.tile(np.arange(cap), 8)
    for N in (1, 3):
        got = GS.gather(*ring_args(q), q["el"], q["head"], cap, idx, 0, 7, 4, R.SPARSE, 0.05, GS.EPISODE, N, 0.98)
        p = (q["head"] + idx) % cap
        cut = idx < q["el"][p]                                           # rows whose episode lost older rows: j < elapsed
        assert cut.any() and (got["back"][cut] == idx[cut]).all()
        hit = np.flatnonzero(got["o"])
        assert (got["o"][hit] < 0).any() and (got["o"][hit] > 0).any()
        assert all(int(g) in live for g in got["g"][hit])
        assert np.array_equal(q["ep"][got["g"][hit]], q["ep"][p[hit]])   # never a row of another episode ..
        # .. and never an evicted one: on this full ring the slot of an evicted row holds a row of ANOTHER episode, and going back
        # past logical index 0 would land on the newest rows
        assert (got["g"][hit] != p[hit]).all()                           # never the row itself
        j_goal = (got["g"][hit] - q["head"]) % cap
        assert np.array_equal(j_goal - idx[hit], got["o"][hit])          # the offset holds in LOGICAL order: no wrap past index 0


# ---------------------------------------------------------------- 5. dishonest tails
@pytest.mark.parametrize("strategy", [GS.FINAL, GS.EPISODE])
@pytest.mark.parametrize("cap", [120, 20])
def test_dishonest_tails_stay_inside_the_ring(strategy, cap):
    q = make_ring(cap, [50, 50, 50], seed=12)
    bad = [float("nan"), -5.0, 1e9, float("inf")]
    gen = np.random.default_rng(13)
    idx = np.tile(np.arange(q["len"]), 6)
    for trial in range(4):
        rem = q["rem"].copy(); el = q["el"].copy()
        for arr in (rem, el):
            where = gen.random(cap) < 0.6
            arr[where] = gen.choice(bad, int(where.sum()))
        if trial == 3:
            rem[:] = bad[trial]; el[:] = bad[(trial + 1) % 4]
        a = ring_args(q); a[6] = rem
        for N in (1, 8):
            got = GS.gather(*a, el, q["head"], cap, idx, 5, 7, 4, R.SPARSE, 0.05, strategy, N, 0.98)
            hit = got["o"] != 0
            assert hit.any()
            assert ((got["g"][hit] >= 0) & (got["g"][hit] < cap)).all() and ((got["last"] >= 0) & (got["last"] < cap)).all()
            rem_max = min(R.FLUSH_LEN, cap) - 1
            assert (np.abs(got["o"]) <= rem_max).all() and (got["back"] <= idx).all() and (-got["o"] <= idx).all()


# ---------------------------------------------------------------- 6. refusals before any device work, and the unit's metadata
def test_python_refusals_name_goal_strategy(gcrl):
    err = gcrl._ffi.GcrlError
    from gcrl_amd.src.buffer import HERBuffer
    for bad in ("random", None, 2):
        with pytest.raises(err, match="goal_strategy"):
            HERBuffer(1000, 50, 2, relabel="sample", goal_strategy=bad)
    for strategy in ("final", "episode"):
        with pytest.raises(err, match="goal_strategy"):
            HERBuffer(1000, 50, 2, relabel="push", goal_strategy=strategy)
        with pytest.raises(err, match="goal_strategy"):
            HERBuffer(1000, 50, 2, goal_strategy=strategy)
    kw = dict(hidden_dim=64, layer_count=3, batch_size=64)
    for name, cls, pop in (("DDPG", gcrl.DDPG, gcrl.DDPGPopulation), ("TD3", gcrl.TD3Agent, gcrl.TD3Population),
                           ("SAC", gcrl.SACAgent, gcrl.SACPopulation), ("TQC", gcrl.TQCAgent, gcrl.TQCPopulation)):
        cfg = make_config(name, **kw)
        with pytest.raises(err, match=f"{cls.__name__}: goal_strategy"):
            cls(10, 3, cfg, None, 2, 4, relabel="sample", goal_strategy="nearest")
        with pytest.raises(err, match=f"{cls.__name__}: goal_strategy"):
            cls(10, 3, cfg, None, 2, 4, relabel="push", goal_strategy="final")
        for bt in ("PER", "REPLAY"):
            c2 = make_config(name, **kw)
            c2.buffer_type = bt
            with pytest.raises(err, match=f"{cls.__name__}: goal_strategy"):
                cls(10, 3, c2, None, 2, 4, goal_strategy="episode")
        for shared in (False, True):
            cfgs = [make_config(name, **kw) for _ in range(2)]
            with pytest.raises(err, match=f"{pop.__name__}: goal_strategy"):
                pop(10, 3, cfgs, 2, 4, relabel="sample", goal_strategy="nearest", shared_ring=shared)
            with pytest.raises(err, match=f"{pop.__name__}: goal_strategy"):
                pop(10, 3, cfgs, 2, 4, relabel="push", goal_strategy="episode", shared_ring=shared)


def test_abi_declares_the_new_entries(gcrl):
    for name in ("gcrl_her_create_goal", "gcrl_her_goal_strategy", "gcrl_her_read_elapsed"):
        assert hasattr(gcrl._ffi.lib, name), name
    assert gcrl._ffi.lib.gcrl_her_goal_strategy(None) == -1
    assert not gcrl._ffi.lib.gcrl_her_create_goal(None, None, 1, 2)      # null config: refused, no device touched


def test_new_kernels_use_no_scratch(tmp_path):
    """her_relabel.hip compiled to gfx950 assembly with the Makefile's flags: the unit has its six kernels and no others, and
    .private_segment_fixed_size is 0 for each"""
    csrc = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)).split()
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1))
    asm = tmp_path / "her_relabel.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "her_relabel.hip"), "-o", str(asm)], check=True, cwd=csrc)
    text = asm.read_text()
    found = re.findall(r"\.name:\s+(\S*_kernel\S*)\n((?:(?!\.name:).)*?)\.private_segment_fixed_size:\s+(\d+)", text, re.S)
    sizes = {n: int(sz) for n, _, sz in found}
    assert len(sizes) == len(re.findall(r"^\s*\.amdhsa_kernel\s", text, re.M)) == 6, sizes         # every kernel of the unit was found
    # one flush, the one-step and n-step gathers <false> and <true>, one public form
    count = lambda part: sum(part in n for n in sizes)
    assert count("her_flush_sample_kernel") == 1 and count("her_gather_relabel_pub_kernel") == 1, sizes
    assert count("her_gather_relabel_kernelILb") == 2 and count("her_gather_nstep_kernelILb") == 2, sizes
    assert all(v == 0 for v in sizes.values()), sizes
