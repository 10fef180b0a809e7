"""GPU (-m gpu): the goal-tail loads of csrc/her_relabel.hip at the widths the other relabelling tests do not reach.  They all run at
G = 3, where a goal row's [r, d, ag] is two 16-byte loads; here G = 2 (one load) and G = 8 (three loads, `elapsed` in the last float
of the gathers' 12-float tail), every goal strategy, one-step and n_step = 3, both gathers bit for bit against the numpy definition
that states the case: tests/her_relabel_ref.py (future, one-step), tests/her_nstep_ref.py (future, n-step), tests/her_strategy_ref.py
(final, episode).  Helpers are those of tests/test_gpu_her_relabel.py and tests/test_gpu_her_strategy.py."""
import functools

import numpy as np
import pytest

import her_nstep_ref as NS
import her_relabel_ref as R
import her_strategy_ref as GS
import test_gpu_her_relabel as T
import test_gpu_her_strategy as TS
from test_gpu_her_relabel import THR, _np, bits

pytestmark = pytest.mark.gpu

DIMS = {"G2_one_load": (10, 3, 2), "G8_three_loads": (14, 3, 8)}        # (S, A, G)
CAP, FLUSH, K, GAMMA = 120, 50, 4, 0.98
LENGTHS = (50, 1, 37, 50, 12)      # 150 rows through 120 slots: head 30, the fourth episode lies across the ring's end
ROWS = 69                          # four full waves of 16 rows and a partial one of 5
OUT = ("s", "a", "r", "ns", "d")


def _layout():
    """`remaining` and `elapsed` by physical slot and the head, from LENGTHS alone (global row g lies at slot g mod CAP)"""
    rem, el = np.zeros(CAP, np.float32), np.zeros(CAP, np.float32)
    g = 0
    for n in LENGTHS:
        for i in range(n):
            rem[g % CAP], el[g % CAP] = n - 1 - i, i
            g += 1
    return rem, el, g % CAP


def _indices(seed):
    return np.random.default_rng(seed).integers(0, CAP, ROWS).astype(np.uint32)


def _conditions(strategy, N, p, o, m):
    """what a gather's decisions must contain for a pass to say something: p the rows' slots, o the signed offsets, m the window lengths"""
    ok = (o != 0).any() and (o == 0).any()                               # a relabelled row and one left as stored
    ok = ok and (((p + o) >= CAP) | ((p + o) < 0))[o != 0].any()         # a goal row reached across the ring's end
    if strategy == "episode":
        ok = ok and (o < 0).any()
    if N > 1:
        ok = ok and (m < N).any()                                        # a window cut short by `remaining`
    return bool(ok)


def _decide(strategy, N, seed, ctr):
    """the decisions of the launch of ROWS rows at relabel counter `ctr`, on the CPU, from the ring's layout alone"""
    rem, el, head = _layout()
    idx = _indices(seed).astype(np.int64)
    p = (head + idx) % CAP
    rem_max = min(FLUSH, CAP) - 1
    rm = [GS.clamp(rem[q], rem_max) for q in p]
    back = [min(GS.clamp(el[q], rem_max), int(j)) if strategy == "episode" else 0 for q, j in zip(p, idx)]
    o = np.array([GS.decide(seed, K, ctr + t, rm[t], back[t], strategy) for t in range(ROWS)])
    return p, o, np.minimum(N, np.array(rm) + 1)


@functools.lru_cache(maxsize=None)
def _seed(strategy, N):
    """the first seed (of the ring and of the indices) at which BOTH launches of a case meet _conditions, found on the CPU"""
    for seed in range(1, 1000):
        if all(_conditions(strategy, N, *_decide(strategy, N, seed, ctr)) for ctr in (0, ROWS)):
            return seed
    raise AssertionError((strategy, N))


def _reference(strategy, N, snap, idx, ctr, seed):
    """-> (the batch, signed offsets, window lengths) by the definition that states the case"""
    head, cap = snap[8], snap[9]
    if strategy == "future" and N == 1:
        want = R.gather(*snap[:7], head, cap, idx, ctr, seed, K, R.SPARSE, THR)
        return want, want["f"], np.ones(len(idx), np.int64)
    if strategy == "future":
        want = NS.gather(*snap[:7], head, cap, idx, ctr, seed, K, R.SPARSE, THR, N, GAMMA)
        return want, want["f"], want["m"]
    want = GS.gather(*snap[:8], head, cap, idx, ctr, seed, K, R.SPARSE, THR, strategy, N, GAMMA)
    return want, want["o"], want["m"]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("strategy", ["future", "final", "episode"])
@pytest.mark.parametrize("dims", list(DIMS.values()), ids=list(DIMS))
def test_both_gathers_bitwise_the_restatement(gcrl, dims, strategy, N):
    seed = _seed(strategy, N)
    buf = TS._buffer(gcrl, CAP, dims, strategy, k=K, seed=seed, **(dict(n_step=N, gamma=GAMMA) if N > 1 else {}))
    TS._fill(buf, dims, LENGTHS, 40)
    assert len(buf) == CAP and T._head(buf) == _layout()[2] == 30        # wrapped
    snap = TS._snapshot(buf)
    idx = _indices(seed)
    p = (snap[8] + idx.astype(np.int64)) % CAP
    # the update engine's gather: sa | nsa | r | d
    want, o, m = _reference(strategy, N, snap, idx, 0, seed)
    assert _conditions(strategy, N, p, o, m), (o, m)
    out = buf.gather_update(ROWS, 1, indices=idx)
    sa, nsa, _ = T._engine_form(want, dims)
    assert np.array_equal(bits(_np(out[0])), bits(sa)), "sa"
    assert np.array_equal(bits(_np(out[1])), bits(nsa)), "nsa"
    assert np.array_equal(bits(_np(out[3])), bits(want["r"])), "r"
    assert np.array_equal(bits(_np(out[4])), bits(want["d"])), "d"
    assert buf.relabel_counter == ROWS
    # the public sample: five dense outputs, the counter carried on
    want, o, m = _reference(strategy, N, snap, idx, ROWS, seed)
    assert _conditions(strategy, N, p, o, m), (o, m)
    out = buf.sample(ROWS, 1, indices=idx)
    got = dict(s=_np(out[0]), a=_np(out[1]), r=_np(out[2]).ravel(), ns=_np(out[3]), d=_np(out[4]).ravel())
    for key in OUT:
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    assert buf.relabel_counter == 2 * ROWS
