"""Host tests (no GPU) of tests/her_relabel_ref.py, the numpy definition of sample-time HER relabelling
(HERBuffer(relabel="sample")): a hand-built ring with rows worked out by hand, the rule's edge cases, and the share of
relabelled rows — whose count tests/test_gpu_her_relabel.py then demands from the device exactly."""
import math

import numpy as np

import her_relabel_ref as R

# ---------------------------------------------------------------- a hand-built ring
# cap 8; episode A (T = 3) was flushed at slots 6, 7, 0 — it crosses the physical end — and episode B (T = 2) at slots 1, 2.
# head = 6, len = 5: logical 0, 1, 2 = A0, A1, A2 and 3, 4 = B0, B1.  S = 4 (two observation entries, then the goal), A = 1, G = 2.
CAP, HEAD = 8, 6
SLOT = {"A0": 6, "A1": 7, "A2": 0, "B0": 1, "B1": 2}
GOAL_A, GOAL_B = (9.0, 9.5), (8.0, 8.5)
AG = {"A0": (0.0, 0.0), "A1": (0.25, 0.0), "A2": (0.0, 0.03125), "B0": (1.0, 1.0), "B1": (1.0, 1.5)}
REM = {"A0": 2, "A1": 1, "A2": 0, "B0": 1, "B1": 0}
THR = 0.1
SEED, KF = 7, 4
IDX = [0, 1, 2, 3, 4, 0, 1, 3, 0, 0]
NAMES = ["A0", "A1", "A2", "B0", "B1"]
# what the counter hash decides for rows c = 0 .. 9 of this seed (asserted below): the future offsets
F_WANT = [1, 1, 0, 1, 0, 2, 1, 1, 2, 0]


def _ring():
    s = np.zeros((CAP, 4), np.float32); a = np.zeros((CAP, 1), np.float32); ns = np.zeros((CAP, 4), np.float32)
    r = np.zeros(CAP, np.float32); d = np.zeros(CAP, np.float32); ag = np.zeros((CAP, 2), np.float32); rem = np.zeros(CAP, np.float32)
    for j, name in enumerate(NAMES):
        p = SLOT[name]
        goal = GOAL_A if name[0] == "A" else GOAL_B
        s[p] = (10 * j + 1, 10 * j + 2) + goal
        ns[p] = (10 * j + 3, 10 * j + 4) + goal
        a[p] = 10 * j + 5
        r[p] = -1.0
        d[p] = 1.0 if REM[name] == 0 else 0.0
        ag[p] = AG[name]
        rem[p] = REM[name]
    return s, a, ns, r, d, ag, rem


def _row(j, goal, r, d):
    """the batch row of logical index j with `goal` in the goal slots"""
    return ((10 * j + 1, 10 * j + 2) + goal, (10 * j + 5,), (10 * j + 3, 10 * j + 4) + goal, r, d)


def test_hand_built_ring_sparse_and_dense():
    assert [R.decide(SEED, KF, c, REM[NAMES[j]]) for c, j in enumerate(IDX)] == F_WANT
    d12 = float(np.sqrt(np.float32(0.0634765625)))       # |A1 - A2|: 0.25^2 + 0.03125^2, both squares and their sum exact in float32
    for kind, (r01, r02, r12, rb) in ((R.SPARSE, (-1.0, -0.0, -1.0, -1.0)), (R.DENSE, (-0.25, -0.03125, -d12, -0.5))):
        got = R.gather(*_ring(), HEAD, CAP, IDX, 0, SEED, KF, kind, THR)
        want = [
            _row(0, AG["A1"], r01, 0.0),      # c 0: A0, f 1 -> slot 7 = A1
            _row(1, AG["A2"], r12, 0.0),      # c 1: A1 at slot 7, f 1 -> slot 8 - 8 = 0 = A2: across the physical end
            _row(2, GOAL_A, -1.0, 1.0),       # c 2: A2 is its episode's last row (rem 0): stored row, done kept
            _row(3, AG["B1"], rb, 0.0),       # c 3: B0, f 1 -> slot 2 = B1
            _row(4, GOAL_B, -1.0, 1.0),       # c 4: B1, rem 0
            _row(0, AG["A2"], r02, 0.0),      # c 5: A0, f 2 -> slot 8 - 8 = 0 = A2
            _row(1, AG["A2"], r12, 0.0),      # c 6: A1, f 1
            _row(3, AG["B1"], rb, 0.0),       # c 7: B0, f 1
            _row(0, AG["A2"], r02, 0.0),      # c 8: A0, f 2
            _row(0, GOAL_A, -1.0, 0.0),       # c 9: the hash says "original" (1 in k + 1): stored row
        ]
        for t, (ws, wa, wns, wr, wd) in enumerate(want):
            assert np.array_equal(got["s"][t], np.array(ws, np.float32)), (kind, t)
            assert np.array_equal(got["a"][t], np.array(wa, np.float32)), (kind, t)
            assert np.array_equal(got["ns"][t], np.array(wns, np.float32)), (kind, t)
            assert got["r"][t].tobytes() == np.float32(wr).tobytes(), (kind, t, got["r"][t], wr)     # bytes: -0.0 is not +0.0
            assert got["d"][t] == np.float32(wd), (kind, t)
        assert list(got["fut"]) == [7, 0, -1, 2, -1, 0, 0, 2, 0, -1]


def test_counter_is_per_row():
    """one launch of n rows = the same rows in pieces, each starting where the last ended"""
    whole = R.gather(*_ring(), HEAD, CAP, IDX, 5, SEED, KF, R.SPARSE, THR)
    a = R.gather(*_ring(), HEAD, CAP, IDX[:3], 5, SEED, KF, R.SPARSE, THR)
    b = R.gather(*_ring(), HEAD, CAP, IDX[3:], 8, SEED, KF, R.SPARSE, THR)
    for key in ("s", "a", "r", "ns", "d", "f"):
        assert np.array_equal(whole[key], np.concatenate([a[key], b[key]])), key


def test_rule_edges():
    for seed in (0, 1, SEED, 2 ** 63 + 5):
        for c in range(300):
            assert R.decide(seed, 4, c, 0) == 0                  # the last row of an episode is never relabelled
            assert R.decide(seed, 0, c, 1 + c % 49) == 0         # k = 0: hash_below(.., 1) is 0, never relabelled
            for rem in (1, 2, 7, 49):
                assert 0 <= R.decide(seed, 4, c, rem) <= rem     # f in [1, rem], or 0
    hit = {R.decide(SEED, 8, c, 3) for c in range(400)}
    assert hit == {0, 1, 2, 3}                                   # every offset is reached, and so is "original"
    # a tail that holds rubbish cannot take an address out of the ring: remaining is clamped to [0, min(flush_len, cap) - 1]
    s, a, ns, r, d, ag, rem = _ring()
    for junk in (1e9, -5.0, float("nan"), float("inf")):
        rem[:] = junk
        got = R.gather(s, a, ns, r, d, ag, rem, HEAD, CAP, IDX, 0, SEED, KF, R.SPARSE, THR)
        assert got["f"].max() <= CAP - 1 and got["fut"].max() < CAP


# the share of relabelled rows: k / (k + 1) in expectation, as the reference's 1 original : k copies.  The device test gathers
# SHARE_N rows that all have rem > 0 from a ring seeded SHARE_SEED, counter 0, and must count exactly share_count() relabels.
SHARE_SEED, SHARE_K, SHARE_N = 12345, 4, 4096


def share_count() -> int:
    return R.relabel_count(SHARE_SEED, SHARE_K, 0, SHARE_N)


def test_share_of_relabelled_rows():
    got = sum(1 for c in range(SHARE_N) if R.decide(SHARE_SEED, SHARE_K, c, 1 + c % 49) != 0)
    assert got == share_count()
    p = SHARE_K / (SHARE_K + 1)
    z = (got - SHARE_N * p) / math.sqrt(SHARE_N * p * (1 - p))
    print(f"relabelled {got} of {SHARE_N}: z = {z:+.3f} against Binomial(n, {p})")
    assert abs(z) <= 4.0, (got, z)
