"""CPU restatement (numpy, float32) of TD-error prioritised replay on a sample-mode HER ring (prioritise="td_error";
csrc/her_td.hip).  The mode is DEFINED by this file together with tests/per_tree_ref.py, which it imports for everything the
device-resident prioritised replay already defines: the tree layout, the reduction order `reduce64`, the descent `draw`, the weights.

Tree.  per_tree_ref's: one float32 leaf per PHYSICAL slot = per stored real transition (a sample-mode ring stores each row once),
64-ary sums, a node always the recomputed xor-butterfly reduction of its 64 children, never-filled slots 0.

p_max.  One float32 word beside the tree, initially 1.0.

Flush (`seed`).  Every row a flush wrote gets the leaf p_max as it stands after the last priority update; then the ancestors of
the written slots are recomputed.  The slots are the last min(total, cap) ones before the ring's tail AFTER the flush, as at most two
contiguous segments; a ring smaller than the flush (total > cap: the flush skips its first total - cap rows) writes every slot once.
Rows present when the tree is attached get p_max's initial value.  NOT the PER buffer's constant 1.0: new rows enter at the largest
priority seen so far, the PER paper's rule.

Draw.  per_tree_ref.draw, unchanged: draw number = the tree's counter (one per batch of B rows, with replacement), logical index
(slot - head) mod cap, the leaf priority beside it.  Weights: per_tree_ref's formula with N = the ring's length.

Update (`update`).  For the step's idx[B], td[B]: v_b = |td_b| + eps in ONE float32 add when alpha == 1 (bit for bit), otherwise
powf(|td_b| + eps, alpha) (held to a float64 evaluation within 1e-6 relative).  The leaf of idx[b] becomes v_b where b is the LAST
occurrence of its index; an index >= cap is skipped.  Then p_max <- fmaxf(p_max, m), m the largest FINITE v_b over all B rows whose
index is inside the ring (overwritten occurrences included), reduced in one fixed order (`pmax_reduce`): per thread t of 1024 its
rows t, t + 1024, ... in order starting from 0, the xor-butterfly 32 .. 1 across each wave of 64 threads, then the 16 waves' words in
wave order.  A NaN or infinite v_b is written to its leaf and never raises p_max; p_max never decreases.  Then the touched ancestors
are recomputed level by level.

Relabelling.  A drawn row is relabelled, n-step-folded and normalised as the ring is configured, and the TD error of whatever the
gather produced updates the stored row's one leaf (the usual HER + PER form).
"""
import numpy as np

import per_tree_ref as R

FAN = R.FAN
THREADS = 1024
P_MAX_INIT = np.float32(1.0)
FLT_MAX = np.float32(3.4028234663852886e38)


def new_values(td, eps, alpha):
    """v_b float32 [B]: the single add for alpha == 1, else this file's own float32 power (numpy's)."""
    x = (np.abs(np.asarray(td, np.float32)) + np.float32(eps)).astype(np.float32)
    if np.float32(alpha) == np.float32(1.0):
        return x
    with np.errstate(invalid="ignore", over="ignore"):
        return np.power(x, np.float32(alpha)).astype(np.float32)


def _fmax(a, b):
    """fmaxf on finite, non-negative operands"""
    return np.maximum(a, b).astype(np.float32)


def pmax_reduce(values, inside):
    """m of a batch in the kernel's order; values float32 [B], inside bool [B] (index < cap).  0 when no row qualifies."""
    v = np.asarray(values, np.float32)
    ok = np.asarray(inside, bool) & (v <= FLT_MAX)          # NaN and +inf fail the compare
    m = np.zeros(THREADS, np.float32)
    for b in range(v.size):                                   # per thread its rows in order
        if ok[b]:
            t = b % THREADS
            m[t] = _fmax(m[t], v[b])
    m = m.reshape(-1, FAN)
    for off in (32, 16, 8, 4, 2, 1):                          # the wave's xor-butterfly
        m = _fmax(m, m[:, R.LANE ^ off])
    out = m[0, 0]
    for w in range(1, m.shape[0]):                            # the waves' words in wave order
        out = _fmax(out, m[w, 0])
    return np.float32(out)


def segments(head: int, length: int, cap: int, total: int):
    """The slots of the last `total` pushed rows of a ring with head / length AFTER the flush: [(a0, a1)] or two segments."""
    m = min(int(total), int(length))
    if m <= 0 or cap <= 0:
        return []
    tail = (head + length) % cap
    first = (tail - m) % cap
    if first + m <= cap:
        return [(first, first + m)]
    return [(first, cap), (0, first + m - cap)]


def recompute(levels, segs):
    for k in range(1, len(levels)):
        segs = [(a // FAN, (b - 1) // FAN + 1) for a, b in segs if b > a]
        child = levels[k - 1].reshape(-1, FAN)
        for a, b in segs:
            levels[k][a:b] = R.reduce64(child[a:b])


def book_append(head: int, length: int, cap: int, total: int):
    """deque(maxlen=cap) bookkeeping of a flush of `total` rows -> (head, length, skip)"""
    for _ in range(int(total)):          # row after row, each into the slot at the tail
        if length < cap:
            length += 1
        else:
            head = (head + 1) % cap
    return head, length, max(0, int(total) - cap)


def seed(levels, head: int, length: int, cap: int, total: int, p_max):
    """In place: the leaves of the rows a flush of `total` rows wrote <- p_max, their ancestors recomputed (head / length: AFTER it)."""
    segs = segments(head, length, cap, total)
    for a, b in segs:
        levels[0][a:b] = np.float32(p_max)
    recompute(levels, segs)
    return segs


def update(levels, head: int, cap: int, idx, td, eps, alpha, p_max, device_leaves=None):
    """In place -> the new p_max.  `device_leaves`: the leaves level read back from the device after ITS update — then the winning
    rows' values are the device's own (a powf differs in the last bits), so that p_max can be held bit for bit."""
    idx = np.asarray(idx).astype(np.int64) & 0xFFFFFFFF
    td = np.asarray(td, np.float32)
    v = new_values(td, eps, alpha)
    inside = idx < cap
    keep = R.last_occurrence(idx) & inside
    slots = (head + idx) % cap
    if device_leaves is not None:
        v = v.copy()
        v[keep] = np.asarray(device_leaves, np.float32)[slots[keep]]
    levels[0][slots[keep]] = v[keep]
    m = pmax_reduce(v, inside)
    recompute(levels, [(int(s), int(s) + 1) for s in slots[inside]])
    return _fmax(np.float32(p_max), m)


def weights32(p, total, N: int, beta):
    """per_weights_kernel's arithmetic in float32: x = powf(N * (p / total), -beta), w = x / max(x)."""
    p = np.asarray(p, np.float32)
    x = np.power((np.float32(N) * (p / np.float32(total)).astype(np.float32)).astype(np.float32), np.float32(-np.float32(beta))).astype(np.float32)
    return (x / x.max()).astype(np.float32)


class RefHerTd:
    """The whole state machine on the CPU: ring bookkeeping, seeding flushes, draws, updates."""

    def __init__(self, cap: int, alpha: float = 0.6, eps: float = 1e-6, seed: int = 0):
        self.cap, self.alpha, self.eps, self.seed = int(cap), np.float32(alpha), np.float32(eps), int(seed)
        self.levels = [np.zeros(p, np.float32) for _, p in R.level_sizes(cap)]
        self.head = self.len = 0
        self.p_max = P_MAX_INIT
        self.counter = 0

    def flush(self, total: int):
        self.head, self.len, _ = book_append(self.head, self.len, self.cap, int(total))
        return seed(self.levels, self.head, self.len, self.cap, int(total), self.p_max)

    def draw(self, B: int):
        out = R.draw(self.levels, self.seed, self.counter, B, self.head, self.cap)
        self.counter += 1
        return out

    def weights(self, p, beta):
        return weights32(p, R.reduce64(self.levels[-1])[0], self.len, beta)

    def update(self, idx, td):
        self.p_max = update(self.levels, self.head, self.cap, idx, td, self.eps, self.alpha, self.p_max)

    def priorities(self):
        return self.levels[0][(self.head + np.arange(self.len)) % self.cap].copy()
