"""CPU restatement (numpy, float32) of the device-resident prioritised replay (csrc/per_tree.hip, csrc/per_host.h).  The device
mode is DEFINED by this file; the GPU tests hold the kernels to it bit for bit where the arithmetic is adds and compares, and
within a stated bound where a `powf` is involved.

Layout.  Level 0 = leaves: one float32 priority per PHYSICAL ring slot, zero-padded to a multiple of 64; never-filled slots
hold 0.  Level k+1 = one float32 sum per 64 entries of level k, zero-padded to a multiple of 64.  The levels end with the first
one of at most 64 entries (the top block).

Reduction order (`reduce64`).  A node is the xor-butterfly sum of its 64 children: x <- x + x[lane ^ 32], then ^ 16, 8, 4, 2, 1;
the node is lane 0 (every lane holds the same bits, float32 addition being commutative).  A node is always recomputed from its
children, never adjusted.

Scan (`scan64`).  Inclusive, by six shifted adds: for off in 1, 2, 4, 8, 16, 32: P[lane] <- P[lane] + P[lane - off] for
lane >= off (all lanes from the values before the step).

Uniform (`uniform24`).  u = float32(h >> 40) * 2^-24 with h = mix64(mix64(seed ^ K) + ctr), K = 0x5045525f54524545,
ctr = (((draw << 20) + b) << 3) + level, all in 64-bit wrap-around arithmetic; draw = the tree's draw counter (one per batch
drawn), b = the batch element, level = the level whose block is being scanned (leaves = 0).  mix64 is the project's counter hash
(csrc/her_ring.h, oracle/her_oracle.py).

Child rule (`descend`).  x = u * P[63] (float32).  Descend into the FIRST child with P > x and value > 0, else the LAST child
with value > 0 (else child 0: an empty block).  A zero slot is never drawn.

Index mapping.  Drawn slot -> logical index (slot - head) mod cap; logical j -> slot (head + j) mod cap.

Update.  leaf <- (|td| + eps)^alpha; when an index occurs more than once in the batch the LAST occurrence wins (the reference's
zip order, src/buffer.py:86-89).  Push.  The pushed row's slot gets 1.0 (src/buffer.py:48), overwriting the evicted row's.

Weights.  w_b = (N * (p_b / total))^(-beta) / max_b(...), total = reduce64 of the top block, N = rows in the ring.
"""
import numpy as np

FAN = 64
K = np.uint64(0x5045525F54524545)
LANE = np.arange(FAN)


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def level_sizes(cap: int):
    """-> [(used, padded)] per level, leaves first."""
    out, used = [], int(cap)
    while True:
        padded = (used + FAN - 1) // FAN * FAN
        out.append((used, padded))
        if padded <= FAN:
            return out
        used = padded // FAN


def reduce64(children):
    """[n, 64] float32 -> [n] float32, the fixed xor-butterfly order."""
    x = np.asarray(children, dtype=np.float32).reshape(-1, FAN).copy()
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[:, LANE ^ off]
    return x[:, 0].copy()


def build(leaves_padded):
    """All levels from the padded leaves (a pure function of them)."""
    levels = [np.asarray(leaves_padded, dtype=np.float32).copy()]
    assert levels[0].size % FAN == 0
    while levels[-1].size > FAN:
        s = reduce64(levels[-1])
        nxt = np.zeros((s.size + FAN - 1) // FAN * FAN, np.float32)
        nxt[:s.size] = s
        levels.append(nxt)
    return levels


def check_invariant(levels):
    """Every level above the leaves == the restated reduction of the level below, bitwise; padding is zero."""
    for k in range(1, len(levels)):
        want = reduce64(levels[k - 1])
        got = levels[k]
        assert got.size % FAN == 0 and got.size >= want.size
        assert np.array_equal(got[:want.size].view(np.uint32), want.view(np.uint32)), f"level {k} is not the reduction of level {k - 1}"
        assert not got[want.size:].any(), f"level {k}: padding is not zero"
    assert levels[-1].size == FAN


def scan64(v):
    """[n, 64] float32 -> inclusive scan along the lanes by six shifted adds."""
    P = np.asarray(v, dtype=np.float32).reshape(-1, FAN).copy()
    for off in (1, 2, 4, 8, 16, 32):
        up = np.zeros_like(P)
        up[:, off:] = P[:, :-off]
        P = np.where(LANE[None, :] >= off, P + up, P).astype(np.float32)
    return P


def uniform24(seed: int, draw, b, level: int):
    draw = np.asarray(draw, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = (((draw << np.uint64(20)) + b) << np.uint64(3)) + np.uint64(level)
        h = mix64(mix64(np.uint64(seed) ^ K) + ctr)
    return (h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def descend(levels, seed: int, draw, b):
    """Vectorised over (draw, b) pairs -> (physical slots int64 [n], leaf priorities float32 [n])."""
    draw = np.atleast_1d(np.asarray(draw, dtype=np.uint64))
    b = np.atleast_1d(np.asarray(b, dtype=np.uint64))
    n = draw.size
    blk = np.zeros(n, np.int64)
    leaf = np.zeros(n, np.float32)
    rows = np.arange(n)
    for k in range(len(levels) - 1, -1, -1):
        v = levels[k].reshape(-1, FAN)[blk]
        P = scan64(v)
        x = (uniform24(seed, draw, b, k) * P[:, 63]).astype(np.float32)
        pos = v > 0
        hit = pos & (P > x[:, None])
        first = np.argmax(hit, axis=1)
        last_pos = FAN - 1 - np.argmax(pos[:, ::-1], axis=1)
        child = np.where(hit.any(axis=1), first, np.where(pos.any(axis=1), last_pos, 0))
        leaf = v[rows, child]
        blk = blk * FAN + child
    return blk, leaf


def draw(levels, seed: int, counter: int, B: int, head: int, cap: int):
    """One batch: draw number `counter`, elements 0..B-1 -> (logical indices uint32 [B], leaf priorities float32 [B])."""
    slots, p = descend(levels, seed, np.full(B, counter, np.uint64), np.arange(B, dtype=np.uint64))
    return ((slots - head) % cap).astype(np.uint32), p


def last_occurrence(idx):
    """Boolean mask: True where idx[b] does not occur again later in the batch (the occurrence that wins)."""
    idx = np.asarray(idx)
    seen, keep = set(), np.zeros(idx.size, bool)
    for b in range(idx.size - 1, -1, -1):
        if int(idx[b]) not in seen:
            keep[b] = True
            seen.add(int(idx[b]))
    return keep


def priority64(td, eps: float, alpha: float):
    """The update's formula evaluated in float64 from float32 inputs (eps and alpha as the float32 values the device holds)."""
    return (np.abs(np.asarray(td, np.float32).astype(np.float64)) + float(np.float32(eps))) ** float(np.float32(alpha))


def weights64(p, total, N: int, beta: float):
    """The weights' formula in float64 from the device's own float32 leaf priorities and top-block total."""
    w = (float(N) * (np.asarray(p, np.float32).astype(np.float64) / float(np.float32(total)))) ** (-float(np.float32(beta)))
    return w / w.max()


class RefPER:
    """The whole state machine on the CPU: ring bookkeeping (deque(maxlen) semantics), pending pushes refreshed as slot
    segments before a draw, incremental recomputation of the touched ancestors.  float32 throughout; its own powf is numpy's."""

    def __init__(self, cap: int, alpha: float, eps: float = 1e-6, seed: int = 0):
        self.cap, self.alpha, self.eps, self.seed = int(cap), np.float32(alpha), np.float32(eps), int(seed)
        self.sizes = level_sizes(cap)
        self.levels = [np.zeros(p, np.float32) for _, p in self.sizes]
        self.head = self.len = 0
        self.pending = 0
        self.counter = 0

    def push(self, n: int = 1):
        for _ in range(n):
            if self.len < self.cap:
                self.len += 1
            else:
                self.head = (self.head + 1) % self.cap
        self.pending += n

    def pending_segments(self):
        """The slots of the pending pushes: a range ending at the tail, as at most two half-open segments."""
        m = min(self.pending, self.len)
        if m <= 0:
            return []
        tail = (self.head + self.len) % self.cap
        first = (tail - m) % self.cap
        if first + m <= self.cap:
            return [(first, first + m)]
        return [(first, self.cap), (0, first + m - self.cap)]

    def _recompute(self, segs):
        for k in range(1, len(self.levels)):
            segs = [(a // FAN, (b - 1) // FAN + 1) for a, b in segs if b > a]
            child = self.levels[k - 1].reshape(-1, FAN)
            for a, b in segs:
                self.levels[k][a:b] = reduce64(child[a:b])

    def refresh(self):
        segs = self.pending_segments()
        self.pending = 0
        for a, b in segs:
            self.levels[0][a:b] = np.float32(1.0)
        self._recompute(segs)

    def draw(self, B: int):
        self.refresh()
        out = draw(self.levels, self.seed, self.counter, B, self.head, self.cap)
        self.counter += 1
        return out

    def update(self, idx, td):
        self.refresh()
        idx = np.asarray(idx, dtype=np.int64)
        td = np.asarray(td, dtype=np.float32)
        keep = last_occurrence(idx)
        slots = (self.head + idx) % self.cap
        self.levels[0][slots[keep]] = ((np.abs(td[keep]) + self.eps) ** self.alpha).astype(np.float32)
        self._recompute([(int(s), int(s) + 1) for s in slots])

    def set_priorities(self, values):
        v = np.asarray(values, dtype=np.float32)
        assert v.size == self.len
        leaves = np.zeros(self.levels[0].size, np.float32)
        leaves[(self.head + np.arange(self.len)) % self.cap] = v
        self.levels = build(leaves)
        self.pending = 0

    def priorities(self):
        self.refresh()
        return self.levels[0][(self.head + np.arange(self.len)) % self.cap].copy()
