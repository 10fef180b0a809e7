"""Sample-time HER relabelling (HERBuffer(relabel="sample"), csrc/her_relabel.hip) restated in numpy.  This file is the
DEFINITION of the mode, as tests/per_tree_ref.py is of the priority tree: the kernels are held to it bit for bit.

The ring stores original transitions only.  Record `p` (a PHYSICAL slot, 0 <= p < cap) carries, besides s | a | ns | r | d,
a tail: ag[p] (the achieved goal pushed with the transition) and rem[p] = T - 1 - i, the number of rows of its episode that
follow it.  An episode's rows are appended by one flush, contiguously and in step order, and eviction is FIFO: if a row is alive,
the rem[p] rows after it are alive too, at slots (p + 1 .. p + rem[p]) mod cap.

Row number c (c counts every row ever gathered from the ring in this mode, across launches: `counter` below is c of idx[0])
that draws logical index j:
    p       = (head + j) mod cap
    rem     = clamp(rem[p], 0, min(flush_len, cap) - 1)
    relabel = rem > 0 and hash_below(seed, K, 2c, k + 1) != 0            (share k / (k + 1))
    f       = 1 + hash_below(seed, K, 2c + 1, rem)                        (only when relabel)
    fut     = (p + f) mod cap
relabelled: the last G entries of s and of ns <- ag[fut]; r <- reward(ag[p], ag[fut]); d <- 0.  Otherwise the stored row.
reward: dist = sqrt(sum_q (ag[p][q] - ag[fut][q])^2) in float32, one rounding per operation, components in order;
sparse (kind 0): -1.0 if dist > thr else -0.0; dense (kind 1): -dist.
"""
import numpy as np

from oracle.her_oracle import hash_below, mix64  # noqa: F401  (mix64: the hash's mixer, re-exported for the tests)

K = 0x52454C4142454C21      # the relabel stream's id ("RELABEL!")
SPARSE, DENSE = 0, 1
FLUSH_LEN = 50


def decide(seed: int, k: int, c: int, rem: int) -> int:
    """future offset f in [1, rem] of the c-th gathered row, or 0: the row stays as stored"""
    if rem <= 0 or hash_below(seed, K, 2 * c, k + 1) == 0:
        return 0
    return 1 + hash_below(seed, K, 2 * c + 1, rem)


def relabel_count(seed: int, k: int, counter: int, n: int) -> int:
    """how many of the rows counter .. counter + n - 1 are relabelled when every one of them has rem > 0"""
    return sum(1 for c in range(counter, counter + n) if hash_below(seed, K, 2 * c, k + 1) != 0)


def reward(ag_i, ag_f, kind: int, thr: float) -> np.float32:
    acc = np.float32(0.0)
    for q in range(len(ag_i)):
        df = np.float32(np.float32(ag_i[q]) - np.float32(ag_f[q]))
        acc = np.float32(acc + np.float32(df * df))
    dist = np.float32(np.sqrt(acc))
    if kind == SPARSE:
        return np.float32(-1.0) if dist > np.float32(thr) else np.float32(-0.0)
    return np.float32(-dist)


def physical(logical, head: int, cap: int):
    """rows in logical (oldest-first) order, as HERBuffer.rows() / tails() return them -> [cap, ...] by physical slot (free slots 0)"""
    logical = np.asarray(logical)
    out = np.zeros((cap,) + logical.shape[1:], logical.dtype)
    for j in range(logical.shape[0]):
        out[(head + j) % cap] = logical[j]
    return out


def gather(s, a, ns, r, d, ag, rem, head: int, cap: int, idx, counter: int, seed: int, k: int, kind: int, thr: float,
           flush_len: int = FLUSH_LEN):
    """s [cap, S], a [cap, A], ns [cap, S], r [cap], d [cap], ag [cap, G], rem [cap]: the ring by PHYSICAL slot; idx: logical indices.
    -> dict(s, a, r, ns, d: the batch; f: future offsets (0 = not relabelled); fut: future slots (-1 = not relabelled))"""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    n, G = idx.size, ag.shape[1]
    S = s.shape[1]
    out = dict(s=np.empty((n, S), np.float32), a=np.empty((n, a.shape[1]), np.float32), r=np.empty(n, np.float32),
               ns=np.empty((n, S), np.float32), d=np.empty(n, np.float32), f=np.zeros(n, np.int64), fut=np.full(n, -1, np.int64))
    rem_max = min(flush_len, cap) - 1
    for t in range(n):
        p = (head + int(idx[t])) % cap
        x = float(rem[p])
        rm = int(min(max(x if x == x else 0.0, 0.0), float(rem_max)))
        f = decide(seed, k, counter + t, rm)
        out["s"][t], out["a"][t], out["ns"][t], out["r"][t], out["d"][t] = s[p], a[p], ns[p], r[p], d[p]
        if f:
            fut = (p + f) % cap
            out["s"][t, S - G:] = ag[fut]
            out["ns"][t, S - G:] = ag[fut]
            out["r"][t] = reward(ag[p], ag[fut], kind, thr)
            out["d"][t] = np.float32(0.0)
            out["f"][t], out["fut"][t] = f, fut
    return out
