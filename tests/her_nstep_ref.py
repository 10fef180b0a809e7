"""n-step returns on a sample-mode HER ring (HERBuffer(relabel="sample", n_step=N, gamma=g); csrc/her_relabel.hip) restated in numpy.
This file is the DEFINITION of the feature and builds on tests/her_relabel_ref.py, the definition of the mode: the kernels are held
to it bit for bit.

1 <= N <= 8; g32 = float32(gamma), the cast the TD kernels apply to the agent's gamma.  The c-th gathered row, of logical index j:
    p    = (head + j) mod cap
    rem  = clamp(rem[p], 0, min(flush_len, cap) - 1)
    f    = decide(seed, k, c, rem)                        exactly as for N = 1: the relabel stream is consumed identically for every N
    m    = min(N, rem + 1)                                the window never leaves the episode
    last = (p + m - 1) mod cap
    s, a <- record p      (goal slot of s <- ag[(p + f) mod cap] when f > 0)
    ns   <- record last   (goal slot <- the same goal when f > 0)
    r_j, j = 0 .. m-1:   f > 0: reward(ag[(p + j) mod cap], ag[(p + f) mod cap])  (her_relabel_ref.reward)    f = 0: r[(p + j) mod cap] as stored
    d_last:              f > 0: 0.0                                                                           f = 0: d[last] as stored
    R:   acc = r_{m-1};  for j = m-2 .. 0: acc = fadd(r_j, fmul(g32, acc))                  (fp32, one rounding per operation)
    d':  m == 1: d_last, bit for bit;  else gp = 1; (m - 1) times gp = fmul(gp, g32);  d' = fsub(1, fmul(gp, fsub(1, d_last)))
    outputs: r <- R, d <- d'
Every TD site of the engine forms y = r + g32 * (1 - d) * q' with d read as a float, so these two outputs give it the n-step target
R + g32^m (1 - d_last) q'.

No inner termination test: under the ring's invariant (her_relabel_ref) an episode's rows are appended by one flush and a `done`
flushes, so only an episode's LAST row can carry d != 0, and the window ends there at the latest (m <= rem + 1).  A goal reached
inside the window of a relabelled row (f < m) does not cut the window either: d_last stays 0, as it does for one-step relabels.
With N = 1, and for any row with rem = 0 whatever N is, the outputs are her_relabel_ref.gather's, bit for bit.
"""
import numpy as np

import her_relabel_ref as R

N_MAX = 8
F32 = np.float32


def fold_rewards(rs, g32) -> np.float32:
    """r_0 + g (r_1 + g (.. r_{m-1})), Horner from the last reward, every operation rounded to fp32"""
    acc = F32(rs[-1])
    for j in range(len(rs) - 2, -1, -1):
        acc = F32(F32(rs[j]) + F32(F32(g32) * acc))
    return acc


def fold_done(d_last, m: int, g32) -> np.float32:
    if m == 1:
        return F32(d_last)
    gp = F32(1.0)
    for _ in range(m - 1):
        gp = F32(gp * F32(g32))
    return F32(F32(1.0) - F32(gp * F32(F32(1.0) - F32(d_last))))


def gather(s, a, ns, r, d, ag, rem, head: int, cap: int, idx, counter: int, seed: int, k: int, kind: int, thr: float,
           n_step: int, gamma: float, flush_len: int = R.FLUSH_LEN):
    """her_relabel_ref.gather's arguments, then n_step and gamma.
    -> dict(s, a, r, ns, d: the batch; f, fut as her_relabel_ref.gather; m: rows of each window; last: the slot ns comes from)"""
    assert 1 <= n_step <= N_MAX
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    n, G, S = idx.size, ag.shape[1], s.shape[1]
    g32 = F32(gamma)
    out = dict(s=np.empty((n, S), F32), a=np.empty((n, a.shape[1]), F32), r=np.empty(n, F32), ns=np.empty((n, S), F32), d=np.empty(n, F32),
               f=np.zeros(n, np.int64), fut=np.full(n, -1, np.int64), m=np.zeros(n, np.int64), last=np.zeros(n, np.int64))
    rem_max = min(flush_len, cap) - 1
    for t in range(n):
        p = (head + int(idx[t])) % cap
        x = float(rem[p])
        rm = int(min(max(x if x == x else 0.0, 0.0), float(rem_max)))
        f = R.decide(seed, k, counter + t, rm)
        m = min(n_step, rm + 1)
        last = (p + m - 1) % cap
        out["s"][t], out["a"][t], out["ns"][t] = s[p], a[p], ns[last]
        if f:
            fut = (p + f) % cap
            out["s"][t, S - G:] = ag[fut]
            out["ns"][t, S - G:] = ag[fut]
            rs = [R.reward(ag[(p + j) % cap], ag[fut], kind, thr) for j in range(m)]
            d_last = F32(0.0)
            out["f"][t], out["fut"][t] = f, fut
        else:
            rs = [r[(p + j) % cap] for j in range(m)]
            d_last = d[last]
        out["r"][t] = fold_rewards(rs, g32)
        out["d"][t] = fold_done(d_last, m, g32)
        out["m"][t], out["last"][t] = m, last
    return out
