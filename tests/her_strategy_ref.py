"""Goal selection of sample-time HER relabelling (HERBuffer(relabel="sample", goal_strategy=...); csrc/her_relabel.hip) restated in
numpy.  This file is the DEFINITION of the `final` and `episode` strategies and builds on tests/her_relabel_ref.py (the mode) and
tests/her_nstep_ref.py (n-step windows): the kernels are held to it bit for bit.  `future` here is those two files' rule, bit for bit.

A record's tail is [ag | remaining], and on a ring created with `episode` [ag | remaining | elapsed]: elapsed[p] = i, the number of
rows of its episode that precede row p.  The c-th row ever gathered from the ring, drawing logical index j:
    p, rem, rem_max   exactly as in her_relabel_ref          (rem_max = min(flush_len, cap) - 1)
    el      = clamp(elapsed[p], 0, rem_max), NaN -> 0         (`episode` only; 0 otherwise)
    back    = min(el, j)
Logical index 0 is the oldest live row and eviction is FIFO, so the min(el, j) rows before p are exactly the live predecessors of
its episode, at slots p - 1 .. p - back mod cap — after a wrap, after load_state re-laid the rows at head 0, on a ring smaller
than a flush.  Candidates n_c:   future: rem      final: 1 if rem > 0 else 0      episode: back + rem
    relabel = n_c > 0 and hash_below(seed, K, 2c, k + 1) != 0            (the stream and key of before: share k / (k + 1))
    offset o (0: the row stays as stored)
        future:  1 + hash_below(seed, K, 2c + 1, rem)
        final:   rem                                                     (key 2c + 1 is not evaluated; it stays reserved)
        episode: u = hash_below(seed, K, 2c + 1, back + rem);  o = u - back if u < back else u - back + 1
                 (uniform over [-back, rem] \\ {0}: never the row itself)
    g = (p + o) mod cap
One-step outputs: her_relabel_ref's with ag[g] for ag[fut] when o != 0.  n-step outputs: her_nstep_ref's — m = min(N, rem + 1), last,
Horner's fold and d' unchanged, `f > 0` read as `o != 0`, every r_j of a relabelled window reward(ag[p + j], ag[g]), d_last = 0; a
goal reached inside the window does not cut it.  An episode's last row (rem = 0) is never relabelled under `final`: its own ag is
the final one.
"""
import numpy as np

import her_nstep_ref as NS
import her_relabel_ref as R

FUTURE, FINAL, EPISODE = "future", "final", "episode"
STRATEGIES = {FUTURE: 0, FINAL: 1, EPISODE: 2}      # include/gcrl.h GCRL_GOAL_*
F32 = np.float32


def clamp(x, hi: int) -> int:
    """a tail word as stored -> an integer in [0, hi]; NaN -> 0"""
    x = float(x)
    return int(min(max(x if x == x else 0.0, 0.0), float(hi)))


def candidates(strategy: str, rem: int, back: int) -> int:
    if strategy == FUTURE:
        return rem
    if strategy == FINAL:
        return 1 if rem > 0 else 0
    if strategy == EPISODE:
        return back + rem
    raise ValueError(f"goal_strategy must be one of {sorted(STRATEGIES)}, got {strategy!r}")


def decide(seed: int, k: int, c: int, rem: int, back: int, strategy: str) -> int:
    """signed offset o of the goal row of the c-th gathered row, or 0: the row stays as stored"""
    n_c = candidates(strategy, rem, back)
    if n_c <= 0 or R.hash_below(seed, R.K, 2 * c, k + 1) == 0:
        return 0
    if strategy == FUTURE:
        return 1 + R.hash_below(seed, R.K, 2 * c + 1, rem)
    if strategy == FINAL:
        return rem
    u = R.hash_below(seed, R.K, 2 * c + 1, back + rem)
    return u - back if u < back else u - back + 1


def gather(s, a, ns, r, d, ag, rem, elapsed, head: int, cap: int, idx, counter: int, seed: int, k: int, kind: int, thr: float,
           strategy: str = FUTURE, n_step: int = 1, gamma: float = 0.0, flush_len: int = R.FLUSH_LEN):
    """her_relabel_ref.gather's ring by PHYSICAL slot plus elapsed [cap] (None unless `episode`), then the strategy, n_step and gamma.
    -> dict(s, a, r, ns, d: the batch; o: signed offsets (0 = not relabelled); g: goal slots (-1 = not relabelled); back; m; last)"""
    assert 1 <= n_step <= NS.N_MAX
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    n, G, S = idx.size, ag.shape[1], s.shape[1]
    g32 = F32(gamma)
    out = dict(s=np.empty((n, S), F32), a=np.empty((n, a.shape[1]), F32), r=np.empty(n, F32), ns=np.empty((n, S), F32), d=np.empty(n, F32),
               o=np.zeros(n, np.int64), g=np.full(n, -1, np.int64), back=np.zeros(n, np.int64), m=np.zeros(n, np.int64),
               last=np.zeros(n, np.int64))
    rem_max = min(flush_len, cap) - 1
    for t in range(n):
        j = int(idx[t])
        p = (head + j) % cap
        rm = clamp(rem[p], rem_max)
        back = min(clamp(elapsed[p], rem_max), j) if strategy == EPISODE else 0
        o = decide(seed, k, counter + t, rm, back, strategy)
        m = min(n_step, rm + 1)
        last = (p + m - 1) % cap
        out["s"][t], out["a"][t], out["ns"][t] = s[p], a[p], ns[last]
        if o:
            g = (p + o) % cap
            out["s"][t, S - G:] = ag[g]
            out["ns"][t, S - G:] = ag[g]
            rs = [R.reward(ag[(p + i) % cap], ag[g], kind, thr) for i in range(m)]
            d_last = F32(0.0)
            out["o"][t], out["g"][t] = o, g
        else:
            rs = [r[(p + i) % cap] for i in range(m)]
            d_last = d[last]
        out["r"][t] = NS.fold_rewards(rs, g32)
        out["d"][t] = NS.fold_done(d_last, m, g32)
        out["back"][t], out["m"][t], out["last"][t] = back, m, last
    return out
