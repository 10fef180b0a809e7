"""Prior-data replay (prior_buffer= / prior_rows=; csrc/her_prior.hip) restated in numpy.  This file is the definition; the reference
project has no counterpart (its agents sample one buffer).

An update call of n batches of B rows with a prior ring and prior_rows = Bd, 1 <= Bd <= B - 1:

  * the main ring gathers n batches of B rows exactly as without a prior ring (same indices, same relabel counter, same draws);
  * the prior ring gathers n batches of Bd rows exactly as its own gather_update(Bd, n) would (its own relabel mode, k_future,
    goal_strategy, n_step and normalisation; the agent's gamma);
  * batch j of the call is rows [0, B - Bd) of the main ring's batch j followed by the prior ring's batch j.

In the engine's matrices (row stride ldx = roundup(S + A, 4), S4 = roundup(S, 4)) a placed row carries
  sa   all ldx columns of the prior gather's row,
  nsa  its S4 leading columns, zeros behind them (nsa = [ns | 0 ..]),
  spa  its S4 leading columns; the columns behind them keep what they held (spa's gather never writes them),
  r, d the prior gather's values.
Rows [0, B - Bd) keep every bit.  The prior ring's counters: relabel_counter += n * Bd (a relabel="sample" ring), draws_done += n.
"""
import numpy as np


def rows_ok(B, Bd):
    return isinstance(Bd, (int, np.integer)) and not isinstance(Bd, bool) and 1 <= int(Bd) <= int(B) - 1


def slot_row(B, Bd, t):
    """scratch row t of a placement launch -> (batch slot relative to the launch's first, row inside the slot)"""
    return t // Bd, (B - Bd) + t % Bd


def mix(main, prior, B, Bd, M, S):
    """main = (sa, nsa, spa or None, r, d) of the main ring's gather_update(B, M), prior = the same of the prior ring's
    gather_update(Bd, M) (spa may be None on either side when the call has none) -> the call's batches, new arrays."""
    assert rows_ok(B, Bd), (B, Bd)
    S4 = (S + 3) // 4 * 4
    sa, nsa, spa, r, d = (None if x is None else np.array(x, copy=True) for x in main)
    psa, pnsa, pspa, pr, pd = prior
    assert sa.shape[0] == M * B and psa.shape[0] == M * Bd and sa.shape[1] == psa.shape[1] and sa.shape[1] % 4 == 0
    for t in range(M * Bd):
        j, row = slot_row(B, Bd, t)
        at = j * B + row
        sa[at] = psa[t]
        nsa[at, :S4] = pnsa[t, :S4]
        nsa[at, S4:] = 0.0
        if spa is not None:
            spa[at, :S4] = pspa[t, :S4]
        r[at] = pr[t]
        d[at] = pd[t]
    return sa, nsa, spa, r, d


def counters_after(relabel_counter, draws_done, n, Bd, sample_mode=True):
    """the prior ring's counters after a call of n batches"""
    return relabel_counter + (n * Bd if sample_mode else 0), draws_done + n
