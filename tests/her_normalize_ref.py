"""Sample-time normalisation of a HER ring (HERBuffer(normalize="sample"); csrc/her_norm.hip) restated in numpy.  This file is the
DEFINITION of the mode.  It restates nothing new: it composes tests/her_strategy_ref.py — which is her_relabel_ref and her_nstep_ref
for `future` — with the normaliser arithmetic of csrc/norm_math.h, taken from oracle/normalizer_oracle.py (the reference's own
expressions, pinned by tests/golden/normalizer*.npz).

The ring holds RAW [obs (D) | dg (G)] states, raw next states and raw achieved goals.  For a gathered row
    s, a, r, ns, d   are what the ring's relabel / n-step / goal-strategy rule gives ON THE RAW RECORDS (every reward recomputed from
                     raw achieved goals: a distance in the environment's units against its threshold)
and then, for x in (s, ns), with the statistics as they stand when the batch is gathered:
    x[c], c < D       -> float32(clip((x[c] - mean_o[c]) / (sqrt(var_o[c]) + 1e-8), -clip_o, clip_o))      when obs_normalize
    x[c], D <= c < S  -> the same with the goal normaliser's (mean_g, var_g, clip_g)                         when g_normalize
in the type numpy's rules give the expression: float64 for a created normaliser or float64 rows, float32 throughout for a loaded
normaliser (float32 statistics) with float32 rows — `rows64` says which dtype the rows have on the trainer's side, as
DeviceRunningNormalizer.rows_dtype does.  a, r, d and every padding column of the engine's matrices pass through untouched.
"""
import numpy as np

import her_strategy_ref as ST

F32 = np.float32


def apply(nz, x, rows64: bool = False):
    """RunningNormalizer.normalize of float32-valued rows x [n, size] -> float32, as the trainer casts it (src/env.py:189-190).
    nz: a RunningNormalizerOracle (float64 statistics when created, float32 after load_state); None: x unchanged."""
    x = np.asarray(x, F32)
    if nz is None:
        return x.copy()
    rows = x.astype(np.float64) if rows64 else x
    with np.errstate(all="ignore"):
        return np.asarray(nz.normalize(rows)).astype(F32)


def normalize_states(x, D: int, nz_obs=None, nz_dg=None, rows64_obs: bool = False, rows64_dg: bool = False):
    """x [n, S] raw states -> normalised copy: columns [0, D) by nz_obs, [D, S) by nz_dg (None: left raw)"""
    x = np.asarray(x, F32)
    out = x.copy()
    if nz_obs is not None:
        out[:, :D] = apply(nz_obs, x[:, :D], rows64_obs)
    if nz_dg is not None:
        out[:, D:] = apply(nz_dg, x[:, D:], rows64_dg)
    return out


def gather(s, a, ns, r, d, ag, rem, elapsed, head, cap, idx, counter, seed, k, kind, thr, D, nz_obs=None, nz_dg=None,
           rows64_obs=False, rows64_dg=False, **rule):
    """her_strategy_ref.gather on the RAW ring (same arguments; **rule: strategy, n_step, gamma, flush_len), then s and ns
    normalised.  -> its dict, with `raw_s` / `raw_ns` beside the normalised `s` / `ns`."""
    out = ST.gather(s, a, ns, r, d, ag, rem, elapsed, head, cap, idx, counter, seed, k, kind, thr, **rule)
    out["raw_s"], out["raw_ns"] = out["s"], out["ns"]
    out["s"] = normalize_states(out["raw_s"], D, nz_obs, nz_dg, rows64_obs, rows64_dg)
    out["ns"] = normalize_states(out["raw_ns"], D, nz_obs, nz_dg, rows64_obs, rows64_dg)
    return out


def engine_matrices(out, A: int, spa: bool = False):
    """the update engine's view of a gathered batch: sa = [s | a | 0] and nsa = [ns | 0] of row stride roundup(S + A, 4); spa receives
    sa's roundup(S, 4) leading columns (the sample-mode gathers copy whole quads: up to three action components ride along) and
    nothing else: the rest is NaN here."""
    n, S = out["s"].shape
    ldx = (S + A + 3) // 4 * 4
    sa = np.zeros((n, ldx), F32); nsa = np.zeros((n, ldx), F32)
    sa[:, :S], sa[:, S:S + A], nsa[:, :S] = out["s"], out["a"], out["ns"]
    sp = None
    if spa:
        sp = np.full((n, ldx), np.nan, F32)
        S4 = (S + 3) // 4 * 4
        sp[:, :S4] = sa[:, :S4]
    return sa, nsa, sp
