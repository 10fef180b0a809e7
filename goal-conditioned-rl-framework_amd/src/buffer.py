"""HERBuffer — drop-in for the reference's class of the same name (src/buffer.py:92-179),
backed by the HBM replay ring of libgcrl_hip.so (csrc/her_ring.hip).

Same constructor, `push`, `sample`, `__len__` and externally assigned attributes
(`compute_reward`, `obs_normalizer`, `dg_normalizer`) as the reference, so src/env.py can use
it unchanged.  What differs is where things happen: transitions are staged in HBM, the HER
"future" relabelling + reward recomputation is one kernel at episode flush, and `sample` is a
gather kernel over host-drawn (CPython-exact Mersenne Twister) indices.
"""
from __future__ import annotations

import ctypes as C
import random as _pyrandom

import numpy as np
import torch

from .. import _ffi
from .._ffi import lib

FLUSH_LEN = 50  # literal in the reference (src/buffer.py:117); max_eps_len is not what triggers it


class MTStream:
    """CPython-exact MT19937 living in the library (csrc/mt19937_cpython.cc).

    mode "python": the generator mirrors Python's global `random` state around every use, so
    HER picks, batch draws and the reference's own random.random() calls (src/agent.py:1348)
    interleave exactly as in the reference.  mode "engine": a private stream seeded once —
    bit-identical to the reference as long as nothing else consumes `random` in between,
    without the ~30 us state round trip per call.  mode "device": no MT stream at all — HER future
    indices come from a counter hash evaluated inside the flush kernel (keyed by seed, episode number,
    pick number) and batch indices from a keyed permutation of the ring positions that the gather
    kernels evaluate per row (no host RNG, no index upload);
    NOT the reference's index stream (restated in oracle/her_oracle.py HashRng), for runs that do not
    need index-level parity with a reference run.
    """

    def __init__(self, mode: str = "python", seed: int | None = None):
        if mode not in ("python", "engine", "device"):
            raise ValueError(f"rng mode must be 'python', 'engine' or 'device', got {mode!r}")
        self.mode = mode
        self.seed_value = 0 if seed is None else int(seed)
        self.handle = _ffi.check_ptr(lib.gcrl_mt_create(), "gcrl_mt_create")
        self._buf = (C.c_uint32 * 625)()
        if mode == "engine":
            self.seed(0 if seed is None else seed)

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            lib.gcrl_mt_destroy(h)

    def seed(self, s: int):
        _ffi.check(lib.gcrl_mt_seed(self.handle, int(s)))

    def pull(self):
        """python mode: copy random.getstate() into the library's generator."""
        if self.mode != "python":
            return
        _, words, self._gauss = _pyrandom.getstate()
        self._buf[:] = words
        _ffi.check(lib.gcrl_mt_set_state(self.handle, self._buf))

    def push_back(self):
        """python mode: write the advanced state back to the `random` module."""
        if self.mode != "python":
            return
        _ffi.check(lib.gcrl_mt_get_state(self.handle, self._buf))
        _pyrandom.setstate((3, tuple(self._buf), self._gauss))

    def random(self) -> float:
        if self.mode in ("python", "device"):   # device mode: the ring never touches an MT stream
            return _pyrandom.random()
        return float(lib.gcrl_mt_random(self.handle))


def _classify_reward(fn, goal_dim: int, default_threshold: float):
    """Map the injected compute_reward callable (src/env.py:105) to a built-in reward kind by
    probing it: sparse -(d > thr) with thr found by bisection, or dense -d."""
    if fn is None:
        return 0, float(default_threshold)
    try:
        return _classify_reward_probe(fn, goal_dim, default_threshold)
    except Exception:   # noqa: BLE001  a callable that cannot take the probe vectors is not a goal-distance reward: host path,
        return 2, float(default_threshold)   # where its exception surfaces from the push that calls it, as in the reference


def _classify_reward_probe(fn, goal_dim: int, default_threshold: float):
    zero = np.zeros(goal_dim, dtype=np.float32)

    def at(dist):
        g = np.zeros(goal_dim, dtype=np.float32)
        g[0] = dist
        return float(np.asarray(fn(zero, g, {})))

    def agrees(kind, thr):
        """The candidate built-in kind against the callable on random goal pairs in general position (the axis probes below
        cannot tell a distance reward from, say, an L1 or a shaped one)."""
        gen = np.random.default_rng(20240229)
        for _ in range(24):
            ag = gen.uniform(-0.3, 0.3, goal_dim).astype(np.float32)
            g = (ag + gen.standard_normal(goal_dim) * gen.choice([0.01, 0.05, 0.3])).astype(np.float32)
            d = float(np.linalg.norm(ag.astype(np.float64) - g.astype(np.float64)))
            got = float(np.asarray(fn(ag, g, {})))
            if kind == 0:
                if abs(d - thr) > 1e-5 * max(1.0, thr) and got != (-1.0 if d > thr else 0.0):
                    return False
            elif abs(got + d) > 1e-5 * max(1.0, d):
                return False
        return True

    probes = [0.0, 1e-3, 0.3, 5.0]
    vals = [at(p) for p in probes]
    if all(v in (0.0, -1.0) for v in vals) and vals[0] == 0.0 and vals[-1] == -1.0:
        lo, hi = 0.0, 5.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if at(mid) == 0.0:
                lo = mid
            else:
                hi = mid
        thr = float(np.float32(0.5 * (lo + hi)))
        # snap to the advertised threshold when the probe agrees with it
        if abs(thr - default_threshold) < 1e-6:
            thr = float(default_threshold)
        if agrees(0, thr):
            return 0, thr
    elif all(abs(v + p) <= 1e-6 * max(1.0, p) for v, p in zip(vals, probes)) and agrees(1, 0.0):
        return 1, float(default_threshold)
    # anything else: the reference calls whatever was injected (src/env.py:105, src/buffer.py:166) — so does the ring,
    # through the host-callback reward kind (include/gcrl.h GCRL_REWARD_HOST): picks and goal swap on the device, the
    # relabel rewards of a flush computed by `fn` on the host
    return 2, float(default_threshold)


RELABEL_MODES = {"push": 0, "sample": 1}    # include/gcrl.h GCRL_RELABEL_*
NSTEP_MAX = 8                               # n_step of a relabel="sample" ring: 1..8 (gcrl_her_set_nstep)


def _check_nstep(who: str, n_step, gamma, relabel: str):
    """-> (n_step, gamma) as the ring takes them, or a GcrlError that names n_step"""
    if isinstance(n_step, bool) or not isinstance(n_step, (int, np.integer)) or not 1 <= int(n_step) <= NSTEP_MAX:
        raise _ffi.GcrlError(f"{who}: n_step: must be an integer in 1..{NSTEP_MAX}, got {n_step!r}")
    n_step = int(n_step)
    if n_step > 1 and relabel != "sample":
        raise _ffi.GcrlError(f"{who}: n_step: n_step={n_step} needs relabel='sample' (the window's rewards are recomputed by the relabelling "
                             f"gather), got relabel={relabel!r}")
    if n_step > 1 and gamma is None:
        raise _ffi.GcrlError(f"{who}: n_step: n_step={n_step} needs a discount: pass gamma=")
    return n_step, (None if gamma is None else float(gamma))


GOAL_STRATEGIES = {"future": 0, "final": 1, "episode": 2}    # include/gcrl.h GCRL_GOAL_*


def _check_goal_strategy(who: str, goal_strategy, relabel: str, buffer_type: str = "HER") -> str:
    """-> the strategy as the ring takes it, or a GcrlError that names goal_strategy; before any device work"""
    if not isinstance(goal_strategy, str) or goal_strategy not in GOAL_STRATEGIES:
        raise _ffi.GcrlError(f"{who}: goal_strategy: must be one of {sorted(GOAL_STRATEGIES)}, got {goal_strategy!r}")
    if goal_strategy != "future" and buffer_type != "HER":
        raise _ffi.GcrlError(f"{who}: goal_strategy: {goal_strategy!r} needs buffer_type 'HER' with relabel='sample', got {buffer_type!r}")
    if goal_strategy != "future" and relabel != "sample":
        raise _ffi.GcrlError(f"{who}: goal_strategy: {goal_strategy!r} needs relabel='sample' (the goal is selected by the relabelling gather), "
                             f"got relabel={relabel!r}")
    return goal_strategy


NORMALIZE_MODES = {"push": 0, "sample": 1}    # include/gcrl.h GCRL_NORMALIZE_*


def _check_normalize(who: str, normalize, obs_normalize, g_normalize, buffer_type: str = "HER") -> str:
    """-> the mode as the ring takes it, or a GcrlError that names normalize; before any device work"""
    if not isinstance(normalize, str) or normalize not in NORMALIZE_MODES:
        raise _ffi.GcrlError(f"{who}: normalize: must be one of {sorted(NORMALIZE_MODES)}, got {normalize!r}")
    if normalize == "sample" and buffer_type != "HER":
        raise _ffi.GcrlError(f"{who}: normalize: 'sample' needs buffer_type 'HER' (the REPLAY and PER buffers store what they are given), "
                             f"got {buffer_type!r}")
    if normalize == "sample" and not (obs_normalize or g_normalize):
        raise _ffi.GcrlError(f"{who}: normalize: 'sample' with obs_normalize=False and g_normalize=False leaves nothing to normalise")
    return normalize


def _check_prior(who: str, prior_buffer, prior_rows, batch_size: int, buffer_type: str = "HER", normalize: str = "push"):
    """-> prior_rows as the engine takes it (0 without a prior ring), or a GcrlError that names prior_buffer or prior_rows; before any
    device work.  The ring's dims and length are known only once it holds rows: the update call asks for them (include/gcrl.h)."""
    if prior_buffer is None and prior_rows is None:
        return 0
    if prior_buffer is None:
        raise _ffi.GcrlError(f"{who}: prior_buffer: prior_rows={prior_rows!r} was given without a prior_buffer")
    if prior_rows is None:
        raise _ffi.GcrlError(f"{who}: prior_rows: a prior_buffer was given without prior_rows (1..batch_size - 1)")
    if not isinstance(prior_buffer, HERBuffer):
        raise _ffi.GcrlError(f"{who}: prior_buffer: must be a HERBuffer, got a {type(prior_buffer).__name__}")
    if isinstance(prior_rows, bool) or not isinstance(prior_rows, (int, np.integer)) or not 1 <= int(prior_rows) <= int(batch_size) - 1:
        raise _ffi.GcrlError(f"{who}: prior_rows: must be an integer in 1..batch_size - 1 = {int(batch_size) - 1}, got {prior_rows!r}")
    if buffer_type != "HER":
        raise _ffi.GcrlError(f"{who}: prior_buffer: prior rows are mixed into batches gathered from a HER ring; buffer_type is {buffer_type!r}")
    if prior_buffer.rng.mode != "device":
        raise _ffi.GcrlError(f"{who}: prior_buffer: the prior ring's gather computes its own row indices and needs rng='device', "
                             f"got rng={prior_buffer.rng.mode!r}")
    if getattr(prior_buffer, "prioritise", None) is not None:
        raise _ffi.GcrlError(f"{who}: prior_buffer: the prior ring carries a priority tree (prioritise={prior_buffer.prioritise!r}); it is "
                             "drawn uniformly")
    if getattr(prior_buffer, "normalize", "push") != normalize:
        raise _ffi.GcrlError(f"{who}: prior_buffer: normalize={normalize!r} here but the prior ring has "
                             f"normalize={getattr(prior_buffer, 'normalize', 'push')!r}: raw and normalised rows would share a batch")
    return int(prior_rows)


PRIORITISE_MODES = (None, "energy", "td_error")
# prioritise="td_error": the exponent and the offset of a leaf (|td| + eps)^alpha — the PER buffer's (csrc/per_tree.hip)
TD_DEFAULTS = dict(alpha=0.6, eps=1e-6)
# prioritise="energy": the constants of the episode energy (tests/her_energy_ref.py is the definition).  The defaults are this
# project's choice — m = 1: potential = m g = 9.81, kinetic = m / (2 dt^2) with dt = 0.04, axis 2 = the height of a 3-component goal
# position (-1, no potential term, for goals with fewer components) — not a claim about anybody's published settings.
ENERGY_DEFAULTS = dict(potential=9.81, kinetic=312.5, axis=None, clip=0.5, alpha=1.0, eps=1e-3)


def _check_energy(who: str, prioritise, energy, relabel: str, per_draw: str = "host", buffer_type: str = "HER"):
    """-> the energy settings as a dict (axis None until the goal width is known), or None for prioritise=None; every refusal names
    `prioritise` or the `energy` key at fault and comes before any device work"""
    if prioritise not in PRIORITISE_MODES:
        raise _ffi.GcrlError(f"{who}: prioritise: must be None, 'energy' or 'td_error', got {prioritise!r}")
    if prioritise is None:
        if energy is not None:
            raise _ffi.GcrlError(f"{who}: prioritise: energy= was given without prioritise='energy'")
        return None
    if prioritise == "td_error":     # the TD-error tree has settings of its own (_check_td)
        if energy is not None:
            raise _ffi.GcrlError(f"{who}: prioritise: energy= belongs to prioritise='energy'; 'td_error' takes td=dict(alpha=, eps=)")
        return None
    if per_draw != "host":       # (asked first: per_draw='device' implies a PER buffer, which the next check would name instead)
        raise _ffi.GcrlError(f"{who}: prioritise: 'energy' and per_draw={per_draw!r} are two trees for one ring; a ring takes one")
    if buffer_type != "HER":
        raise _ffi.GcrlError(f"{who}: prioritise: 'energy' needs buffer_type 'HER' with relabel='sample', got {buffer_type!r}")
    if relabel != "sample":
        raise _ffi.GcrlError(f"{who}: prioritise: 'energy' reads an episode's achieved goals from the tails of a relabel='sample' ring, "
                             f"got relabel={relabel!r}")
    cfg = dict(ENERGY_DEFAULTS)
    for k, v in dict(energy or {}).items():
        if k not in cfg:
            raise _ffi.GcrlError(f"{who}: energy: unknown key {k!r} (one of {sorted(cfg)})")
        cfg[k] = v
    for k in ("potential", "kinetic", "clip", "alpha", "eps"):
        v = cfg[k]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(np.float32(v)):
            raise _ffi.GcrlError(f"{who}: energy: {k}: must be a finite number, got {v!r}")
        cfg[k] = float(np.float32(v))
    if cfg["clip"] <= 0:
        raise _ffi.GcrlError(f"{who}: energy: clip: must be > 0, got {cfg['clip']!r}")
    if cfg["eps"] <= 0:
        raise _ffi.GcrlError(f"{who}: energy: eps: must be > 0, got {cfg['eps']!r}")
    if cfg["alpha"] < 0:
        raise _ffi.GcrlError(f"{who}: energy: alpha: must be >= 0, got {cfg['alpha']!r}")
    ax = cfg["axis"]
    if ax is not None and (isinstance(ax, bool) or not isinstance(ax, (int, np.integer))):
        raise _ffi.GcrlError(f"{who}: energy: axis: must be an integer (negative: no potential term) or None, got {ax!r}")
    if ax is not None:
        cfg["axis"] = max(int(ax), -1)     # every negative axis is the one setting "no potential term": held, saved and compared as -1
    return cfg


def _check_td(who: str, prioritise, td, relabel: str, per_draw: str = "host", buffer_type: str = "HER", default_alpha: float | None = None):
    """-> the settings of prioritise="td_error" as a dict(alpha, eps) of float32-exact floats, or None for every other mode; every
    refusal names `prioritise` and comes before any device work (the mode itself is judged by _check_energy)"""
    if prioritise != "td_error":
        if td is not None:
            raise _ffi.GcrlError(f"{who}: prioritise: td= was given without prioritise='td_error'")
        return None
    if per_draw != "host":
        raise _ffi.GcrlError(f"{who}: prioritise: 'td_error' and per_draw={per_draw!r} are two trees for one ring; a ring takes one")
    if buffer_type != "HER":
        raise _ffi.GcrlError(f"{who}: prioritise: 'td_error' needs buffer_type 'HER' with relabel='sample', got {buffer_type!r}")
    if relabel != "sample":
        raise _ffi.GcrlError(f"{who}: prioritise: 'td_error' keeps one leaf per stored transition and needs a relabel='sample' ring, "
                             f"got relabel={relabel!r}")
    cfg = dict(TD_DEFAULTS)
    if default_alpha is not None:
        cfg["alpha"] = default_alpha
    if td is not None and not isinstance(td, dict):
        raise _ffi.GcrlError(f"{who}: prioritise: td must be a dict with at most the keys {sorted(cfg)}, got {td!r}")
    for k, v in dict(td or {}).items():
        if k not in cfg:
            raise _ffi.GcrlError(f"{who}: prioritise: td: unknown key {k!r} (one of {sorted(cfg)})")
        cfg[k] = v
    for k in ("alpha", "eps"):
        v = cfg[k]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(np.float32(v)):
            raise _ffi.GcrlError(f"{who}: prioritise: td: {k}: must be a finite number, got {v!r}")
        cfg[k] = float(np.float32(v))
    if cfg["alpha"] < 0:
        raise _ffi.GcrlError(f"{who}: prioritise: td: alpha: must be >= 0, got {cfg['alpha']!r}")
    if cfg["eps"] <= 0:
        raise _ffi.GcrlError(f"{who}: prioritise: td: eps: must be > 0, got {cfg['eps']!r}")
    return cfg


def _energy_axis(who: str, cfg: dict, G: int) -> int:
    ax = cfg["axis"]
    if ax is None:
        return 2 if G >= 3 else -1
    if int(ax) >= G:
        raise _ffi.GcrlError(f"{who}: energy: axis: {int(ax)} of a goal with {G} components")
    return max(int(ax), -1)


class _RingState:
    """save_state / load_state shared by the three buffers (extension of SURVEY.md §8f-2)."""

    def save_state(self, path: str) -> dict:
        """Ring rows (logical order), staged partial episodes and the MT19937 stream -> `path`; returns the metadata
        load_state needs.  An untouched buffer (no transition pushed yet) saves as empty."""
        meta = dict(dims=self._dims, rng_mode=self.rng.mode, py_random=None, mt=None, bytes=0)
        meta["relabel"] = getattr(self, "relabel", "push")
        meta["prioritise"] = getattr(self, "prioritise", None)
        meta["goal_strategy"] = getattr(self, "goal_strategy", "future")
        meta["normalize"] = getattr(self, "normalize", "push")
        if meta["normalize"] == "sample":
            meta["obs_normalize"], meta["g_normalize"] = bool(self.obs_normalize), bool(self.g_normalize)
        if self.rng.mode == "python":
            st = _pyrandom.getstate()
            meta["py_random"] = [st[0], list(st[1]), st[2]]
        elif self.rng.mode == "engine":
            _ffi.check(lib.gcrl_mt_get_state(self.rng.handle, self.rng._buf))
            meta["mt"] = list(self.rng._buf)
        if self._h is not None:
            n = int(lib.gcrl_her_state_size(self._h))
            blob = np.empty(n, np.uint8)
            _ffi.check(lib.gcrl_her_save_state(self._h, blob.ctypes.data, n))
            blob.tofile(path)
            meta["bytes"] = n
        if hasattr(self, "priorities"):
            meta["priorities"] = [float(p) for p in self.priorities]
        if meta["prioritise"] == "td_error":
            meta["td"] = dict(self.td)
            if self._h is not None:    # the leaves (logical order) and p_max as bit patterns, the draw counter, the head the sums depend on
                meta["prio_leaves"] = self.get_priorities().view(np.uint32).tolist()
                meta["td_pmax"] = int(np.float32(self.p_max).view(np.uint32))
                meta["td_draw_counter"] = self.draw_counter
                meta["prio_head"] = int(lib.gcrl_her_head(self._h))
        elif meta["prioritise"] is not None:
            meta["energy"] = dict(self.energy)
            if self._h is not None:    # the leaves (logical order), the draw counter, and the head the tree's sums depend on
                meta["prio_leaves"] = self.get_priorities().view(np.uint32).tolist()
                meta["prio_counter"] = self.prio_counter
                meta["prio_head"] = int(lib.gcrl_her_head(self._h))
        return meta

    def _check_td_state(self, meta: dict, mode: bool = True):
        """prioritise="td_error" on either side: a state saved under another `prioritise` (`mode`), alpha or eps is refused naming the
        field — asked by an agent's load_state before anything of the agent is overwritten, and (the settings: load_state has compared
        the modes itself) by load_state"""
        mine = getattr(self, "prioritise", None)
        if "td_error" not in (mine, meta.get("prioritise")):
            return
        who = f"{type(self).__name__}.load_state"
        if mode and meta.get("prioritise") != mine:
            raise _ffi.GcrlError(f"{who}: prioritise: the state was saved with prioritise={meta.get('prioritise')!r}, this buffer has "
                                 f"prioritise={mine!r}")
        for k in ("alpha", "eps"):
            saved = (meta.get("td") or {}).get(k)
            if saved != self.td[k]:
                raise _ffi.GcrlError(f"{who}: prioritise: td: {k}: the state was saved with {k}={saved!r}, this buffer has {k}={self.td[k]!r}")

    def load_state(self, path: str, meta: dict):
        if meta.get("relabel", "push") != getattr(self, "relabel", "push"):    # refused before any device work
            raise _ffi.GcrlError(f"{type(self).__name__}.load_state: relabel: the state was saved with relabel={meta.get('relabel', 'push')!r}, "
                                 f"this buffer has relabel={getattr(self, 'relabel', 'push')!r}")
        if meta.get("goal_strategy", "future") != getattr(self, "goal_strategy", "future"):
            raise _ffi.GcrlError(f"{type(self).__name__}.load_state: goal_strategy: the state was saved with "
                                 f"goal_strategy={meta.get('goal_strategy', 'future')!r}, this buffer has "
                                 f"goal_strategy={getattr(self, 'goal_strategy', 'future')!r}")
        mine_n = getattr(self, "normalize", "push")
        if meta.get("normalize", "push") != mine_n:
            raise _ffi.GcrlError(f"{type(self).__name__}.load_state: normalize: the state was saved with normalize={meta.get('normalize', 'push')!r}, "
                                 f"this buffer has normalize={mine_n!r}")
        if mine_n == "sample":
            for flag in ("obs_normalize", "g_normalize"):
                if bool(meta.get(flag)) != bool(getattr(self, flag)):
                    raise _ffi.GcrlError(f"{type(self).__name__}.load_state: normalize: the state was saved with {flag}={bool(meta.get(flag))!r}, "
                                         f"this buffer has {flag}={bool(getattr(self, flag))!r}")
        if meta.get("prioritise") != getattr(self, "prioritise", None):
            raise _ffi.GcrlError(f"{type(self).__name__}.load_state: prioritise: the state was saved with prioritise={meta.get('prioritise')!r}, "
                                 f"this buffer has prioritise={getattr(self, 'prioritise', None)!r}")
        is_td = getattr(self, "prioritise", None) == "td_error"
        self._check_td_state(meta, mode=False)
        mine = dict(self.energy) if getattr(self, "prioritise", None) is not None and not is_td else None
        if mine is not None and mine["axis"] is None and meta.get("dims"):     # (the default axis follows the goal width: known once a ring exists)
            mine["axis"] = _energy_axis(type(self).__name__, mine, int(meta["dims"][2]))
        if meta.get("prioritise") is not None and not is_td and meta.get("energy") != mine:
            raise _ffi.GcrlError(f"{type(self).__name__}.load_state: prioritise: the state was saved with energy={meta.get('energy')!r}, "
                                 f"this buffer has energy={mine!r}")
        if meta["bytes"]:
            self._ensure(*meta["dims"])
            blob = np.fromfile(path, dtype=np.uint8)
            _ffi.check(lib.gcrl_her_load_state(self._h, blob.ctypes.data, blob.size))
        if meta.get("py_random") is not None and self.rng.mode == "python":
            v, words, gauss = meta["py_random"]
            _pyrandom.setstate((v, tuple(words), gauss))
        if meta.get("mt") is not None and self.rng.mode == "engine":
            self.rng._buf[:] = meta["mt"]
            _ffi.check(lib.gcrl_mt_set_state(self.rng.handle, self.rng._buf))
        if hasattr(self, "priorities") and "priorities" in meta:
            self.priorities.clear()
            self.priorities.extend(np.float32(p) for p in meta["priorities"])
        if meta.get("prioritise") is not None and "prio_leaves" in meta and self._h is not None:
            _ffi.check(lib.gcrl_her_set_head(self._h, int(meta["prio_head"])))     # the rows back at their slots, then the leaves
            leaves = np.asarray(meta["prio_leaves"], dtype=np.uint32).view(np.float32)
            _ffi.check(lib.gcrl_per_set_priorities(self._h, leaves.ctypes.data, leaves.size))
            if meta["prioritise"] == "td_error":
                self.p_max = np.asarray([meta["td_pmax"]], dtype=np.uint32).view(np.float32)[0]
                self.draw_counter = int(meta["td_draw_counter"])
            else:
                self.prio_counter = int(meta["prio_counter"])


class HERBuffer(_RingState):
    def __init__(self, max_mem_len: int, max_eps_len: int, nenvs: int, threshold: float = 0.05,
                 k_future: int = 4, *, rng: str = "python", seed: int | None = None,
                 device_index: int = 0, relabel: str = "push", n_step: int = 1, gamma: float | None = None,
                 prioritise: str | None = None, energy: dict | None = None, goal_strategy: str = "future",
                 normalize: str = "push", obs_normalize: bool = True, g_normalize: bool = False, td: dict | None = None):
        # relabel="push" (default): the reference's form, a flush stores every step's k_future relabelled copies and max_mem_len
        # counts copies.  relabel="sample": a flush stores the T original rows once and a row is relabelled when a batch is drawn
        # (the original paper's and SB3's form); max_mem_len then counts REAL transitions — for the same number of episodes
        # resident as in push mode, divide it by about 1 + k_future.
        if relabel not in RELABEL_MODES:
            raise ValueError(f"relabel must be 'push' or 'sample', got {relabel!r}")
        self.relabel = relabel
        # n_step = N in 2..8 (relabel="sample" only): a gathered row becomes a window of up to N rows of its episode — r the
        # discounted sum of the window's rewards (recomputed against the new goal when the row is relabelled), ns the window's last
        # next state, d folded so that r + gamma (1 - d) q' is the n-step target (tests/her_nstep_ref.py is the definition).  `gamma`
        # discounts this buffer's own sample() / gather_update(); an agent's update calls discount by the agent's gamma.  The values
        # are held here until the first push creates the ring.  Every refusal before any device work.
        self.n_step, self.gamma = _check_nstep("HERBuffer", n_step, gamma, relabel)
        # prioritise="energy" (relabel="sample" only): an episode is drawn in proportion to the energy its achieved-goal trajectory
        # gained, a row uniformly inside it (csrc/her_prio.hip; tests/her_energy_ref.py is the definition).  The leaves of a priority
        # tree beside the ring are written once, by the flush; sample() / gather_update() without indices= and the update engine draw
        # their rows from it.  A deliberate sampling bias with no importance correction.  None (default): nothing changes.
        self.energy = _check_energy("HERBuffer", prioritise, energy, relabel)
        # prioritise="td_error" (relabel="sample" only): TD-error prioritised replay, "HER + PER" (csrc/her_td.hip; tests/her_td_ref.py
        # is the definition).  The tree beside the ring has one leaf per stored transition; a drawn row's leaf becomes
        # (|td| + eps)^alpha through update_priorities() or an agent's update calls, and a NEW row enters at p_max, the largest
        # priority seen so far (the PER paper's rule), seeded by the flush on the device.  sample() without indices= draws from the
        # tree and, given beta=, returns the importance-sampling weights.  td=dict(alpha=0.6, eps=1e-6) at most.
        self.td = _check_td("HERBuffer", prioritise, td, relabel)
        self.prioritise = prioritise
        # goal_strategy (relabel="sample" only): which row of its episode a relabelled row takes its goal from — "future" (default:
        # a later row, nothing changes), "final" (the episode's last row) or "episode" (any other live row of the episode, earlier ones
        # included; the ring's records then carry `elapsed` beside `remaining`).  csrc/her_relabel.hip; tests/her_strategy_ref.py is
        # the definition.  Fixed when the ring is created.
        self.goal_strategy = _check_goal_strategy("HERBuffer", goal_strategy, relabel)
        # normalize="sample" (either relabel mode): the ring stores RAW [obs | dg] states, next states and achieved goals, and every
        # batch that leaves it — sample(), gather_update(), an agent's update calls — is normalised on the device with the statistics
        # of `obs_normalizer` (obs_normalize) and `dg_normalizer` (g_normalize) as they stand when the batch is gathered; rewards the
        # gathers recompute compare raw achieved goals (csrc/her_norm.hip; tests/her_normalize_ref.py is the definition).  The two must be
        # DeviceRunningNormalizer objects; they are bound to the ring whenever they are assigned.  Rows handed to push / push_batch /
        # push_episode are stored as given: hand them over raw.  "push" (default): nothing changes.
        self.normalize = _check_normalize("HERBuffer", normalize, obs_normalize, g_normalize)
        self.obs_normalize, self.g_normalize = bool(obs_normalize), bool(g_normalize)
        if not torch.cuda.is_available() or lib.gcrl_device_count() <= 0:
            raise _ffi.GcrlError("HERBuffer needs a HIP device: the replay ring lives in HBM and "
                                 "there is no CPU fallback")
        if int(max_eps_len) < FLUSH_LEN:
            # the reference's staging deque(maxlen=max_eps_len) would silently drop the oldest transitions and never
            # reach the len >= 50 flush (src/buffer.py:102,117); the ring's staging always holds 50: refuse, do not diverge
            raise ValueError(f"max_eps_len={max_eps_len} < {FLUSH_LEN}: the reference flushes at the literal 50 "
                             "(src/buffer.py:117) and would drop staged transitions; not emulated")
        self.max_mem_len = int(max_mem_len)
        self.max_eps_len = int(max_eps_len)
        self.nenvs = int(nenvs)
        self.device = "cuda"
        self.device_index = device_index
        self._h = None
        self._threshold = threshold
        self.k_future = int(k_future)
        self._compute_reward = None
        self._obs_normalizer = None
        self._dg_normalizer = None
        self.rng = MTStream(rng, seed)
        self._dims = None
        self._reward_cfg = None

    # the trainer assigns the normalisers after construction (src/env.py:93-98); a normalize="sample" ring is told at once
    @property
    def obs_normalizer(self):
        return self._obs_normalizer

    @obs_normalizer.setter
    def obs_normalizer(self, nz):
        self._assign_normalizer("_obs_normalizer", "obs_normalizer", self.obs_normalize, nz)

    @property
    def dg_normalizer(self):
        return self._dg_normalizer

    @dg_normalizer.setter
    def dg_normalizer(self, nz):
        self._assign_normalizer("_dg_normalizer", "dg_normalizer", self.g_normalize, nz)

    def _assign_normalizer(self, slot: str, name: str, needed: bool, nz):
        if self.normalize == "sample" and needed and nz is not None:
            from .utils import DeviceRunningNormalizer
            if not isinstance(nz, DeviceRunningNormalizer):    # refused before any device work
                raise _ffi.GcrlError(f"HERBuffer.{name}: normalize: normalize='sample' normalises the gathered batch on the device and needs a "
                                     f"DeviceRunningNormalizer, got a {type(nz).__name__}")
        old = getattr(self, slot)
        setattr(self, slot, nz)
        try:
            self._bind_normalizers()
        except (_ffi.GcrlError, ValueError):
            setattr(self, slot, old)
            self._bind_normalizers()
            raise

    def _bind_normalizers(self):
        """normalize="sample": (re-)bind the device normalisers to the ring (borrowed handles) and say which ones its gathers need."""
        if self.normalize != "sample" or self._h is None:
            return
        S, _, G = self._dims
        on = self._obs_normalizer.handle if (self.obs_normalize and self._obs_normalizer is not None) else None
        gn = self._dg_normalizer.handle if (self.g_normalize and self._dg_normalizer is not None) else None
        _ffi.check(lib.gcrl_her_set_normalize(self._h, on, gn, S - G))
        _ffi.check(lib.gcrl_her_require_normalize(self._h, 1 if self.obs_normalize else 0, 1 if self.g_normalize else 0))

    # the trainer assigns compute_reward after construction (src/env.py:105); classification into a built-in reward
    # kind happens when the ring is created — a later reassignment that changes the kind / threshold is refused
    # rather than silently ignored
    @property
    def compute_reward(self):
        return self._compute_reward

    @compute_reward.setter
    def compute_reward(self, fn):
        self._compute_reward = fn
        self._recheck_reward()

    @property
    def threshold(self):
        return self._threshold

    @threshold.setter
    def threshold(self, v):
        self._threshold = v
        self._recheck_reward()

    def _recheck_reward(self):
        if self._h is None or self._reward_cfg is None:
            return
        now = _classify_reward(self._compute_reward, self._dims[2], self._threshold)
        if now[0] == 2 and self._reward_cfg[0] == 2:
            return      # host-callback ring: the callable in use is whatever is assigned now, as in the reference
        if now != self._reward_cfg:
            raise ValueError(f"compute_reward / threshold changed after the replay ring was created with reward config "
                             f"{self._reward_cfg} (now {now}): create a new buffer")

    # ------------------------------------------------------------------ handle management
    def _ensure(self, S: int, A: int, G: int):
        if self._h is not None:
            if self._dims != (S, A, G):
                raise ValueError(f"transition dims {(S, A, G)} differ from the ring's {self._dims}")
            return
        if self.prioritise == "energy":               # refused before any device work
            self.energy["axis"] = _energy_axis("HERBuffer", self.energy, G)
        kind, thr = _classify_reward(self.compute_reward, G, self.threshold)
        if self.relabel == "sample" and kind == 2:    # refused before any device work
            raise _ffi.GcrlError("HERBuffer: compute_reward: relabel='sample' computes the relabel rewards in the gather kernel and takes the "
                                 "built-in sparse or dense reward only; this callable is neither (use relabel='push')")
        self._reward_cfg = (kind, thr)
        cfg = _ffi.HerConfig(state_dim=S, action_dim=A, goal_dim=G, capacity=self.max_mem_len,
                             nenvs=self.nenvs, k_future=self.k_future, flush_len=FLUSH_LEN,
                             reward_kind=kind, reward_threshold=thr, device=self.device_index,
                             rng_mode=1 if self.rng.mode == "device" else 0, seed=self.rng.seed_value)
        if self.goal_strategy == "future":
            self._h = _ffi.check_ptr(lib.gcrl_her_create_relabel(C.byref(cfg), self.rng.handle, RELABEL_MODES[self.relabel]), "gcrl_her_create")
        else:
            self._h = _ffi.check_ptr(lib.gcrl_her_create_goal(C.byref(cfg), self.rng.handle, RELABEL_MODES[self.relabel],
                                                              GOAL_STRATEGIES[self.goal_strategy]), "gcrl_her_create")
        self._dims = (S, A, G)
        try:
            self._bind_normalizers()
        except (_ffi.GcrlError, ValueError):     # (a normaliser of another size: no ring is left behind in the other mode)
            h, self._h, self._dims = self._h, None, None
            lib.gcrl_her_destroy(h)
            raise
        if self.n_step > 1:
            _ffi.check(lib.gcrl_her_set_nstep(self._h, self.n_step, self.gamma))
        if self.prioritise == "td_error":
            _ffi.check(lib.gcrl_her_td_attach(self._h, self.td["alpha"], self.td["eps"]))
        elif self.prioritise is not None:
            e = self.energy
            ecfg = _ffi.EnergyConfig(potential=e["potential"], kinetic=e["kinetic"], axis=e["axis"], clip=e["clip"], alpha=e["alpha"], eps=e["eps"])
            _ffi.check(lib.gcrl_her_prio_attach(self._h, C.byref(ecfg)))
        if kind == 2:
            self._install_reward_callback()

    def _install_reward_callback(self):
        """GCRL_REWARD_HOST: compute_reward(ag_i, ag_f, {}) per relabelled row, one call per pair in the reference's order
        (src/buffer.py:166), float32 like the stored rewards (src/buffer.py:129).  An exception raised by the callable is
        kept and re-raised by the push that triggered the flush."""
        import weakref
        wself = weakref.ref(self)

        def cb(ag_p, goal_p, n, G, out_p, _user):
            me = wself()
            try:
                ag = np.ctypeslib.as_array(ag_p, shape=(n, G))
                goal = np.ctypeslib.as_array(goal_p, shape=(n, G))
                out = np.ctypeslib.as_array(out_p, shape=(n,))
                fn = me._compute_reward
                for i in range(n):
                    out[i] = np.float32(np.asarray(fn(ag[i].copy(), goal[i].copy(), {})))
                return 0
            except BaseException as e:   # noqa: BLE001  (must not propagate through the C frames)
                if me is not None:
                    me._reward_exc = e
                return 1

        self._reward_exc = None
        self._reward_cb = _ffi.REWARD_FN(cb)          # kept alive as long as the ring
        _ffi.check(lib.gcrl_her_set_reward_callback(self._h, C.cast(self._reward_cb, C.c_void_p), None))

    def _check_rows(self, rows: int) -> int:
        """Status of a push-like native call; a failure caused by the compute_reward callable re-raises ITS exception."""
        exc, self._reward_exc = getattr(self, "_reward_exc", None), None
        if exc is not None:
            raise exc
        return _ffi.check(int(rows))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.gcrl_her_destroy(h)

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return 0 if self._h is None else int(lib.gcrl_her_len(self._h))

    # ------------------------------------------------------------------ reference surface
    @staticmethod
    def _state_arg(x):
        """-> (keepalive, pointer, on_device) for a state given as cuda/cpu tensor or ndarray."""
        if isinstance(x, torch.Tensor):
            t = x.detach()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.float().contiguous()
            return t, t.data_ptr(), 1 if t.is_cuda else 0
        arr = np.ascontiguousarray(x, dtype=np.float32)
        return arr, arr.ctypes.data, 0

    def push(self, idx, state, action, next_state, reward, done, desired_goal, achieved_goal):
        act = np.ascontiguousarray(action, dtype=np.float32).reshape(-1)
        dg = np.ascontiguousarray(desired_goal, dtype=np.float32).reshape(-1)
        ag = np.ascontiguousarray(achieved_goal, dtype=np.float32).reshape(-1)
        ks, ps, ds = self._state_arg(state)
        kn, pn, dn = self._state_arg(next_state)
        S = int(ks.numel() if isinstance(ks, torch.Tensor) else ks.size)
        self._ensure(S, act.size, ag.size)
        flushing = bool(done) or lib.gcrl_her_staged(self._h, int(idx)) + 1 >= FLUSH_LEN
        if flushing:
            self.rng.pull()
        rows = lib.gcrl_her_push(self._h, int(idx), ps, ds, act.ctypes.data, pn, dn,
                                 float(reward), 1 if done else 0, dg.ctypes.data, ag.ctypes.data,
                                 _ffi.stream_handle())
        self._check_rows(rows)
        if flushing:
            self.rng.push_back()

    def push_batch(self, states, actions, next_states, rewards, dones, achieved_goals, env0: int = 0):
        """One vector-env step: the `for i in range(num_envs): push_her(i, ...)` loop of the reference's
        trainer (src/env.py:192-201) as ONE call.  states / next_states: [n, S] cuda tensors (the
        obs_batch / next_obs_batch that _process_step builds); the rest host arrays.  Same rows, same
        order and same RNG draws as n push() calls; envs finishing together are flushed together."""
        s = states.detach().to(device="cuda", dtype=torch.float32).contiguous()
        ns = next_states.detach().to(device="cuda", dtype=torch.float32).contiguous()
        a = np.ascontiguousarray(actions, dtype=np.float32)
        r = np.ascontiguousarray(rewards, dtype=np.float32).reshape(-1)
        d = np.ascontiguousarray(np.asarray(dones).astype(np.uint8)).reshape(-1)
        ag = np.ascontiguousarray(achieved_goals, dtype=np.float32)
        n = s.shape[0]
        assert a.shape[0] == n and ns.shape[0] == n and r.size == n and d.size == n and ag.shape[0] == n
        self._ensure(s.shape[1], a.shape[1], ag.shape[1])
        self.rng.pull()
        rows = lib.gcrl_her_push_batch(self._h, int(env0), n, s.data_ptr(), s.shape[1], a.ctypes.data, ns.data_ptr(),
                                       ns.shape[1], r.ctypes.data, d.ctypes.data, ag.ctypes.data, _ffi.stream_handle())
        self._check_rows(rows)
        self.rng.push_back()
        return int(rows)

    def push_episode(self, idx, states, actions, next_states, rewards, dones, achieved_goals):
        """Whole-episode fast path (one upload + one flush launch); same result as T push calls."""
        s = np.ascontiguousarray(states, dtype=np.float32)
        a = np.ascontiguousarray(actions, dtype=np.float32)
        ns = np.ascontiguousarray(next_states, dtype=np.float32)
        r = np.ascontiguousarray(rewards, dtype=np.float32).reshape(-1)
        d = np.ascontiguousarray(dones, dtype=np.float32).reshape(-1)
        ag = np.ascontiguousarray(achieved_goals, dtype=np.float32)
        T = s.shape[0]
        self._ensure(s.shape[1], a.shape[1], ag.shape[1])
        self.rng.pull()
        rows = lib.gcrl_her_push_episode(self._h, int(idx), T, s.ctypes.data, a.ctypes.data,
                                         ns.ctypes.data, r.ctypes.data, d.ctypes.data,
                                         ag.ctypes.data, None, _ffi.stream_handle())
        self._check_rows(rows)
        self.rng.push_back()
        return int(rows)

    def collect_scripted(self, env, steps: int, noise_std: float = 0.0, seed: int = 0, counter: int | None = None) -> int:
        """`steps` vector steps of a `DeviceGoalEnv("pick", ...)` or `DeviceGoalEnv("glide", ...)` under its scripted controller into this ring as ONE native call: per step
        the controller's launch, the env's step and the process-step launch, plus the flush launches of the envs that finish — no
        host <-> device copy, no synchronisation (include/gcrl.h gcrl_her_collect_scripted).  Demonstrations for a prior-data ring
        without the host.  The normalisers assigned to `obs_normalizer` / `dg_normalizer` are used and updated where the constructor's
        flags are on, as `process_step_dev` takes them (they must be DeviceRunningNormalizer objects); a normalize="sample" ring
        stores the rows raw.  noise_std > 0 perturbs the actions with counter-hash normals keyed by `seed`; `counter` (default: the
        vector steps this buffer has collected so far) is the first step's.  Returns the ring rows appended.  Refusals name their
        field and come before anything is consumed."""
        who = "HERBuffer.collect_scripted"
        from .device_env import SCRIPTED, DeviceGoalEnv
        from .utils import DeviceRunningNormalizer
        if not isinstance(env, DeviceGoalEnv):
            raise ValueError(f"{who}: env: a gcrl_amd.DeviceGoalEnv required")
        if env.kind not in SCRIPTED:
            raise _ffi.GcrlError(f"{who}: kind: the 'pick' and 'glide' kinds alone have a scripted controller, this env is {env.kind!r}")
        if int(steps) < 1:
            raise ValueError(f"{who}: steps: {steps} (>= 1 required)")
        nz = []
        for flag, obj, name in ((self.obs_normalize, self._obs_normalizer, "obs_normalizer"), (self.g_normalize, self._dg_normalizer, "dg_normalizer")):
            if flag and obj is not None and not isinstance(obj, DeviceRunningNormalizer):
                raise _ffi.GcrlError(f"{who}: normalize: the device loop needs a DeviceRunningNormalizer as buffer.{name}, got a {type(obj).__name__}")
            nz.append(obj if flag else None)
        if self.normalize == "sample" and ((self.obs_normalize and nz[0] is None) or (self.g_normalize and nz[1] is None)):
            raise _ffi.GcrlError(f"{who}: normalize: normalize='sample' needs DeviceRunningNormalizer objects assigned to buffer.obs_normalizer / "
                                 "buffer.dg_normalizer for the flags that are on")
        self._ensure(env.obs_dim + env.goal_dim, env.ac_dim, env.goal_dim)
        for obj in nz:
            if obj is not None:
                obj.rows_dtype(np.float32)
        c0 = int(getattr(self, "_scripted_steps", 0)) if counter is None else int(counter)
        self.rng.pull()
        rows = lib.gcrl_her_collect_scripted(self._h, env.handle, nz[0].handle if nz[0] is not None else None, nz[1].handle if nz[1] is not None else None,
                                             int(steps), float(noise_std), int(seed) & (2**64 - 1), c0 & (2**64 - 1), _ffi.stream_handle())
        self.rng.push_back()
        self._check_rows(rows)
        self._scripted_steps = c0 + int(steps)
        return int(rows)

    def sample(self, batch_size: int, num_batches: int = 1, indices=None, return_indices: bool = False, beta: float | None = None):
        assert len(self) >= batch_size, "[ERROR] Not enough in buffer to sample"
        S, A, _ = self._dims
        n = batch_size * num_batches
        dev = torch.device("cuda", self.device_index)
        if beta is not None and (self.prioritise != "td_error" or indices is not None):
            raise _ffi.GcrlError("HERBuffer.sample: prioritise: beta= asks for the importance-sampling weights of a draw from a "
                                 "prioritise='td_error' tree (no indices= given)")
        if self.prioritise == "td_error" and indices is None:
            # num_batches draws of batch_size rows from the tree (with replacement), weights normalised per batch, then the ring's own
            # relabelling gather of those rows; everything in stream order on the device
            idx = torch.empty(n, dtype=torch.int32, device=dev)
            w = torch.empty(n, dtype=torch.float32, device=dev) if beta is not None else None
            for m in range(num_batches):
                o = m * batch_size
                _ffi.check(lib.gcrl_per_draw(self._h, int(batch_size), float(beta or 0.0), idx[o:].data_ptr(),
                                             w[o:].data_ptr() if w is not None else None, _ffi.stream_handle()))
            out = tuple(torch.empty(shape, dtype=torch.float32, device=dev) for shape in ((n, S), (n, A), (n, 1), (n, S), (n, 1)))
            _ffi.check(lib.gcrl_her_sample_dev(self._h, n, idx.data_ptr(), out[0].data_ptr(), S, out[1].data_ptr(), A, out[2].data_ptr(),
                                               out[3].data_ptr(), S, out[4].data_ptr(), _ffi.stream_handle()))
            if return_indices:
                out += (idx.cpu().numpy().view(np.uint32),)
            return out + (w,) if w is not None else out
        states = torch.empty((n, S), dtype=torch.float32, device=dev)
        actions = torch.empty((n, A), dtype=torch.float32, device=dev)
        rewards = torch.empty((n, 1), dtype=torch.float32, device=dev)
        next_states = torch.empty((n, S), dtype=torch.float32, device=dev)
        dones = torch.empty((n, 1), dtype=torch.float32, device=dev)
        idx_in = None
        if indices is not None:
            idx_in = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
            assert idx_in.size == n
        drawn = np.empty(n, dtype=np.uint32) if return_indices else None
        if idx_in is None:
            self.rng.pull()
        _ffi.check(lib.gcrl_her_sample(
            self._h, batch_size, num_batches, idx_in.ctypes.data if idx_in is not None else None,
            states.data_ptr(), S, actions.data_ptr(), A, rewards.data_ptr(), next_states.data_ptr(), S,
            dones.data_ptr(), drawn.ctypes.data if drawn is not None else None, _ffi.stream_handle()))
        if idx_in is None:
            self.rng.push_back()
        out = (states, actions, rewards, next_states, dones)
        return out + (drawn,) if return_indices else out

    def rows(self, first: int = 0, count: int | None = None):
        """Test helper: ring rows in logical (oldest-first) order as numpy arrays."""
        n = len(self) - first if count is None else count
        S, A, _ = self._dims
        s = np.empty((n, S), np.float32); a = np.empty((n, A), np.float32)
        ns = np.empty((n, S), np.float32); r = np.empty(n, np.float32); d = np.empty(n, np.float32)
        _ffi.check(lib.gcrl_her_read_rows(self._h, first, n, s.ctypes.data, a.ctypes.data,
                                          ns.ctypes.data, r.ctypes.data, d.ctypes.data))
        return s, a, ns, r, d

    def gather_update(self, batch_size: int, num_batches: int = 1, indices=None, spa: bool = False, side=None):
        """The update engine's batch gather on its own (tests, tools): -> (sa, nsa, spa or None, r, d) cuda tensors, sa / nsa / spa of
        row stride roundup(S + A, 4) (spa pre-filled with NaN: the launch writes its roundup(S, 4) leading columns only).  `side`: a
        cuda uint8 tensor (a multiple of 16 bytes) the launch also copies — the engine's call-start form; its copy is returned last."""
        assert len(self) >= batch_size, "[ERROR] Not enough in buffer to sample"
        S, A, _ = self._dims
        n, ldx = batch_size * num_batches, (S + A + 3) // 4 * 4
        dev = torch.device("cuda", self.device_index)
        sa = torch.empty((n, ldx), dtype=torch.float32, device=dev)
        nsa = torch.empty((n, ldx), dtype=torch.float32, device=dev)
        sp = torch.full((n, ldx), float("nan"), dtype=torch.float32, device=dev) if spa else None
        r = torch.empty(n, dtype=torch.float32, device=dev)
        d = torch.empty(n, dtype=torch.float32, device=dev)
        idx_in = None
        if indices is not None:
            idx_in = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
            assert idx_in.size == n
        side_out = torch.zeros_like(side) if side is not None else None
        if idx_in is None:
            self.rng.pull()
        _ffi.check(lib.gcrl_her_gather_update(
            self._h, batch_size, num_batches, idx_in.ctypes.data if idx_in is not None else None, sa.data_ptr(), nsa.data_ptr(),
            sp.data_ptr() if spa else None, ldx, r.data_ptr(), d.data_ptr(), side.data_ptr() if side is not None else None,
            side_out.data_ptr() if side is not None else None, side.numel() if side is not None else 0, _ffi.stream_handle()))
        if idx_in is None:
            self.rng.push_back()
        out = (sa, nsa, sp, r, d)
        return out + (side_out,) if side is not None else out

    def gather_update_mixed(self, prior, prior_rows: int, batch_size: int, num_batches: int = 1, spa: bool = False):
        """`gather_update(batch_size, num_batches)` of this ring with rows [batch_size - prior_rows, batch_size) of every batch
        replaced by the `prior` ring's own `gather_update(prior_rows, num_batches)` (include/gcrl.h gcrl_her_gather_update_mixed;
        tests/her_prior_ref.py is the definition): what an agent built with `prior_buffer=` / `prior_rows=` trains on, without the
        agent.  -> (sa, nsa, spa or None, r, d) as `gather_update`.  Both rings' counters advance as by their own gathers."""
        prior_rows = _check_prior("HERBuffer.gather_update_mixed", prior, prior_rows, batch_size, "HER", self.normalize)
        assert len(self) >= batch_size, "[ERROR] Not enough in buffer to sample"
        if prior.handle is None:
            raise _ffi.NotEnoughSamples("[ERROR] Not enough in buffer to sample (prior_buffer holds no rows yet)")
        S, A, _ = self._dims
        n, ldx = batch_size * num_batches, (S + A + 3) // 4 * 4
        dev = torch.device("cuda", self.device_index)
        sa = torch.empty((n, ldx), dtype=torch.float32, device=dev)
        nsa = torch.empty((n, ldx), dtype=torch.float32, device=dev)
        sp = torch.full((n, ldx), float("nan"), dtype=torch.float32, device=dev) if spa else None
        r = torch.empty(n, dtype=torch.float32, device=dev)
        d = torch.empty(n, dtype=torch.float32, device=dev)
        self.rng.pull()
        try:
            _ffi.check(lib.gcrl_her_gather_update_mixed(self._h, prior.handle, batch_size, prior_rows, num_batches, sa.data_ptr(), nsa.data_ptr(),
                                                        sp.data_ptr() if spa else None, ldx, r.data_ptr(), d.data_ptr(), _ffi.stream_handle()))
        finally:
            self.rng.push_back()
        return sa, nsa, sp, r, d

    def tails(self, first: int = 0, count: int | None = None):
        """relabel="sample": the tails of ring rows in logical order — (ag [n, G], remaining [n]) — for tests and state."""
        if self._h is None:
            raise _ffi.GcrlError("HERBuffer.tails: the ring has no rows yet")
        n = len(self) - first if count is None else count
        G = self._dims[2]
        ag = np.empty((n, G), np.float32); rem = np.empty(n, np.float32)
        _ffi.check(lib.gcrl_her_read_tails(self._h, first, n, ag.ctypes.data, rem.ctypes.data))
        return ag, rem

    def elapsed(self, first: int = 0, count: int | None = None):
        """goal_strategy="episode": the `elapsed` word of ring rows in logical order — [n], the rows of its episode before each row."""
        if self.goal_strategy != "episode":
            raise _ffi.GcrlError(f"HERBuffer.elapsed: goal_strategy: only an 'episode' ring stores it, this buffer has {self.goal_strategy!r}")
        if self._h is None:
            raise _ffi.GcrlError("HERBuffer.elapsed: the ring has no rows yet")
        n = len(self) - first if count is None else count
        el = np.empty(n, np.float32)
        _ffi.check(lib.gcrl_her_read_elapsed(self._h, first, n, el.ctypes.data))
        return el

    # ------------------------------------------------------------------ prioritise="energy": test and logging helpers
    def _need_prio(self, what: str):
        if self.prioritise is None:
            raise _ffi.GcrlError(f"HERBuffer.{what}: prioritise: this buffer was built with prioritise=None and has no tree")
        if self._h is None:
            raise _ffi.GcrlError(f"HERBuffer.{what}: the ring is created by the first push")

    def get_priorities(self) -> np.ndarray:
        """The leaves in logical order (0 = oldest row), float32: p_ep / T of each row's episode (synchronises)."""
        self._need_prio("get_priorities")
        out = np.empty(len(self), np.float32)
        if out.size:
            _ffi.check(lib.gcrl_per_get_priorities(self._h, out.ctypes.data, out.size))
        return out

    # ------------------------------------------------------------------ prioritise="td_error"
    def _need_td(self, what: str):
        if self.prioritise != "td_error":
            raise _ffi.GcrlError(f"HERBuffer.{what}: prioritise: needs prioritise='td_error', this buffer has {self.prioritise!r}")
        if self._h is None:
            raise _ffi.GcrlError(f"HERBuffer.{what}: the ring is created by the first push")

    def update_priorities(self, indices, td_abs):
        """Leaves of the logical rows `indices` <- (|td_abs| + eps)^alpha, last occurrence wins, and p_max raised; device tensors, one
        launch in stream order, no host synchronisation."""
        self._need_td("update_priorities")
        dev = torch.device("cuda", self.device_index)
        idx = torch.as_tensor(indices).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
        td = torch.as_tensor(td_abs).to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
        assert idx.numel() == td.numel()
        _ffi.check(lib.gcrl_per_update(self._h, idx.data_ptr(), td.data_ptr(), idx.numel(), _ffi.stream_handle()))

    def set_priorities(self, values):
        """Replace every stored row's leaf (logical order) and rebuild the tree, one launch per level (synchronises)."""
        self._need_td("set_priorities")
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        _ffi.check(lib.gcrl_per_set_priorities(self._h, v.ctypes.data, v.size))

    @property
    def p_max(self) -> float:
        """The device word new rows are seeded with: the largest finite priority an update has written, 1.0 before any (synchronises)."""
        self._need_td("p_max")
        out = np.empty(1, np.float32)
        _ffi.check(lib.gcrl_her_td_get_pmax(self._h, out.ctypes.data))
        return np.float32(out[0])

    @p_max.setter
    def p_max(self, v):
        self._need_td("p_max")
        _ffi.check(lib.gcrl_her_td_set_pmax(self._h, float(np.float32(v))))

    @property
    def draw_counter(self) -> int:
        """Number of the tree's next draw of a batch (the key of its uniform stream beside the buffer's seed)."""
        self._need_td("draw_counter")
        return int(lib.gcrl_per_get_draw_counter(self._h))

    @draw_counter.setter
    def draw_counter(self, v: int):
        self._need_td("draw_counter")
        _ffi.check(lib.gcrl_per_set_draw_counter(self._h, int(v)))

    def tree_levels(self):
        """Every level of the tree as stored, leaves (by physical slot) first."""
        self._need_prio("tree_levels")
        out = []
        for k in range(int(lib.gcrl_per_levels(self._h))):
            a = np.empty(int(lib.gcrl_per_level_size(self._h, k)), np.float32)
            _ffi.check(lib.gcrl_per_read_level(self._h, k, a.ctypes.data, a.size))
            out.append(a)
        return out

    @property
    def prio_counter(self) -> int:
        """Rows drawn from the tree so far: the counter of its draw stream (0 before the ring exists)."""
        return 0 if self._h is None else int(lib.gcrl_her_get_prio_counter(self._h))

    @prio_counter.setter
    def prio_counter(self, v: int):
        self._need_prio("prio_counter")
        _ffi.check(lib.gcrl_her_set_prio_counter(self._h, int(v)))

    @property
    def relabel_counter(self) -> int:
        """relabel="sample": rows gathered from the ring so far, the counter of its relabel stream (0 before the ring exists)."""
        return 0 if self._h is None else int(lib.gcrl_her_get_relabel_counter(self._h))

    @relabel_counter.setter
    def relabel_counter(self, v: int):
        if self._h is None:
            raise _ffi.GcrlError("HERBuffer.relabel_counter: the ring is created by the first push")
        _ffi.check(lib.gcrl_her_set_relabel_counter(self._h, int(v)))

    def compute_termination(self, dg, ag):
        return np.linalg.norm(dg - ag, axis=-1) < self.threshold


class ReplayBuffer(_RingState):
    """Drop-in for the reference's ReplayBuffer (src/buffer.py:8-35): FIFO rows in the HBM ring (same packed record as
    HERBuffer, no staging, no relabelling), `sample` = `random.sample` over the stored rows (CPython-exact index stream)
    + the gather kernel.  `push(state, action, reward, next_state, done)` appends ONE row at once."""

    def __init__(self, max_len: int, *, rng: str = "python", seed: int | None = None, device_index: int = 0):
        if not torch.cuda.is_available() or lib.gcrl_device_count() <= 0:
            raise _ffi.GcrlError(f"{type(self).__name__} needs a HIP device: the replay ring lives in HBM and there is no CPU fallback")
        self.max_len = int(max_len)
        self.device = "cuda"
        self.device_index = device_index
        self.rng = MTStream(rng, seed)
        self._h = None
        self._dims = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.gcrl_her_destroy(h)

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return 0 if self._h is None else int(lib.gcrl_her_len(self._h))

    def _ensure(self, S: int, A: int):
        if self._h is not None:
            if self._dims != (S, A):
                raise ValueError(f"transition dims {(S, A)} differ from the ring's {self._dims}")
            return
        cfg = _ffi.HerConfig(state_dim=S, action_dim=A, goal_dim=1, capacity=self.max_len, nenvs=1, k_future=0,
                             flush_len=FLUSH_LEN, reward_kind=0, reward_threshold=0.0, device=self.device_index,
                             rng_mode=1 if self.rng.mode == "device" else 0, seed=self.rng.seed_value)
        self._h = _ffi.check_ptr(lib.gcrl_her_create(C.byref(cfg), self.rng.handle), "gcrl_her_create")
        self._dims = (S, A)

    def push(self, state, action, reward, next_state, done):
        act = np.ascontiguousarray(action, dtype=np.float32).reshape(-1)
        ks, ps, ds = HERBuffer._state_arg(state)
        kn, pn, dn = HERBuffer._state_arg(next_state)
        S = int(ks.numel() if isinstance(ks, torch.Tensor) else ks.size)
        self._ensure(S, act.size)
        _ffi.check(int(lib.gcrl_her_append(self._h, ps, ds, act.ctypes.data, float(reward), pn, dn, 1 if done else 0,
                                           _ffi.stream_handle())))

    def _gather(self, batch_size: int, indices=None):
        S, A = self._dims
        dev = torch.device("cuda", self.device_index)
        out = (torch.empty((batch_size, S), dtype=torch.float32, device=dev), torch.empty((batch_size, A), dtype=torch.float32, device=dev),
               torch.empty((batch_size, 1), dtype=torch.float32, device=dev), torch.empty((batch_size, S), dtype=torch.float32, device=dev),
               torch.empty((batch_size, 1), dtype=torch.float32, device=dev))
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        if idx is None:
            self.rng.pull()
        _ffi.check(lib.gcrl_her_sample(self._h, batch_size, 1, idx.ctypes.data if idx is not None else None, out[0].data_ptr(), S,
                                       out[1].data_ptr(), A, out[2].data_ptr(), out[3].data_ptr(), S, out[4].data_ptr(), None,
                                       _ffi.stream_handle()))
        if idx is None:
            self.rng.push_back()
        return out

    def sample(self, batch_size: int):
        assert len(self) >= batch_size, "Not enough in buffer to sample"
        return self._gather(batch_size)

    def rows(self, first: int = 0, count: int | None = None):
        n = len(self) - first if count is None else count
        S, A = self._dims
        s = np.empty((n, S), np.float32); a = np.empty((n, A), np.float32)
        ns = np.empty((n, S), np.float32); r = np.empty(n, np.float32); d = np.empty(n, np.float32)
        _ffi.check(lib.gcrl_her_read_rows(self._h, first, n, s.ctypes.data, a.ctypes.data, ns.ctypes.data, r.ctypes.data, d.ctypes.data))
        return s, a, ns, r, d


class TdHistoryOverwritten(RuntimeError):
    """A lazily fetched td_error was read after a later update call reused the device history buffer."""


class PERBuffer(ReplayBuffer):
    """Drop-in for the reference's proportional PERBuffer (src/buffer.py:38-89).  Rows live in the HBM ring.

    draw="host" (default, the parity mode): the priorities and the draw stay on the host in numpy, operation for operation as
    the reference writes them (`np.random.choice(N, B, p=P)` consumes numpy's global stream; float32 priorities / weights),
    with one |td| read-back per step, as in the reference.

    draw="device": priorities, draw, importance-sampling weights and the priority update are device state and HIP kernels on a
    priority tree beside the ring (csrc/per_tree.hip).  NOT the reference's index stream: the draw is defined by the restatement
    tests/per_tree_ref.py (a counter hash keyed by the buffer's seed and a draw counter).  `sample` returns weights and indices
    as CUDA tensors, `update_priorities` takes device tensors, and nothing synchronises with the host."""

    def __init__(self, max_len: int, alpha: float, draw: str = "host", **kw):
        if draw not in ("host", "device"):
            raise ValueError(f"PERBuffer: draw must be 'host' or 'device', got {draw!r}")
        super().__init__(max_len, **kw)
        self.draw_mode = draw
        self.alpha = alpha
        self.epsilon = 1e-6
        if draw == "host":
            from collections import deque
            self.priorities = deque(maxlen=int(max_len))

    # ------------------------------------------------------------------ device mode
    def _ensure(self, S: int, A: int):
        fresh = self._h is None
        super()._ensure(S, A)
        if fresh and self.draw_mode == "device":
            _ffi.check(lib.gcrl_per_attach(self._h, float(self.alpha), float(self.epsilon)))

    def _need_device(self, what: str):
        if self.draw_mode != "device":
            raise _ffi.GcrlError(f"PERBuffer.{what} needs draw='device' (this buffer keeps its priorities on the host)")
        if self._h is None:
            raise _ffi.GcrlError(f"PERBuffer.{what}: nothing has been pushed yet")

    def get_priorities(self) -> np.ndarray:
        """Priorities in logical order (0 = oldest row), float32; device mode reads them back (synchronises)."""
        if self.draw_mode == "host":
            return np.array(self.priorities, dtype=np.float32)
        self._need_device("get_priorities")
        out = np.empty(len(self), np.float32)
        _ffi.check(lib.gcrl_per_get_priorities(self._h, out.ctypes.data, out.size))
        return out

    def set_priorities(self, values):
        """Replace every stored row's priority (logical order); device mode rebuilds the tree, one launch per level."""
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        if self.draw_mode == "host":
            assert v.size == len(self.priorities)
            self.priorities.clear()
            self.priorities.extend(np.float32(p) for p in v)
            return
        self._need_device("set_priorities")
        _ffi.check(lib.gcrl_per_set_priorities(self._h, v.ctypes.data, v.size))

    def tree_levels(self):
        """Test helper (device mode): every level of the priority tree as stored, leaves first."""
        self._need_device("tree_levels")
        out = []
        for k in range(int(lib.gcrl_per_levels(self._h))):
            a = np.empty(int(lib.gcrl_per_level_size(self._h, k)), np.float32)
            _ffi.check(lib.gcrl_per_read_level(self._h, k, a.ctypes.data, a.size))
            out.append(a)
        return out

    @property
    def draw_counter(self) -> int:
        self._need_device("draw_counter")
        return int(lib.gcrl_per_get_draw_counter(self._h))

    @draw_counter.setter
    def draw_counter(self, v: int):
        self._need_device("draw_counter")
        _ffi.check(lib.gcrl_per_set_draw_counter(self._h, int(v)))

    def save_state(self, path: str) -> dict:
        meta = super().save_state(path)
        meta["per_draw"] = self.draw_mode
        if self.draw_mode == "device" and self._h is not None:
            meta["priorities"] = [float(p) for p in self.get_priorities()]
            meta["per_draw_counter"] = self.draw_counter
            meta["per_head"] = int(lib.gcrl_her_head(self._h))    # the tree's sums depend on where the leaves lie
        return meta

    def load_state(self, path: str, meta: dict):
        if meta.get("per_draw", "host") != self.draw_mode:
            raise ValueError(f"PERBuffer.load_state: the state was saved with draw={meta.get('per_draw', 'host')!r}, this buffer has draw={self.draw_mode!r}")
        super().load_state(path, meta)
        if self.draw_mode == "device" and self._h is not None and "priorities" in meta:
            _ffi.check(lib.gcrl_her_set_head(self._h, int(meta.get("per_head", 0))))
            self.set_priorities(np.asarray(meta["priorities"], dtype=np.float32))
            self.draw_counter = int(meta.get("per_draw_counter", 0))

    # ------------------------------------------------------------------ reference surface
    def push(self, state, action, reward, next_state, done):
        super().push(state, action, reward, next_state, done)
        if self.draw_mode == "host":
            self.priorities.append(1.0)      # (device mode: the tree gives a pushed row's slot 1.0 at its next refresh)

    def draw(self, batch_size: int, beta: float):
        """host mode -> (indices, weights float32 [B]) exactly as src/buffer.py:50-65; device mode -> (indices int32 [B],
        weights float32 [B]) as CUDA tensors, drawn by the priority tree in stream order."""
        assert len(self) >= batch_size, "Not enough in buffer to sample"
        if self.draw_mode == "device":
            dev = torch.device("cuda", self.device_index)
            idx = torch.empty(batch_size, dtype=torch.int32, device=dev)
            w = torch.empty(batch_size, dtype=torch.float32, device=dev)
            _ffi.check(lib.gcrl_per_draw(self._h, int(batch_size), float(beta), idx.data_ptr(), w.data_ptr(), _ffi.stream_handle()))
            return idx, w
        N = len(self)
        P = np.array(self.priorities, dtype=np.float32)
        P_sum = P.sum()
        if P_sum > 0:
            P /= P_sum
        else:
            P[:] = 1.0 / N
        indices = np.random.choice(N, batch_size, p=P)
        weights = (N * P[indices]) ** (-beta)
        weights /= weights.max()
        return indices, weights

    def _gather_dev(self, idx: torch.Tensor):
        S, A = self._dims
        n, dev = idx.numel(), idx.device
        out = (torch.empty((n, S), dtype=torch.float32, device=dev), torch.empty((n, A), dtype=torch.float32, device=dev),
               torch.empty((n, 1), dtype=torch.float32, device=dev), torch.empty((n, S), dtype=torch.float32, device=dev),
               torch.empty((n, 1), dtype=torch.float32, device=dev))
        _ffi.check(lib.gcrl_her_sample_dev(self._h, n, idx.data_ptr(), out[0].data_ptr(), S, out[1].data_ptr(), A, out[2].data_ptr(),
                                           out[3].data_ptr(), S, out[4].data_ptr(), _ffi.stream_handle()))
        return out

    def sample(self, batch_size: int, beta: float):
        indices, weights = self.draw(batch_size, beta)
        if self.draw_mode == "device":
            return self._gather_dev(indices) + (weights.unsqueeze(-1), indices)
        batch = self._gather(batch_size, indices)
        w = torch.as_tensor(weights, dtype=torch.float32).unsqueeze(-1).to(batch[0].device)
        return batch + (w, indices)

    def update_priorities(self, indices, priorities):
        if self.draw_mode == "device":
            dev = torch.device("cuda", self.device_index)
            idx = torch.as_tensor(indices).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
            td = torch.as_tensor(priorities).to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
            assert idx.numel() == td.numel()
            _ffi.check(lib.gcrl_per_update(self._h, idx.data_ptr(), td.data_ptr(), idx.numel(), _ffi.stream_handle()))
            return
        priorities = np.asarray(priorities).squeeze(-1)
        for index, priority in zip(indices, priorities):
            self.priorities[index] = (abs(priority) + self.epsilon) ** self.alpha
