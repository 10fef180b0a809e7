"""DDPG / TD3Agent / SACAgent / TQCAgent — drop-ins for the reference's classes of the same
names (src/agent.py), backed by the update engine of libgcrl_hip.so (csrc/agent.hip).

Constructor signature `(obs_dim, ac_dim, config, weights, nenvs, gradient_step)` and the
methods the trainer calls (src/env.py: select_action, push_her, update(step), is_buffer_filled,
update_normalizers, normalize_*, save_weights, reset, set_train/set_eval) are the reference's;
`update` returns the same tuple shapes (DDPG 6/4, TD3 8/6, SAC & TQC 9/6 entries) because the
trainer dispatches on the length (src/env.py:448-506).  The entries are lazily materialised
scalars by default (float(x), np.asarray(x), x.item() all work) so that a run of updates is
enqueued without a host sync per step; `sync_metrics=True` returns plain floats with `td_error`
as a 0-d numpy array, exactly like the reference (src/agent.py:1342).
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import weakref

import numpy as np
import torch

from .. import _ffi
from .._ffi import lib
from .buffer import (HERBuffer, PERBuffer, ReplayBuffer, TdHistoryOverwritten, _check_energy, _check_goal_strategy, _check_normalize,
                     _check_nstep, _check_prior, _check_td)
from .model import Actor, Critic, SACActorModel

KIND = {"DDPG": 0, "TD3": 1, "SAC": 2, "TQC": 3}


class LazyScalar:
    """One entry of an update()'s return tuple, fetched from the device on first use."""
    __slots__ = ("_agent", "_ticket", "_n", "_i", "_as_array", "_val", "__weakref__")

    def __init__(self, agent, ticket, n, i, as_array=False):
        self._agent, self._ticket, self._n, self._i, self._as_array = agent, ticket, n, i, as_array
        self._val = None

    def _value(self) -> float:
        if self._val is None:   # kept: the engine's metric slots are a ring, a trainer may hold this object for long
            self._val = self._agent._metrics(self._ticket, self._n)[self._i]
            self._agent = None
        return self._val

    def __float__(self):
        return float(self._value())

    def item(self):
        return float(self._value())

    def __array__(self, dtype=None, copy=None):
        # td_error is a 0-d float32 array in the reference (src/agent.py:1342), the other entries Python floats
        return np.asarray(self._value(), dtype=dtype or (np.float32 if self._as_array else np.float64))

    def __repr__(self):
        return f"LazyScalar({self._value()!r})"

    def _bin(op):
        def f(self, other):
            return op(float(self), float(other))
        return f

    __add__ = _bin(lambda a, b: a + b)
    __radd__ = _bin(lambda a, b: b + a)
    __sub__ = _bin(lambda a, b: a - b)
    __rsub__ = _bin(lambda a, b: b - a)
    __mul__ = _bin(lambda a, b: a * b)
    __rmul__ = _bin(lambda a, b: b * a)
    __truediv__ = _bin(lambda a, b: a / b)
    __lt__ = _bin(lambda a, b: a < b)
    __gt__ = _bin(lambda a, b: a > b)
    del _bin


class LazyTdError:
    """td_error of a device-drawn prioritised step (per_draw="device"): the reference's [B, 1] float32 array (src/agent.py:1387),
    fetched on first use from the engine's per-call history buffer [n][B].  The buffer belongs to the LAST update call: a read
    after a later call has overwritten it raises TdHistoryOverwritten rather than returning another step's values."""
    __slots__ = ("_agent", "_call", "_row", "_val")

    def __init__(self, agent, call, row):
        self._agent, self._call, self._row, self._val = agent, call, row, None

    def _value(self) -> np.ndarray:
        if self._val is None:
            a = self._agent
            if a is None or self._row < 0 or a._per_call != self._call:
                raise TdHistoryOverwritten("td_error of a per_draw='device' step was read after a later update call overwrote the "
                                           "history buffer: read it before the next update()/update_many()")
            B = a.batch_size
            hist = np.empty(a._per_rows * B, np.float32)
            _ffi.check(lib.gcrl_agent_get(a._h, b"per_td_hist", hist.ctypes.data, hist.size))
            self._val = hist.reshape(-1, B)[self._row].reshape(-1, 1).copy()
            self._agent = None
        return self._val

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self._value(), dtype=dtype or np.float32)

    @property
    def shape(self):
        return self._value().shape

    def __getitem__(self, k):
        return self._value()[k]

    def __repr__(self):
        return f"LazyTdError({self._value()!r})"


class _AlphaView:
    """`agent.alpha.item()` (src/env.py:574,604)."""

    def __init__(self, agent):
        self._agent_ref = weakref.ref(agent)   # (no reference cycle: the agent must die with its last user reference)

    def item(self):
        a = self._agent_ref()
        if a is None:
            raise ReferenceError("the agent of this alpha view is gone")
        if not a._sac:
            raise AttributeError("alpha")
        buf = np.empty(1, np.float32)
        _ffi.check(lib.gcrl_agent_get(a._h, b"alpha", buf.ctypes.data, 1))
        return float(buf[0])


def native_config(kind: int, obs_dim: int, ac_dim: int, config, gradient_step: int, *, num_critics: int = 1, top_drop: int = 0,
                  n_quantiles: int = 1, device_index: int = 0, use_graph=True, pipeline=True, seed=None) -> _ffi.AgentConfig:
    """The engine's gcrl_agent_config of an agent (no device work)."""
    return _ffi.AgentConfig(
        kind=kind, obs_dim=obs_dim, ac_dim=ac_dim, hidden_dim=config.hidden_dim,
        layer_count=config.layer_count, batch_size=config.batch_size,
        num_critics=num_critics, top_drop=top_drop,
        ac_update_freq=config.ac_update_freq, gradient_step=gradient_step, polyak_every=40,
        gamma=config.gamma, tau=config.tau,
        grad_clip=-1.0 if config.grad_clip is None else float(config.grad_clip),
        policy_noise=config.policy_noise, noise_clamp=config.noise_clamp,
        actor_lr=config.actor_lr, actor_lr_min=config.actor_lr_min,
        critic_lr=config.critic_lr, critic_lr_min=config.critic_lr_min,
        alpha_lr=float(getattr(config, "alpha_lr", 0.0003)),
        ac_scheduler_steps=config.ac_scheduler_steps, cr_scheduler_steps=config.cr_scheduler_steps,
        alpha_min_steps=float(getattr(config, "alpha_min_steps", 10000)),
        device=device_index, use_graph=int(use_graph), pipeline_steps=(2 if pipeline is True else int(pipeline)),
        n_quantiles=n_quantiles,
        seed=0 if seed is None else int(seed))


# the fields `set_hyperparameters` (and a population's `explore`) may change on a live agent — the reference's config field names; what a
# population lets its members differ in (src/population.py SHARED lists the fields it does not)
HPARAM_FIELDS = ("actor_lr", "actor_lr_min", "critic_lr", "critic_lr_min", "ac_scheduler_steps", "cr_scheduler_steps", "gamma", "tau", "grad_clip")
HPARAM_FIELDS_SAC = ("alpha_lr", "alpha_min_steps")
_FIXED_FIELDS = ("hidden_dim", "layer_count", "batch_size", "ac_update_freq", "num_critics")


def check_hyperparameters(who: str, sac: bool, hparams: dict):
    """Refusals of `set_hyperparameters` that must come before any device work: unknown or fixed fields, values that are not
    numbers, non-positive learning rates.  Raises GcrlError naming the field.  Everything else about the values is the engine's
    to judge (include/gcrl.h gcrl_agent_set_hparams), which takes gamma, tau and grad_clip as a constructor takes them."""
    import math
    allowed = HPARAM_FIELDS + (HPARAM_FIELDS_SAC if sac else ())

    def refuse(field, why):
        raise _ffi.GcrlError(f"{who}: {field}: {why}")
    if not hparams:
        refuse("hparams", "no field given")
    for k, v in hparams.items():
        if k in _FIXED_FIELDS:
            refuse(k, "fixed when the agent is built (it sets shapes and the launch pattern)")
        if k not in allowed:
            refuse(k, f"not a hyper-parameter of a live {'SAC / TQC' if sac else 'DDPG / TD3'} agent (one of {', '.join(allowed)})")
        if k == "grad_clip" and v is None:      # (no clipping, as in the reference's config)
            continue
        if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v):
            refuse(k, f"{v!r} is not a finite number")
        if k in ("actor_lr", "critic_lr", "alpha_lr") and v <= 0:
            refuse(k, f"{v!r}: a learning rate is > 0")
        if k in ("ac_scheduler_steps", "cr_scheduler_steps") and int(v) != v:
            refuse(k, f"{v!r}: a scheduler length is an integer")


def _check_bc(who: str, kind_name: str, bc_weight, q_filter, prior_buffer, buffer_type: str = "HER", per_draw: str = "host",
              member: bool = False):
    """-> bc_weight as a float, or None when the term is off; or a GcrlError that names bc_weight (q_filter for its own type); before
    any device work."""
    import math
    if not isinstance(q_filter, (bool, np.bool_)):
        raise _ffi.GcrlError(f"{who}: q_filter: must be True or False, got {q_filter!r}")
    if bc_weight is None:
        return None
    if kind_name in ("SAC", "TQC"):
        raise _ffi.GcrlError(f"{who}: bc_weight: the behaviour-cloning term is for the deterministic actors (DDPG / TD3); the "
                             "tanh-Gaussian actors have none yet")
    if member:
        raise _ffi.GcrlError(f"{who}: bc_weight: populations do not step the behaviour-cloning term")
    if isinstance(bc_weight, bool) or not isinstance(bc_weight, (int, float, np.integer, np.floating)) or not math.isfinite(bc_weight) \
            or not bc_weight > 0:
        raise _ffi.GcrlError(f"{who}: bc_weight: must be a finite number > 0 (None: off), got {bc_weight!r}")
    if prior_buffer is None:
        raise _ffi.GcrlError(f"{who}: bc_weight: the term acts on the prior rows of a batch and needs prior_buffer / prior_rows")
    if buffer_type == "PER" or per_draw == "device":
        raise _ffi.GcrlError(f"{who}: bc_weight: the term does not combine with importance-sampling weights (prioritised replay)")
    return float(bc_weight)


class _EngineAgent:
    KIND_NAME = "DDPG"
    TD_INDEX = {6: 2, 4: 1}  # position of td_error in the tuple, by tuple length

    def __init__(self, obs_dim: int, ac_dim: int, config, weights, nenvs: int, gradient_step: int, *,
                 use_graph: bool = True, pipeline: bool = True, sync_metrics: bool = False, rng: str = "python",
                 seed: int | None = None, device_index: int = 0, num_critics: int = 5,
                 top_quantiles_to_drop: int = 2, n_quantiles: int = 1, per_draw: str = "host", relabel: str = "push",
                 n_step: int = 1, prioritise: str | None = None, energy: dict | None = None, goal_strategy: str = "future",
                 normalize: str = "push", obs_normalize: bool = True, g_normalize: bool = False, prior_buffer=None,
                 prior_rows: int | None = None, bc_weight: float | None = None, q_filter: bool = True, td: dict | None = None, _member=None):
        # relabel="sample": the HER ring stores original rows only and relabels when a batch is gathered (buffer.HERBuffer).
        if relabel not in ("push", "sample"):
            raise ValueError(f"relabel must be 'push' or 'sample', got {relabel!r}")
        if relabel == "sample" and config.buffer_type != "HER":
            raise _ffi.GcrlError(f"{type(self).__name__}: relabel: 'sample' needs buffer_type 'HER', got {config.buffer_type!r}")
        self.relabel = relabel
        # n_step=N (2..8, relabel="sample"): the ring's gathers hand the engine n-step windows (buffer.HERBuffer); gamma is the config's.
        if n_step != 1 and config.buffer_type != "HER":
            raise _ffi.GcrlError(f"{type(self).__name__}: n_step: n_step={n_step!r} needs buffer_type 'HER' with relabel='sample', "
                                 f"got {config.buffer_type!r}")
        self.n_step = _check_nstep(type(self).__name__, n_step, config.gamma, relabel)[0]
        # goal_strategy="final" | "episode" (relabel="sample"): which row of its episode a relabelled row takes its goal from
        # (buffer.HERBuffer); "future", the default, changes nothing.
        self.goal_strategy = _check_goal_strategy(type(self).__name__, goal_strategy, relabel, config.buffer_type)
        # normalize="sample": the HER ring stores raw rows and every gathered batch is normalised with the statistics of that moment
        # (buffer.HERBuffer); `obs_normalize` / `g_normalize` are then the flags `observe_act` and `process_step` must be called with.
        self.normalize = _check_normalize(type(self).__name__, normalize, obs_normalize, g_normalize, config.buffer_type)
        self.obs_normalize, self.g_normalize = bool(obs_normalize), bool(g_normalize)
        # prior_buffer=<HERBuffer, rng="device">, prior_rows=Bd (1..batch_size - 1): prior-data replay.  Rows [B - Bd, B) of every batch
        # the engine gathers from the agent's ring are the prior ring's own gather of Bd rows per batch, the other rows exactly those
        # of an agent without the keywords (csrc/her_prior.hip; tests/her_prior_ref.py is the definition).  The agent never pushes into
        # the prior ring: fill it with push_episode / push, at any time between calls.  Every refusal here before any device work.
        self.prior_rows = _check_prior(type(self).__name__, prior_buffer, prior_rows, config.batch_size, config.buffer_type, self.normalize)
        if prior_buffer is not None and self.normalize == "sample" and (
                bool(prior_buffer.obs_normalize), bool(prior_buffer.g_normalize)) != (self.obs_normalize, self.g_normalize):
            raise _ffi.GcrlError(f"{type(self).__name__}: prior_buffer: normalize='sample' normalises the prior ring's rows with this agent's "
                                 f"statistics: its obs_normalize / g_normalize must be {self.obs_normalize!r} / {self.g_normalize!r}")
        self.prior_buffer = prior_buffer
        self._prior_bound = None              # (prior ring handle, rows) the engine holds
        # bc_weight=W (> 0; None: off), q_filter=True: Q-filtered behaviour cloning on the prior rows (DDPG / TD3; csrc/her_bc.hip;
        # tests/her_bc_ref.py is the definition).  The actor loss gains W / prior_rows * sum over the accepted prior rows of
        # |pi(s) - a|^2; with q_filter a row is accepted where the stepped critic rates the stored action above the actor's.  The term
        # runs on the layer-per-launch schedule, so pipeline becomes 0 below.  Every refusal here before any device work.
        self.bc_weight = _check_bc(type(self).__name__, self.KIND_NAME, bc_weight, q_filter, prior_buffer, config.buffer_type,
                                   per_draw, _member is not None)
        self.q_filter = bool(q_filter)
        self._bc_ticket = None                # ticket of the last actor step (bc_metrics)
        if self.bc_weight is not None:
            pipeline = 0
        # per_draw="device": the prioritised draw, weights and priority update on the device (buffer.PERBuffer draw="device").
        # Every refusal before any device work.
        if per_draw not in ("host", "device"):
            raise ValueError(f"per_draw must be 'host' or 'device', got {per_draw!r}")
        if per_draw == "device" and prioritise == "td_error":     # (asked first: the per_draw checks below would name the buffer type instead)
            raise _ffi.GcrlError(f"{type(self).__name__}: prioritise: 'td_error' and per_draw='device' are two trees for one ring; a ring takes one")
        if per_draw == "device":
            who = type(self).__name__
            if config.buffer_type != "PER":
                raise _ffi.GcrlError(f"{who}: per_draw: 'device' needs buffer_type 'PER', got {config.buffer_type!r}")
            if _member is not None:
                raise _ffi.GcrlError(f"{who}: per_draw: populations train from HER rings and do not take per_draw='device'")
            if self.KIND_NAME == "TQC" and int(n_quantiles) > 1:
                raise _ffi.GcrlError(f"{who}: per_draw: the distributional TQC variant (n_quantiles > 1) has no importance-weighted loss; "
                                     "per_draw='device' needs scalar critics")
        self.per_draw = per_draw
        # prioritise="energy" (relabel="sample"): the HER ring draws every batch from its energy tree (buffer.HERBuffer); every agent
        # kind and launch form runs as without it, only the row indices the call's gather reads change.  Refused before any device work.
        _check_energy(type(self).__name__, prioritise, energy, relabel, per_draw, config.buffer_type)
        if prioritise is not None and _member is not None:
            raise _ffi.GcrlError(f"{type(self).__name__}: prioritise: populations do not draw from an energy tree")
        self.prioritise = prioritise
        # prioritise="td_error" (relabel="sample"): TD-error prioritised replay on the HER ring, "HER + PER" (buffer.HERBuffer;
        # csrc/her_td.hip).  Every update step draws its batch from the ring's tree, weighs the critic losses with the importance-sampling
        # weights (beta follows beta_scheduler, as for PER agents) and feeds |td| back into the drawn rows' leaves, all on the device in
        # one native call per update() / update_many(); td_error is lazy.  td=dict(alpha=config.alpha, eps=1e-6) at most.  The weights
        # enter the loss on the layer-per-launch schedule, so pipeline becomes 0.  Every refusal here before any device work.
        self.td = _check_td(type(self).__name__, prioritise, td, relabel, per_draw, config.buffer_type, default_alpha=config.alpha)
        if self.td is not None:
            who = type(self).__name__
            if self.KIND_NAME == "TQC" and int(n_quantiles) > 1:
                raise _ffi.GcrlError(f"{who}: prioritise: the distributional TQC variant (n_quantiles > 1) has no importance-weighted loss; "
                                     "'td_error' needs scalar critics")
            if prior_buffer is not None or bc_weight is not None:
                raise _ffi.GcrlError(f"{who}: prioritise: 'td_error' weighs and re-prioritises every row of a batch; prior_buffer / bc_weight "
                                     "rows have no leaf in the ring's tree")
            pipeline = 0
        if not torch.cuda.is_available() or lib.gcrl_device_count() <= 0:
            raise _ffi.GcrlError(f"{type(self).__name__} needs a HIP device; there is no CPU fallback")
        self.device = "cuda"
        self.device_index = device_index
        self.config = config
        self.gradient_step = int(gradient_step)
        self.obs_dim, self.ac_dim = int(obs_dim), int(ac_dim)
        self.sync_metrics = sync_metrics
        kind = KIND[self.KIND_NAME]
        self._sac = kind >= 2

        # buffer factory of the reference (src/agent.py:1214-1228 and its copies)
        if config.buffer_type == "PER":
            self.buffer = PERBuffer(config.max_len, config.alpha, draw=per_draw, rng=rng, seed=seed, device_index=device_index)
            pipeline = 0      # importance-sampling weights enter the loss in the layer-per-launch schedule
        elif config.buffer_type == "REPLAY":
            self.buffer = ReplayBuffer(config.max_len, rng=rng, seed=seed, device_index=device_index)
        elif config.buffer_type == "HER":
            self.buffer = HERBuffer(config.max_len, config.max_eps_len, nenvs, k_future=config.k_future,
                                    rng=rng, seed=seed, device_index=device_index, relabel=relabel,
                                    n_step=self.n_step, gamma=config.gamma if self.n_step > 1 else None,
                                    prioritise=prioritise, energy=energy, goal_strategy=self.goal_strategy,
                                    normalize=self.normalize, obs_normalize=self.obs_normalize, g_normalize=self.g_normalize, td=self.td)
        else:
            raise ValueError(f"[ERROR] Invalid Buffer type. Received {config.buffer_type}.")

        # the YAML keys num_critics / top_quantiles_to_drop are dropped by pydantic in the
        # reference, so getattr(config, ..., 5/2) always yields the defaults (src/agent.py:789-790)
        self.num_critics = int(getattr(config, "num_critics", num_critics)) if kind == 3 else (1 if kind == 0 else 2)
        self.top_quantiles_to_drop = int(getattr(config, "top_quantiles_to_drop", top_quantiles_to_drop))
        # n_quantiles > 1: the DISTRIBUTIONAL TQC variant of BASELINE.json configs[3] (no reference counterpart: the reference's
        # critics are scalar; include/gcrl.h gcrl_agent_config.n_quantiles, oracle/quantile_tqc_oracle.py)
        self.n_quantiles = int(n_quantiles) if kind == 3 else 1
        if self.n_quantiles > 1 and kind == 3:
            self.num_critics = int(num_critics)

        cfg = native_config(kind, obs_dim, ac_dim, config, self.gradient_step, num_critics=self.num_critics,
                            top_drop=self.top_quantiles_to_drop if kind == 3 else 0, n_quantiles=self.n_quantiles,
                            device_index=device_index, use_graph=use_graph, pipeline=pipeline, seed=seed)
        if _member is None:
            self._owner = None
            self._h = _ffi.check_ptr(lib.gcrl_agent_create(C.byref(cfg)), "gcrl_agent_create")
        else:   # a population member (src/population.py): the population made the handle and owns it
            self._owner, self._h = _member(cfg)
        if self.bc_weight is not None:
            _ffi.check(lib.gcrl_agent_set_bc(self._h, float(self.bc_weight), 1 if self.q_filter else 0, int(self.prior_rows)))
        self._metric_cache: dict[int, list[float]] = {}
        self._live = collections.deque()      # (ticket, n) of returned tuples, oldest first
        self._lazy: dict[int, list] = {}      # ticket -> weak references to its unresolved LazyScalars
        self._per_call = 0                    # per_draw="device": number of the last update call (owner of the td history buffer)
        self._per_rows = min(128, max(1, self.gradient_step))   # steps the history buffer holds (the engine's steps per call)

        self.noise_std = config.noise_std
        self.noise_clamp = config.noise_clamp
        self.policy_noise = config.policy_noise
        self.gamma = config.gamma
        self.batch_size = config.batch_size
        self.ac_update_freq = config.ac_update_freq
        self.grad_clip = config.grad_clip
        self.tau = config.tau
        self.beta = config.beta
        self.beta_start = config.beta
        self.beta_max = 1.0
        self.beta_end = config.beta_end
        self.alpha_min = getattr(config, "alpha_min", 0.05)
        self.alpha_min_steps = getattr(config, "alpha_min_steps", 10000)
        self.alpha = _AlphaView(self)

        # The network views reach the native handle through a weak reference: a closure over `self` made every agent part
        # of a reference cycle, so dropping one left its HBM ring, pinned blocks and streams alive until the cyclic
        # collector happened to run — and a process building agents one after another (sweeps) ran the next one 60 %
        # slower beside the undead (tools/rowchain_vs_batch.py found it).
        wself = weakref.ref(self)

        def get():
            a = wself()
            return a._h if a is not None else None
        H, L = config.hidden_dim, config.layer_count
        if self._sac:
            self.actor = SACActorModel(get, "actor", obs_dim, H, ac_dim, L)
        else:
            self.actor = Actor(get, "actor", obs_dim, H, ac_dim, L)
            self.target_actor = Actor(get, "target_actor", obs_dim, H, ac_dim, L)
        self.critics = [Critic(get, f"critic_{i}", obs_dim + ac_dim, H, self.n_quantiles, L) for i in range(self.num_critics)]
        self.target_critics = [Critic(get, f"target_critic_{i}", obs_dim + ac_dim, H, self.n_quantiles, L)
                               for i in range(self.num_critics)]
        self._bind_names()
        if weights:
            self._load_weights(weights)
        self.update_target_network()

    # reference attribute names (critic / critic_1 / critic_2 ...)
    def _bind_names(self):
        pass

    def _load_weights(self, weights: str):
        raise NotImplementedError

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self, "_owner", None) is None:
            lib.gcrl_agent_destroy(h)

    def set_meetings(self, on: bool = True) -> int:
        """Switch the launch forms whose workgroups wait for each other inside a kernel (csrc/meet.h) on (where the device
        admits them) or off; returns the bit mask of the forms now active.  Off is the safe setting whenever the GPU is
        shared with other processes or streams (`gcrl_set_shared_device` / GCRL_SHARED_GPU=1 do it process-wide)."""
        return _ffi.check(lib.gcrl_agent_set_meetings(self._h, 1 if on else 0))

    def meetings(self) -> int:
        """Bit mask of the launch forms with in-kernel waits that are active on this handle (1 BatchNorm slab row groups, 2 row-chain
        roles, 4 reserved (always 0), 8 the fused dW + optimiser launch of the row-chain DDPG step); changes nothing."""
        return _ffi.check(lib.gcrl_agent_get_meetings(self._h))

    def rowchain_form(self) -> int:
        """Bit mask of the fused DDPG row-chain launches of this handle that read the backward chains' multipliers from LDS
        (csrc/rowchain.h): 1 critic-phase launches, 2 actor-phase launches, 4 the overlapped launch; 0: the global-multiplier form
        everywhere (GCRL_RC_GLOBAL_MUL=1, a shape the LDS rule refuses, or an agent without that launch).  Changes nothing."""
        return _ffi.check(lib.gcrl_agent_rowchain_form(self._h))

    def rowchain_stream(self) -> bool:
        """Whether the fused DDPG row-chain launches of this handle take the stream form of their chained layer passes
        (csrc/rowchain.h WStream); False under GCRL_RC_NO_STREAM=1, at another shape, or for an agent without that launch.
        Same bits either way.  Changes nothing."""
        return bool(_ffi.check(lib.gcrl_agent_rowchain_stream(self._h)))

    def rowchain_warm(self) -> int:
        """Number of L2-warming rider workgroups behind the role workgroups of this handle's overlapped fused DDPG row-chain launch
        (csrc/rowchain.hip rc_warm_rider); 0 under GCRL_RC_NO_WARM=1, for a launch that does not take the stream form or leaves no
        idle CUs, for an agent without that launch, or with a library built before the riders.  Same bits either way.  Changes nothing."""
        if not hasattr(lib, "gcrl_agent_rowchain_warm"):
            return 0
        return _ffi.check(lib.gcrl_agent_rowchain_warm(self._h))

    UPDATE_FORM_FIELDS = ("rows_per_workgroup", "rowchain", "split_roles", "rc_merge", "split_k", "rc_merge_k", "ddpg_ksplit", "opt_fuse",
                          "bn_slab", "bn_rsplit")

    def update_forms(self) -> dict:
        """The launch rules this handle's update step runs under, as the engine settled them at creation (and switched since, where
        a form with in-kernel waits went off): include/gcrl.h gcrl_agent_update_forms.  Read-only: for tests that name the form
        they ran on."""
        out = (C.c_int32 * len(self.UPDATE_FORM_FIELDS))()
        n = _ffi.check(lib.gcrl_agent_update_forms(self._h, out, len(out)))
        assert n == len(out), n
        return dict(zip(self.UPDATE_FORM_FIELDS, (int(x) for x in out)))

    # ------------------------------------------------------------------ prior-data replay
    def _bind_prior(self):
        """Tell the engine which ring the tail rows of the next call's batches come from (gcrl_agent_set_prior); called by every update
        entry before anything is consumed.  The prior ring exists once it holds rows; with normalize="sample" it is given this agent's
        normalisers, so that its rows leave through its own pass with the same statistics."""
        pb = self.prior_buffer
        if pb is None:
            if self._prior_bound is not None:
                _ffi.check(lib.gcrl_agent_set_prior(self._h, None, 0))
                self._prior_bound = None
            return
        if pb.handle is None or len(pb) < self.prior_rows:
            raise _ffi.NotEnoughSamples(f"[ERROR] Not enough in buffer to sample (prior_buffer holds {len(pb)} rows, prior_rows = {self.prior_rows})")
        if self.normalize == "sample":
            for name in ("obs_normalizer", "dg_normalizer"):
                mine = getattr(self.buffer, name, None)
                if mine is not None and getattr(pb, name) is not mine:
                    setattr(pb, name, mine)
        key = (pb.handle, self.prior_rows)
        if self._prior_bound != key:
            _ffi.check(lib.gcrl_agent_set_prior(self._h, pb.handle, self.prior_rows))
            self._prior_bound = key

    def prior_counts(self):
        """(prior_gathers, placements): gathers of the prior ring and placement launches issued since the agent was created — one of
        each per gather part, at most two parts per call (include/gcrl.h gcrl_agent_prior_counts); (0, 0) without a prior ring."""
        g, p = C.c_int64(0), C.c_int64(0)
        _ffi.check(lib.gcrl_agent_prior_counts(self._h, C.byref(g), C.byref(p)))
        return int(g.value), int(p.value)

    def read_batch(self, slot: int):
        """Batch slot `slot` of the last update call as numpy arrays (sa, nsa, r, d) (include/gcrl.h gcrl_agent_read_batch; synchronises;
        for tests and tools).  nsa's columns from the state width on hold what the steps left there."""
        B, ldx = int(self.batch_size), (self.obs_dim + self.ac_dim + 3) // 4 * 4
        sa, nsa = np.empty((B, ldx), np.float32), np.empty((B, ldx), np.float32)
        r, d = np.empty(B, np.float32), np.empty(B, np.float32)
        _ffi.check(lib.gcrl_agent_read_batch(self._h, int(slot), sa.ctypes.data, nsa.ctypes.data, r.ctypes.data, d.ctypes.data))
        return sa, nsa, r, d

    # ------------------------------------------------------------------ update
    def _metrics(self, ticket: int, n: int):
        vals = self._metric_cache.get(ticket)
        if vals is None:
            buf = (C.c_double * n)()
            _ffi.check(lib.gcrl_agent_metrics(self._h, ticket, buf, n))
            vals = list(buf)
            if len(self._metric_cache) > 2048:
                self._metric_cache.clear()
            self._metric_cache[ticket] = vals
        return vals

    def bc_metrics(self):
        """(bc_loss, pass_fraction) of the last actor step: the behaviour-cloning term of its actor loss, bc_weight included, and the
        share of the prior rows its Q-filter accepted (1.0 with q_filter=False).  Fetched on call (waits for that step)."""
        if self.bc_weight is None:
            raise _ffi.GcrlError(f"{type(self).__name__}.bc_metrics: bc_weight: the agent was built without the behaviour-cloning term")
        if self._bc_ticket is None:
            raise _ffi.GcrlError(f"{type(self).__name__}.bc_metrics: bc_weight: no actor step has run yet")
        out = (C.c_double * 2)()
        _ffi.check(lib.gcrl_agent_bc_metrics(self._h, int(self._bc_ticket), out))
        return float(out[0]), float(out[1])

    def _note_bc(self, tickets, lens):
        """remember the ticket of a call's last actor step (the longer tuple) for bc_metrics"""
        full = max(self.TD_INDEX)
        for t, l in zip(tickets, lens):
            if int(l) == full:
                self._bc_ticket = int(t)

    def _tuple(self, ticket: int, n: int):
        td = self.TD_INDEX[n]
        self._live.append((ticket, n))
        # the engine keeps 4096 metric records: resolve what the caller still holds before its slot comes round again
        while self._live and self._live[0][0] <= ticket - 2048:
            t0, n0 = self._live.popleft()
            for ref in self._lazy.pop(t0, ()):
                ls = ref()
                if ls is not None:
                    ls._value()
        if self.sync_metrics:
            vals = self._metrics(ticket, n)
            return tuple(np.asarray(v, dtype=np.float32) if i == td else v for i, v in enumerate(vals))
        out = tuple(LazyScalar(self, ticket, n, i, i == td) for i in range(n))
        self._lazy[ticket] = [weakref.ref(x) for x in out]
        return out

    def beta_scheduler(self, step: int):
        ratio = step / self.beta_end
        self.beta = min(self.beta_max, self.beta_start + ratio * (self.beta_max - self.beta_start))

    @staticmethod
    def _inject(batch=None, noise=None, eps_next=None, eps_cur=None):
        """-> (gcrl_update_inputs or None, tensors to keep alive) for an explicit batch / injected noise."""
        if batch is None and noise is None and eps_next is None and eps_cur is None:
            return None, []
        inputs, keep = _ffi.UpdateInputs(), []

        def dev(t):
            t = torch.as_tensor(t).to(device="cuda", dtype=torch.float32).contiguous()
            keep.append(t)
            return t

        if batch is not None:
            s, a, r, ns, d = (dev(t) for t in batch)
            inputs.s_dev, inputs.ld_s = s.data_ptr(), s.shape[1]
            inputs.a_dev, inputs.ld_a = a.data_ptr(), a.shape[1]
            inputs.r_dev, inputs.d_dev = r.data_ptr(), d.data_ptr()
            inputs.ns_dev, inputs.ld_ns = ns.data_ptr(), ns.shape[1]
        if noise is not None:
            inputs.noise_dev = dev(noise).data_ptr()
        if eps_next is not None:
            inputs.eps_next_dev = dev(eps_next).data_ptr()
        if eps_cur is not None:
            inputs.eps_cur_dev = dev(eps_cur).data_ptr()
        return inputs, keep

    def update(self, step: int, *, batch=None, noise=None, eps_next=None, eps_cur=None):
        """agent.update(step).  Keyword arguments inject an explicit batch / noise (parity tests):
        batch = (states, actions, rewards, next_states, dones) cuda float32 tensors."""
        self.set_train()
        inputs, keep = self._inject(batch, noise, eps_next, eps_cur)
        her = None
        per = isinstance(self.buffer, PERBuffer) and batch is None
        if per and self.buffer.draw_mode == "device":
            return self._update_per_device(step, 1, inputs)[0]
        if self.prioritise == "td_error" and batch is None:     # the HER ring's TD-error tree: the same per-step loop in the engine
            return self._update_per_device(step, 1, inputs)[0]
        if per:   # src/agent.py:1380-1387: the prioritised draw (host, numpy-exact), weights into the critic losses
            indices, weights = self.buffer.draw(self.batch_size, self.beta)
            if inputs is None:
                inputs = _ffi.UpdateInputs()
            idx32 = np.ascontiguousarray(indices, dtype=np.uint32)
            w32 = np.ascontiguousarray(weights, dtype=np.float32)
            keep += [idx32, w32]
            inputs.idx_host, inputs.weights_host = idx32.ctypes.data, w32.ctypes.data
        if batch is None:
            her = self.buffer.handle
            assert her is not None and len(self.buffer) >= self.batch_size, "[ERROR] Not enough in buffer to sample"
            self._bind_prior()
            self.buffer.rng.pull()
        ticket = C.c_int64(-1)
        n = _ffi.check(lib.gcrl_agent_update(self._h, her, int(step), C.byref(inputs) if inputs is not None else None,
                                             C.byref(ticket), _ffi.stream_handle()))
        if batch is None:
            self.buffer.rng.push_back()
        if per:   # update_priorities(indices, td_error) with the per-sample |td| (src/agent.py:1387); td_error stays an array
            td = np.empty(self.batch_size, np.float32)
            _ffi.check(lib.gcrl_agent_get(self._h, b"td_abs", td.ctypes.data, td.size))
            td = td.reshape(-1, 1)
            self.buffer.update_priorities(indices=indices, priorities=td)
        self.beta_scheduler(step)
        if self._sac:
            self.actor.num_batches_tracked += 1 + (1 if n == 9 else 0)
        if self.bc_weight is not None:
            self._note_bc((ticket.value,), (n,))
        out = self._tuple(ticket.value, n)
        if per:
            i = self.TD_INDEX[n]
            out = out[:i] + (td,) + out[i + 1:]
        return out

    def _update_per_device(self, step0: int, n: int, inputs):
        """per_draw="device": n steps as ONE native call; per step the engine refreshes the pushed rows' priorities, draws, weighs,
        gathers, steps and updates the priorities on the device (csrc/agent.hip run_per_device).  No read-back: td_error is lazy.
        Step i uses the beta the schedule left after step i - 1, as update() does."""
        her = self.buffer.handle
        assert her is not None and len(self.buffer) >= self.batch_size, "[ERROR] Not enough in buffer to sample"
        betas = np.empty(n, np.float32)
        beta0 = self.beta
        for i in range(n):
            betas[i] = self.beta
            self.beta_scheduler(step0 + i)
        tickets = (C.c_int64 * n)()
        lens = (C.c_int32 * n)()
        try:
            _ffi.check(lib.gcrl_per_set_betas(her, betas.ctypes.data, n))
            if n == 1:
                t1 = C.c_int64(-1)
                lens[0] = _ffi.check(lib.gcrl_agent_update(self._h, her, int(step0), C.byref(inputs) if inputs is not None else None,
                                                           C.byref(t1), _ffi.stream_handle()))
                tickets[0] = t1.value
            else:
                _ffi.check(lib.gcrl_agent_update_n(self._h, her, int(step0), int(n), tickets, lens, _ffi.stream_handle()))
        except (_ffi.GcrlError, ValueError):
            if self.prioritise == "td_error":
                self.beta = beta0   # a refused call consumed nothing: the schedule neither
            raise
        self._per_call += 1
        if self._sac:
            self.actor.num_batches_tracked += sum(1 + (1 if l == 9 else 0) for l in lens)
        # the history buffer holds the last chunk of the call (the engine runs at most _per_rows steps per chunk)
        last0 = ((n - 1) // self._per_rows) * self._per_rows
        outs = []
        for i, (t, l) in enumerate(zip(tickets, lens)):
            out = self._tuple(int(t), int(l))
            k = self.TD_INDEX[int(l)]
            outs.append(out[:k] + (LazyTdError(self, self._per_call, i - last0),) + out[k + 1:])
        return outs

    def drawn_indices(self, n: int = 1) -> np.ndarray:
        """per_draw="device": the logical row indices the last update call drew, [n, B] (reads back; for tests and logging)."""
        B = self.batch_size
        raw = np.empty(self._per_rows * B, np.float32)
        _ffi.check(lib.gcrl_agent_get(self._h, b"per_idx_hist", raw.ctypes.data, raw.size))
        return raw.view(np.uint32).reshape(-1, B)[:n].copy()

    def update_many(self, step0: int, n: int):
        """The trainer's `for _ in range(gradient_step): update(step)` loop (src/env.py:384-385) as
        one call: all n batches are drawn (same RNG stream order) and gathered by one launch."""
        if (isinstance(self.buffer, PERBuffer) and self.buffer.draw_mode == "device") or self.prioritise == "td_error":
            self.set_train()
            return self._update_per_device(step0, n, None)
        if isinstance(self.buffer, PERBuffer):   # the priorities change after every step: one draw per step (src/agent.py:1380-1387)
            return [self.update(step0 + i) for i in range(n)]
        self.set_train()
        her = self.buffer.handle
        assert her is not None and len(self.buffer) >= self.batch_size, "[ERROR] Not enough in buffer to sample"
        tickets = (C.c_int64 * n)()
        lens = (C.c_int32 * n)()
        self._bind_prior()
        self.buffer.rng.pull()
        try:
            _ffi.check(lib.gcrl_agent_update_n(self._h, her, int(step0), int(n), tickets, lens, _ffi.stream_handle()))
        finally:
            self.buffer.rng.push_back()
        self.beta_scheduler(step0 + n - 1)
        if self._sac:
            self.actor.num_batches_tracked += sum(1 + (1 if l == 9 else 0) for l in lens)
        if self.bc_weight is not None:
            self._note_bc(tickets, lens)
        return [self._tuple(int(t), int(l)) for t, l in zip(tickets, lens)]

    # ------------------------------------------------------------------ acting
    def _actor_forward(self, obs, eps=None) -> torch.Tensor:
        if eps is None and not self._sac and not (isinstance(obs, torch.Tensor) and obs.is_cuda):
            # host rows in, host actions out, one native call (staging, both copies and the sync inside)
            x = np.ascontiguousarray(np.asarray(obs, dtype=np.float32))
            if x.ndim == 1:
                x = x[None, :]
            if x.shape[0] <= int(self.config.batch_size):
                out = np.empty((x.shape[0], self.ac_dim), dtype=np.float32)
                _ffi.check(lib.gcrl_agent_act_host(self._h, x.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data,
                                                   self.ac_dim, _ffi.stream_handle()))
                return torch.from_numpy(out)
        obs_t = torch.as_tensor(np.asarray(obs), dtype=torch.float32).to("cuda").contiguous()
        if obs_t.dim() == 1:
            obs_t = obs_t.unsqueeze(0)
        out = torch.empty((obs_t.shape[0], self.ac_dim), dtype=torch.float32, device="cuda")
        _ffi.check(lib.gcrl_agent_act(self._h, obs_t.data_ptr(), obs_t.shape[0], obs_t.shape[1], out.data_ptr(),
                                      self.ac_dim, eps.data_ptr() if eps is not None else None,
                                      _ffi.stream_handle()))
        return out

    # ------------------------------------------------------------------ fused acting side
    def _device_normalizers(self, obs_normalize: bool, g_normalize: bool):
        """(obs handle, goal handle) when the normalisers this step needs live on the device, else None."""
        from .utils import DeviceRunningNormalizer
        on, gn = getattr(self.buffer, "obs_normalizer", None), getattr(self.buffer, "dg_normalizer", None)
        if obs_normalize and not isinstance(on, DeviceRunningNormalizer):
            return None
        if g_normalize and not isinstance(gn, DeviceRunningNormalizer):
            return None
        return (on.handle if obs_normalize else None, gn.handle if g_normalize else None)

    def _check_normalize_call(self, what: str, obs_normalize: bool, g_normalize: bool, need_device: bool = False):
        """normalize="sample": the ring's gathers normalise with the constructor's flags, so a step that acts or pushes with other
        flags is refused by the flag's name; `need_device`: and so is a step whose normalisers are not on the device."""
        if getattr(self, "normalize", "push") != "sample":
            return
        who = f"{type(self).__name__}.{what}"
        if bool(obs_normalize) != self.obs_normalize:
            raise _ffi.GcrlError(f"{who}: obs_normalize: {bool(obs_normalize)!r} differs from the constructor's {self.obs_normalize!r} "
                                 "(normalize='sample' normalises every gathered batch with the constructor's flags)")
        if bool(g_normalize) != self.g_normalize:
            raise _ffi.GcrlError(f"{who}: g_normalize: {bool(g_normalize)!r} differs from the constructor's {self.g_normalize!r} "
                                 "(normalize='sample' normalises every gathered batch with the constructor's flags)")
        if need_device and self._device_normalizers(obs_normalize, g_normalize) is None:
            raise _ffi.GcrlError(f"{who}: normalize: normalize='sample' stores raw rows through the fused device entry and needs "
                                 "DeviceRunningNormalizer objects assigned to buffer.obs_normalizer / buffer.dg_normalizer")

    def _rows_dtypes(self, obs_dtype, goal_dtype, obs_normalize: bool, g_normalize: bool):
        """numpy's type rules decide the reference normaliser's arithmetic: tell the device normalisers which dtype the rows
        have on the caller's side (the trainer's observation batches are float64 arrays, its goal batches float32)."""
        if obs_normalize:
            self.buffer.obs_normalizer.rows_dtype(obs_dtype)
        if g_normalize:
            self.buffer.dg_normalizer.rows_dtype(goal_dtype)

    _ACT_MODE_EXPLORE, _ACT_MODE_EVAL = 1, 0      # DDPG; TD3 overrides eval (raw network output)

    def _staging(self, tag: str, key: tuple, shapes):
        """Persistent host staging arrays of the fused acting entries (fixed addresses: their ctypes pointers are built once — a
        fresh numpy array per argument and per call cost more host time than the native call itself, tools/acting_breakdown.py).
        `shapes()` -> {name: (shape, dtype)} is only called when `key` (the dims) changed."""
        cache = self.__dict__.setdefault("_stage_cache", {})
        st = cache.get(tag)
        if st is None or st[0] != key:
            arrs = {k: np.empty(shp, dt) for k, (shp, dt) in shapes().items()}
            st = cache[tag] = (key, arrs, {k: C.c_void_p(v.ctypes.data) for k, v in arrs.items()})
        return st[1], st[2]

    def observe_act(self, observation, desired_goal, eval_action: bool = False, obs_normalize: bool = True,
                    g_normalize: bool = False):
        """`select_action(normalize_state_batch(obs, dg, ...))` for one vector-env step (src/env.py:348-355) as ONE native
        call: raw rows up, normalisation + actor + exploration noise on the device, float64 actions back.  The host
        generators are consumed exactly as in the reference (`random.random()` for DDPG's epsilon branch, `np.random`
        for the Gaussian noise, torch's for SAC / TQC eps).  Falls back to the two separate calls when the normalisers
        are host objects."""
        self._check_normalize_call("observe_act", obs_normalize, g_normalize)
        nz = self._device_normalizers(obs_normalize, g_normalize)
        obs_in = observation if isinstance(observation, np.ndarray) else np.asarray(observation)
        dg_in = desired_goal if isinstance(desired_goal, np.ndarray) else np.asarray(desired_goal)
        n = obs_in.shape[0]
        if nz is None or n > int(self.config.batch_size) or obs_in.ndim != 2 or dg_in.ndim != 2:
            obs, dg = np.ascontiguousarray(obs_in, np.float32), np.ascontiguousarray(dg_in, np.float32)
            return self.select_action(self.normalize_state_batch(obs, dg, obs_normalize, g_normalize), eval_action)
        self.set_eval()
        self._rows_dtypes(obs_in.dtype, dg_in.dtype, obs_normalize, g_normalize)
        noise, mode = self._act_noise(n, eval_action)
        if mode is None:
            return noise                              # DDPG's epsilon-random action: no network involved
        D, G, A = obs_in.shape[1], dg_in.shape[1], self.ac_dim
        buf, ptr = self._staging("act", (n, D, G, A), lambda: dict(obs=((n, D), np.float32), dg=((n, G), np.float32),
                                                                    noise=((n, A), np.float64), out=((n, A), np.float64)))
        np.copyto(buf["obs"], obs_in, casting="unsafe")
        np.copyto(buf["dg"], dg_in, casting="unsafe")
        if noise is not None:
            np.copyto(buf["noise"], noise)
        _ffi.check(lib.gcrl_agent_observe_act(self._h, nz[0], nz[1], ptr["obs"], D, ptr["dg"], G, n,
                                              ptr["noise"] if noise is not None else None, mode, ptr["out"], _ffi.stream_handle()))
        return buf["out"].copy()

    def acting_counts(self) -> dict:
        """What `observe_act`'s native entry has issued since this agent was created: calls, kernel launches, host <-> device copies
        and stream synchronisations (include/gcrl.h gcrl_agent_acting_counts).  The one-launch forms add one launch and nothing else
        per call; calls that never reach the entry (host normalisers, DDPG's epsilon-random action) are not counted."""
        v = [C.c_int64(0) for _ in range(4)]
        _ffi.check(lib.gcrl_agent_acting_counts(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("calls", "launches", "copies", "syncs"), (int(x.value) for x in v)))

    def _act_noise(self, n, eval_action):
        """-> (noise or None, mode); DDPG overrides for the epsilon branch."""
        if eval_action:
            return None, self._ACT_MODE_EVAL
        return np.ascontiguousarray(np.random.normal(0, self.noise_std, size=(n, self.ac_dim))), self._ACT_MODE_EXPLORE

    def process_step(self, state, actions, next_obs_raw, rewards, dones, obs_normalize: bool = True, g_normalize: bool = False,
                     env0: int = 0):
        """The reference trainer's `_process_step` (src/env.py:163-201) for one vector-env step as ONE native call:
        normaliser update with [obs ; next_obs], both normalised state matrices built on the device from the updated
        statistics, all envs pushed (episode flush + HER relabel on the device when an env finishes).  `state` /
        `next_obs_raw`: the env's dict observations; `dones` = `terminated` (src/env.py:372).  With `g_normalize` the goal
        normaliser is updated from [dg ; next_dg ; ag ; next_ag] and goals are normalised on the device too (src/env.py:167-175,
        :222-223).  Falls back to the separate calls when a normaliser this step needs is a host object (or, with
        g_normalize, when compute_reward runs through the host callback).  `env0`: the ring's episode slot of this call's first
        env (agents that share one ring each push into their own slots)."""
        self._check_normalize_call("process_step", obs_normalize, g_normalize, need_device=True)
        nz = self._device_normalizers(obs_normalize, g_normalize)
        buf = self.buffer
        if nz is not None and g_normalize:   # (the ring — and with it the reward kind — exists from here on)
            buf._ensure(np.shape(state["observation"])[1] + np.shape(state["desired_goal"])[1], np.shape(actions)[1],
                        np.shape(next_obs_raw["achieved_goal"])[1])
        if nz is None or (g_normalize and buf._reward_cfg[0] == 2):
            if self.normalize == "sample":
                raise _ffi.GcrlError(f"{type(self).__name__}.process_step: normalize: normalize='sample' with g_normalize and a host-callback "
                                     "compute_reward has no fused entry to store raw rows through")
            self.update_normalizers([state["observation"], next_obs_raw["observation"]],
                                    [state["desired_goal"], next_obs_raw["desired_goal"], state["achieved_goal"],
                                     next_obs_raw["achieved_goal"]], obs_normalize, g_normalize)
            s = torch.from_numpy(self.normalize_state_batch(state["observation"], state["desired_goal"], obs_normalize, g_normalize)).float().cuda()
            ns = torch.from_numpy(self.normalize_state_batch(next_obs_raw["observation"], next_obs_raw["desired_goal"], obs_normalize, g_normalize)).float().cuda()
            return buf.push_batch(s, actions, ns, rewards, dones, self.normalize_goal(next_obs_raw["achieved_goal"], g_normalize), env0=int(env0))
        as_arr = lambda x: x if isinstance(x, np.ndarray) else np.asarray(x)
        obs_i, nobs_i = as_arr(state["observation"]), as_arr(next_obs_raw["observation"])
        dg_i, ndg_i, nag_i = as_arr(state["desired_goal"]), as_arr(next_obs_raw["desired_goal"]), as_arr(next_obs_raw["achieved_goal"])
        ag_i = as_arr(state["achieved_goal"]) if g_normalize else None
        act_i = as_arr(actions)
        # np.concatenate's result type, as the reference's update_normalizers forms it (src/agent.py:343-350)
        odt = obs_i.dtype if obs_i.dtype == nobs_i.dtype else np.result_type(obs_i.dtype, nobs_i.dtype)
        gdt = dg_i.dtype
        if g_normalize and not (dg_i.dtype == ndg_i.dtype == ag_i.dtype == nag_i.dtype):
            gdt = np.result_type(dg_i.dtype, ndg_i.dtype, ag_i.dtype, nag_i.dtype)
        self._rows_dtypes(odt, gdt, obs_normalize, g_normalize)
        n, D, G, A = obs_i.shape[0], obs_i.shape[1], dg_i.shape[1], act_i.shape[1]
        buf._ensure(D + G, A, nag_i.shape[1])
        f32 = np.float32
        b, p = self._staging("proc", (n, D, G, A), lambda: dict(obs=((n, D), f32), nobs=((n, D), f32), dg=((n, G), f32), ndg=((n, G), f32),
                                                                ag=((n, G), f32), nag=((n, G), f32), act=((n, A), f32), rew=((n,), f32),
                                                                dn=((n,), np.uint8)))
        cp = np.copyto
        cp(b["obs"], obs_i, casting="unsafe"); cp(b["nobs"], nobs_i, casting="unsafe"); cp(b["dg"], dg_i, casting="unsafe")
        cp(b["ndg"], ndg_i, casting="unsafe"); cp(b["nag"], nag_i, casting="unsafe"); cp(b["act"], act_i, casting="unsafe")
        cp(b["rew"], rewards if (isinstance(rewards, np.ndarray) and rewards.ndim == 1) else np.reshape(rewards, -1), casting="unsafe")
        cp(b["dn"], dones if (isinstance(dones, np.ndarray) and dones.ndim == 1) else np.reshape(dones, -1), casting="unsafe")
        if g_normalize:
            np.copyto(b["ag"], ag_i, casting="unsafe")
        buf.rng.pull()
        rows = lib.gcrl_her_process_step_g(buf.handle, nz[0], 1 if obs_normalize else 0, nz[1], 1 if g_normalize else 0, p["obs"],
                                           p["nobs"], D, p["dg"], p["ndg"], p["ag"] if g_normalize else None, p["nag"], p["act"], p["rew"],
                                           p["dn"], int(env0), n, _ffi.stream_handle())
        buf._check_rows(rows)
        buf.rng.push_back()
        return int(rows)

    # ------------------------------------------------------------------ device rows: acting, process_step and the collect loop
    COLLECT_EPSILON = 0.0      # DDPG: 0.2, the reference's epsilon-random branch (src/agent.py:1348)

    def _dev_normalizers(self, who: str, obs_normalize: bool, g_normalize: bool):
        nz = self._device_normalizers(obs_normalize, g_normalize)
        if nz is None:
            raise _ffi.GcrlError(f"{type(self).__name__}.{who}: normalize: the device-row entries need DeviceRunningNormalizer objects assigned "
                                 "to buffer.obs_normalizer / buffer.dg_normalizer for the flags that are on")
        return nz

    @staticmethod
    def _dev_f32(who: str, name: str, t, shape=None):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) or (shape is not None and tuple(t.shape) != shape):
            raise ValueError(f"{who}: {name}: a contiguous CUDA float32 tensor{'' if shape is None else ' ' + str(list(shape))} required")
        return t

    def _collect_stream(self):
        """(seed, noise_std, epsilon, counter) of the device exploration stream; the seed defaults to the constructor's."""
        if not self.__dict__.get("_collect_bound"):
            _ffi.check(lib.gcrl_agent_collect_set(self._h, int(self._collect_seed()) & (2**64 - 1), float(self.noise_std) if not self._sac else 1.0,
                                                  float(self.COLLECT_EPSILON), 0))
            self._collect_bound = True
        sd, ns, ep, ctr = C.c_uint64(), C.c_double(), C.c_double(), C.c_uint64()
        _ffi.check(lib.gcrl_agent_collect_get(self._h, C.byref(sd), C.byref(ns), C.byref(ep), C.byref(ctr)))
        return int(sd.value), float(ns.value), float(ep.value), int(ctr.value)

    def _collect_seed(self) -> int:
        return int(getattr(self.buffer.rng, "seed_value", 0) or 0)

    def set_collect_stream(self, seed: int | None = None, counter: int | None = None):
        """Re-key the device exploration stream (`collect`, and `observe_act_dev` without `noise`) or move its vector-step counter."""
        sd, ns, ep, ctr = self._collect_stream()
        _ffi.check(lib.gcrl_agent_collect_set(self._h, (sd if seed is None else int(seed)) & (2**64 - 1), ns, ep, ctr if counter is None else int(counter)))

    def observe_act_dev(self, observation, desired_goal=None, eval_action: bool = False, noise=None, obs_normalize: bool = True, g_normalize: bool = False,
                        obs_dim: int | None = None):
        """`observe_act` for a simulator whose state lives on the GPU: raw rows in, float32 actions out, both CUDA tensors, no copy and no
        synchronisation.  `observation` [n, obs_dim] and `desired_goal` [n, goal_dim] CUDA float32 tensors — or, with `desired_goal=None`,
        `observation` is the packed [n, obs_dim + goal_dim] rows (`DeviceGoalEnv.acting_rows()["rows"]`), read in place.  `noise`: CUDA
        float64 [n, A] (the Gaussian noise of DDPG / TD3, the eps of SAC / TQC); None with `eval_action=False` draws vector step c of the
        device exploration stream (and advances c).  The result is the float32 rounding of `observe_act`'s float64 action for the same
        rows and noise, bit for bit.  DDPG's epsilon-random branch is `collect`'s; this entry always runs the actor."""
        who = f"{type(self).__name__}.observe_act_dev"
        self._check_normalize_call("observe_act_dev", obs_normalize, g_normalize)
        nz = self._dev_normalizers("observe_act_dev", obs_normalize, g_normalize)
        S = self.obs_dim
        if desired_goal is None:
            rows = self._dev_f32(who, "observation", observation)
            if rows.ndim != 2 or rows.shape[1] != S:
                raise ValueError(f"{who}: observation: packed rows [n, {S}] required")
            D = obs_dim if obs_dim is not None else getattr(getattr(self.buffer, "obs_normalizer", None), "size", None)
            if D is None:
                raise ValueError(f"{who}: obs_dim: packed rows need obs_dim when no observation normaliser tells it")
            D = int(D)
        else:
            o, g = self._dev_f32(who, "observation", observation), self._dev_f32(who, "desired_goal", desired_goal)
            if o.ndim != 2 or g.ndim != 2 or o.shape[0] != g.shape[0] or o.shape[1] + g.shape[1] != S:
                raise ValueError(f"{who}: observation / desired_goal: [n, obs_dim] and [n, goal_dim] with obs_dim + goal_dim = {S} required")
            D = int(o.shape[1])
            rows = torch.cat([o, g], dim=1)
        n = int(rows.shape[0])
        self.set_eval()
        self._rows_dtypes(np.float32, np.float32, obs_normalize, g_normalize)
        if eval_action:
            noise, mode = None, (2 if self._sac else self._ACT_MODE_EVAL)
        else:
            mode = 2 if self._sac else self._ACT_MODE_EXPLORE
            if noise is None:
                sd, ns, _, ctr = self._collect_stream()
                z = torch.empty((n, self.ac_dim), dtype=torch.float32, device=rows.device)
                _ffi.check(lib.gcrl_hash_normal_fill(C.c_uint64(sd), C.c_uint64((ctr * n * self.ac_dim) & (2**64 - 1)), n * self.ac_dim, z.data_ptr(),
                                                     _ffi.stream_handle()))
                noise = z.double().mul_(ns)
                self.set_collect_stream(counter=ctr + 1)
            elif not (isinstance(noise, torch.Tensor) and noise.is_cuda and noise.dtype == torch.float64 and noise.is_contiguous()
                      and tuple(noise.shape) == (n, self.ac_dim)):
                raise ValueError(f"{who}: noise: a contiguous CUDA float64 tensor [{n}, {self.ac_dim}] required")
        out = torch.empty((n, self.ac_dim), dtype=torch.float32, device=rows.device)
        _ffi.check(lib.gcrl_agent_observe_act_dev(self._h, nz[0], nz[1], rows.data_ptr(), D, n, noise.data_ptr() if noise is not None else None,
                                                  mode, out.data_ptr(), _ffi.stream_handle()))
        return out

    def process_step_dev(self, state, actions, next_obs_raw, rewards, dones=None, obs_normalize: bool = True, g_normalize: bool = False, env0: int = 0):
        """`process_step` for CUDA float32 tensors: `state` / `next_obs_raw` are dicts of [n, .] tensors (observation, desired_goal,
        achieved_goal), `actions` [n, A], `rewards` [n]; `dones`: None (no env terminated) or a host bool array.  One pack launch builds
        the step's blocks on the device, then the launch and the bookkeeping of `process_step` — nothing crosses to the host."""
        who = f"{type(self).__name__}.process_step_dev"
        self._check_normalize_call("process_step_dev", obs_normalize, g_normalize, need_device=True)
        nz = self._dev_normalizers("process_step_dev", obs_normalize, g_normalize)
        f = self._dev_f32
        obs, nobs = f(who, "state['observation']", state["observation"]), f(who, "next_obs_raw['observation']", next_obs_raw["observation"])
        n, D = int(obs.shape[0]), int(obs.shape[1])
        dg, ndg = f(who, "state['desired_goal']", state["desired_goal"]), f(who, "next_obs_raw['desired_goal']", next_obs_raw["desired_goal"])
        G = int(dg.shape[1])
        nag = f(who, "next_obs_raw['achieved_goal']", next_obs_raw["achieved_goal"], (n, G))
        ag = f(who, "state['achieved_goal']", state["achieved_goal"], (n, G)) if g_normalize else None
        act = f(who, "actions", actions)
        A = int(act.shape[1])
        rew = f(who, "rewards", rewards.reshape(-1) if isinstance(rewards, torch.Tensor) else rewards, (n,))
        for name, t, shp in (("next_obs_raw['observation']", nobs, (n, D)), ("state['desired_goal']", dg, (n, G)), ("next_obs_raw['desired_goal']", ndg, (n, G)),
                             ("actions", act, (n, A))):
            f(who, name, t, shp)
        buf = self.buffer
        buf._ensure(D + G, A, G)
        self._rows_dtypes(np.float32, np.float32, obs_normalize, g_normalize)
        t_host = np.array([int(lib.gcrl_her_staged(buf.handle, int(env0) + i)) for i in range(n)], np.int32)
        raw = torch.empty(n * (2 * D + 4 * G), dtype=torch.float32, device=obs.device)
        pay = torch.zeros((n, 32), dtype=torch.float32, device=obs.device)
        t_dev = None
        if n and not np.all(t_host == t_host[0]):
            t_dev = torch.from_numpy(t_host).to(obs.device)
        st = _ffi.stream_handle()
        _ffi.check(lib.gcrl_proc_pack(obs.data_ptr(), nobs.data_ptr(), dg.data_ptr(), ndg.data_ptr(), ag.data_ptr() if ag is not None else None,
                                      nag.data_ptr(), act.data_ptr(), rew.data_ptr(), t_dev.data_ptr() if t_dev is not None else None,
                                      int(t_host[0]) if n else 0, n, D, G, A, raw.data_ptr(), pay.data_ptr(), st))
        dn = None if dones is None else np.ascontiguousarray(np.reshape(dones, -1), np.uint8)
        if dn is not None and dn.any():   # the done flags are the host's: they reach the payload's done word from there
            pay[:, 2] = torch.from_numpy(dn.astype(np.float32)).to(obs.device)
        buf.rng.pull()
        rows = lib.gcrl_her_process_step_dev(buf.handle, nz[0], 1 if obs_normalize else 0, nz[1], 1 if g_normalize else 0, raw.data_ptr(), pay.data_ptr(),
                                             D, t_host.ctypes.data, dn.ctypes.data if dn is not None else None, int(env0), n, st)
        buf._check_rows(rows)
        buf.rng.push_back()
        raw.record_stream(torch.cuda.current_stream()); pay.record_stream(torch.cuda.current_stream())
        return int(rows)

    def collect(self, env, steps: int, explore: bool = True, obs_normalize: bool = True, g_normalize: bool = False, practice=None) -> int:
        """`steps` vector steps of a `DeviceGoalEnv` into this agent's ring as ONE native call: per step the acting launch on the env's
        rows, the env's step and the process-step launch, plus the flush launches of the envs that finish — no host <-> device copy and
        no synchronisation.  `explore=True`: the device exploration stream (counter-hash normals scaled by noise_std;
        DDPG's epsilon branch from one counter-hash uniform per vector step); False: `observe_act`'s eval action.  Returns the ring rows
        appended.  Refusals name their field and come before anything is consumed (include/gcrl.h gcrl_agent_collect).
        `practice`: None, or a `GoalProposer` whose `step(env)` launches follow each env step inside the native loop (the host loop
        `observe_act -> env.step -> proposer.step(env) -> process_step`): one more launch a step, and one more in a step in which an env
        rolled over and the archive held `min_fill` entries; still no copy and no synchronisation."""
        who = f"{type(self).__name__}.collect"
        if getattr(self, "_owner", None) is not None:
            raise _ffi.GcrlError(f"{who}: collect: a population member acts through its population's entries: call pop.collect(group, steps) with a DeviceGoalEnvGroup")
        if getattr(self, "_dp_driven", False):
            raise _ffi.GcrlError(f"{who}: collect: an agent driven by a DataParallelUpdater does not collect (the data-parallel form is not built)")
        from .device_env import DeviceGoalEnv
        if not isinstance(env, DeviceGoalEnv):
            raise ValueError(f"{who}: env: a gcrl_amd.DeviceGoalEnv required")
        if int(steps) < 1:
            raise ValueError(f"{who}: steps: {steps} (>= 1 required)")
        if practice is not None:
            from .goal_propose import GoalProposer
            if not isinstance(practice, GoalProposer):
                raise ValueError(f"{who}: practice: a gcrl_amd.GoalProposer or None required")
        self._check_normalize_call("collect", obs_normalize, g_normalize, need_device=True)
        nz = self._dev_normalizers("collect", obs_normalize, g_normalize)
        buf = self.buffer
        if env.obs_dim + env.goal_dim != self.obs_dim or env.ac_dim != self.ac_dim:
            raise ValueError(f"{who}: env: obs_dim {env.obs_dim} + goal_dim {env.goal_dim} / ac_dim {env.ac_dim} differ from the agent's "
                             f"state_dim {self.obs_dim} / ac_dim {self.ac_dim}")
        buf._ensure(env.obs_dim + env.goal_dim, env.ac_dim, env.goal_dim)
        self._collect_stream()
        self.set_eval()
        self._rows_dtypes(np.float32, np.float32, obs_normalize, g_normalize)
        rows = C.c_int64(0)
        buf.rng.pull()
        args = (self._h, env.handle, buf.handle, nz[0], 1 if obs_normalize else 0, nz[1], 1 if g_normalize else 0, int(steps),
                1 if explore else 0, 2 if self._sac else self._ACT_MODE_EVAL)
        if practice is None:
            rc = lib.gcrl_agent_collect(*args, C.byref(rows), _ffi.stream_handle())
        else:
            rc = lib.gcrl_agent_collect_practice(*args, practice.handle, C.byref(rows), _ffi.stream_handle())
        buf.rng.push_back()
        _ffi.check(rc)
        buf._check_rows(int(rows.value))
        return int(rows.value)

    def evaluate(self, env, episodes: int, reset: bool = True, obs_normalize: bool = True, g_normalize: bool = False) -> dict:
        """Deterministic evaluation on a `DeviceGoalEnv` as ONE native call: ceil(episodes / N) * max_steps vector steps of the acting
        launch in eval mode (`observe_act(eval_action=True)`) and the env's step — no ring, no process-step; the normalisers are read
        and never updated, the exploration stream does not move.  `reset=True` resets the env first, so the call scores episodes 0, 1, ...
        of the env's seed (a fixed evaluation set); `reset=False` needs every env at the start of an episode (refused by `t` otherwise)
        and reports the counters' difference over the call.  Synchronises once, at the end.  Returns dict(episodes, successes,
        success_rate, reward_sum); `episodes` is what was run, a multiple of N (include/gcrl.h gcrl_agent_evaluate)."""
        who = f"{type(self).__name__}.evaluate"
        from .device_env import DeviceGoalEnv
        if not isinstance(env, DeviceGoalEnv):
            raise ValueError(f"{who}: env: a gcrl_amd.DeviceGoalEnv required")
        if int(episodes) < 1:
            raise ValueError(f"{who}: episodes: {episodes} (>= 1 required)")
        self._check_normalize_call("evaluate", obs_normalize, g_normalize)
        nz = self._dev_normalizers("evaluate", obs_normalize, g_normalize)
        if env.obs_dim + env.goal_dim != self.obs_dim or env.ac_dim != self.ac_dim:
            raise ValueError(f"{who}: env: obs_dim {env.obs_dim} + goal_dim {env.goal_dim} / ac_dim {env.ac_dim} differ from the agent's "
                             f"state_dim {self.obs_dim} / ac_dim {self.ac_dim}")
        self.set_eval()
        self._rows_dtypes(np.float32, np.float32, obs_normalize, g_normalize)
        ep, su, rs = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        _ffi.check(lib.gcrl_agent_evaluate(self._h, env.handle, nz[0], nz[1], int(episodes), 1 if reset else 0, 2 if self._sac else self._ACT_MODE_EVAL,
                                           C.byref(ep), C.byref(su), C.byref(rs), _ffi.stream_handle()))
        n = int(ep.value)
        return dict(episodes=n, successes=int(su.value), success_rate=int(su.value) / n if n else 0.0, reward_sum=float(rs.value))

    def collect_counts(self) -> dict:
        """What `collect` (and `observe_act_dev`) have issued since this agent was created: calls and vector steps of `collect`, kernel
        launches, host <-> device copies and stream synchronisations (include/gcrl.h gcrl_agent_collect_counts)."""
        v = [C.c_int64(0) for _ in range(5)]
        _ffi.check(lib.gcrl_agent_collect_counts(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("calls", "steps", "launches", "copies", "syncs"), (int(x.value) for x in v)))

    def push(self, state, action, reward, next_state, done):
        # (with a HERBuffer the reference passes 5 args to a push that takes 8 -> TypeError there too)
        self.buffer.push(state, action, reward, next_state, done)

    def push_her(self, idx, state, action, next_state, reward, done, desired_goal, achieved_goal):
        self.buffer.push(idx, state, action, next_state, reward, done, desired_goal, achieved_goal)

    def is_buffer_filled(self):
        return len(self.buffer) >= self.batch_size

    def set_train(self):
        self.actor.train()
        for c in self.critics:
            c.train()

    def set_eval(self):
        self.actor.eval()
        for c in self.critics:
            c.eval()

    # ------------------------------------------------------------------ normalisers (host, src/agent.py:1425-1459)
    def update_normalizers(self, obs_list, dg_list, obs_normalize, g_normalize):
        if hasattr(self.buffer, "obs_normalizer") and obs_list and obs_normalize:
            self.buffer.obs_normalizer.update(np.concatenate(obs_list, axis=0))
        if hasattr(self.buffer, "dg_normalizer") and dg_list and g_normalize:
            self.buffer.dg_normalizer.update(np.concatenate(dg_list, axis=0))

    def normalize_obs(self, obs, normalize: bool):
        if hasattr(self.buffer, "obs_normalizer") and normalize:
            return self.buffer.obs_normalizer.normalize(obs)
        return obs

    def normalize_goal(self, goal, normalize: bool):
        if hasattr(self.buffer, "dg_normalizer") and normalize:
            return self.buffer.dg_normalizer.normalize(goal)
        return goal

    def normalize_state_batch(self, obs_batch, dg_batch, obs_normalize, g_normalize):
        return np.concatenate([self.normalize_obs(obs_batch, obs_normalize),
                               self.normalize_goal(dg_batch, g_normalize)], axis=-1)

    # ------------------------------------------------------------------ targets / reset
    def update_target_network(self, hard_update: bool = True, tau: float = 0.005):
        """src/agent.py:1255-1271: hard copy, or tau*net + (1-tau)*target for every target network."""
        if hard_update:
            _ffi.check(lib.gcrl_agent_hard_update_targets(self._h))
        else:
            _ffi.check(lib.gcrl_agent_soft_update_targets(self._h, float(tau), _ffi.stream_handle()))

    # ------------------------------------------------------------------ full resume state (SURVEY.md §8f-2 extension)
    def save_state(self, path: str):
        """Everything a bitwise-identical continuation needs, which the reference's checkpoints (weights + normalisers,
        src/env.py:430-440) do not hold: parameters and targets, Adam moments, scheduler positions and step counts,
        BatchNorm statistics, alpha, the replay ring's rows + staged partial episodes, the MT19937 stream."""
        import json
        os.makedirs(path, exist_ok=True)
        n = int(lib.gcrl_agent_state_size(self._h))
        blob = np.empty(n, np.uint8)
        _ffi.check(lib.gcrl_agent_save_state(self._h, blob.ctypes.data, n))
        blob.tofile(os.path.join(path, "agent.bin"))
        meta = dict(kind=self.KIND_NAME, beta=self.beta, num_batches_tracked=int(self.actor.num_batches_tracked),
                    ring=self.buffer.save_state(os.path.join(path, "ring.bin")))
        if self.prior_buffer is not None:     # prior-data replay: the prior ring next to the main ring, through the same path
            meta["prior"] = dict(rows=int(self.prior_rows), ring=self.prior_buffer.save_state(os.path.join(path, "prior_ring.bin")))
        if self.bc_weight is not None:        # the behaviour-cloning term's settings: a resume under other settings is refused
            meta["bc"] = dict(bc_weight=float(self.bc_weight), q_filter=bool(self.q_filter))
        if self.__dict__.get("_collect_bound"):   # the device exploration stream of collect: its key and its vector-step counter
            sd, _, _, ctr = self._collect_stream()
            meta["collect"] = dict(seed=sd, counter=ctr)
        for name in ("obs_normalizer", "dg_normalizer"):
            nz = getattr(self.buffer, name, None)
            if nz is not None:
                meta[name] = dict(mean=np.asarray(nz.mean, np.float64).tolist(), var=np.asarray(nz.var, np.float64).tolist(),
                                  count=float(nz.count), clip_range=float(nz.clip_range),
                                  float32=bool(np.asarray(nz.mean).dtype == np.float32),   # (the regime after RunningNormalizer.load)
                                  rows64=bool(getattr(nz, "_rows64", 0)))   # (a device normaliser: the dtype its rows have on the trainer's side)
        with open(os.path.join(path, "meta.json"), "w") as f:
            json.dump(meta, f)

    def load_state(self, path: str):
        import json
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        if meta["kind"] != self.KIND_NAME:      # checked before anything of this agent is overwritten
            raise ValueError(f"state of a {meta['kind']} agent loaded into a {self.KIND_NAME}")
        saved_prior = meta.get("prior")
        if (saved_prior is None) != (self.prior_buffer is None):
            raise _ffi.GcrlError(f"{type(self).__name__}.load_state: prior_buffer: the state was saved "
                                 f"{'with' if saved_prior is not None else 'without'} a prior ring, this agent was built "
                                 f"{'with' if self.prior_buffer is not None else 'without'} one")
        if saved_prior is not None and int(saved_prior["rows"]) != int(self.prior_rows):
            raise _ffi.GcrlError(f"{type(self).__name__}.load_state: prior_rows: the state was saved with prior_rows={saved_prior['rows']}, "
                                 f"this agent has prior_rows={self.prior_rows}")
        saved_bc = meta.get("bc")
        if (saved_bc is None) != (self.bc_weight is None) or (saved_bc is not None and float(saved_bc["bc_weight"]) != float(self.bc_weight)):
            raise _ffi.GcrlError(f"{type(self).__name__}.load_state: bc_weight: the state was saved with bc_weight="
                                 f"{None if saved_bc is None else saved_bc['bc_weight']!r}, this agent has bc_weight={self.bc_weight!r}")
        if saved_bc is not None and bool(saved_bc["q_filter"]) != bool(self.q_filter):
            raise _ffi.GcrlError(f"{type(self).__name__}.load_state: q_filter: the state was saved with q_filter={bool(saved_bc['q_filter'])!r}, "
                                 f"this agent has q_filter={self.q_filter!r}")
        self.buffer._check_td_state(meta["ring"])     # prioritise="td_error" on either side: refused before anything is overwritten
        blob = np.fromfile(os.path.join(path, "agent.bin"), dtype=np.uint8)
        _ffi.check(lib.gcrl_agent_load_state(self._h, blob.ctypes.data, blob.size))
        self._bc_ticket = None
        if "collect" in meta:
            self.set_collect_stream(seed=int(meta["collect"]["seed"]), counter=int(meta["collect"]["counter"]))
        self.beta = meta["beta"]
        self.actor.num_batches_tracked = meta["num_batches_tracked"]
        self.buffer.load_state(os.path.join(path, "ring.bin"), meta["ring"])
        if saved_prior is not None:
            self.prior_buffer.load_state(os.path.join(path, "prior_ring.bin"), saved_prior["ring"])
        for name in ("obs_normalizer", "dg_normalizer"):
            nz = getattr(self.buffer, name, None)
            if name in meta and nz is not None:
                d = meta[name]
                if hasattr(nz, "set_state"):     # DeviceRunningNormalizer: its statistics live on the device
                    nz.set_state(np.array(d["mean"]), np.array(d["var"]), d["count"], d["clip_range"], float32=bool(d.get("float32", False)))
                    if "rows64" in d:     # (normalize="sample" normalises a gathered batch before the next acting call says it again)
                        nz.rows_dtype(np.float64 if d["rows64"] else np.float32)
                else:
                    dt = np.float32 if d.get("float32", False) else np.float64
                    nz.mean, nz.var = np.array(d["mean"], dtype=dt), np.array(d["var"], dtype=dt)
                    nz.count, nz.clip_range = d["count"], d["clip_range"]
        self._metric_cache.clear()

    def set_hyperparameters(self, **hparams):
        """Change learning rates (with their minima and scheduler lengths), gamma, tau, grad_clip — SAC / TQC: alpha_lr and
        alpha_min_steps too — of this live agent, between update calls (include/gcrl.h gcrl_agent_set_hparams).  Field names are the
        reference config's.  From the next step on the agent computes bit for bit what an agent constructed with the new values
        computes from the same state; scheduler positions are kept.  `self.config` becomes a copy holding the new values (configs
        are often shared between agents), so `save_state` and a later `replace` see the truth.  Refusals name the field and come
        before any device work."""
        check_hyperparameters(type(self).__name__, self._sac, hparams)
        self._apply_hyperparameters(hparams)

    def _apply_hyperparameters(self, hparams: dict):
        """`set_hyperparameters` after its host-side check (a population's `explore` has made it under its own name)."""
        import copy
        cfg = copy.copy(self.config)
        for k, v in hparams.items():
            setattr(cfg, k, int(v) if k.endswith("scheduler_steps") else v)
        h = _ffi.HParams(actor_lr=cfg.actor_lr, actor_lr_min=cfg.actor_lr_min, critic_lr=cfg.critic_lr, critic_lr_min=cfg.critic_lr_min,
                         ac_scheduler_steps=cfg.ac_scheduler_steps, cr_scheduler_steps=cfg.cr_scheduler_steps,
                         gamma=cfg.gamma, tau=cfg.tau, grad_clip=-1.0 if cfg.grad_clip is None else float(cfg.grad_clip),
                         alpha_lr=float(getattr(cfg, "alpha_lr", 0.0003)), alpha_min_steps=float(getattr(cfg, "alpha_min_steps", 10000)))
        _ffi.check(lib.gcrl_agent_set_hparams(self._h, C.byref(h)))
        self.config = cfg
        self.gamma, self.tau, self.grad_clip = cfg.gamma, cfg.tau, cfg.grad_clip
        self.alpha_min_steps = getattr(cfg, "alpha_min_steps", 10000)

    def reset(self):
        """Re-initialise Linear layers (src/agent.py:1461-1465, :760-769)."""
        seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
        _ffi.check(lib.gcrl_agent_init_weights(self._h, seed, 1 if self._sac else 0))

    def get_gradient_norm(self, model) -> float:
        g = model.grad_flat().astype(np.float64)
        return float(np.sqrt(np.sum(g * g)))


class DDPG(_EngineAgent):
    KIND_NAME = "DDPG"
    TD_INDEX = {6: 2, 4: 1}

    def _bind_names(self):
        self.critic, self.target_critic = self.critics[0], self.target_critics[0]

    def _load_weights(self, weights):
        self.actor.load(os.path.join(weights, "actor.pth"))
        p = os.path.join(weights, "critic.pth")
        self.critic.load(p if os.path.exists(p) else os.path.join(weights, "critic_1.pth"))

    def select_action(self, obs_tensor, eval_action: bool = False):
        self.set_eval()
        if not eval_action:
            if self.buffer.rng.random() < 0.2:  # src/agent.py:1348 — shares the HER stream
                return np.clip(np.random.randn(np.asarray(obs_tensor).shape[0], self.ac_dim), a_min=-1, a_max=1)
            action = torch.tanh(self._actor_forward(obs_tensor)).cpu().numpy()  # double tanh, as the reference
            return np.clip(action + np.random.normal(0, self.noise_std, size=action.shape), -1, 1)
        return np.clip(torch.tanh(self._actor_forward(obs_tensor)).cpu().numpy(), -1, 1)

    COLLECT_EPSILON = 0.2      # src/agent.py:1348, drawn from the device exploration stream's own uniform

    def _act_noise(self, n, eval_action):
        if not eval_action and self.buffer.rng.random() < 0.2:      # src/agent.py:1348
            return np.clip(np.random.randn(n, self.ac_dim), a_min=-1, a_max=1), None
        return super()._act_noise(n, eval_action)

    def save_weights(self, path: str):
        self.actor.save(os.path.join(path, "actor.pth"))
        self.critic.save(os.path.join(path, "critic.pth"))


class TD3Agent(_EngineAgent):
    KIND_NAME = "TD3"
    TD_INDEX = {8: 3, 6: 2}
    _ACT_MODE_EVAL = 2      # eval returns the network output as it is (src/agent.py:265-270)

    def _bind_names(self):
        self.critic_1, self.critic_2 = self.critics
        self.target_critic_1, self.target_critic_2 = self.target_critics

    def _load_weights(self, weights):
        self.actor.load(os.path.join(weights, "actor.pth"))
        self.critic_1.load(os.path.join(weights, "critic_1.pth"))
        self.critic_2.load(os.path.join(weights, "critic_2.pth"))

    def select_action(self, obs_tensor, eval_action: bool = False):
        self.set_eval()
        if not eval_action:
            action = torch.tanh(self._actor_forward(obs_tensor)).cpu().numpy()
            return np.clip(action + np.random.normal(0, self.noise_std, size=action.shape), -1, 1)
        return self._actor_forward(obs_tensor).cpu().numpy()

    def save_weights(self, path: str):
        self.actor.save(os.path.join(path, "actor.pth"))
        self.critic_1.save(os.path.join(path, "critic_1.pth"))
        self.critic_2.save(os.path.join(path, "critic_2.pth"))


class _StochasticAgent(_EngineAgent):
    TD_INDEX = {9: 3, 6: 2}

    def _act_noise(self, n, eval_action):
        if eval_action:
            return None, 2
        # rsample's eps (src/model.py:134); drawn on the host generator here — one fewer device round trip
        return np.ascontiguousarray(torch.randn((n, self.ac_dim), dtype=torch.float32).numpy().astype(np.float64)), 2

    def select_action(self, obs_tensor, eval_action: bool = False):
        self.set_eval()
        eps = None
        if not eval_action:
            n = np.asarray(obs_tensor).reshape(-1, self.obs_dim).shape[0]
            # rsample's eps (src/model.py:134: loc + empty(shape).normal_() * scale on the module's device).  Drawn from
            # torch's HOST generator here — what the reference itself uses on a CPU box, and one device round trip less
            eps = torch.randn((n, self.ac_dim), dtype=torch.float32).cuda()
        return self._actor_forward(obs_tensor, eps).cpu().numpy()

    def _log_alpha_tensor(self):
        buf = np.empty(1, np.float32)
        _ffi.check(lib.gcrl_agent_get(self._h, b"log_alpha", buf.ctypes.data, 1))
        return torch.tensor(buf, requires_grad=True)

    @property
    def log_alpha(self):
        return self._log_alpha_tensor()

    def _save_log_alpha(self, path):
        torch.save(self._log_alpha_tensor(), os.path.join(path, "log_alpha.pth"))


class SACAgent(_StochasticAgent):
    KIND_NAME = "SAC"

    def __init__(self, obs_dim, ac_dim, config, weights, nenvs, gradient_step, **kw):
        super().__init__(obs_dim, ac_dim, config, weights, nenvs, gradient_step, **kw)
        self.target_entropy = -ac_dim * 0.5
        self.train_alpha = False

    def _bind_names(self):
        self.critic_1, self.critic_2 = self.critics
        self.target_critic_1, self.target_critic_2 = self.target_critics

    def _load_weights(self, weights):
        self.actor.load(os.path.join(weights, "actor.pth"))
        self.critic_1.load(os.path.join(weights, "critic_1.pth"))
        self.critic_2.load(os.path.join(weights, "critic_2.pth"))

    def save_weights(self, path: str):
        self.actor.save(os.path.join(path, "actor.pth"))
        self.critic_1.save(os.path.join(path, "critic_1.pth"))
        self.critic_2.save(os.path.join(path, "critic_2.pth"))
        self._save_log_alpha(path)


class TQCAgent(_StochasticAgent):
    KIND_NAME = "TQC"

    def __init__(self, obs_dim, ac_dim, config, weights, nenvs, gradient_step, **kw):
        super().__init__(obs_dim, ac_dim, config, weights, nenvs, gradient_step, **kw)
        self.target_entropy = -ac_dim

    def _load_weights(self, weights):
        self.actor.load(os.path.join(weights, "actor.pth"))
        for i, c in enumerate(self.critics):
            p = os.path.join(weights, f"critic_{i}.pth")
            if os.path.exists(p):
                c.load(p)
        p = os.path.join(weights, "log_alpha.pth")
        if os.path.exists(p):
            la = torch.load(p, map_location="cpu").detach().float().reshape(-1).numpy()
            _ffi.check(lib.gcrl_agent_set(self._h, b"log_alpha", la.ctypes.data, 1))

    def save_weights(self, path: str):
        self.actor.save(os.path.join(path, "actor.pth"))
        for i, c in enumerate(self.critics):
            c.save(os.path.join(path, f"critic_{i}.pth"))
        self._save_log_alpha(path)
