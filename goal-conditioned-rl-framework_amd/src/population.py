"""DDPGPopulation / TD3Population / SACPopulation / TQCPopulation — P independent agents of one kind whose update steps share launches (include/gcrl.h gcrl_pop_*).

RL results are reported over several seeds and hyper-parameter searches run many trials of one shape; with one agent per
trial, N agents cost N times one agent.  A population of 1..16 DDPG, TD3, SAC or TQC agents of equal shapes issues each stage of a
training step once for all members (csrc/agent_pop.inc), and every member computes bit for bit what a standalone `DDPG` /
`TD3Agent` / `SACAgent` / `TQCAgent` with the same config, seed and ring computes (SAC, TQC: a standalone agent running the launch
forms `forms()` reports).

`.members` are ordinary `DDPG` / `TD3Agent` objects (own `HERBuffer`, the whole single-agent API, including `update` /
`update_many` on the member alone); `update_many(step0, n)` steps all of them and returns, per member, what the agent's own
`update_many` returns.  `observe_act` / `process_step` are the members' fused acting entries for all members at once: one launch
per call (gcrl_pop_observe_act — SAC's BatchNorm actors: gcrl_pop_observe_act_bn —, gcrl_pop_process_step), the host generators
consumed in member order.  `collect(group, steps)` / `evaluate(group, episodes)` run the same stages on a `DeviceGoalEnvGroup` as one
native call each, with nothing crossing to the host between the launches (gcrl_pop_collect, gcrl_pop_evaluate).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _ffi
from .._ffi import lib
from .agent import DDPG, KIND, SACAgent, TD3Agent, TQCAgent, check_hyperparameters, native_config
from .buffer import HERBuffer, MTStream, _check_goal_strategy, _check_normalize, _check_nstep, _check_prior

MAX_MEMBERS = 16
MAX_PAIRS = 16          # (source, destination) pairs of one `exploit` call
MANIFEST = "population.json"

# fields every member must share (the population runs one launch pattern); the others (seed, gamma, tau, grad_clip, learning
# rates and their schedules, SAC's alpha_lr and alpha_min_steps, the ring's own settings) may differ
SHARED = ("hidden_dim", "layer_count", "batch_size", "ac_update_freq")
# the replay ring's own settings: with `shared_ring` there is one ring, built from member 0's, so these must agree too
RING_FIELDS = ("max_len", "max_eps_len", "k_future")


def check_shared_prior_normalizers(who: str, members):
    """normalize="sample": a prior ring normalises what it gathers with the normalisers bound to IT, and a population binds every
    member's prior ring before the one native call that issues all members' prior parts.  Members that share a prior ring must
    therefore share the normaliser objects their flags need (`shared_ring=True` does; so does assigning one pair to every member):
    otherwise all but the last member's prior rows would leave with another member's statistics.  Refused naming prior_buffer,
    before anything is bound or consumed.  Standalone agents that share a prior ring are not concerned: each rebinds before its
    own call."""
    first = {}
    for i, m in enumerate(members):
        pb = getattr(m, "prior_buffer", None)
        if pb is None or getattr(m, "normalize", "push") != "sample":
            continue
        mine = (getattr(m.buffer, "obs_normalizer", None) if m.obs_normalize else None,
                getattr(m.buffer, "dg_normalizer", None) if m.g_normalize else None)
        j, theirs = first.setdefault(id(pb), (i, mine))
        if any(a is not b for a, b in zip(theirs, mine)):
            raise _ffi.GcrlError(f"{who}: prior_buffer: members {j} and {i} share one prior ring but not their normalisers; with "
                                 "normalize='sample' the ring's rows leave with the statistics bound to it, so members that share it "
                                 "must share the same obs_normalizer / dg_normalizer objects (shared_ring=True, or one prior ring per member)")


class _PopHandle:
    """Owner of the native population; the members keep it alive."""

    def __init__(self, cfgs, entry="gcrl_pop_create"):
        arr = (_ffi.AgentConfig * len(cfgs))(*cfgs)
        self.h = _ffi.check_ptr(getattr(lib, entry)(arr, len(cfgs)), entry)

    def member(self, i: int) -> int:
        out = C.c_void_p()
        _ffi.check(lib.gcrl_pop_member(self.h, i, C.byref(out)))
        return out.value

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            lib.gcrl_pop_destroy(h)


class _Population:
    AGENT = None          # the member class
    NUM_CRITICS = 1
    SAME_FORMS = False    # the class's guarantee is "a standalone agent running the same forms" (gcrl_pop_create_forms)
    ENTRY = None          # the engine entry that creates the population (None: gcrl_pop_create_forms / gcrl_pop_create by SAME_FORMS)

    def _native_configs(self, kind, obs_dim, ac_dim, configs, seeds, gradient_step, device_index):
        """The members' gcrl_agent_config records, as the member agents' own constructors form them (no device work)."""
        return [native_config(kind, obs_dim, ac_dim, c, int(gradient_step), num_critics=self.NUM_CRITICS, device_index=device_index, seed=s)
                for c, s in zip(configs, seeds)]

    def _refuse(self, field: str, why: str):
        raise _ffi.GcrlError(f"{type(self).__name__}: {field}: {why}")

    # update calls gather all members' batches in one launch (gcrl_pop_set_gather_merge) from this many members on.  DESIGN.md 4g's
    # rule: the smallest P from which the merged side's whole range lies below the member-by-member range at both shapes
    # (tools/population_bench.py --gather), never guessed; not measured yet, so no population merges by default and
    # `pop.merge_gather = True` takes the population launch.
    MERGE_GATHER_FROM = MAX_MEMBERS + 1

    def __init__(self, obs_dim: int, ac_dim: int, configs, nenvs: int, gradient_step: int, *, rng: str = "python",
                 seeds=None, device_index: int = 0, shared_ring: bool = False, per_draw: str = "host",
                 relabel: str = "push", n_step: int = 1, prioritise: str | None = None, energy: dict | None = None,
                 goal_strategy: str = "future", normalize: str = "push", obs_normalize: bool = True, g_normalize: bool = False,
                 prior_buffer=None, prior_rows: int | None = None, bc_weight: float | None = None, q_filter: bool = True):
        # bc_weight: accepted only to be refused by name — the behaviour-cloning term (agent._EngineAgent) is a single-agent mode
        if bc_weight is not None:
            self._refuse("bc_weight", f"populations do not step the behaviour-cloning term, got bc_weight={bc_weight!r}")
        # prioritise: accepted only to be refused by name — the energy-prioritised draw (buffer.HERBuffer) is a single-agent mode
        if prioritise is not None or energy is not None:
            self._refuse("prioritise", f"populations (and their shared ring) do not draw from an energy tree, got prioritise={prioritise!r}")
        # relabel="sample": every member's ring (or the shared one) relabels at gather time (buffer.HERBuffer); such gathers have no
        # population launch, so merge_gather = True then reports no merged launch (gather_counts()).
        if relabel not in ("push", "sample"):
            raise ValueError(f"relabel must be 'push' or 'sample', got {relabel!r}")
        self.relabel = relabel
        configs = list(configs)
        # goal_strategy: passed through to every member's ring (or the shared one); their sample-mode gathers stay member by member
        for c in configs or [None]:
            self.goal_strategy = _check_goal_strategy(type(self).__name__, goal_strategy, relabel, getattr(c, "buffer_type", "HER"))
        # normalize="sample": every member's ring (or the shared one, whose normalisers the members share) stores raw rows and
        # normalises what it gathers — one pass per member behind the population's gather launch, merged or not (buffer.HERBuffer)
        for c in configs or [None]:
            self.normalize = _check_normalize(type(self).__name__, normalize, obs_normalize, g_normalize, getattr(c, "buffer_type", "HER"))
        self.obs_normalize, self.g_normalize = bool(obs_normalize), bool(g_normalize)
        # prior_buffer / prior_rows: prior-data replay for every member (agent._EngineAgent) — ONE prior ring shared by all members
        # (read only, consumed in member order) or a list of one ring per member.  The main gathers keep merging as before; the
        # members' prior parts follow them member by member.  `exploit(copy_ring=True)` leaves prior rings alone.
        priors = list(prior_buffer) if isinstance(prior_buffer, (list, tuple)) else [prior_buffer] * max(1, len(configs))
        if isinstance(prior_buffer, (list, tuple)) and len(priors) != len(configs):
            self._refuse("prior_buffer", f"{len(priors)} prior rings for {len(configs)} members (one shared ring, or one per member)")
        for c, pb in zip(configs or [None], priors):
            self.prior_rows = _check_prior(type(self).__name__, pb, prior_rows, getattr(c, "batch_size", 2), getattr(c, "buffer_type", "HER"),
                                           self.normalize)
        self.prior_buffers = priors if prior_buffer is not None else None
        # n_step=N: every member's ring (or the shared one) gathers n-step windows; each member's update calls discount by its own gamma
        if n_step != 1:
            for i, c in enumerate(configs):
                if getattr(c, "buffer_type", "HER") != "HER":
                    self._refuse("n_step", f"member {i}: n_step={n_step!r} needs buffer_type 'HER' with relabel='sample', got {c.buffer_type!r}")
        self.n_step = _check_nstep(type(self).__name__, n_step, configs[0].gamma if configs else 0.0, relabel)[0]
        P = len(configs)
        self.shared_ring = bool(shared_ring)
        # every refusal before any device work
        if per_draw != "host":
            self._refuse("per_draw", f"populations train from HER rings; the device-resident prioritised draw (per_draw={per_draw!r}) is a "
                                     "single-agent mode")
        if not 1 <= P <= MAX_MEMBERS:
            self._refuse("members", f"a population has 1..{MAX_MEMBERS} members, got {P}")
        seeds = [None] * P if seeds is None else list(seeds)
        if len(seeds) != P:
            self._refuse("seeds", f"{len(seeds)} seeds for {P} members")
        for i, c in enumerate(configs):
            if getattr(c, "buffer_type", "HER") != "HER":
                self._refuse("buffer_type", f"member {i}: populations train from HER rings only, got {c.buffer_type!r}")
            for f in SHARED:
                if getattr(c, f) != getattr(configs[0], f):
                    self._refuse(f, f"member {i} has {getattr(c, f)!r}, member 0 {getattr(configs[0], f)!r}: members must share shapes")
            if self.shared_ring:
                for f in RING_FIELDS:
                    if getattr(c, f) != getattr(configs[0], f):
                        self._refuse(f, f"member {i} has {getattr(c, f)!r}, member 0 {getattr(configs[0], f)!r}: with shared_ring the members "
                                        "learn from one replay ring, built from member 0's settings")
        kind = KIND[self.AGENT.KIND_NAME]
        cfgs = self._native_configs(kind, obs_dim, ac_dim, configs, seeds, gradient_step, device_index)
        entry = self.ENTRY or ("gcrl_pop_create_forms" if self.SAME_FORMS else "gcrl_pop_create")
        self._pop = _PopHandle(cfgs, entry)   # (the engine checks the rest — kind, row-chain shape — before it touches the device)
        pop = self._pop
        self.members = []
        for i, (c, s) in enumerate(zip(configs, seeds)):
            self.members.append(self.AGENT(obs_dim, ac_dim, c, None, nenvs, gradient_step, rng=rng, seed=s, device_index=device_index, relabel=relabel,
                                           n_step=self.n_step, goal_strategy=self.goal_strategy, normalize=self.normalize, obs_normalize=self.obs_normalize,
                                           g_normalize=self.g_normalize, prior_buffer=priors[i] if prior_buffer is not None else None,
                                           prior_rows=prior_rows if prior_buffer is not None else None,
                                           _member=lambda cfg, i=i: (pop, pop.member(i))))
        self.rng_mode = rng
        self._merge_gather = False
        if P >= self.MERGE_GATHER_FROM:
            self.merge_gather = True
        if self.shared_ring:
            # ONE ring for all members (as the agent's own constructor builds it, with an episode slot per env of every member:
            # member i's envs stage in slots i * nenvs ...), its normalisers shared with it; seeded as member 0's ring
            c0 = configs[0]
            self.nenvs = int(nenvs)
            self.buffer = HERBuffer(c0.max_len, c0.max_eps_len, int(nenvs) * P, k_future=c0.k_future, rng=rng, seed=seeds[0],
                                    device_index=device_index, relabel=relabel, n_step=self.n_step,
                                    goal_strategy=self.goal_strategy, normalize=self.normalize, obs_normalize=self.obs_normalize,
                                    g_normalize=self.g_normalize,
                                    gamma=c0.gamma if self.n_step > 1 else None)   # (the ring's own gathers; a member's calls use the member's gamma)
            for m in self.members:
                m.buffer = self.buffer
        if rng == "python":
            # every use of a python-mode stream is bracketed by pull / push_back of `random`'s state, so the members may share one
            # generator — and a population call then draws member after member from one stream, exactly as the standalone
            # agents called in member order do
            self._shared_rng = MTStream("python")
            for m in self.members:
                m.buffer.rng = self._shared_rng
        else:
            self._shared_rng = None

    def __len__(self) -> int:
        return len(self.members)

    def update_many(self, step0: int, n: int):
        """The agent's `update_many(step0, n)` of every member; returns the members' lists of tuples, in member order."""
        P = len(self.members)
        rings = (C.c_void_p * P)()
        for i, m in enumerate(self.members):
            m.set_train()
            her = m.buffer.handle
            assert her is not None and len(m.buffer) >= m.batch_size, f"[ERROR] Not enough in buffer to sample (member {i})"
            rings[i] = her
        check_shared_prior_normalizers(type(self).__name__, self.members)
        for m in self.members:     # prior-data replay: every member's prior ring is bound before any member's call is planned
            m._bind_prior()
        tickets = (C.c_int64 * (P * n))()
        lens = (C.c_int32 * (P * n))()
        if self._shared_rng is not None:
            self._shared_rng.pull()
        try:
            _ffi.check(lib.gcrl_pop_update_n(self._pop.h, rings, int(step0), int(n), tickets, lens, _ffi.stream_handle()))
        finally:
            if self._shared_rng is not None:
                self._shared_rng.push_back()
        out = []
        for i, m in enumerate(self.members):
            m.beta_scheduler(step0 + n - 1)
            if m._sac:   # (as the agent's own update_many: BatchNorm's forward count, one per actor forward)
                m.actor.num_batches_tracked += sum(1 + (1 if lens[i * n + j] == 9 else 0) for j in range(n))
            out.append([m._tuple(int(tickets[i * n + j]), int(lens[i * n + j])) for j in range(n)])
        return out

    @property
    def merge_gather(self) -> bool:
        """Whether an update call gathers all members' batches in ONE launch of the gather kernel's population form (include/gcrl.h
        gcrl_pop_set_gather_merge) or member by member; the bits are the same either way."""
        return self._merge_gather

    @merge_gather.setter
    def merge_gather(self, on: bool):
        _ffi.check(lib.gcrl_pop_set_gather_merge(self._pop.h, 1 if on else 0))
        self._merge_gather = bool(on)

    def gather_counts(self):
        """(calls, merged, alone): update calls so far (one per chunk of at most the engine's steps-per-call limit), population
        gather launches, and member-by-member gather launches (include/gcrl.h gcrl_pop_gather_counts)."""
        v = [C.c_int64() for _ in range(3)]
        _ffi.check(lib.gcrl_pop_gather_counts(self._pop.h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def update(self, step: int):
        """One step of every member: the members' `update(step)` tuples, in member order."""
        return [r[0] for r in self.update_many(step, 1)]

    # ------------------------------------------------------------------ acting side
    # populations of at least this many members issue the population launches; smaller ones call the members' own entries (a
    # one-member population has nothing to merge).  Measured (profiles/r08_population_acting.jsonl): at P = 2 a DDPG
    # population's two calls take 55-63 us per vector step against 53-58 us member by member — the host work per member outweighs one
    # saved launch pair — while TD3 wins from P = 2 (51-63 against 58-65 us) and both win from P = 4 (1.4-1.7 x) to P = 16 (2.1-2.8 x)
    MERGE_ACTING_FROM = 2
    MERGE_PROCESS_FROM = None   # process_step's own threshold (None: MERGE_ACTING_FROM)

    def _staging(self, tag: str, key: tuple, shapes):
        """Persistent host staging of the acting entries (as `_EngineAgent._staging`: fixed addresses, ctypes pointers built once)."""
        cache = self.__dict__.setdefault("_stage_cache", {})
        st = cache.get(tag)
        if st is None or st[0] != key:
            arrs = {k: np.empty(shp, dt) for k, (shp, dt) in shapes().items()}
            P = len(self.members)
            st = cache[tag] = (key, arrs, {k: C.c_void_p(v.ctypes.data) for k, v in arrs.items()},
                               dict(nzo=(C.c_void_p * P)(), nzg=(C.c_void_p * P)(), rings=(C.c_void_p * P)(), rows=(C.c_int64 * P)()))
        return st[1], st[2], st[3]

    def _per_member(self, name: str, seq):
        if len(seq) != len(self.members):
            self._refuse("members", f"{name} has {len(seq)} entries for {len(self.members)} members")

    def _native_observe_act(self, nzo, nzg, ptr, D, G, n, with_noise):
        """The native call of `observe_act` on the filled staging arrays (the row-chain actors' entry; SACPopulation overrides)."""
        return lib.gcrl_pop_observe_act(self._pop.h, nzo, nzg, ptr["obs"], D, ptr["dg"], G, n, ptr["noise"] if with_noise else None,
                                        ptr["modes"], ptr["out"], _ffi.stream_handle())

    def observe_act(self, observations, desired_goals, eval_action: bool = False, obs_normalize: bool = True, g_normalize: bool = False):
        """`members[i].observe_act(observations[i], desired_goals[i], ...)` for every member as ONE native call and one launch;
        returns the members' float64 action arrays [n, A] in member order.  The host generators (`random`, `np.random`, the
        shared stream) are consumed member after member, exactly as by the members' own calls made in member order; a DDPG
        member on its epsilon-random branch takes no part in the launch.  Runs the members' own methods one after another
        when a normaliser this step needs is a host object or the members' row counts differ."""
        self._per_member("observations", observations)
        self._per_member("desired_goals", desired_goals)
        ms = self.members
        P = len(ms)
        if getattr(self, "normalize", "push") == "sample":    # the constructor's flags (the members share them)
            ms[0]._check_normalize_call("observe_act", obs_normalize, g_normalize)
        obs = [x if isinstance(x, np.ndarray) else np.asarray(x) for x in observations]
        dgs = [x if isinstance(x, np.ndarray) else np.asarray(x) for x in desired_goals]
        nzs = [m._device_normalizers(obs_normalize, g_normalize) for m in ms]
        shp, gshp = obs[0].shape, dgs[0].shape
        if (P < self.MERGE_ACTING_FROM or any(z is None for z in nzs) or len(shp) != 2 or len(gshp) != 2
                or any(o.shape != shp for o in obs) or any(g.shape != gshp for g in dgs)):
            return [m.observe_act(o, g, eval_action, obs_normalize, g_normalize) for m, o, g in zip(ms, obs, dgs)]
        n, D, G, A = shp[0], shp[1], gshp[1], ms[0].ac_dim
        if n > int(ms[0].config.batch_size):      # (before a generator is touched)
            raise ValueError(f"{type(self).__name__}.observe_act: n: {n} rows per member (1..batch_size = {ms[0].config.batch_size})")
        buf, ptr, arr = self._staging("act", (n, D, G, A), lambda: dict(obs=((P, n, D), np.float32), dg=((P, n, G), np.float32),
                                                                         noise=((P, n, A), np.float64), out=((P, n, A), np.float64),
                                                                         modes=((P,), np.int32)))
        modes, b_obs, b_dg, b_noise = buf["modes"], buf["obs"], buf["dg"], buf["noise"]
        nzo, nzg = arr["nzo"], arr["nzg"]
        out = [None] * P
        with_noise = False
        for i, m in enumerate(ms):
            m.set_eval()
            m._rows_dtypes(obs[i].dtype, dgs[i].dtype, obs_normalize, g_normalize)
            noise, mode = m._act_noise(n, eval_action)
            nzo[i], nzg[i] = nzs[i]
            if mode is None:
                modes[i], out[i] = -1, noise              # DDPG's epsilon-random action: no network involved
                continue
            modes[i] = mode
            np.copyto(b_obs[i], obs[i], casting="unsafe")
            np.copyto(b_dg[i], dgs[i], casting="unsafe")
            if noise is not None:
                np.copyto(b_noise[i], noise)
                with_noise = True
        _ffi.check(self._native_observe_act(nzo, nzg, ptr, D, G, n, with_noise))
        b_out = buf["out"]
        for i in range(P):
            if out[i] is None:
                out[i] = b_out[i].copy()
        return out

    def process_step(self, states, actions, next_obs_raws, rewards, dones, obs_normalize: bool = True, g_normalize: bool = False):
        """`members[i].process_step(states[i], actions[i], next_obs_raws[i], rewards[i], dones[i], ...)` for every member as ONE
        native call: one launch stages all members' transitions (each with its own normalisers), the members' episode flushes
        follow in member order.  Returns the rows appended per member.  Runs the members' own methods one after another when
        a normaliser this step needs is a host object, compute_reward runs through the host callback with g_normalize, or
        the members' row counts differ."""
        for name, seq in (("states", states), ("actions", actions), ("next_obs_raws", next_obs_raws), ("rewards", rewards), ("dones", dones)):
            self._per_member(name, seq)
        ms = self.members
        P = len(ms)
        if getattr(self, "normalize", "push") == "sample":    # the constructor's flags and device normalisers, before any member has pushed
            for m in ms:
                m._check_normalize_call("process_step", obs_normalize, g_normalize, need_device=True)
        if getattr(self, "shared_ring", False):
            # one ring and one pair of normalisers: the merged staging launch would update them from P members at once, so the members
            # push one after another, each into its own episode slots
            for i, a in enumerate(actions):
                if np.shape(a)[0] > self.nenvs:
                    self._refuse("actions", f"member {i} steps {np.shape(a)[0]} envs, the shared ring has {self.nenvs} episode slots per member")
            return [m.process_step(s, a, nx, r, d, obs_normalize, g_normalize, env0=i * self.nenvs)
                    for i, (m, s, a, nx, r, d) in enumerate(zip(ms, states, actions, next_obs_raws, rewards, dones))]
        as_arr = lambda x: x if isinstance(x, np.ndarray) else np.asarray(x)
        nzs = [m._device_normalizers(obs_normalize, g_normalize) for m in ms]
        rows_in = []
        for st, ac, nx in zip(states, actions, next_obs_raws):
            rows_in.append((as_arr(st["observation"]), as_arr(nx["observation"]), as_arr(st["desired_goal"]), as_arr(nx["desired_goal"]),
                            as_arr(nx["achieved_goal"]), as_arr(st["achieved_goal"]) if g_normalize else None, as_arr(ac)))
        merged = P >= (self.MERGE_ACTING_FROM if self.MERGE_PROCESS_FROM is None else self.MERGE_PROCESS_FROM) and all(z is not None for z in nzs)
        if merged:
            o0, _, g0, _, a0, _, c0 = rows_in[0]
            merged = all(r[0].shape == o0.shape and r[2].shape == g0.shape and r[4].shape == a0.shape and r[6].shape == c0.shape for r in rows_in)
        if merged:
            n, D, G, A = o0.shape[0], o0.shape[1], g0.shape[1], c0.shape[1]
            for m in ms:   # (the rings — and with them the reward kinds — exist from here on)
                m.buffer._ensure(D + G, A, a0.shape[1])
            merged = not (g_normalize and any(m.buffer._reward_cfg[0] == 2 for m in ms))
        if not merged:
            return [m.process_step(s, a, nx, r, d, obs_normalize, g_normalize)
                    for m, s, a, nx, r, d in zip(ms, states, actions, next_obs_raws, rewards, dones)]
        f32 = np.float32
        b, p, arr = self._staging("proc", (n, D, G, A), lambda: dict(obs=((P, n, D), f32), nobs=((P, n, D), f32), dg=((P, n, G), f32),
                                                                      ndg=((P, n, G), f32), ag=((P, n, G), f32), nag=((P, n, G), f32),
                                                                      act=((P, n, A), f32), rew=((P, n), f32), dn=((P, n), np.uint8)))
        cp = np.copyto
        nzo, nzg, rings = arr["nzo"], arr["nzg"], arr["rings"]
        for i, (m, (obs_i, nobs_i, dg_i, ndg_i, nag_i, ag_i, act_i)) in enumerate(zip(ms, rows_in)):
            # np.concatenate's result type, as the reference's update_normalizers forms it (src/agent.py:343-350)
            odt = obs_i.dtype if obs_i.dtype == nobs_i.dtype else np.result_type(obs_i.dtype, nobs_i.dtype)
            gdt = dg_i.dtype
            if g_normalize and not (dg_i.dtype == ndg_i.dtype == ag_i.dtype == nag_i.dtype):
                gdt = np.result_type(dg_i.dtype, ndg_i.dtype, ag_i.dtype, nag_i.dtype)
            m._rows_dtypes(odt, gdt, obs_normalize, g_normalize)
            cp(b["obs"][i], obs_i, casting="unsafe"); cp(b["nobs"][i], nobs_i, casting="unsafe"); cp(b["dg"][i], dg_i, casting="unsafe")
            cp(b["ndg"][i], ndg_i, casting="unsafe"); cp(b["nag"][i], nag_i, casting="unsafe"); cp(b["act"][i], act_i, casting="unsafe")
            cp(b["rew"][i], np.reshape(rewards[i], -1), casting="unsafe")
            cp(b["dn"][i], np.reshape(dones[i], -1), casting="unsafe")
            if g_normalize:
                cp(b["ag"][i], ag_i, casting="unsafe")
            nzo[i], nzg[i] = nzs[i]
            rings[i] = m.buffer.handle
        streams = list({id(m.buffer.rng): m.buffer.rng for m in ms}.values())   # (python mode: the one shared stream)
        for r in streams:
            r.pull()
        rc = lib.gcrl_pop_process_step(self._pop.h, rings, nzo, 1 if obs_normalize else 0, nzg, 1 if g_normalize else 0, p["obs"], p["nobs"], D,
                                       p["dg"], p["ndg"], p["ag"] if g_normalize else None, p["nag"], p["act"], p["rew"], p["dn"], 0, n,
                                       arr["rows"], _ffi.stream_handle())
        for m in ms:
            m.buffer._check_rows(0)      # (a failure caused by a compute_reward callable re-raises ITS exception)
        _ffi.check(rc)
        for r in streams:
            r.push_back()
        return [int(x) for x in arr["rows"]]

    # ------------------------------------------------------------------ device-resident collect and evaluation (DeviceGoalEnvGroup)
    def _group_call(self, name: str, group, obs_normalize: bool, g_normalize: bool, need_device: bool):
        """What `collect` and `evaluate` check and gather before their native call: the group, the members' device normalisers."""
        who = f"{type(self).__name__}.{name}"
        from .device_env import DeviceGoalEnvGroup
        if not isinstance(group, DeviceGoalEnvGroup):
            raise ValueError(f"{who}: env: a gcrl_amd.DeviceGoalEnvGroup required")
        ms = self.members
        P = len(ms)
        if group.members != P:
            raise ValueError(f"{who}: env: the group has {group.members} members, the population {P}")
        for i, m in enumerate(ms):
            if getattr(m, "_dp_driven", False):
                raise _ffi.GcrlError(f"{who}: {name}: member {i} is driven by a DataParallelUpdater (the data-parallel form is not built)")
        if group.obs_dim + group.goal_dim != ms[0].obs_dim or group.ac_dim != ms[0].ac_dim:
            raise ValueError(f"{who}: env: obs_dim {group.obs_dim} + goal_dim {group.goal_dim} / ac_dim {group.ac_dim} differ from the members' "
                             f"state_dim {ms[0].obs_dim} / ac_dim {ms[0].ac_dim}")
        nzo, nzg = (C.c_void_p * P)(), (C.c_void_p * P)()
        for i, m in enumerate(ms):
            m._check_normalize_call(name, obs_normalize, g_normalize, need_device=need_device)
            nzo[i], nzg[i] = m._dev_normalizers(name, obs_normalize, g_normalize)
        return who, nzo, nzg

    def collect(self, group, steps: int, explore: bool = True, obs_normalize: bool = True, g_normalize: bool = False):
        """`members[m].collect(env_m, steps)` for every member on a `DeviceGoalEnvGroup` as ONE native call: per vector step one acting
        launch, one env-step launch and one process-step launch for ALL members, plus the rings' flush launches in member order — no
        host <-> device copy and no synchronisation.  Each member keeps its own exploration stream (`set_collect_stream` on the
        member) and leaves what a standalone agent's `collect` on `DeviceGoalEnv(kind, N, seeds[m])` leaves, bit for bit.  Returns the
        ring rows appended per member.  Refusals name their field and come before anything is consumed (include/gcrl.h
        gcrl_pop_collect); a population with `shared_ring` is refused."""
        if self.shared_ring:
            self._refuse("shared_ring", "collect is not built for a shared ring: one ring and one normaliser pair cannot take the merged staging launch")
        who, nzo, nzg = self._group_call("collect", group, obs_normalize, g_normalize, True)
        if int(steps) < 1:
            raise ValueError(f"{who}: steps: {steps} (>= 1 required)")
        ms = self.members
        P = len(ms)
        rings = (C.c_void_p * P)()
        for i, m in enumerate(ms):
            m.buffer._ensure(group.obs_dim + group.goal_dim, group.ac_dim, group.goal_dim)
            m._collect_stream()
            m.set_eval()
            m._rows_dtypes(np.float32, np.float32, obs_normalize, g_normalize)
            rings[i] = m.buffer.handle
        rows = (C.c_int64 * P)()
        streams = list({id(m.buffer.rng): m.buffer.rng for m in ms}.values())   # (python mode: the one shared stream)
        for r in streams:
            r.pull()
        rc = lib.gcrl_pop_collect(self._pop.h, group.handle, rings, nzo, 1 if obs_normalize else 0, nzg, 1 if g_normalize else 0, int(steps),
                                  1 if explore else 0, 2 if ms[0]._sac else ms[0]._ACT_MODE_EVAL, rows, _ffi.stream_handle())
        for r in streams:
            r.push_back()
        _ffi.check(rc)
        for m in ms:
            m.buffer._check_rows(0)
        return [int(x) for x in rows]

    def collect_counts(self) -> dict:
        """What `collect` has issued since the population was created: calls, vector steps, kernel launches, host <-> device copies and
        stream synchronisations (include/gcrl.h gcrl_pop_collect_counts)."""
        v = [C.c_int64(0) for _ in range(5)]
        _ffi.check(lib.gcrl_pop_collect_counts(self._pop.h, *[C.byref(x) for x in v]))
        return dict(zip(("calls", "steps", "launches", "copies", "syncs"), (int(x.value) for x in v)))

    def evaluate(self, group, episodes: int, reset: bool = True, obs_normalize: bool = True, g_normalize: bool = False):
        """`members[m].evaluate(env_m, episodes, ...)` for every member on a `DeviceGoalEnvGroup` as ONE native call: two launches per
        vector step for ALL members (the acting launch in eval mode, the env step), one synchronisation at the end.  Nothing is pushed,
        no normaliser is updated, no exploration stream moves.  Returns one dict(episodes, successes, success_rate, reward_sum) per
        member; a group whose members share a seed ranks them on identical episodes (include/gcrl.h gcrl_pop_evaluate)."""
        who, nzo, nzg = self._group_call("evaluate", group, obs_normalize, g_normalize, False)
        if int(episodes) < 1:
            raise ValueError(f"{who}: episodes: {episodes} (>= 1 required)")
        ms = self.members
        P = len(ms)
        for m in ms:
            m.set_eval()
            m._rows_dtypes(np.float32, np.float32, obs_normalize, g_normalize)
        ep, su, rs = (C.c_int64 * P)(), (C.c_int64 * P)(), (C.c_double * P)()
        _ffi.check(lib.gcrl_pop_evaluate(self._pop.h, group.handle, nzo, nzg, int(episodes), 1 if reset else 0,
                                         2 if ms[0]._sac else ms[0]._ACT_MODE_EVAL, ep, su, rs, _ffi.stream_handle()))
        return [dict(episodes=int(ep[k]), successes=int(su[k]), success_rate=int(su[k]) / int(ep[k]) if ep[k] else 0.0, reward_sum=float(rs[k]))
                for k in range(P)]

    def acting_counts(self):
        """(act_calls, act_launches, proc_calls, proc_launches, act_staged): native calls of `observe_act` / `process_step` and the
        kernel launches they issued for the network / the process-step stage (flush launches not counted); act_staged: network
        launches that took the staged form (more rows per member than the pinned block holds).  Calls that ran the members'
        own methods advance none of them (include/gcrl.h gcrl_pop_acting_counts)."""
        v = [C.c_int64() for _ in range(5)]
        _ffi.check(lib.gcrl_pop_acting_counts(self._pop.h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def launch_counts(self):
        """(merged, alone): how the recorded launch positions of every update call so far were issued — as one launch of the
        kernel's population form for all members, or member by member (include/gcrl.h gcrl_pop_launch_counts)."""
        merged, alone = C.c_int64(), C.c_int64()
        _ffi.check(lib.gcrl_pop_launch_counts(self._pop.h, C.byref(merged), C.byref(alone)))
        return int(merged.value), int(alone.value)

    def forms(self):
        """Bits of the launch forms with waits between workgroups the next `update_many` runs, as `agent.meetings()` reports them
        for one agent: 1 row-split BatchNorm slab launches (SAC), 2 merged chain launch, 8 fused optimiser launch.  A form is on when
        every member has it on, the device is this process's own and the whole population launch is resident at once
        (include/gcrl.h gcrl_pop_forms)."""
        return _ffi.check(lib.gcrl_pop_forms(self._pop.h))

    def forms_terms(self):
        """{bit: (want, capacity)} for the form bits 1, 2 and 8: `len(self)` times a member's workgroups of the form against the
        workgroups of the population kernel resident at once, as fixed at creation (include/gcrl.h gcrl_pop_forms_terms)."""
        want, cap = (C.c_int64 * 3)(), (C.c_int64 * 3)()
        _ffi.check(lib.gcrl_pop_forms_terms(self._pop.h, want, cap))
        return {bit: (int(want[i]), int(cap[i])) for i, bit in enumerate((1, 2, 8))}


    # ------------------------------------------------------------------ population-based training: exploit / explore / replace
    def _check_pairs(self, pairs):
        """`exploit`'s argument as two index lists; every refusal names the argument and needs no device."""
        P = len(self.members)
        try:
            pairs = [(int(s), int(d)) for s, d in pairs]
        except (TypeError, ValueError):
            self._refuse("pairs", "a list of (source, destination) member indices")
        if not 1 <= len(pairs) <= MAX_PAIRS:
            self._refuse("pairs", f"{len(pairs)} pairs in one call (1..{MAX_PAIRS})")
        for s, d in pairs:
            if not 0 <= s < P:
                self._refuse("src", f"member {s} of {P}")
            if not 0 <= d < P:
                self._refuse("dst", f"member {d} of {P}")
        dsts = [d for _, d in pairs]
        for d in dsts:
            if dsts.count(d) > 1:
                self._refuse("dst", f"member {d} is a destination twice")
        both = sorted({s for s, _ in pairs} & set(dsts))
        if both:
            self._refuse("dst", f"member {both[0]} is both a source and a destination in one call")
        return pairs

    def exploit(self, pairs, copy_ring: bool = False):
        """For every `(src, dst)` of `pairs`, member `dst` takes over member `src`'s training state — parameters and targets, Adam
        moments, step counts and scheduler positions, BatchNorm statistics, alpha, the device-RNG position — in ONE launch for all
        pairs and without a host synchronisation (include/gcrl.h gcrl_pop_clone); bit for bit what `src.save_state` followed by
        `dst.load_state` leaves.  The destination keeps its own config (gamma, tau, grad_clip, the schedules' base and minimum
        rates and lengths, alpha_lr, seed): change those with `explore`.  On the Python side the destination gets what `load_state`
        sets: `beta`, the actor's `num_batches_tracked`, an empty metric cache.  With `copy_ring` the replay ring (rows, staged
        partial episodes, counters) travels in the same launch, an engine-mode index stream is copied, and the observation / goal
        normalisers' statistics are copied through `set_state` (a host round trip of a few hundred bytes per normaliser, as
        `load_state` does it — not device to device).  One source may serve several destinations; a member cannot be both in one call."""
        pairs = self._check_pairs(pairs)
        if copy_ring and getattr(self, "shared_ring", False):
            self._refuse("copy_ring", "the members learn from one shared replay ring (shared_ring=True): there is no ring to copy")
        ms = self.members
        P, n = len(ms), len(pairs)
        rings = None
        if copy_ring:
            for s, d in pairs:
                if ms[s].buffer.handle is None:
                    self._refuse("copy_ring", f"member {s} has no replay ring yet (nothing was pushed)")
                ra, rb = getattr(ms[s].buffer, "relabel", "push"), getattr(ms[d].buffer, "relabel", "push")
                if ra != rb:
                    self._refuse("relabel", f"member {s}'s ring has relabel={ra!r}, member {d}'s relabel={rb!r}: records of one mode do not "
                                            "fit a ring of the other (copy_ring=True)")
                na, nb = getattr(ms[s].buffer, "normalize", "push"), getattr(ms[d].buffer, "normalize", "push")
                if na != nb:
                    self._refuse("normalize", f"member {s}'s ring has normalize={na!r}, member {d}'s normalize={nb!r}: raw rows do not belong "
                                              "in a ring whose gathers do not normalise, nor the reverse (copy_ring=True)")
                ga, gb = getattr(ms[s].buffer, "goal_strategy", "future"), getattr(ms[d].buffer, "goal_strategy", "future")
                if ga != gb:
                    self._refuse("goal_strategy", f"member {s}'s ring has goal_strategy={ga!r}, member {d}'s goal_strategy={gb!r}: their "
                                                  "record widths differ (copy_ring=True)")
                ms[d].buffer._ensure(*ms[s].buffer._dims)
            rings = (C.c_void_p * P)(*[m.buffer.handle for m in ms])
        src = (C.c_int32 * n)(*[s for s, _ in pairs])
        dst = (C.c_int32 * n)(*[d for _, d in pairs])
        what = _ffi.CLONE_AGENT | (_ffi.CLONE_RING if copy_ring else 0)
        _ffi.check(lib.gcrl_pop_clone(self._pop.h, rings, src, dst, n, what, _ffi.stream_handle()))
        for s, d in pairs:
            a, b = ms[s], ms[d]
            b.beta = a.beta
            b.actor.num_batches_tracked = int(a.actor.num_batches_tracked)
            b._metric_cache.clear()
            if copy_ring:
                if a.buffer.rng.mode == "engine" and b.buffer.rng.mode == "engine":
                    _ffi.check(lib.gcrl_mt_get_state(a.buffer.rng.handle, a.buffer.rng._buf))
                    _ffi.check(lib.gcrl_mt_set_state(b.buffer.rng.handle, a.buffer.rng._buf))
                for name in ("obs_normalizer", "dg_normalizer"):
                    za, zb = getattr(a.buffer, name, None), getattr(b.buffer, name, None)
                    if za is None or zb is None:
                        continue
                    mean, var = np.asarray(za.mean), np.asarray(za.var)
                    f32 = bool(mean.dtype == np.float32)
                    if hasattr(zb, "set_state"):
                        zb.set_state(mean.astype(np.float64), var.astype(np.float64), float(za.count), float(za.clip_range), float32=f32)
                    else:
                        zb.mean, zb.var = mean.copy(), var.copy()
                        zb.count, zb.clip_range = float(za.count), float(za.clip_range)

    def explore(self, i: int, **hparams):
        """`members[i].set_hyperparameters(**hparams)`: new learning rates (minima, scheduler lengths), gamma, tau, grad_clip — SAC /
        TQC: alpha_lr, alpha_min_steps — for one member of the live population; the others are untouched and no launch form
        changes.  Fields every member must share (`SHARED`, num_critics) and unknown fields are refused naming the field."""
        if not 0 <= int(i) < len(self.members):
            self._refuse("i", f"member {i} of {len(self.members)}")
        m = self.members[int(i)]
        check_hyperparameters(type(self).__name__, m._sac, hparams)
        m._apply_hyperparameters(hparams)

    def _check_replace(self, i, config):
        if not 0 <= int(i) < len(self.members):
            self._refuse("i", f"member {i} of {len(self.members)}")
        cur = self.members[int(i)].config
        if getattr(config, "buffer_type", "HER") != "HER":
            self._refuse("buffer_type", f"populations train from HER rings only, got {config.buffer_type!r}")
        for f in SHARED + (("num_critics",) if self.NUM_CRITICS is None else ()):
            if getattr(config, f, None) != getattr(cur, f, None):
                self._refuse(f, f"the new member has {getattr(config, f, None)!r}, the population {getattr(cur, f, None)!r}: members must share shapes")
        for f in ("max_len", "max_eps_len", "k_future"):
            if getattr(config, f) != getattr(cur, f):
                self._refuse(f, f"the new member has {getattr(config, f)!r}, the slot's replay ring {getattr(cur, f)!r}: the ring is kept")

    def replace(self, i: int, config, seed=None):
        """Member `i` becomes what the population's constructor would have made of `config` / `seed` in that slot: freshly
        initialised weights, hard-copied targets, zero moments and step counts, initial BatchNorm statistics and log_alpha, a re-keyed
        device RNG (include/gcrl.h gcrl_pop_replace: in place, nothing of the agent reallocated, the other members and `forms()`
        unaffected) and fresh Python-side state.  Its replay ring is emptied: the same `HERBuffer` object with its reward function,
        but the ring's device memory is released here and allocated again by the next push — a fresh ring's counters and device index
        stream, at the price of one free and one allocation per replacement.  The normalisers stay the same objects (a trainer may hold
        them) and are reset in place to a new normaliser's statistics.  `config` must agree with the population in `SHARED` (TQC:
        num_critics too) and with the slot's ring settings; refusals name the field and come before any device work."""
        self._check_replace(i, config)
        i = int(i)
        m = self.members[i]
        kind = KIND[self.AGENT.KIND_NAME]
        cfg = self._native_configs(kind, m.obs_dim, m.ac_dim, [config], [seed], m.gradient_step, m.device_index)[0]
        _ffi.check(lib.gcrl_pop_replace(self._pop.h, i, C.byref(cfg)))
        m.config = config
        m.noise_std, m.noise_clamp, m.policy_noise = config.noise_std, config.noise_clamp, config.policy_noise
        m.gamma, m.tau, m.grad_clip = config.gamma, config.tau, config.grad_clip
        m.beta = m.beta_start = config.beta
        m.beta_end = config.beta_end
        m.alpha_min = getattr(config, "alpha_min", 0.05)
        m.alpha_min_steps = getattr(config, "alpha_min_steps", 10000)
        if kind == 3:
            m.top_quantiles_to_drop = int(getattr(config, "top_quantiles_to_drop", 2))
        m.actor.num_batches_tracked = 0
        m._metric_cache.clear()
        m._live.clear()
        m._lazy.clear()
        if getattr(self, "shared_ring", False):   # the ring and its normalisers belong to all members: kept as they are
            return
        buf = m.buffer
        if buf._h is not None:     # an emptied ring is a fresh one: the next push creates it (counters and device index stream at zero)
            h, buf._h = buf._h, None
            lib.gcrl_her_destroy(h)
            buf._dims = buf._reward_cfg = None
        if buf.rng is not getattr(self, "_shared_rng", None):        # (python mode: one stream for all members, which no member's seed touches)
            buf.rng.seed_value = 0 if seed is None else int(seed)
            if buf.rng.mode == "engine":
                buf.rng.seed(buf.rng.seed_value)
        for name in ("obs_normalizer", "dg_normalizer"):
            z = getattr(buf, name, None)
            if z is None:
                continue
            # in place, as a new normaliser starts: mean 0, var 1, count eps, float64 statistics (src/utils.py)
            size, eps = int(np.asarray(z.mean).shape[0]), float(getattr(z, "eps", 1e-8))
            if hasattr(z, "set_state"):
                z.set_state(np.zeros(size), np.ones(size), eps, float32=False)
            else:
                z.mean, z.var, z.count = np.zeros(size), np.ones(size), eps

    # ------------------------------------------------------------------ resume state of the whole population
    def _manifest(self):
        c0 = self.members[0].config
        shared = {f: getattr(c0, f) for f in SHARED}
        if self.NUM_CRITICS is None:
            shared["num_critics"] = int(self.members[0].num_critics)
        return dict(kind=self.AGENT.KIND_NAME, members=len(self.members), obs_dim=int(self.members[0].obs_dim), ac_dim=int(self.members[0].ac_dim),
                    shared=shared)

    def _check_manifest(self, got: dict):
        """A saved population's manifest against this population: kind, size and shapes, refused before anything is overwritten."""
        want = self._manifest()
        for f in ("kind", "members", "obs_dim", "ac_dim"):
            if got.get(f) != want[f]:
                self._refuse(f, f"the saved population has {got.get(f)!r}, this one {want[f]!r}")
        for f, v in want["shared"].items():
            if got.get("shared", {}).get(f) != v:
                self._refuse(f, f"the saved population has {got.get('shared', {}).get(f)!r}, this one {v!r}")

    def save_state(self, path: str):
        """Every member's `save_state` under `path`/member_00 ..., and `population.json` (kind, member count, shared fields)."""
        import json
        import os
        if getattr(self, "shared_ring", False):
            self._refuse("shared_ring", "save_state of a population with one shared replay ring is not supported yet")
        pbs = getattr(self, "prior_buffers", None)
        if pbs is not None and len({id(b) for b in pbs}) < len(pbs):
            self._refuse("prior_buffer", "save_state of a population whose members share a prior ring is not supported yet")
        os.makedirs(path, exist_ok=True)
        for i, m in enumerate(self.members):
            m.save_state(os.path.join(path, f"member_{i:02d}"))
        with open(os.path.join(path, MANIFEST), "w") as f:
            json.dump(self._manifest(), f)

    def load_state(self, path: str):
        """The members' `load_state` from a directory `save_state` wrote; a population of another kind, size or shape is refused
        (naming the field) before any member is overwritten."""
        import json
        import os
        if getattr(self, "shared_ring", False):
            self._refuse("shared_ring", "load_state into a population with one shared replay ring is not supported yet")
        with open(os.path.join(path, MANIFEST)) as f:
            self._check_manifest(json.load(f))
        for i in range(len(self.members)):
            if not os.path.isdir(os.path.join(path, f"member_{i:02d}")):
                self._refuse("members", f"{path} holds no member_{i:02d}")
        for i, m in enumerate(self.members):
            m.load_state(os.path.join(path, f"member_{i:02d}"))


class DDPGPopulation(_Population):
    """1..16 `DDPG` agents of equal shapes stepped together."""
    AGENT = DDPG
    NUM_CRITICS = 1
    MERGE_ACTING_FROM = 4


class SACPopulation(_Population):
    """1..16 `SACAgent`s of equal shapes stepped together (batch_size <= 512, hidden_dim % 16 == 0: the slab launches and the
    role-split chain launches with the actor's heads folded in); update_many returns, per member, `SACAgent.update_many`'s tuples (9
    entries on actor steps, 6 on critic-only steps).  Every member is bitwise a standalone `SACAgent` running the launch forms
    `forms()` reports.  `process_step` is the merged launch.  `observe_act` has one too (gcrl_pop_observe_act_bn: the population form
    of the BatchNorm actors' acting kernel, every member bit for bit its own `observe_act`), taken from `MERGE_ACTING_FROM` members
    on; below that the members' own one-launch entries run in member order."""
    AGENT = SACAgent
    NUM_CRITICS = 2
    SAME_FORMS = True
    # observe_act: the threshold is set from a measurement (the smallest P from which the merged form's whole range lies
    # below the member-by-member range at both shapes), never guessed.  The merged launch has not been timed yet, so the default stays
    # member by member; `pop.MERGE_ACTING_FROM = 2` takes the merged launch.
    MERGE_ACTING_FROM = MAX_MEMBERS + 1
    MERGE_PROCESS_FROM = 2                # process_step: the merged launch (it does not involve the network)

    def _native_observe_act(self, nzo, nzg, ptr, D, G, n, with_noise):
        # (SAC's _act_noise: mode 2 for every member, and eps for every member or — eval — for none)
        return lib.gcrl_pop_observe_act_bn(self._pop.h, nzo, nzg, ptr["obs"], D, ptr["dg"], G, n, ptr["noise"] if with_noise else None,
                                           ptr["out"], _ffi.stream_handle())


class TD3Population(_Population):
    """1..16 `TD3Agent`s of equal shapes stepped together (batch_size <= 1020: below the role-split critic phase); update_many
    returns, per member, `TD3Agent.update_many`'s tuples (8 entries on actor steps, 6 on critic-only steps)."""
    AGENT = TD3Agent
    NUM_CRITICS = 2


class TQCPopulation(_Population):
    """1..16 `TQCAgent`s of equal shapes stepped together (scalar critics, batch_size <= 512, hidden_dim % 16 == 0: the layer-per-launch
    step with the BatchNorm actor's slab launches; engine entry gcrl_pop_create_layered).  `num_critics` (2..8) comes from the configs
    as `TQCAgent` reads it and must be shared; `top_quantiles_to_drop` may differ per member.  update_many returns, per member,
    `TQCAgent.update_many`'s tuples (9 entries on actor steps, 6 on critic-only steps).  Every member is bitwise a standalone
    `TQCAgent` running the launch forms `forms()` reports.  Acting is SAC's (the same BatchNorm actor): `process_step` is the merged
    launch, `observe_act` has one too and — untimed for this kind — takes it only once `MERGE_ACTING_FROM` is lowered."""
    AGENT = TQCAgent
    NUM_CRITICS = None    # from the configs
    SAME_FORMS = True
    ENTRY = "gcrl_pop_create_layered"
    MERGE_ACTING_FROM = MAX_MEMBERS + 1   # (DESIGN.md 4g's rule: the merged acting launch is untimed for this kind)
    MERGE_PROCESS_FROM = 2
    _native_observe_act = SACPopulation._native_observe_act   # the BatchNorm actors' entry (gcrl_pop_observe_act_bn)

    def _native_configs(self, kind, obs_dim, ac_dim, configs, seeds, gradient_step, device_index):
        # (TQCAgent's own reading of the two keys: src/agent.py)
        ncs = [int(getattr(c, "num_critics", 5)) for c in configs]
        for i, nc in enumerate(ncs):
            if nc != ncs[0]:
                self._refuse("num_critics", f"member {i} has {nc}, member 0 {ncs[0]}: members must share the critic count")
        return [native_config(kind, obs_dim, ac_dim, c, int(gradient_step), num_critics=nc, top_drop=int(getattr(c, "top_quantiles_to_drop", 2)),
                              n_quantiles=1, device_index=device_index, seed=s)
                for c, nc, s in zip(configs, ncs, seeds)]
