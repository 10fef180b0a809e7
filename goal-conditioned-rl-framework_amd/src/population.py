"""DDPGPopulation / TD3Population — P independent agents of one kind whose update steps share launches (include/gcrl.h gcrl_pop_*).

RL results are reported over several seeds and hyper-parameter searches run many trials of one shape; with one agent per
trial, N agents cost N times one agent.  A population of 1..16 DDPG or TD3 agents of equal shapes issues each stage of a
training step once for all members (csrc/agent_pop.inc), and every member computes bit for bit what a standalone `DDPG` /
`TD3Agent` with the same config, seed and ring computes.

`.members` are ordinary `DDPG` / `TD3Agent` objects (own `HERBuffer`, the whole single-agent API, including `update` /
`update_many` on the member alone); `update_many(step0, n)` steps all of them and returns, per member, what the agent's own
`update_many` returns.
"""
from __future__ import annotations

import ctypes as C

from .. import _ffi
from .._ffi import lib
from .agent import DDPG, KIND, TD3Agent, native_config
from .buffer import MTStream

MAX_MEMBERS = 16

# fields every member must share (the population runs one launch pattern); the others (seed, gamma, tau, grad_clip, learning
# rates and their schedules, the ring's own settings) may differ
SHARED = ("hidden_dim", "layer_count", "batch_size", "ac_update_freq")


class _PopHandle:
    """Owner of the native population; the members keep it alive."""

    def __init__(self, cfgs):
        arr = (_ffi.AgentConfig * len(cfgs))(*cfgs)
        self.h = _ffi.check_ptr(lib.gcrl_pop_create(arr, len(cfgs)), "gcrl_pop_create")

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

    def _refuse(self, field: str, why: str):
        raise _ffi.GcrlError(f"{type(self).__name__}: {field}: {why}")

    def __init__(self, obs_dim: int, ac_dim: int, configs, nenvs: int, gradient_step: int, *, rng: str = "python",
                 seeds=None, device_index: int = 0):
        configs = list(configs)
        P = len(configs)
        # every refusal before any device work
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
        kind = KIND[self.AGENT.KIND_NAME]
        cfgs = [native_config(kind, obs_dim, ac_dim, c, int(gradient_step), num_critics=self.NUM_CRITICS, device_index=device_index, seed=s)
                for c, s in zip(configs, seeds)]
        self._pop = _PopHandle(cfgs)   # (the engine checks the rest — kind, row-chain shape — before it touches the device)
        pop = self._pop
        self.members = []
        for i, (c, s) in enumerate(zip(configs, seeds)):
            self.members.append(self.AGENT(obs_dim, ac_dim, c, None, nenvs, gradient_step, rng=rng, seed=s, device_index=device_index,
                                           _member=lambda cfg, i=i: (pop, pop.member(i))))
        self.rng_mode = rng
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
        tickets = (C.c_int64 * (P * n))()
        lens = (C.c_int32 * (P * n))()
        if self._shared_rng is not None:
            self._shared_rng.pull()
        _ffi.check(lib.gcrl_pop_update_n(self._pop.h, rings, int(step0), int(n), tickets, lens, _ffi.stream_handle()))
        if self._shared_rng is not None:
            self._shared_rng.push_back()
        out = []
        for i, m in enumerate(self.members):
            m.beta_scheduler(step0 + n - 1)
            out.append([m._tuple(int(tickets[i * n + j]), int(lens[i * n + j])) for j in range(n)])
        return out

    def update(self, step: int):
        """One step of every member: the members' `update(step)` tuples, in member order."""
        return [r[0] for r in self.update_many(step, 1)]

    def launch_counts(self):
        """(merged, alone): how the recorded launch positions of every update call so far were issued — as one launch of the
        kernel's population form for all members, or member by member (include/gcrl.h gcrl_pop_launch_counts)."""
        merged, alone = C.c_int64(), C.c_int64()
        _ffi.check(lib.gcrl_pop_launch_counts(self._pop.h, C.byref(merged), C.byref(alone)))
        return int(merged.value), int(alone.value)


class DDPGPopulation(_Population):
    """1..16 `DDPG` agents of equal shapes stepped together."""
    AGENT = DDPG
    NUM_CRITICS = 1


class TD3Population(_Population):
    """1..16 `TD3Agent`s of equal shapes stepped together (batch_size <= 1020: below the role-split critic phase); update_many
    returns, per member, `TD3Agent.update_many`'s tuples (8 entries on actor steps, 6 on critic-only steps)."""
    AGENT = TD3Agent
    NUM_CRITICS = 2
