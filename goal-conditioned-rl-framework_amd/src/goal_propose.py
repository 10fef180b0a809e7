"""Practice goals for the device goal envs (csrc/goal_propose.hip): a `GoalProposer` keeps an archive of the raw achieved goals a
`DeviceGoalEnv` visits and, when an env's episode ends at its horizon, may replace the new episode's task goal by an archived
achieved goal of low density — the least crowded of `candidates` hashed picks, crowding counted inside `radius` — so the agent
practises on the frontier of what it has reached (the min-density rule of MEGA, Pitis et al. 2020, on an own archive in the env's
units).  `share` is the probability that a finished env takes a proposal; the others keep the goal the env's seed gives them.

The rule — hash streams, operation order, tie rule — is restated in numpy in tests/goal_propose_ref.py, which is its definition; the
device result is that file's bit for bit.  Host loop: `observe_act_dev -> env.step -> proposer.step(env) -> process_step_dev`;
`agent.collect(env, steps, practice=proposer)` is that loop as one native call.

`env.stats()` counts an episode's success against the goal the episode had, practised or task.  `agent.evaluate(env, n)` (reset=True)
restarts the env and so scores task goals only; it never appends and never proposes.  After `env.reset(mask)` the selected envs'
next episode has its task goal.  What practice goals do to a learning curve has not been measured."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _ffi
from .._ffi import lib

# the state blob's header (include/gcrl.h gcrl_goal_proposer_save_state); the archive's capacity * 3 float32 follow at their physical slots
STATE_HEADER = np.dtype([("magic", "<u4"), ("capacity", "<i4"), ("candidates", "<i4"), ("min_fill", "<i4"), ("radius", "<f4"), ("share", "<f4"),
                         ("seed", "<u8"), ("num_envs", "<i4"), ("head", "<i4"), ("len", "<i4"), ("pad", "<i4"), ("counter", "<u8"),
                         ("appended", "<i8"), ("roll_steps", "<i8"), ("patched", "<i8")])


class GoalProposer:
    """capacity 1..65536 archive entries (at least the env's num_envs), candidates 1..64, radius > 0 in the env's units, share in
    (0, 1], min_fill 1..capacity (no proposal before the archive holds that many entries).  Bound to one `DeviceGoalEnv` at its
    first use; refusals name their field and consume nothing."""

    def __init__(self, capacity: int = 8192, candidates: int = 16, radius: float = 0.05, share: float = 0.5, min_fill: int = 256, seed: int = 0,
                 device_index: int = 0):
        self._h = None
        h = lib.gcrl_goal_proposer_create(int(capacity), int(candidates), float(radius), float(share), int(min_fill), int(seed) & (2**64 - 1),
                                          int(device_index))
        if not h:
            msg = _ffi.last_error()
            if "no usable HIP device" in msg or "allocation failed" in msg:
                raise _ffi.GcrlError(f"gcrl_goal_proposer_create failed: {msg}")
            raise ValueError(msg)
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.gcrl_goal_proposer_destroy(h)

    @property
    def handle(self):
        return self._h

    def _get(self) -> dict:
        i = {k: C.c_int() for k in ("capacity", "candidates", "min_fill", "device_index", "num_envs", "head", "len", "tile")}
        f = {k: C.c_float() for k in ("radius", "share")}
        u = {k: C.c_uint64() for k in ("seed", "counter")}
        r = C.byref
        _ffi.check(lib.gcrl_goal_proposer_get(self._h, r(i["capacity"]), r(i["candidates"]), r(f["radius"]), r(f["share"]), r(i["min_fill"]), r(u["seed"]),
                                              r(i["device_index"]), r(i["num_envs"]), r(i["head"]), r(i["len"]), r(u["counter"]), r(i["tile"])))
        out = {k: int(v.value) for k, v in {**i, **u}.items()}
        out.update({k: float(v.value) for k, v in f.items()})
        return out

    capacity = property(lambda self: self._get()["capacity"])
    candidates = property(lambda self: self._get()["candidates"])
    radius = property(lambda self: self._get()["radius"])
    share = property(lambda self: self._get()["share"])
    min_fill = property(lambda self: self._get()["min_fill"])
    seed = property(lambda self: self._get()["seed"])
    device_index = property(lambda self: self._get()["device_index"])
    num_envs = property(lambda self: self._get()["num_envs"], doc="envs of the env this proposer is bound to; 0 before its first use")
    head = property(lambda self: self._get()["head"], doc="physical slot of the oldest archive entry")
    len = property(lambda self: self._get()["len"])
    counter = property(lambda self: self._get()["counter"], doc="q: the steps seen so far in which an env rolled over")
    tile = property(lambda self: self._get()["tile"], doc="archive slots the propose kernel stages per pass")

    def __len__(self):
        return self._get()["len"]

    def step(self, env):
        """Call after `env.step(actions)` on the same stream: the step's achieved goals go to the archive (one launch) and, when an env
        rolled over, the propose launch patches the new episodes' goals.  No copy, no synchronisation."""
        from .device_env import DeviceGoalEnv
        if not isinstance(env, DeviceGoalEnv):
            raise ValueError("GoalProposer.step: env: a gcrl_amd.DeviceGoalEnv required (members: groups are not served)")
        _ffi.check(lib.gcrl_goal_proposer_step(self._h, env.handle, _ffi.stream_handle()))

    def stats(self) -> dict:
        """Rows appended, steps in which an env rolled over, proposals patched — host counters, no synchronisation."""
        v = [C.c_int64(0) for _ in range(3)]
        _ffi.check(lib.gcrl_goal_proposer_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("appended", "roll_steps", "patched"), (int(x.value) for x in v)))

    def archive(self) -> np.ndarray:
        """The archive in logical order (oldest first), float32 [len, 3].  Synchronises."""
        out = np.empty((self._get()["len"], 3), np.float32)
        if out.size:
            _ffi.check(lib.gcrl_goal_proposer_read(self._h, out.ctypes.data, _ffi.stream_handle()))
        return out

    def save_state(self) -> np.ndarray:
        """Settings, head, len, counter, stats and the archive as one uint8 array (`STATE_HEADER`, then the archive at its physical
        slots); `load_state` resumes bitwise.  Save behind `step`, not between `env.step` and it."""
        n = int(lib.gcrl_goal_proposer_state_bytes(self._h))
        blob = np.empty(n, np.uint8)
        _ffi.check(lib.gcrl_goal_proposer_save_state(self._h, blob.ctypes.data, n, _ffi.stream_handle()))
        return blob

    def load_state(self, blob):
        """Refuses a state of other settings or of another num_envs by that field's name before anything is overwritten."""
        blob = np.ascontiguousarray(blob, np.uint8)
        _ffi.check(lib.gcrl_goal_proposer_load_state(self._h, blob.ctypes.data, blob.size, _ffi.stream_handle()))
