"""Device-resident goal environments (csrc/dev_env.hip): `num_envs` independent envs of a built-in kind whose state, counters and
step blocks live in device memory.  `agent.collect(env, steps)` drives them without the host in the loop; `acting_rows()` and
`step_blocks()` hand out tensor views for callers who drive `observe_act_dev` / `process_step_dev` themselves.

The rule of every kind — constants, operation order, random-number keys — is restated in numpy in tests/dev_env_ref.py (`reach`,
`push`), tests/dev_env_pick_ref.py (`pick`) and tests/dev_env_glide_ref.py (`glide`), which are its definition.  The envs are not panda-gym: `reach` is the point mass of
examples/trainer_standin.py in float32 (obs 7, action 3), `push` a pusher that carries a puck along while it is inside a contact
radius (obs 13, action 3), `pick` a gripper whose fingers grasp an object by closing around it, at the dimensions of
PandaPickAndPlace (obs 20, goal 3, action 4: gripper velocity and finger velocity); half of its goals lie above the table, `glide` a
pusher and a puck that keeps 0.9 of its displacement per step once it is let go (obs 16, action 3), with goals beyond the pusher's box:
the puck has to be struck, not carried (it is not PandaSlide; the name "slide" stays an unknown kind).  `pick` and `glide` have their
scripted controllers on the device: `scripted_actions()`, and `HERBuffer.collect_scripted(env, steps)` fills a ring from them."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _ffi
from .._ffi import lib

KINDS = {"reach": 0, "push": 1, "pick": 2, "glide": 3}
SCRIPTED = ("pick", "glide")      # the kinds whose scripted controller is built
PAY_W = 32


class _DevBlock:
    """Zero-copy torch view of a float32 device block the env handle owns (it lives as long as the handle)."""

    def __init__(self, ptr: int, numel: int):
        self.__cuda_array_interface__ = {"shape": (int(numel),), "typestr": "<f4", "data": (int(ptr), False), "version": 2, "strides": None}


class _DevBlock64(_DevBlock):
    """The same for a float64 block."""

    def __init__(self, ptr: int, numel: int):
        super().__init__(ptr, numel)
        self.__cuda_array_interface__["typestr"] = "<f8"


class DeviceGoalEnvGroup:
    """`members` x `num_envs` envs in single allocations for a population (`pop.collect(group, steps)`, `pop.evaluate(group, episodes)`).
    Member m IS a `DeviceGoalEnv(kind, num_envs, seeds[m], ...)` — the same state, counters, random-number keys and arithmetic — whose
    blocks are slices at the strides the population kernels read.  One launch steps or resets all members.  The engine has this one
    handle type: a `DeviceGoalEnv` is a group of one member under its own name, in the same layout."""

    HEADER_BYTES = 24           # of the group's state blob; the members' records follow, each a standalone env's blob

    def __init__(self, kind: str, members: int, num_envs: int, seeds, max_steps: int = 50, threshold: float = 0.05, device_index: int = 0):
        if kind not in KINDS:
            raise ValueError(f"DeviceGoalEnvGroup: kind: {kind!r} (one of {sorted(KINDS)})")
        seeds = [int(s) & (2**64 - 1) for s in seeds]
        if len(seeds) != int(members):
            raise ValueError(f"DeviceGoalEnvGroup: seeds: {len(seeds)} seeds for {members} members")
        self.kind, self.device_index = kind, int(device_index)
        arr = (C.c_uint64 * max(1, len(seeds)))(*seeds)
        self._h = _ffi.check_ptr(lib.gcrl_env_group_create(KINDS[kind], int(members), int(num_envs), arr, int(max_steps), float(threshold),
                                                           self.device_index), "gcrl_env_group_create")
        ints = [C.c_int() for _ in range(7)]
        thr, tail = C.c_float(), [C.c_int() for _ in range(3)]
        _ffi.check(lib.gcrl_env_group_dims(self._h, *[C.byref(x) for x in ints], C.byref(thr), None, *[C.byref(x) for x in tail]))
        _, self.members, self.num_envs, self.obs_dim, self.goal_dim, self.ac_dim, self.max_steps = (int(x.value) for x in ints)
        self.stride_n, self.stride, self.raw_floats = (int(x.value) for x in tail)
        self.threshold = float(thr.value)
        self._views = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.gcrl_env_group_destroy(h)

    @property
    def handle(self):
        return self._h

    @property
    def seeds(self):
        sd = (C.c_uint64 * self.members)()
        _ffi.check(lib.gcrl_env_group_dims(self._h, None, None, None, None, None, None, None, None, sd, None, None, None))
        return [int(x) for x in sd]

    # ------------------------------------------------------------------ views of the handle's device blocks
    def _blocks(self):
        if self._views is None:
            p = [C.c_void_p() for _ in range(4)]
            _ffi.check(lib.gcrl_env_group_buffers(self._h, *[C.byref(x) for x in p]))
            P, sn, W, A = self.members, self.stride_n, self.obs_dim + self.goal_dim, self.ac_dim
            dev = f"cuda:{self.device_index}"
            self._views = (torch.as_tensor(_DevBlock(p[0].value, P * sn * W), device=dev).view(P, sn, W),
                           torch.as_tensor(_DevBlock(p[1].value, P * self.stride), device=dev).view(P, self.stride),
                           torch.as_tensor(_DevBlock64(p[2].value, P * sn * A), device=dev).view(P, sn, A),
                           torch.as_tensor(_DevBlock64(p[3].value, P * sn * A), device=dev).view(P, sn, A))
        return self._views

    def padded_blocks(self):
        """(rows [P, stride_n, W], data [P, stride], noise64 [P, stride_n, A], act64 [P, stride_n, A]): the whole allocations, the rows
        and floats past each member's share included (they are never read and never written)."""
        return self._blocks()

    def acting_rows(self):
        """As `DeviceGoalEnv.acting_rows()` with a leading member dimension: views [P, N, .] of the group's memory."""
        rows = self._blocks()[0][:, :self.num_envs]
        return {"rows": rows, "observation": rows[:, :, :self.obs_dim], "desired_goal": rows[:, :, self.obs_dim:]}

    def step_blocks(self):
        """(raw [P, raw_floats], pay [P, N, 32]) of the LAST step: member m's slices as `DeviceGoalEnv.step_blocks()` lays them out."""
        data = self._blocks()[1]
        n = self.num_envs
        return data[:, :self.raw_floats], data[:, self.raw_floats:self.raw_floats + n * PAY_W].unflatten(1, (n, PAY_W))

    # ------------------------------------------------------------------ stepping by hand
    def reset(self, mask=None, members=None):
        """Nothing given: every env of every member back to its episode 0 and the counters to zero.  mask [P, N] bool (host): those envs go
        on to their next episode; members=[...]: every env of those members does.  One launch."""
        m = None
        if members is not None:
            if mask is not None:
                raise ValueError("DeviceGoalEnvGroup.reset: mask: give a mask or members, not both")
            m = np.zeros((self.members, self.num_envs), np.uint8)
            for k in members:
                if not 0 <= int(k) < self.members:
                    raise ValueError(f"DeviceGoalEnvGroup.reset: members: {k} outside [0, {self.members})")
                m[int(k)] = 1
        elif mask is not None:
            m = np.ascontiguousarray(np.asarray(mask).reshape(-1), np.uint8)
            if m.size != self.members * self.num_envs:
                raise ValueError(f"DeviceGoalEnvGroup.reset: mask: {m.size} entries for {self.members} x {self.num_envs} envs")
        _ffi.check(lib.gcrl_env_group_reset(self._h, m.ctypes.data if m is not None else None, _ffi.stream_handle()))
        return self.acting_rows()

    def step(self, actions, eps=None):
        """One vector step of every member from a CUDA float32 or float64 tensor [P, N, ac_dim], one launch.  eps: {member: (seed, counter0)} —
        those members' envs form their own actions clamp(hash_normal(seed, counter0 + env * ac_dim + component), -1, 1) (the epsilon step of
        a DDPG collect) and their slice of `actions` is not read."""
        shape = (self.members, self.num_envs, self.ac_dim)
        if not (isinstance(actions, torch.Tensor) and actions.is_cuda and actions.is_contiguous() and actions.dtype in (torch.float32, torch.float64)
                and tuple(actions.shape) == shape):
            raise ValueError(f"DeviceGoalEnvGroup.step: actions: a contiguous CUDA float32 / float64 tensor {list(shape)} required")
        sel = sd = ct = None
        if eps:
            sel, sd, ct = np.zeros(self.members, np.uint8), np.zeros(self.members, np.uint64), np.zeros(self.members, np.uint64)
            for k, (seed, ctr0) in eps.items():
                if not 0 <= int(k) < self.members:
                    raise ValueError(f"DeviceGoalEnvGroup.step: eps: member {k} outside [0, {self.members})")
                sel[int(k)], sd[int(k)], ct[int(k)] = 1, int(seed) & (2**64 - 1), int(ctr0) & (2**64 - 1)
        _ffi.check(lib.gcrl_env_group_step(self._h, actions.data_ptr(), 1 if actions.dtype == torch.float64 else 0,
                                           sel.ctypes.data if sel is not None else None, sd.ctypes.data if sel is not None else None,
                                           ct.ctypes.data if sel is not None else None, _ffi.stream_handle()))

    def stats(self) -> list:
        """Synchronises once.  One dict per member: what `DeviceGoalEnv.stats()` reports for it."""
        P = self.members
        ep, su, rs = (C.c_int64 * P)(), (C.c_int64 * P)(), (C.c_double * P)()
        _ffi.check(lib.gcrl_env_group_stats(self._h, ep, su, rs, _ffi.stream_handle()))
        return [dict(episodes=int(ep[k]), successes=int(su[k]), reward_sum=float(rs[k])) for k in range(P)]

    # ------------------------------------------------------------------ resume
    def save_state(self) -> np.ndarray:
        n = int(lib.gcrl_env_group_state_bytes(self._h))
        blob = np.empty(n, np.uint8)
        _ffi.check(lib.gcrl_env_group_save_state(self._h, blob.ctypes.data, n, _ffi.stream_handle()))
        return blob

    def load_state(self, blob):
        """Refuses a state of other members, kind, num_envs, max_steps or threshold by that field's name before anything is overwritten."""
        blob = np.ascontiguousarray(blob, np.uint8)
        _ffi.check(lib.gcrl_env_group_load_state(self._h, blob.ctypes.data, blob.size, _ffi.stream_handle()))

    def member_state(self, m: int) -> np.ndarray:
        """The blob a standalone `DeviceGoalEnv` in member m's state would save, byte for byte."""
        if not 0 <= int(m) < self.members:
            raise ValueError(f"DeviceGoalEnvGroup.member_state: members: {m} outside [0, {self.members})")
        blob = self.save_state()
        per = (blob.size - self.HEADER_BYTES) // self.members
        return blob[self.HEADER_BYTES + int(m) * per:self.HEADER_BYTES + (int(m) + 1) * per].copy()


class DeviceGoalEnv:
    """`num_envs` envs of one kind and one seed: in the engine a one-member `DeviceGoalEnvGroup` (the same allocations, padded the
    same way; the views below cover the envs' own share of them)."""

    def __init__(self, kind: str, num_envs: int, seed: int = 0, max_steps: int = 50, threshold: float = 0.05, device_index: int = 0):
        if kind not in KINDS:
            raise ValueError(f"DeviceGoalEnv: kind: {kind!r} (one of {sorted(KINDS)})")
        self.kind, self.device_index = kind, int(device_index)
        self._h = _ffi.check_ptr(lib.gcrl_env_create(KINDS[kind], int(num_envs), int(seed) & (2**64 - 1), int(max_steps), float(threshold),
                                                     self.device_index), "gcrl_env_create")
        ints = [C.c_int() for _ in range(6)]
        thr, sd = C.c_float(), C.c_uint64()
        _ffi.check(lib.gcrl_env_dims(self._h, *[C.byref(x) for x in ints], C.byref(thr), C.byref(sd)))
        _, self.num_envs, self.obs_dim, self.goal_dim, self.ac_dim, self.max_steps = (int(x.value) for x in ints)
        self.threshold = float(thr.value)
        self._views = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.gcrl_env_destroy(h)

    @property
    def handle(self):
        return self._h

    @property
    def seed(self) -> int:
        sd = C.c_uint64()
        _ffi.check(lib.gcrl_env_dims(self._h, None, None, None, None, None, None, None, C.byref(sd)))
        return int(sd.value)

    # ------------------------------------------------------------------ views of the handle's device blocks
    def _blocks(self):
        if self._views is None:
            p = [C.c_void_p() for _ in range(3)]
            _ffi.check(lib.gcrl_env_buffers(self._h, *[C.byref(x) for x in p]))
            n, D, G = self.num_envs, self.obs_dim, self.goal_dim
            dev = f"cuda:{self.device_index}"
            self._views = (torch.as_tensor(_DevBlock(p[0].value, n * (D + G)), device=dev).view(n, D + G),
                           torch.as_tensor(_DevBlock(p[1].value, n * (2 * D + 4 * G)), device=dev),
                           torch.as_tensor(_DevBlock(p[2].value, n * PAY_W), device=dev).view(n, PAY_W))
        return self._views

    def acting_rows(self):
        """{"rows": [N, obs_dim + goal_dim] raw [obs | goal] rows of the NEXT step, "observation": ..., "desired_goal": ...}: views of
        the handle's memory, rewritten by every step."""
        rows = self._blocks()[0]
        return {"rows": rows, "observation": rows[:, :self.obs_dim], "desired_goal": rows[:, self.obs_dim:]}

    def step_blocks(self):
        """(raw, pay) of the LAST step in the layout `process_step_dev` takes: raw = [obs | next_obs | dg | next_dg | ag | next_ag] blocks,
        pay [N, 32] = t | reward | done | action(ac_dim) | next_ag.  `split_raw` cuts raw into its six [N, .] blocks."""
        return self._blocks()[1], self._blocks()[2]

    def split_raw(self, raw=None):
        raw = self._blocks()[1] if raw is None else raw
        n, D, G = self.num_envs, self.obs_dim, self.goal_dim
        out, o = [], 0
        for w in (D, D, G, G, G, G):
            out.append(raw[o:o + n * w].view(n, w))
            o += n * w
        return out

    # ------------------------------------------------------------------ stepping by hand
    def reset(self, mask=None):
        """No mask: every env back to its episode 0 and the counters to zero.  mask [N] bool (host): those envs go on to their next episode."""
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask).reshape(-1), np.uint8)
            if m.size != self.num_envs:
                raise ValueError(f"DeviceGoalEnv.reset: mask: {m.size} entries for {self.num_envs} envs")
        _ffi.check(lib.gcrl_env_reset(self._h, m.ctypes.data if m is not None else None, _ffi.stream_handle()))
        return self.acting_rows()

    def step(self, actions):
        """One vector step from a CUDA float32 or float64 tensor [N, ac_dim]; returns nothing: read `step_blocks()` / `acting_rows()`."""
        if not (isinstance(actions, torch.Tensor) and actions.is_cuda and actions.is_contiguous() and actions.dtype in (torch.float32, torch.float64)
                and tuple(actions.shape) == (self.num_envs, self.ac_dim)):
            raise ValueError(f"DeviceGoalEnv.step: actions: a contiguous CUDA float32 / float64 tensor [{self.num_envs}, {self.ac_dim}] required")
        _ffi.check(lib.gcrl_env_step(self._h, actions.data_ptr(), 1 if actions.dtype == torch.float64 else 0, _ffi.stream_handle()))

    def scripted_actions(self, noise_std: float = 0.0, seed: int = 0, counter: int = 0):
        """The `pick` or `glide` kind's scripted controller on the envs as they stand, one launch: a CUDA float32 tensor [N, ac_dim].
        `pick`: go to the object with open fingers, close them over it, carry it to the goal (tests/dev_env_pick_ref.py scripted_action
        is the definition).  `glide`: travel to a point behind the puck, descend, carry it while the goal is too far for one strike,
        strike it with the speed whose glide ends on the goal, and let go (tests/dev_env_glide_ref.py scripted_action).
        noise_std > 0 adds float32(float64(hash_normal(seed, (counter * N + env) * ac_dim + component)) * noise_std) before a final
        clamp to [-1, 1].  `reach` / `push` have no controller: refused naming `kind`."""
        if self.kind not in SCRIPTED:
            raise _ffi.GcrlError(f"DeviceGoalEnv.scripted_actions: kind: the 'pick' and 'glide' kinds alone have a scripted controller, this env is {self.kind!r}")
        out = torch.empty((self.num_envs, self.ac_dim), dtype=torch.float32, device=f"cuda:{self.device_index}")
        _ffi.check(lib.gcrl_env_scripted_act(self._h, out.data_ptr(), float(noise_std), int(seed) & (2**64 - 1), int(counter) & (2**64 - 1),
                                             _ffi.stream_handle()))
        return out

    def stats(self) -> dict:
        """Synchronises.  Episodes finished, episodes that ended within the threshold, reward sum — since the last full reset."""
        ep, su, rs = C.c_int64(), C.c_int64(), C.c_double()
        _ffi.check(lib.gcrl_env_stats(self._h, C.byref(ep), C.byref(su), C.byref(rs), _ffi.stream_handle()))
        return dict(episodes=int(ep.value), successes=int(su.value), reward_sum=float(rs.value))

    # ------------------------------------------------------------------ resume
    def save_state(self) -> np.ndarray:
        """State arrays, counters, acting rows and the seed as one uint8 array; `load_state` resumes bitwise."""
        n = int(lib.gcrl_env_state_bytes(self._h))
        blob = np.empty(n, np.uint8)
        _ffi.check(lib.gcrl_env_save_state(self._h, blob.ctypes.data, n, _ffi.stream_handle()))
        return blob

    def load_state(self, blob):
        """Refuses a state of another kind, num_envs, max_steps or threshold by that field's name before anything is overwritten."""
        blob = np.ascontiguousarray(blob, np.uint8)
        _ffi.check(lib.gcrl_env_load_state(self._h, blob.ctypes.data, blob.size, _ffi.stream_handle()))
