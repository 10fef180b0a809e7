"""Practice goals (csrc/goal_propose.hip) restated in numpy.  THIS FILE IS THE DEFINITION: the kernels are held to it bit for bit
(tests/test_gpu_goal_propose.py).

A proposer owns an archive: a circular buffer of `capacity` raw achieved goals, float32 [capacity][3] in the env's own units, never
normalised, with `head` (the physical slot of the oldest entry) and `len`.  Logical index j lives at slot (head + j) mod capacity.
It serves one numpy env of N envs (tests/dev_env_ref.py RefEnv, dev_env_pick_ref.py RefPickEnv, dev_env_glide_ref.py RefGlideEnv) and
has the settings candidates = C, radius, share, min_fill, seed, and a counter q: the number of roll-over steps seen so far.

After every vector step of the env (`after_step`, or `step_env` which does both):

  1. append    the step's N next_ag rows (the last block of the env's raw buffer; for an env that just finished, the finished
               episode's last achieved goal) go to logical positions len .. len + N - 1.  A full archive drops its oldest entries:
               head advances, len stays at capacity.
  2. propose   only in a step in which at least one env rolled over: its t was max_steps - 1 before the step.  An env put to t = 0
               by reset(mask) has not rolled over and keeps its task goal.  q is read, then incremented, whether or not anything is
               patched.  L = len after the append; L < min_fill patches nothing.  Otherwise every rolled-over env i
       take        takes a proposal iff float32(hash_below(seed, TAKE_STREAM, q N + i, 2^24)) * 2^-24 < float32(share); an env that
                   does not keeps the task goal the env's seed gave it;
       candidates  k = 0 .. C - 1: logical index j_k = hash_below(seed, CAND_STREAM, (q N + i) C + k, L);
       density     count_k = the number of entries m in [0, L) with d2(archive[m], archive[j_k]) < rho2, where
                   d2 = (dx dx + dy dy) + dz dz in float32, one rounding per operation, and rho2 = float32(radius) * float32(radius);
                   the candidate counts itself;
       choice      the smallest count wins, ties go to the smallest k;
       patch       the three float32 words of archive[j_best] become the env's goal: its state record's goal and the goal columns
                   of its acting row (the numpy envs derive their rows from `goal`).  The finished step's dg / next_dg keep the old
                   goal.

The counters (q N + i) and ((q N + i) C + k) are 64-bit and wrap.  Counts are integers: any split of the density sum is exact."""
import numpy as np

from oracle.her_oracle import hash_below

f32 = np.float32
M64 = (1 << 64) - 1
TAKE_STREAM = 0x5052414354414B45     # "PRACTAKE"
CAND_STREAM = 0x5052414343414E44     # "PRACCAND"


def takes(seed, q, n, i, share):
    h = hash_below(int(seed), TAKE_STREAM, (int(q) * int(n) + int(i)) & M64, 1 << 24)
    return bool(f32(f32(h) * f32(2.0 ** -24)) < f32(share))


def candidate_indices(seed, q, n, i, C, L):
    base = (int(q) * int(n) + int(i)) & M64
    return [hash_below(int(seed), CAND_STREAM, (base * int(C) + k) & M64, int(L)) for k in range(int(C))]


def density_counts(entries, cands, radius):
    """entries [L][3], cands [C][3] float32 -> int64 [C]: entries within the radius of each candidate (strictly)."""
    entries, cands = np.asarray(entries, f32), np.asarray(cands, f32)
    rho2 = f32(f32(radius) * f32(radius))
    d = (entries[:, None, :] - cands[None, :, :]).astype(f32)
    sq = (d * d).astype(f32)
    d2 = ((sq[:, :, 0] + sq[:, :, 1]).astype(f32) + sq[:, :, 2]).astype(f32)
    return (d2 < rho2).sum(axis=0).astype(np.int64)


class RefProposer:
    def __init__(self, capacity=8192, candidates=16, radius=0.05, share=0.5, min_fill=256, seed=0):
        self.cap, self.C, self.radius, self.share = int(capacity), int(candidates), f32(radius), f32(share)
        self.min_fill, self.seed = int(min_fill), int(seed) & M64
        self.arch = np.zeros((self.cap, 3), f32)          # physical slots
        self.head, self.len, self.q = 0, 0, 0
        self.appended, self.roll_steps, self.patched = 0, 0, 0
        self.last = []        # the decisions of the last propose: dict(env, took, js, counts, best) per rolled-over env

    def logical(self):
        return self.arch[(self.head + np.arange(self.len)) % self.cap].copy()

    def stats(self):
        return dict(appended=self.appended, roll_steps=self.roll_steps, patched=self.patched)

    def append(self, next_ag):
        next_ag = np.asarray(next_ag, f32).reshape(-1, 3)
        n = next_ag.shape[0]
        assert n <= self.cap
        for i in range(n):
            self.arch[(self.head + self.len + i) % self.cap] = next_ag[i]
        over = self.len + n - self.cap
        if over > 0:
            self.head, self.len = (self.head + over) % self.cap, self.cap
        else:
            self.len += n
        self.appended += n

    def after_step(self, env, next_ag, rolled):
        """next_ag [N][3] of the step just taken; rolled [N] bool: the env's t was max_steps - 1 before it."""
        n = env.n
        self.append(next_ag)
        self.last = []
        rolled = np.asarray(rolled, bool).reshape(n)
        if not rolled.any():
            return
        q = self.q
        self.q += 1
        self.roll_steps += 1
        L = self.len
        if L < self.min_fill:
            return
        entries = self.logical()
        for i in np.flatnonzero(rolled):
            rec = dict(env=int(i), took=takes(self.seed, q, n, i, self.share), js=None, counts=None, best=None)
            self.last.append(rec)
            if not rec["took"]:
                continue
            js = candidate_indices(self.seed, q, n, i, self.C, L)
            counts = density_counts(entries, entries[js], self.radius)
            best = int(np.argmin(counts))               # numpy's argmin returns the first minimum: ties go to the smallest k
            rec.update(js=js, counts=counts, best=best)
            env.goal[i] = entries[js[best]]
            self.patched += 1

    def step_env(self, env, actions):
        """One vector step of the numpy env followed by this proposer's step; returns the env's (raw, pay)."""
        rolled = env.t == env.T - 1
        raw, pay = env.step(actions)
        self.after_step(env, env.split(raw)[5], rolled)
        return raw, pay


def state_words(env):
    """[N][SW] float32: the env's state record as the device keeps it (p, q, vel, goal, then the kind's extras)."""
    if hasattr(env, "state_array"):
        return env.state_array()
    return np.concatenate([env.p, env.q, env.vel, env.goal], axis=1).astype(f32)
