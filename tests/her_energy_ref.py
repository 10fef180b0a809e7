"""CPU restatement (numpy, float32) of the energy-prioritised replay draw of a sample-mode HER ring
(HERBuffer(relabel="sample", prioritise="energy"); csrc/her_prio.hip).  The mode is DEFINED by this file; the GPU tests hold the
kernels to it bit for bit where the arithmetic is adds, multiplies, a divide and compares, and within 1e-6 relative where a `powf`
is involved (alpha != 1).  The tree, its reduction order and the descent are tests/per_tree_ref.py's.

Idea (Zhao & Tresp, "Energy-Based Hindsight Experience Prioritization", CoRL 2018): an episode is drawn in proportion to the
energy its achieved-goal trajectory GAINED, a row uniformly inside its episode.  Nothing feeds back from the loss and no
importance-sampling weights are used.  The default constants below are this project's choice (m = 1, g = 9.81, dt = 0.04), not a
claim about anybody's published settings.

Episode energy.  Achieved goals ag_0 .. ag_{T-1} (float32, G components, T <= 64), every operation one float32 rounding, the sum
over the components in order, no contraction:
    kin_0 = 0;  kin_i = kinetic * sum_c (ag_i[c] - ag_{i-1}[c])^2
    pot_i = potential * ag_i[axis]          (0 when axis < 0)
    E_i   = pot_i + kin_i
    e_0   = 0;  e_i = fmin(fmax(E_i - E_{i-1}, 0), clip)      (fmaxf / fminf: a NaN difference counts as 0, +inf as clip)
    E_traj = per_tree_ref.reduce64([e_0 .. e_{T-1}, 0, ...])  (the xor-butterfly over 64 lanes)
    p_ep  = (E_traj + eps)^alpha;  alpha == 1: p_ep = E_traj + eps exactly, no powf
    leaf  = p_ep / T  for every row of the episode the flush wrote (T = the episode's full length, also when a too-small ring
            skipped some of its rows)
Never-filled slots hold 0 and are never drawn; a row evicted by a later flush has its leaf overwritten by that flush.

Draw.  For the c-th row ever drawn from the ring in this mode (prio_ctr, a 64-bit counter the host advances by the rows of each
launch): slot = per_tree_ref.descend(levels, seed, c >> 20, c & 0xFFFFF), i.e. the uniform of level k is keyed by (c << 3) + k;
logical index = (slot - head) mod cap.  Counters are per row: one launch of n * B rows equals n launches of B.  With replacement.
"""
import numpy as np

import per_tree_ref as PT

F32 = np.float32
MAX_T = 64
DEFAULTS = dict(potential=9.81, kinetic=312.5, axis=None, clip=0.5, alpha=1.0, eps=1e-3)


def config(G: int, **kw):
    """The energy configuration as the ring holds it (float32 values; axis = 2 when G >= 3, else -1, unless given)."""
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    c = dict(DEFAULTS)
    c.update({k: v for k, v in kw.items() if v is not None})
    if c["axis"] is None:
        c["axis"] = 2 if G >= 3 else -1
    c["axis"] = int(c["axis"])
    assert c["axis"] < G
    for k in ("potential", "kinetic", "clip", "alpha", "eps"):
        c[k] = F32(c[k])
    return c


def gains(ag, cfg):
    """[T, G] float32 -> e [T] float32, every e_i in [0, clip]"""
    ag = np.asarray(ag, F32)
    T, G = ag.shape
    assert 1 <= T <= MAX_T
    E = np.zeros(T, F32)
    with np.errstate(all="ignore"):
        for i in range(T):
            acc = F32(0.0)
            if i > 0:
                for c in range(G):
                    df = F32(ag[i, c] - ag[i - 1, c])
                    acc = F32(acc + F32(df * df))
            kin = F32(cfg["kinetic"] * acc) if i > 0 else F32(0.0)
            pot = F32(cfg["potential"] * ag[i, cfg["axis"]]) if cfg["axis"] >= 0 else F32(0.0)
            E[i] = F32(pot + kin)
        e = np.zeros(T, F32)
        for i in range(1, T):
            e[i] = np.fmin(np.fmax(F32(E[i] - E[i - 1]), F32(0.0)), cfg["clip"])
    return e


def trajectory_energy(ag, cfg):
    lanes = np.zeros(PT.FAN, F32)
    e = gains(ag, cfg)
    lanes[:e.size] = e
    return PT.reduce64(lanes)[0]


def episode_priority(ag, cfg):
    """-> p_ep float32 (alpha == 1: exact; otherwise numpy's float32 power, which the device is NOT held to bit for bit)"""
    x = F32(trajectory_energy(ag, cfg) + cfg["eps"])
    return x if cfg["alpha"] == F32(1.0) else F32(np.power(x, cfg["alpha"]))


def episode_priority64(ag, cfg):
    """(E_traj + eps)^alpha in float64 from the float32 E_traj: what a powf result is held to within 1e-6 relative"""
    return (float(trajectory_energy(ag, cfg)) + float(cfg["eps"])) ** float(cfg["alpha"])


def leaf(ag, cfg):
    return F32(episode_priority(ag, cfg) / F32(np.asarray(ag).shape[0]))


def leaf64(ag, cfg):
    return episode_priority64(ag, cfg) / float(np.asarray(ag).shape[0])


def draw_slots(levels, seed: int, ctr: int, n: int):
    """rows ctr .. ctr + n - 1 of the ring's draw stream -> physical slots int64 [n]"""
    c = (np.uint64(ctr) + np.arange(n, dtype=np.uint64))
    slots, _ = PT.descend(levels, seed, c >> np.uint64(20), c & np.uint64(0xFFFFF))
    return slots


def draw(levels, seed: int, ctr: int, n: int, head: int, cap: int):
    """-> logical indices uint32 [n]"""
    return ((draw_slots(levels, seed, ctr, n) - head) % cap).astype(np.uint32)


class RefEnergyRing:
    """The ring's bookkeeping (deque(maxlen) semantics, FIFO eviction, one flush launch of up to 8 episodes appended contiguously)
    with the leaves an energy tree holds for it.  `leaf_fn`: leaf (bitwise for alpha == 1) or leaf64."""

    def __init__(self, cap: int, G: int, seed: int = 0, leaf_fn=leaf, **energy):
        self.cap, self.seed, self.cfg, self.leaf_fn = int(cap), int(seed), config(G, **energy), leaf_fn
        self.leaves = np.zeros(PT.level_sizes(cap)[0][1], np.float64 if leaf_fn is leaf64 else F32)
        self.episode_of = np.full(self.cap, -1, np.int64)       # per slot: number of the episode whose row lies there
        self.p_ep = []                                          # per episode number: leaf * T
        self.head = self.len = 0
        self.ctr = 0

    def flush(self, episodes):
        """`episodes`: the achieved goals [T, G] of the episodes of ONE flush launch, in launch order"""
        total = sum(np.asarray(a).shape[0] for a in episodes)
        skip = max(0, total - self.cap)
        tail = (self.head + self.len) % self.cap
        g = 0
        for ag in episodes:
            ag = np.asarray(ag, F32)
            v = self.leaf_fn(ag, self.cfg)
            self.p_ep.append(float(v) * ag.shape[0])
            for _ in range(ag.shape[0]):
                if g >= skip:
                    self.leaves[(tail + g) % self.cap] = v
                    self.episode_of[(tail + g) % self.cap] = len(self.p_ep) - 1
                g += 1
        newlen = self.len + total
        if newlen > self.cap:
            self.head = (self.head + newlen - self.cap) % self.cap
            newlen = self.cap
        self.len = newlen

    def levels(self):
        return PT.build(self.leaves.astype(F32))

    def priorities(self):
        """leaves in logical order"""
        return self.leaves[(self.head + np.arange(self.len)) % self.cap].copy()

    def draw(self, n: int):
        out = draw(self.levels(), self.seed, self.ctr, n, self.head, self.cap)
        self.ctr += n
        return out
