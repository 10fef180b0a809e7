"""The two device-resident goal environments of csrc/dev_env.hip, restated in numpy.  THIS FILE IS THE DEFINITION: the
kernels are held to it bit for bit (tests/test_gpu_dev_env.py), operation by operation.

Every value is float32 and every operation is one rounding (the unit is built without contraction).  Only + - * /,
comparisons, min / max and one correctly rounded square root (the distance of the sparse reward, formed exactly as the replay
ring's relabelling kernels form it, so that a relabelled reward and the env's agree) are used.

Common to both kinds: G = 3, A = 3, horizon T = max_steps, reward = -(dist > thr) (-1.0 or -0.0), no termination on success.

    action   a NaN component counts as 0; then clamp to [-1, 1]                  (any bits in, a finite state out)
    vel    = 0.04 * a
    pos    = clamp(pos + vel, -0.3, 0.3)

reach (D = 7):   obs = [pos, vel, t / T], ag = pos.  Reset: pos, goal uniform in +-0.15 per component, vel = 0.
push  (D = 13):  pusher p, puck q with q.z = 0.  obs = [p, q, q - p, vel_p, t / T], ag = q.  The pusher moves as above.  When the NEW
                 pusher position is closer to the puck than CONTACT (squared distance compared with CONTACT * CONTACT), the puck's x
                 and y move by the pusher's actual displacement and are clamped to the box.  Reset: q.xy and p.xy uniform in
                 +-0.15, p.z = LIFT (above the contact radius: the pusher never starts in contact), goal.x = q.x +- m with
                 m = 2 thr + u (0.15 - 2 thr) (so |goal.x - q.x| >= 2 thr: no episode starts solved, no rejection loop), goal.y uniform
                 in +-0.15, goal.z = 0.

Random numbers: u(env, episode, component) = hash_below(seed, ENV_STREAM + env, 8 * episode + component, 2^24) * 2^-24 — the
replay ring's counter hash (csrc/her_ring.h, restated in oracle/her_oracle.py).  There is no state besides the counters: an
env's episode j is the same whatever N is and whenever it is reached.

Exploration stream of agent.collect (csrc/agent.hip): element (c, i, j) of vector step c is
float64(hash_normal(seed, (c N + i) A + j)) * noise_std; DDPG's epsilon uniform of step c is
hash_below(seed, EPS_STREAM, c, 2^24) * 2^-24 (float64), and below 0.2 every env takes clip(hash_normal(seed ^ EPS_STREAM, (c N + i) A + j), -1, 1).
"""
import numpy as np

from oracle.device_rng_oracle import hash_normal
from oracle.her_oracle import hash_below

f32 = np.float32
ENV_STREAM = 0x4445562D454E5621      # "DEV-ENV!"
EPS_STREAM = 0x455053494C4F4E21      # "EPSILON!"
STEP, BOX, SPAWN = f32(0.04), f32(0.3), f32(0.15)
CONTACT, LIFT = f32(0.05), f32(0.1)
KINDS = {"reach": 0, "push": 1}
OBS_DIM = {"reach": 7, "push": 13}
G = A = 3
PAY_W = 32                           # floats per env of the payload block (csrc/her_ring.hip kPayW)


def uniform01(seed, env, episode, comp):
    return f32(hash_below(int(seed), (ENV_STREAM + int(env)) & 0xFFFFFFFFFFFFFFFF, 8 * int(episode) + comp, 1 << 24)) * f32(2.0 ** -24)


def spawn(u):
    return (u * f32(2.0) - f32(1.0)) * SPAWN


def clean_action(a):
    a = np.asarray(a, f32)
    a = np.where(np.isnan(a), f32(0.0), a)
    return np.minimum(np.maximum(a, f32(-1.0)), f32(1.0)).astype(f32)


def clamp_box(x):
    return np.minimum(np.maximum(x, -BOX), BOX).astype(f32)


def reward_of(ag, goal, thr):
    """-(||ag - goal|| > thr): squares summed in component order, one rounding per operation."""
    acc = f32(0.0)
    for q in range(G):
        df = f32(ag[q] - goal[q])
        acc = f32(acc + f32(df * df))
    dist = np.sqrt(acc, dtype=f32)
    return (f32(-1.0) if dist > thr else f32(-0.0)), dist


class RefEnv:
    """N envs; `step(actions)` returns the raw / pay blocks the step kernel writes and leaves `rows` (the next acting rows)."""

    def __init__(self, kind, num_envs, seed=0, max_steps=50, threshold=0.05):
        assert kind in KINDS
        self.kind, self.n, self.seed, self.T, self.thr = kind, int(num_envs), int(seed), int(max_steps), f32(threshold)
        self.D = OBS_DIM[kind]
        n = self.n
        self.p = np.zeros((n, 3), f32); self.q = np.zeros((n, 3), f32); self.vel = np.zeros((n, 3), f32)
        self.goal = np.zeros((n, 3), f32); self.t = np.zeros(n, np.int32)
        self.episode = np.zeros(n, np.uint64)
        self.episodes = np.zeros(n, np.uint64); self.successes = np.zeros(n, np.uint64); self.reward_sum = np.zeros(n, np.float64)
        self.reset()

    # -------------------------------------------------------------------------------------------- state
    def _seed_env(self, i):
        u = lambda c: uniform01(self.seed, i, self.episode[i], c)
        self.vel[i] = 0; self.t[i] = 0
        if self.kind == "reach":
            self.p[i] = [spawn(u(0)), spawn(u(1)), spawn(u(2))]
            self.q[i] = 0
            self.goal[i] = [spawn(u(3)), spawn(u(4)), spawn(u(5))]
        else:
            self.q[i] = [spawn(u(0)), spawn(u(1)), f32(0.0)]
            self.p[i] = [spawn(u(2)), spawn(u(3)), LIFT]
            two = f32(f32(2.0) * self.thr)
            m = f32(two + f32(u(4) * f32(SPAWN - two)))
            gx = f32(self.q[i, 0] - m) if u(5) < f32(0.5) else f32(self.q[i, 0] + m)
            self.goal[i] = [gx, spawn(u(6)), f32(0.0)]

    def reset(self, mask=None):
        """mask None: every env back to its episode 0 and the counters to zero; else the selected envs go on to their next episode
        (not counted)."""
        for i in range(self.n):
            if mask is None:
                self.episode[i] = 0; self.episodes[i] = 0; self.successes[i] = 0; self.reward_sum[i] = 0.0
            elif mask[i]:
                self.episode[i] += np.uint64(1)
            else:
                continue
            self._seed_env(i)

    def ag(self, i):
        return self.p[i] if self.kind == "reach" else self.q[i]

    def obs(self, i):
        tt = f32(f32(self.t[i]) / f32(self.T))
        if self.kind == "reach":
            return np.concatenate([self.p[i], self.vel[i], [tt]]).astype(f32)
        return np.concatenate([self.p[i], self.q[i], (self.q[i] - self.p[i]).astype(f32), self.vel[i], [tt]]).astype(f32)

    @property
    def rows(self):
        return np.stack([np.concatenate([self.obs(i), self.goal[i]]) for i in range(self.n)]).astype(f32)

    def state_dict(self):
        return {"observation": np.stack([self.obs(i) for i in range(self.n)]), "achieved_goal": np.stack([self.ag(i).copy() for i in range(self.n)]),
                "desired_goal": self.goal.copy()}

    # -------------------------------------------------------------------------------------------- step
    def step(self, actions):
        n, D = self.n, self.D
        actions = np.asarray(actions, f32).reshape(n, A)
        raw = np.zeros(n * (2 * D + 4 * G), f32)
        pay = np.zeros((n, PAY_W), f32)
        o_obs, o_nobs, o_dg = 0, n * D, 2 * n * D
        o_ndg, o_ag, o_nag = o_dg + n * G, o_dg + 2 * n * G, o_dg + 3 * n * G
        for i in range(n):
            raw[o_obs + i * D:o_obs + (i + 1) * D] = self.obs(i)
            raw[o_dg + i * G:o_dg + (i + 1) * G] = self.goal[i]
            raw[o_ndg + i * G:o_ndg + (i + 1) * G] = self.goal[i]
            raw[o_ag + i * G:o_ag + (i + 1) * G] = self.ag(i)
            a = clean_action(actions[i])
            vel = (STEP * a).astype(f32)
            p_new = clamp_box((self.p[i] + vel).astype(f32))
            if self.kind == "push":
                d2 = f32(0.0)
                for c in range(3):
                    df = f32(p_new[c] - self.q[i, c])
                    d2 = f32(d2 + f32(df * df))
                if d2 < f32(CONTACT * CONTACT):
                    for c in range(2):
                        self.q[i, c] = clamp_box(f32(self.q[i, c] + f32(p_new[c] - self.p[i, c])))
            self.p[i] = p_new; self.vel[i] = vel
            pay[i, 0] = np.int32(self.t[i]).view(f32)
            self.t[i] += 1
            raw[o_nobs + i * D:o_nobs + (i + 1) * D] = self.obs(i)
            raw[o_nag + i * G:o_nag + (i + 1) * G] = self.ag(i)
            r, dist = reward_of(self.ag(i), self.goal[i], self.thr)
            pay[i, 1] = r; pay[i, 2] = 0.0
            pay[i, 3:3 + A] = actions[i]
            pay[i, 3 + A:3 + A + G] = self.ag(i)
            self.reward_sum[i] += float(r)
            if self.t[i] == self.T:
                self.episodes[i] += np.uint64(1)
                if dist < self.thr:
                    self.successes[i] += np.uint64(1)
                self.episode[i] += np.uint64(1)
                self._seed_env(i)
        return raw, pay

    def split(self, raw):
        """The six blocks of `raw` as [n][.] arrays: obs, next_obs, dg, next_dg, ag, next_ag."""
        n, D = self.n, self.D
        cuts = np.cumsum([0, n * D, n * D, n * G, n * G, n * G, n * G])
        widths = [D, D, G, G, G, G]
        return [raw[cuts[k]:cuts[k + 1]].reshape(n, widths[k]) for k in range(6)]

    def stats(self):
        return dict(episodes=int(self.episodes.sum()), successes=int(self.successes.sum()), reward_sum=float(self.reward_sum.sum()))


# ------------------------------------------------------------------------------------------------ exploration stream
def explore_noise(seed, c, n, noise_std):
    """[n][A] float64: the Gaussian noise (DDPG / TD3) or the eps (SAC / TQC, noise_std = 1) of vector step c."""
    ctr = (np.uint64(c) * np.uint64(n) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)[None, :]
    return hash_normal(seed, ctr).astype(np.float64) * float(noise_std)


def epsilon_uniform(seed, c):
    return float(hash_below(int(seed), EPS_STREAM, int(c), 1 << 24)) * 2.0 ** -24


def epsilon_actions(seed, c, n):
    """[n][A] float32: the clipped normals every env takes on an epsilon step."""
    ctr = (np.uint64(c) * np.uint64(n) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)[None, :]
    z = hash_normal(np.uint64(int(seed) ^ EPS_STREAM), ctr)
    return np.minimum(np.maximum(z, f32(-1.0)), f32(1.0)).astype(f32)
