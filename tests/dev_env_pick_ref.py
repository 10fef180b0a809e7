"""The third device-resident goal environment of csrc/dev_env.hip, `pick`, restated in numpy.  THIS FILE IS THE DEFINITION of the
kind, of the exploration streams at its action width and of its scripted controller (csrc/dev_env_script.hip): the kernels are held
to it bit for bit (tests/test_gpu_dev_env_pick.py), operation by operation.  The helpers and the constants the three kinds share
come from tests/dev_env_ref.py, whose arithmetic rules hold here unchanged: every value is float32, every operation is one
rounding, only + - * /, comparisons, min / max and the reward's one square root are used.

pick (D = 20, G = 3, A = 4): a gripper p with finger opening w and an object q that rests on the table z = 0.

    reset    q = (spawn(u0), spawn(u1), 0); p = (spawn(u2), spawn(u3), LIFT); w = OPEN; held = 0; every velocity 0
             goal.x = q.x -+ m with m = 2 thr + u4 (0.15 - 2 thr), the sign from u5 < 0.5 (push's construction: no episode starts solved)
             goal.y = spawn(u6); goal.z = max(spawn(u7), 0): half the goals lie on the table, half in the air
    action   4 components; a NaN component counts as 0; then clamp to [-1, 1]
    step     vel_p = STEP * a[0..2]; pn.xy = clamp_box(p.xy + vel_p.xy); pn.z = min(max(p.z + vel_p.z, 0), BOX)
             wn = min(max(w + FINGER * a[3], 0), OPEN); vel_w = wn - w
             d2 = sum_c (pn[c] - q[c])^2 in component order; near = d2 < CONTACT * CONTACT; closed = wn < CLOSE
             held' = closed if held else (near and closed and w >= CLOSE)        (a grasp: the fingers close while around the object)
             held':      qn = q + (pn - p) per component; x, y through clamp_box, z clamped to [0, BOX]
             not held':  near and closed: qn.xy = clamp_box(q.xy + (pn.xy - p.xy))   (a closed fist pushes, as `push`)
                         qn.z = max(q.z - FALL, 0)                                   (a released object falls)
             vel_q = qn - q
    obs      [p | q | q - p | vel_p | vel_q | w | vel_w | held | near(p, q) | t / T], near recomputed from the stored p and q
    ag = q; reward, success count at the horizon, re-seeding and the payload (t | r | 0 | action(4) | next_ag(3)) as the other kinds.

State record of an env (18 floats): p(3) q(3) vel_p(3) goal(3) w held vel_q(3) vel_w.

Scripted controller (scripted_action): held: move the object to the goal with the fingers closing; else go to the object with
the fingers open, and close them once the gripper is within 0.01 of it.
"""
import numpy as np

from dev_env_ref import BOX, CONTACT, EPS_STREAM, G, LIFT, PAY_W, SPAWN, STEP, RefEnv, clamp_box, reward_of, spawn, uniform01
from oracle.device_rng_oracle import hash_normal

f32 = np.float32
FINGER, OPEN, CLOSE, FALL = f32(0.02), f32(0.08), f32(0.04), f32(0.04)
REACHED = f32(f32(0.01) * f32(0.01))          # the controller closes the fingers below this squared distance
KIND, OBS_DIM, A, STATE_W = 2, 20, 4, 18
ZERO = f32(0.0)


def clean_action(a):
    a = np.asarray(a, f32)
    a = np.where(np.isnan(a), ZERO, a)
    return np.minimum(np.maximum(a, f32(-1.0)), f32(1.0)).astype(f32)


def clamp_z(x):
    return f32(min(max(f32(x), ZERO), BOX))


def dist2(a, b):
    d2 = ZERO
    for c in range(3):
        df = f32(a[c] - b[c])
        d2 = f32(d2 + f32(df * df))
    return d2


class RefPickEnv(RefEnv):
    """N `pick` envs with RefEnv's interface: `step(actions)` returns the raw / pay blocks the step kernel writes and leaves `rows`."""

    def __init__(self, num_envs, seed=0, max_steps=50, threshold=0.05):
        self.kind, self.n, self.seed, self.T, self.thr = "pick", int(num_envs), int(seed), int(max_steps), f32(threshold)
        assert f32(2.0) * self.thr <= SPAWN
        self.D = OBS_DIM
        n = self.n
        self.p = np.zeros((n, 3), f32); self.q = np.zeros((n, 3), f32); self.vel = np.zeros((n, 3), f32)
        self.goal = np.zeros((n, 3), f32); self.t = np.zeros(n, np.int32)
        self.w = np.zeros(n, f32); self.held = np.zeros(n, f32); self.vel_q = np.zeros((n, 3), f32); self.vel_w = np.zeros(n, f32)
        self.episode = np.zeros(n, np.uint64)
        self.episodes = np.zeros(n, np.uint64); self.successes = np.zeros(n, np.uint64); self.reward_sum = np.zeros(n, np.float64)
        self.reset()

    # -------------------------------------------------------------------------------------------- state
    def _seed_env(self, i):
        u = lambda c: uniform01(self.seed, i, self.episode[i], c)
        self.vel[i] = 0; self.vel_q[i] = 0; self.vel_w[i] = 0; self.t[i] = 0
        self.w[i] = OPEN; self.held[i] = 0
        self.q[i] = [spawn(u(0)), spawn(u(1)), ZERO]
        self.p[i] = [spawn(u(2)), spawn(u(3)), LIFT]
        two = f32(f32(2.0) * self.thr)
        m = f32(two + f32(u(4) * f32(SPAWN - two)))
        gx = f32(self.q[i, 0] - m) if u(5) < f32(0.5) else f32(self.q[i, 0] + m)
        self.goal[i] = [gx, spawn(u(6)), f32(max(spawn(u(7)), ZERO))]

    def ag(self, i):
        return self.q[i]

    def near(self, i):
        return dist2(self.p[i], self.q[i]) < f32(CONTACT * CONTACT)

    def obs(self, i):
        tt = f32(f32(self.t[i]) / f32(self.T))
        return np.concatenate([self.p[i], self.q[i], (self.q[i] - self.p[i]).astype(f32), self.vel[i], self.vel_q[i],
                               [self.w[i], self.vel_w[i], self.held[i], f32(1.0) if self.near(i) else ZERO, tt]]).astype(f32)

    def state_array(self):
        """[n][18]: the env's state records as the device keeps (and saves) them."""
        return np.concatenate([self.p, self.q, self.vel, self.goal, self.w[:, None], self.held[:, None], self.vel_q, self.vel_w[:, None]], axis=1).astype(f32)

    # -------------------------------------------------------------------------------------------- step
    def _move(self, i, a):
        p, q, w = self.p[i], self.q[i], self.w[i]
        vel = (STEP * a[:3]).astype(f32)
        pn = np.array([clamp_box(f32(p[0] + vel[0])), clamp_box(f32(p[1] + vel[1])), clamp_z(f32(p[2] + vel[2]))], f32)
        wn = f32(min(max(f32(w + f32(FINGER * a[3])), ZERO), OPEN))
        near = dist2(pn, q) < f32(CONTACT * CONTACT)
        closed = wn < CLOSE
        held = closed if self.held[i] != 0 else (near and closed and w >= CLOSE)
        qn = q.copy()
        if held:
            for c in range(3):
                qn[c] = f32(q[c] + f32(pn[c] - p[c]))
            qn[0], qn[1], qn[2] = clamp_box(qn[0]), clamp_box(qn[1]), clamp_z(qn[2])
        else:
            if near and closed:
                for c in range(2):
                    qn[c] = clamp_box(f32(q[c] + f32(pn[c] - p[c])))
            qn[2] = f32(max(f32(q[2] - FALL), ZERO))
        self.vel[i] = vel; self.vel_w[i] = f32(wn - w); self.vel_q[i] = (qn - q).astype(f32)
        self.p[i] = pn; self.q[i] = qn; self.w[i] = wn; self.held[i] = f32(1.0) if held else ZERO

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
            self._move(i, clean_action(actions[i]))
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


# ------------------------------------------------------------------------------------------------ exploration stream at A = 4
def _counters(c, n):
    return (np.uint64(c) * np.uint64(n) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)[None, :]


def explore_noise(seed, c, n, noise_std):
    """[n][4] float64: the Gaussian noise (DDPG / TD3) or the eps (SAC / TQC, noise_std = 1) of vector step c."""
    return hash_normal(seed, _counters(c, n)).astype(np.float64) * float(noise_std)


def epsilon_actions(seed, c, n):
    """[n][4] float32: the clipped normals every env takes on an epsilon step."""
    z = hash_normal(np.uint64(int(seed) ^ EPS_STREAM), _counters(c, n))
    return np.minimum(np.maximum(z, f32(-1.0)), f32(1.0)).astype(f32)


# ------------------------------------------------------------------------------------------------ scripted controller
def scripted_action(env, i):
    """[4] float32: the controller's action for env i of a RefPickEnv, before any noise."""
    a = np.zeros(A, f32)
    unit = lambda x: f32(min(max(f32(x), f32(-1.0)), f32(1.0)))
    if env.held[i] != 0:
        for c in range(3):
            a[c] = unit(f32(env.goal[i, c] - env.q[i, c]) / STEP)
        a[3] = f32(-1.0)
        return a
    d = (env.q[i] - env.p[i]).astype(f32)
    s = ZERO
    for c in range(3):
        s = f32(s + f32(d[c] * d[c]))
    if s < REACHED:
        a[3] = f32(-1.0)
    else:
        for c in range(3):
            a[c] = unit(f32(d[c]) / STEP)
        a[3] = f32(1.0)
    return a


def scripted_actions(env, noise_std=0.0, seed=0, c=0, normals=None):
    """[n][4] float32: every env's scripted action of vector step c; noise_std > 0 adds float32(float64(hash_normal(seed, (c n + i) 4 + j)) *
    noise_std) before a final clamp to [-1, 1].  normals: those hash values [n][4] float32 from elsewhere — the GPU tests take them from
    the device's own gcrl_hash_normal_fill, whose transcendental functions differ from numpy's by ulps (tests/test_device_rng.py)."""
    out = np.stack([scripted_action(env, i) for i in range(env.n)]).astype(f32)
    if noise_std:
        z = hash_normal(seed, _counters(c, env.n)) if normals is None else np.asarray(normals, f32).reshape(env.n, A)
        out = (out + (z.astype(np.float64) * float(noise_std)).astype(f32)).astype(f32)
        out = np.minimum(np.maximum(out, f32(-1.0)), f32(1.0)).astype(f32)
    return out
