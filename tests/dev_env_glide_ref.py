"""The fourth device-resident goal environment of csrc/dev_env.hip, `glide`, restated in numpy.  THIS FILE IS THE DEFINITION of the
kind and of its scripted controller (csrc/dev_env_script.hip): the kernels are held to it bit for bit
(tests/test_gpu_dev_env_glide.py), operation by operation.  The helpers and the constants the kinds share come from
tests/dev_env_ref.py, whose arithmetic rules hold here unchanged: every value is float32, every operation is one rounding, only
+ - * /, comparisons, min / max and correctly rounded square roots are used (the reward's, and three in the controller).

glide (D = 16, G = 3, A = 3): a pusher p and a puck q on the table z = 0 that keeps moving after it is struck; the goals lie
beyond the pusher's box, so the puck has to be given a velocity and let go.  (The name `slide` stays refused as an unknown kind.)

    reset    q = (spawn(u0), spawn(u1), 0); p = (spawn(u2), spawn(u3), LIFT); vel_p = vel_q = 0
             goal = (0.45 + u4 * 0.2, spawn(u5), 0)            goal.x in [0.45, 0.65]: at least 0.15 beyond the pusher's box
    action   3 components; a NaN component counts as 0; then clamp to [-1, 1]
    step     vel_p = STEP * a; pn = clamp_box(p + vel_p) per component
             contact = sum_c (pn[c] - q[c])^2 (component order) < CONTACT * CONTACT
             d.xy = pn.xy - p.xy if contact else FRICTION * vel_q.xy      a touched puck takes the pusher's displacement, a free one glides
             qn.x = min(max(q.x + d.x, -BOX), FAR); qn.y = clamp_box(q.y + d.y); qn.z = 0
             vel_q = qn - q  (a wall stops that component); q = qn; p = pn
    obs      [p | q | q - p | vel_p | vel_q | t / T]
    ag = q; reward, success count at the horizon, re-seeding, counters and the payload (t | r | 0 | action(3) | next_ag(3)) as push.

After a contact step q.x < 0.39 (the pusher is inside its box, the puck inside the contact radius, the displacement at most STEP)
and a goal has x >= 0.45, so with a threshold of 0.05 no episode ends solved while the pusher touches the puck.

State record of an env (15 floats): p(3) q(3) vel_p(3) goal(3) vel_q(3).

Scripted controller (scripted_action; stateless; it reads p, q, vel_q, goal and the threshold), with u the unit vector from the puck to the goal,
L that distance and rest = |vel_q| FRICTION / (1 - FRICTION) the way the puck still glides by itself:

    L < 1e-6                            a = 0
    rest >= L - 0.5 thr                 a = (-u.x, -u.y, 0)                       hands off: the puck will arrive by itself
    b = q.xy - 0.03 u; e = b - p.xy; off = e.x^2 + e.y^2                          b: the striking position behind the puck
    off > 0.005^2:  p.z < LIFT - 0.005 and off > 0.02^2:  a = (0, 0, unit((LIFT - p.z) / STEP))          rise before travelling
                    else a.xy = unit(e / STEP); a.z = unit(((LIFT if off > 0.02^2 else 0) - p.z) / STEP)
    p.z > 0.005:    a.xy = unit(e / STEP); a.z = unit(-p.z / STEP)                descend behind the puck
    else            v = STEP if L > 0.9 (STEP / (1 - FRICTION)) else L (1 - FRICTION); a.xy = unit(u v / STEP); a.z = 0

The last line carries the puck at full speed while the goal is too far for one strike, then strikes once with the speed whose glide,
v / (1 - FRICTION), ends on the goal.
"""
import numpy as np

from dev_env_ref import A, BOX, CONTACT, G, LIFT, PAY_W, STEP, RefEnv, clamp_box, clean_action, reward_of, spawn, uniform01
from oracle.device_rng_oracle import hash_normal

f32 = np.float32
FRICTION, FAR = f32(0.9), f32(0.9)
KIND, OBS_DIM, STATE_W = 3, 16, 15
ZERO, ONE = f32(0.0), f32(1.0)
GOAL_X0, GOAL_DX = f32(0.45), f32(0.2)
# the controller's constants, each formed in float32
ONE_MINUS_F = f32(ONE - FRICTION)
BEHIND = f32(0.03)                                  # the striking position lies this far behind the puck
NEAR2 = f32(f32(0.005) * f32(0.005))                # within this squared distance of it the pusher is in place
AWAY2 = f32(f32(0.02) * f32(0.02))                  # beyond this one it travels at LIFT
SLACK = f32(0.005)
CARRY = f32(f32(0.9) * f32(STEP / ONE_MINUS_F))     # beyond this distance one strike cannot reach the goal
TINY = f32(1e-6)


def sqrt32(x):
    return np.sqrt(f32(x), dtype=f32)


class RefGlideEnv(RefEnv):
    """N `glide` envs with RefEnv's interface: `step(actions)` returns the raw / pay blocks the step kernel writes and leaves `rows`."""

    def __init__(self, num_envs, seed=0, max_steps=50, threshold=0.05):
        self.kind, self.n, self.seed, self.T, self.thr = "glide", int(num_envs), int(seed), int(max_steps), f32(threshold)
        self.D = OBS_DIM
        n = self.n
        self.p = np.zeros((n, 3), f32); self.q = np.zeros((n, 3), f32); self.vel = np.zeros((n, 3), f32)
        self.goal = np.zeros((n, 3), f32); self.vel_q = np.zeros((n, 3), f32); self.t = np.zeros(n, np.int32)
        self.episode = np.zeros(n, np.uint64)
        self.episodes = np.zeros(n, np.uint64); self.successes = np.zeros(n, np.uint64); self.reward_sum = np.zeros(n, np.float64)
        # what the last step did, per env (the tests' coverage checks): contact, a clamp at FAR, a clamp in y
        self.contact = np.zeros(n, bool); self.hit_far = np.zeros(n, bool); self.hit_y = np.zeros(n, bool)
        self.reset()

    # -------------------------------------------------------------------------------------------- state
    def _seed_env(self, i):
        u = lambda c: uniform01(self.seed, i, self.episode[i], c)
        self.vel[i] = 0; self.vel_q[i] = 0; self.t[i] = 0
        self.q[i] = [spawn(u(0)), spawn(u(1)), ZERO]
        self.p[i] = [spawn(u(2)), spawn(u(3)), LIFT]
        self.goal[i] = [f32(GOAL_X0 + f32(u(4) * GOAL_DX)), spawn(u(5)), ZERO]

    def ag(self, i):
        return self.q[i]

    def obs(self, i):
        tt = f32(f32(self.t[i]) / f32(self.T))
        return np.concatenate([self.p[i], self.q[i], (self.q[i] - self.p[i]).astype(f32), self.vel[i], self.vel_q[i], [tt]]).astype(f32)

    def state_array(self):
        """[n][15]: the env's state records as the device keeps (and saves) them."""
        return np.concatenate([self.p, self.q, self.vel, self.goal, self.vel_q], axis=1).astype(f32)

    # -------------------------------------------------------------------------------------------- step
    def _move(self, i, a):
        p, q, vq = self.p[i], self.q[i], self.vel_q[i]
        vel = (STEP * a).astype(f32)
        pn = clamp_box((p + vel).astype(f32))
        d2 = ZERO
        for c in range(3):
            df = f32(pn[c] - q[c])
            d2 = f32(d2 + f32(df * df))
        contact = bool(d2 < f32(CONTACT * CONTACT))
        dx = f32(pn[0] - p[0]) if contact else f32(FRICTION * vq[0])
        dy = f32(pn[1] - p[1]) if contact else f32(FRICTION * vq[1])
        fx, fy = f32(q[0] + dx), f32(q[1] + dy)
        qn = np.array([min(max(fx, -BOX), FAR), clamp_box(fy), ZERO], f32)
        self.contact[i], self.hit_far[i], self.hit_y[i] = contact, fx > FAR, abs(fy) > BOX
        self.vel[i] = vel; self.vel_q[i] = (qn - q).astype(f32)
        self.p[i] = pn; self.q[i] = qn

    def step(self, actions):
        n, D = self.n, self.D
        actions = np.asarray(actions, f32).reshape(n, A)
        raw = np.zeros(n * (2 * D + 4 * G), f32)
        pay = np.zeros((n, PAY_W), f32)
        o_obs, o_nobs, o_dg = 0, n * D, 2 * n * D
        o_ndg, o_ag, o_nag = o_dg + n * G, o_dg + 2 * n * G, o_dg + 3 * n * G
        self.reseeded = np.zeros(n, bool)
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
                self.reseeded[i] = True
        return raw, pay


# ------------------------------------------------------------------------------------------------ scripted controller
def _counters(c, n):
    return (np.uint64(c) * np.uint64(n) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)[None, :]


def unit(x):
    return f32(min(max(f32(x), f32(-1.0)), ONE))


def scripted_action(env, i):
    """[3] float32: the controller's action for env i of a RefGlideEnv, before any noise."""
    a = np.zeros(A, f32)
    p, q, vq, goal = env.p[i], env.q[i], env.vel_q[i], env.goal[i]
    dx, dy = f32(goal[0] - q[0]), f32(goal[1] - q[1])
    L = sqrt32(f32(f32(dx * dx) + f32(dy * dy)))
    if L < TINY:
        return a
    ux, uy = f32(dx / L), f32(dy / L)
    sp = sqrt32(f32(f32(vq[0] * vq[0]) + f32(vq[1] * vq[1])))
    rest = f32(f32(sp * FRICTION) / ONE_MINUS_F)
    if rest >= f32(L - f32(f32(0.5) * env.thr)):
        a[0], a[1] = unit(-ux), unit(-uy)            # (a rounded quotient may exceed 1 by an ulp: every action lies in [-1, 1])
        return a
    ex = f32(f32(q[0] - f32(BEHIND * ux)) - p[0])
    ey = f32(f32(q[1] - f32(BEHIND * uy)) - p[1])
    off = f32(f32(ex * ex) + f32(ey * ey))
    if off > NEAR2:
        if p[2] < f32(LIFT - SLACK) and off > AWAY2:
            a[2] = unit(f32(LIFT - p[2]) / STEP)
        else:
            a[0], a[1] = unit(ex / STEP), unit(ey / STEP)
            a[2] = unit(f32((LIFT if off > AWAY2 else ZERO) - p[2]) / STEP)
    elif p[2] > SLACK:
        a[0], a[1] = unit(ex / STEP), unit(ey / STEP)
        a[2] = unit(f32(ZERO - p[2]) / STEP)
    else:
        v = STEP if L > CARRY else f32(L * ONE_MINUS_F)
        a[0], a[1] = unit(f32(ux * v) / STEP), unit(f32(uy * v) / STEP)
    return a


def scripted_actions(env, noise_std=0.0, seed=0, c=0, normals=None):
    """[n][3] float32: every env's scripted action of vector step c; noise_std > 0 adds float32(float64(hash_normal(seed, (c n + i) 3 + j)) *
    noise_std) before a final clamp to [-1, 1].  normals: those hash values [n][3] float32 from elsewhere — the GPU tests take them from
    the device's own gcrl_hash_normal_fill, whose transcendental functions differ from numpy's by ulps (tests/test_device_rng.py)."""
    out = np.stack([scripted_action(env, i) for i in range(env.n)]).astype(f32)
    if noise_std:
        z = hash_normal(seed, _counters(c, env.n)) if normals is None else np.asarray(normals, f32).reshape(env.n, A)
        out = (out + (z.astype(np.float64) * float(noise_std)).astype(f32)).astype(f32)
        out = np.minimum(np.maximum(out, f32(-1.0)), ONE).astype(f32)
    return out
