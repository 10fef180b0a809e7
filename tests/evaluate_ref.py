"""The evaluation rule of agent.evaluate / pop.evaluate (csrc/agent.hip gcrl_agent_evaluate, csrc/agent_pop.inc gcrl_pop_evaluate)
and the group rule of gcrl_amd.DeviceGoalEnvGroup, restated in numpy over tests/dev_env_ref.py.

    evaluate(env, policy, episodes, reset)   runs ceil(episodes / N) * T vector steps of `policy` on the env.  An episode is counted
                                             when an env's t reaches T; it is a success when dist < thr at that last step (the
                                             env's own counters).  reset=True: a full reset first, so episodes 0, 1, ... of the
                                             env's seed are scored.  reset=False: every env must stand at t == 0 (ValueError naming
                                             `t` otherwise) and the counters' difference over the call is reported.
    RefGroup(kind, P, N, seeds, ...)         member m IS RefEnv(kind, N, seeds[m], ...): P independent definitions, nothing shared.
"""
import numpy as np

import dev_env_ref as E


def evaluate(env, policy, episodes, reset=True):
    """policy(state_dict) -> actions [N, 3].  Returns dict(episodes, successes, success_rate, reward_sum)."""
    if int(episodes) < 1:
        raise ValueError("episodes: >= 1 required")
    if reset:
        env.reset()
    elif np.any(env.t != 0):
        i = int(np.flatnonzero(env.t != 0)[0])
        raise ValueError(f" t: env {i} is at step {int(env.t[i])} of its episode")
    before = env.stats()
    rounds = -(-int(episodes) // env.n)
    for _ in range(rounds * env.T):
        env.step(np.asarray(policy(env.state_dict()), E.f32))
    after = env.stats()
    n = after["episodes"] - before["episodes"]
    su = after["successes"] - before["successes"]
    return dict(episodes=n, successes=su, success_rate=su / n if n else 0.0, reward_sum=after["reward_sum"] - before["reward_sum"])


def proportional(state):
    """the controller that walks the achieved goal onto the desired one: reach's point mass gets there within an episode"""
    return np.clip((state["desired_goal"] - state["achieved_goal"]) / E.STEP, -1, 1).astype(E.f32)


def idle(state):
    return np.zeros_like(state["desired_goal"])


class RefGroup:
    def __init__(self, kind, members, num_envs, seeds, max_steps=50, threshold=0.05):
        seeds = list(seeds)
        assert len(seeds) == members
        self.envs = [E.RefEnv(kind, num_envs, seed=s, max_steps=max_steps, threshold=threshold) for s in seeds]

    def step(self, actions):
        """actions [P, N, 3] -> the members' (raw, pay) pairs"""
        return [e.step(a) for e, a in zip(self.envs, actions)]

    def reset(self, mask=None, members=None):
        if members is not None:
            for m in members:
                self.envs[m].reset(np.ones(self.envs[m].n, bool))
        else:
            for m, e in enumerate(self.envs):
                e.reset(None if mask is None else np.asarray(mask).reshape(len(self.envs), -1)[m])

    def stats(self):
        return [e.stats() for e in self.envs]
