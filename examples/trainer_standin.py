#!/usr/bin/env python3
"""Stand-in for the reference trainer's HER loop: the calls `GoalEnvHER._train_her` makes
(reference src/env.py:334-406, `_process_step` :163-201, `_push_to_buffer` :203-232), in the same
order, against a synthetic vectorised goal environment — panda-gym is not installable here, and the
trainer itself is outside the hot path.  What it exercises end to end:

    normalize_state_batch -> select_action -> env.step -> update_normalizers
        -> HERBuffer.push_batch (all envs of a step in one call; episode flush + HER relabel on device)
        -> every `max_episode` episodes: agent.update_many(gradient_step)

and what it reports: success rate per cycle (does it learn?), env steps/s, gradient steps/s.

    python examples/trainer_standin.py --agent DDPG --cycles 60

--device-env reach|push|pick|glide runs the same cycle with the environment on the device (gcrl_amd.DeviceGoalEnv) and `agent.collect` in
place of the Python loop: acting, the env's step and _process_step are three launches per vector step and nothing crosses to the host.
`pick` has the dimensions of PandaPickAndPlace (state 23, action 4); with it --prior-episodes fills the prior ring on the device too,
from the env's scripted controller (HERBuffer.collect_scripted on a second DeviceGoalEnv of another seed).  `glide` (state 19, action 3:
a puck that has to be struck towards goals out of the pusher's reach) has its controller too and fills the prior ring the same way.
With --bc-weight the agent
runs the layer-per-launch schedule, which `collect` does not serve: its actions then come from `observe_act`, while the env's step and
`process_step_dev` stay on the device.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class PointReachVecEnv:
    """`num_envs` point masses in a box; dict observations shaped like panda-gym's Reach task with the
    reference's time feature appended (src/utils.py:137-174): observation = [pos, vel, t/T]."""

    def __init__(self, num_envs, dim=3, max_steps=50, threshold=0.05, seed=0):
        self.n, self.dim, self.T, self.thr = num_envs, dim, max_steps, threshold
        self.gen = np.random.default_rng(seed)
        self.obs_dim, self.goal_dim, self.ac_dim = 2 * dim + 1, dim, dim
        self.pos = np.zeros((num_envs, dim)); self.vel = np.zeros((num_envs, dim))
        self.goal = np.zeros((num_envs, dim)); self.t = np.zeros(num_envs, dtype=np.int64)

    def compute_reward(self, achieved_goal, desired_goal, info):
        d = np.linalg.norm(np.asarray(achieved_goal) - np.asarray(desired_goal), axis=-1)
        return -(d > self.thr).astype(np.float32)

    def _reset(self, idx):
        k = len(idx)
        self.pos[idx] = self.gen.uniform(-0.15, 0.15, (k, self.dim))
        self.vel[idx] = 0.0
        self.goal[idx] = self.gen.uniform(-0.15, 0.15, (k, self.dim))
        self.t[idx] = 0

    def _obs(self):
        o = np.concatenate([self.pos, self.vel, (self.t / self.T)[:, None]], axis=1).astype(np.float32)
        return {"observation": o, "achieved_goal": self.pos.astype(np.float32).copy(),
                "desired_goal": self.goal.astype(np.float32).copy()}

    def reset(self):
        self._reset(np.arange(self.n))
        return self._obs(), {}

    def step(self, actions):
        a = np.clip(np.asarray(actions, dtype=np.float64), -1, 1)
        self.vel = 0.04 * a                      # position control: the displacement of a step is the action
        self.pos = np.clip(self.pos + self.vel, -0.3, 0.3)
        self.t += 1
        obs = self._obs()
        rewards = self.compute_reward(obs["achieved_goal"], obs["desired_goal"], None)
        terminated = np.zeros(self.n, dtype=bool)
        truncated = self.t >= self.T
        return obs, rewards, terminated, truncated, {}


def fill_prior_ring(agent, prior, episodes, normalize, seed):
    """`episodes` scripted episodes of the synthetic goal environment into the prior ring: the action closes the distance to the goal,
    so most of them succeed — a stand-in for demonstrations or logged data.  normalize="push": the rings hold rows normalised at push
    time, so the scripted observations first update the agent's normalisers and are then stored normalised with those statistics
    (like the main ring's rows they keep the statistics of that moment).  normalize="sample": stored raw; the agent binds its
    normalisers to the prior ring and its rows leave normalised with the statistics of the moment of the gather."""
    env = PointReachVecEnv(1, seed=seed + 4242)
    eps = []
    for _ in range(episodes):
        state, _ = env.reset()
        rows = []
        for _ in range(env.T):
            action = np.clip((state["desired_goal"] - state["achieved_goal"]) / 0.04, -1, 1).astype(np.float32)
            nxt, reward, _, _, _ = env.step(action)
            rows.append((state, action, nxt, reward))
            state = nxt
        eps.append(rows)
    if normalize == "push":
        agent.update_normalizers([x[0]["observation"] for rows in eps for x in rows] + [x[2]["observation"] for rows in eps for x in rows],
                                 [], True, False)
        enc = lambda st: agent.normalize_state_batch(st["observation"], st["desired_goal"], True, False)
    else:
        enc = lambda st: np.concatenate([st["observation"], st["desired_goal"]], axis=-1)
    for rows in eps:
        prior.push_episode(0, np.concatenate([enc(x[0]) for x in rows]), np.concatenate([x[1] for x in rows]),
                           np.concatenate([enc(x[2]) for x in rows]), np.concatenate([x[3] for x in rows]), np.zeros(len(rows), np.float32),
                           np.concatenate([x[2]["achieved_goal"] for x in rows]))


def train(agent_name="DDPG", num_envs=8, cycles=60, max_episode=8, gradient_step=40, hidden=64, layers=3, batch=256,
          seed=0, verbose=True, per_env_push=False, fused=False, relabel="push", n_step=1, prioritise=None,
          goal_strategy="future", normalize="push", prior_episodes=0, prior_rows=0, bc_weight=None, q_filter=True, device_env=None,
          practice=False, practice_share=0.5, practice_radius=0.05):
    import gcrl_amd
    from gcrl_amd.src.utils import DeviceRunningNormalizer, RunningNormalizer
    if device_env is not None:
        fused = True          # collect needs the normalisers on the device
        if (prior_episodes or prior_rows) and device_env not in ("pick", "glide"):
            raise SystemExit("--device-env: the scripted prior episodes come from the host point-mass environment; not combined here")
    if practice and device_env is None:
        raise SystemExit("--practice proposes goals for a device env: it needs --device-env")
    if fused:   # the normalisers live on the device; acting and _process_step are one native call each per vector step
        RunningNormalizer = DeviceRunningNormalizer
    if normalize == "sample" and not fused:
        raise SystemExit("--normalize sample stores raw rows through the fused process_step and needs --fused (device normalisers)")
    from gcrl_amd.src.synthetic import agent_config as make_config   # hyper-parameter container with the YAML field names

    np.random.seed(seed)
    env = PointReachVecEnv(num_envs, seed=seed)
    host_env = env
    if device_env is not None:   # the env's state, its step blocks and its counters live on the device; the host env only lends its compute_reward
        env = gcrl_amd.DeviceGoalEnv(device_env, num_envs, seed=seed, max_steps=host_env.T, threshold=host_env.thr)
        env.thr = env.threshold
    cfg = make_config(agent_name, hidden_dim=hidden, layer_count=layers, batch_size=batch, max_len=200_000, k_future=4,
                      gamma=0.95, tau=0.05, grad_clip=10.0, ac_update_freq=2 if agent_name == "TD3" else 1,
                      policy_noise=0.2 if agent_name == "TD3" else 0.0)
    if relabel == "sample":   # the ring then counts real transitions: the same episodes resident in 1 / (1 + k_future) of the rows
        cfg.max_len //= 1 + cfg.k_future
    cls = dict(DDPG=gcrl_amd.DDPG, TD3=gcrl_amd.TD3Agent, SAC=gcrl_amd.SACAgent, TQC=gcrl_amd.TQCAgent)[agent_name]
    prior_kw, prior = {}, None
    if prior_episodes or prior_rows:   # prior-data replay: prior_rows of every batch come from a second ring the agent never pushes into
        if not (prior_episodes and prior_rows):
            raise SystemExit("--prior-episodes and --prior-rows go together")
        # pick, glide: the demonstrations come from a second device env under its scripted controller, up to 16 episodes side by side
        demo_envs = min(prior_episodes, 16) if device_env in ("pick", "glide") else 1
        demo_rounds = -(-prior_episodes // demo_envs)
        prior = gcrl_amd.HERBuffer(50 * demo_rounds * demo_envs, 50, demo_envs, threshold=env.thr, k_future=cfg.k_future, rng="device", seed=seed,
                                   relabel="sample", normalize=normalize)
        prior.compute_reward = host_env.compute_reward
        prior_kw = dict(prior_buffer=prior, prior_rows=prior_rows)
    if bc_weight is not None:   # Q-filtered behaviour cloning on the prior rows (DDPG / TD3): the weight is the caller's; the library has no default
        if prior is None:
            raise SystemExit("--bc-weight acts on the prior rows: it needs --prior-episodes and --prior-rows")
        prior_kw.update(bc_weight=bc_weight, q_filter=q_filter)
    agent = cls(env.obs_dim + env.goal_dim, env.ac_dim, cfg, None, nenvs=num_envs, gradient_step=gradient_step,
                rng="engine", seed=seed, relabel=relabel, n_step=n_step, prioritise=prioritise, goal_strategy=goal_strategy,
                normalize=normalize, **prior_kw)
    # what GoalEnvHER.__init__ injects (src/env.py:93-105)
    agent.buffer.obs_normalizer = RunningNormalizer(env.obs_dim)
    agent.buffer.dg_normalizer = RunningNormalizer(env.goal_dim)
    agent.buffer.compute_reward = host_env.compute_reward
    if prior is not None and device_env in ("pick", "glide"):
        # demonstrations without the host: the controller's launch, the env's step and the process-step launch per vector step.  The prior
        # ring takes the agent's normalisers: the scripted rows update them and (normalize="push") are stored normalised with them
        prior.obs_normalizer, prior.dg_normalizer = agent.buffer.obs_normalizer, agent.buffer.dg_normalizer
        demo = gcrl_amd.DeviceGoalEnv(device_env, demo_envs, seed=seed + 4242, max_steps=host_env.T, threshold=host_env.thr)
        prior.collect_scripted(demo, demo_rounds * demo.max_steps)
        st = demo.stats()
        if verbose:
            print(f"prior ring: {len(prior)} rows of {st['episodes']} scripted episodes, {st['successes']} solved")
    elif prior is not None:
        fill_prior_ring(agent, prior, prior_episodes, normalize, seed)

    if device_env is None:
        state, _ = env.reset()
    # practice goals: an env that finishes an episode may start the next one on an archived achieved goal of low density instead of its task goal
    proposer = gcrl_amd.GoalProposer(candidates=16, radius=practice_radius, share=practice_share, min_fill=max(256, num_envs), seed=seed) if practice else None
    grad_counter, env_steps = 1, 0
    success_per_cycle, final_success = [], []
    t_env = t_upd = 0.0
    t0 = time.perf_counter()
    for cycle in range(1, cycles + 1):
        episode_count = 0
        tc = time.perf_counter()
        if device_env is not None:   # the envs run in lockstep: every `max_steps` vector steps all of them finish an episode
            rounds = -(-max_episode // num_envs)
            before = env.stats()
            if bc_weight is None:
                agent.collect(env, rounds * env.max_steps, practice=proposer)
            else:
                # a behaviour-cloning agent runs the layer-per-launch schedule, which has no one-launch acting kernel for `collect`:
                # its actions come from the host entry, the env's step and the process-step stay on the device
                rows = env.acting_rows()
                for _ in range(rounds * env.max_steps):
                    act = agent.observe_act(rows["observation"].cpu().numpy(), rows["desired_goal"].cpu().numpy())
                    act = torch.from_numpy(np.asarray(act, dtype=np.float32)).cuda()
                    env.step(act)
                    if proposer is not None:     # the host-loop call order: observe_act -> env.step -> proposer.step(env) -> process_step
                        proposer.step(env)
                    raw, pay = env.step_blocks()
                    o, no, g, ng, a_, na = env.split_raw(raw)
                    agent.process_step_dev(dict(observation=o, desired_goal=g, achieved_goal=a_), act,
                                           dict(observation=no, desired_goal=ng, achieved_goal=na), pay[:, 1].contiguous())
            after = env.stats()       # (synchronises: the cycle's collection is over)
            done_eps = after["episodes"] - before["episodes"]
            final_success.extend([True] * (after["successes"] - before["successes"]) + [False] * (done_eps - (after["successes"] - before["successes"])))
            env_steps += rounds * env.max_steps * num_envs
            episode_count = max_episode
        while episode_count < max_episode:
            if fused:
                actions = np.asarray(agent.observe_act(state["observation"], state["desired_goal"]), dtype=np.float32)
            else:
                state_input = agent.normalize_state_batch(state["observation"], state["desired_goal"], True, False)
                actions = np.asarray(agent.select_action(state_input), dtype=np.float32)
            next_obs, rewards, terminateds, truncateds, _ = env.step(actions)
            dones = np.logical_or(terminateds, truncateds)
            if fused:
                agent.process_step(state, actions, next_obs, rewards, terminateds)
                env_steps += num_envs
                if dones.any():
                    idx = np.nonzero(dones)[0]
                    d = np.linalg.norm(next_obs["achieved_goal"][idx] - next_obs["desired_goal"][idx], axis=1)
                    final_success.extend((d < env.thr).tolist())
                    episode_count += len(idx)
                    env._reset(idx)
                    next_obs = env._obs()
                state = next_obs
                continue
            # _process_step: normaliser update, normalised [obs | goal] rows, one push for all envs
            agent.update_normalizers([state["observation"], next_obs["observation"]],
                                     [state["desired_goal"], next_obs["desired_goal"], state["achieved_goal"],
                                      next_obs["achieved_goal"]], True, False)
            obs_b = torch.from_numpy(agent.normalize_state_batch(state["observation"], state["desired_goal"], True, False)).float().cuda()
            nxt_b = torch.from_numpy(agent.normalize_state_batch(next_obs["observation"], next_obs["desired_goal"], True, False)).float().cuda()
            if per_env_push:   # the reference's own loop (src/env.py:192-201): one push_her per env
                for i in range(num_envs):
                    agent.push_her(i, obs_b[i].detach(), actions[i], nxt_b[i].detach(), rewards[i], terminateds[i],
                                   agent.normalize_goal(next_obs["desired_goal"][i], False),
                                   agent.normalize_goal(next_obs["achieved_goal"][i], False))
            else:
                agent.buffer.push_batch(obs_b, actions, nxt_b, rewards, terminateds, next_obs["achieved_goal"])
            env_steps += num_envs
            if dones.any():
                idx = np.nonzero(dones)[0]
                d = np.linalg.norm(next_obs["achieved_goal"][idx] - next_obs["desired_goal"][idx], axis=1)
                final_success.extend((d < env.thr).tolist())
                episode_count += len(idx)
                env._reset(idx)
                next_obs = env._obs()
            state = next_obs
        t_env += time.perf_counter() - tc
        tu = time.perf_counter()
        if agent.is_buffer_filled():
            infos = agent.update_many(grad_counter, gradient_step)
            grad_counter += gradient_step
            float(infos[-1][0])   # reads one metric: waits for the cycle's updates
        t_upd += time.perf_counter() - tu
        recent = final_success[-(max_episode if device_env is None else done_eps):]
        success_per_cycle.append(float(np.mean(recent)))
        if verbose and cycle % 10 == 0:
            print(f"cycle {cycle:4d}  success(last {len(recent)} episodes) {success_per_cycle[-1]:.2f}  buffer {len(agent.buffer)}")
            if bc_weight is not None and grad_counter > 1:
                print("            bc_loss %.4g  accepted share of the prior rows %.2f" % agent.bc_metrics())
    wall = time.perf_counter() - t0
    if proposer is not None:
        # with practice goals the per-cycle success above is measured against the goals the episodes had, practised ones included;
        # evaluate() restarts the env and so scores the task goals of the env's seed alone
        task = agent.evaluate(env, 4 * num_envs)
        print(f"practice goals: {proposer.stats()}, archive {len(proposer)}; task success of agent.evaluate: "
              f"{task['successes']} / {task['episodes']} = {task['success_rate']:.2f}")
    return dict(success_per_cycle=success_per_cycle, env_steps=env_steps, gradient_steps=grad_counter - 1, wall_s=wall,
                env_steps_per_s=env_steps / max(t_env, 1e-9), gradient_steps_per_s=(grad_counter - 1) / max(t_upd, 1e-9))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--agent", default="DDPG", choices=["DDPG", "TD3", "SAC", "TQC"])
    ap.add_argument("--cycles", type=int, default=60)
    ap.add_argument("--nenv", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-env", default=None, choices=["reach", "push", "pick", "glide"],
                    help="run the environment on the device (gcrl_amd.DeviceGoalEnv) and collect with agent.collect: no host in the acting loop")
    ap.add_argument("--practice", action="store_true",
                    help="with --device-env: practice goals (gcrl_amd.GoalProposer) — a finished env may start its next episode on an archived "
                         "achieved goal of low density; prints the proposer's stats and the task success of agent.evaluate at the end")
    ap.add_argument("--practice-share", type=float, default=0.5, help="with --practice: the share of finished envs that take a proposal, in (0, 1]")
    ap.add_argument("--practice-radius", type=float, default=0.05, help="with --practice: the radius inside which archive entries count as neighbours")
    ap.add_argument("--per-env-push", action="store_true", help="push one env at a time, exactly as the reference's trainer does")
    ap.add_argument("--fused", action="store_true", help="device normalisers + one native call for acting and one for _process_step")
    ap.add_argument("--relabel", default="push", choices=["push", "sample"],
                    help="push: relabelled copies stored at every flush (the reference's form); sample: rows stored once, relabelled when a batch is drawn")
    ap.add_argument("--n-step", type=int, default=1,
                    help="with --relabel sample: n-step returns, 1..8 (the gather folds the next N - 1 rows of the episode into reward and done)")
    ap.add_argument("--prioritise", default=None, choices=["energy", "td_error"],
                    help="with --relabel sample: 'energy' draws episodes in proportion to the energy their achieved-goal trajectory gained; "
                         "'td_error' is TD-error prioritised replay on the HER ring (HER + PER: the priorities follow the loss, new rows "
                         "enter at the largest priority seen so far, the critic losses carry importance-sampling weights)")
    ap.add_argument("--goal-strategy", default="future", choices=["future", "final", "episode"],
                    help="with --relabel sample: a relabelled row's goal comes from a later row of its episode, its last row, or any other row of it")
    ap.add_argument("--normalize", default="push", choices=["push", "sample"],
                    help="push: rows are stored normalised with the statistics of the moment of the push (the reference's form); sample (with "
                         "--fused): rows are stored raw and every gathered batch is normalised with the statistics of that moment")
    ap.add_argument("--prior-episodes", type=int, default=0,
                    help="fill a prior ring with this many scripted episodes of the synthetic goal environment (with --prior-rows); with "
                         "--device-env pick or glide they come from the device env's scripted controller, rounded up to a multiple of min(E, 16)")
    ap.add_argument("--prior-rows", type=int, default=0,
                    help="rows of every batch that come from the prior ring, 1 .. batch - 1 (prior-data replay; the batch is 256)")
    ap.add_argument("--bc-weight", type=float, default=None,
                    help="DDPG / TD3 with --prior-rows: weight of the behaviour-cloning term on the prior rows of every batch (> 0).  No default: "
                         "the library has none, and any value used here is this example's choice, not a published setting")
    ap.add_argument("--no-q-filter", action="store_true",
                    help="with --bc-weight: clone every prior row, not only those whose stored action the critic rates above the actor's")
    args = ap.parse_args()
    out = train(args.agent, num_envs=args.nenv, cycles=args.cycles, seed=args.seed, per_env_push=args.per_env_push, fused=args.fused,
                relabel=args.relabel, n_step=args.n_step, prioritise=args.prioritise, goal_strategy=args.goal_strategy,
                normalize=args.normalize, prior_episodes=args.prior_episodes, prior_rows=args.prior_rows,
                bc_weight=args.bc_weight, q_filter=not args.no_q_filter, device_env=args.device_env,
                practice=args.practice, practice_share=args.practice_share, practice_radius=args.practice_radius)
    tail = out["success_per_cycle"][-10:]
    print(f"{args.agent}: success over the last 10 cycles {np.mean(tail):.2f}; {out['env_steps']} env steps "
          f"({out['env_steps_per_s']:.0f}/s in the acting phase), {out['gradient_steps']} gradient steps "
          f"({out['gradient_steps_per_s']:.0f}/s in the update phase), {out['wall_s']:.1f} s")
