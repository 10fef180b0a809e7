#!/usr/bin/env python3
"""The stand-in trainer loop (examples/trainer_standin.py; reference src/env.py:334-406) for a POPULATION: P independent DDPG, TD3, SAC or TQC
agents, each with its own synthetic vector env, HER ring and normalisers, driven through the population's calls —

    pop.observe_act -> P env steps -> pop.process_step -> every `max_episode` episodes: pop.update_many(gradient_step)

— one launch per call and stage for all members instead of one per member.  Reports env steps/s and gradient steps/s in aggregate
(over all members) and every member's success rate.

    python examples/population_trainer.py --agent DDPG --members 4 --cycles 40

`--pbt N`: population-based training — every N cycles the bottom quarter of the members by success rate `exploit`s the top quarter
(weights, optimiser state and replay ring, one launch for all pairs) and `explore`s by x0.8 / x1.25 on both learning rates; the
overwritten slots are printed.  Without the flag the members run to the end as fixed trials.

`--shared-ring`: the members learn from ONE replay ring (and one pair of normalisers) that all their envs fill — every member sees the
experience every member collects; with `--pbt` an exploit then copies weights and optimiser state only (there is no ring to copy).

`--device-env reach|push|pick|glide`: the envs live on the device (gcrl_amd.DeviceGoalEnvGroup) and the acting phase of a cycle is ONE native
call, `pop.collect(group, steps)`: three launches per vector step for all members, nothing crossing to the host.  The reported
success rates — and the fitness of `--pbt` — come from `pop.evaluate` on a held-out group in which every member meets the same
episodes (one seed for all members), run deterministically.  Without the flag the host path above is unchanged.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from trainer_standin import PointReachVecEnv  # noqa: E402


def train_device(device_env, agent_name="DDPG", members=4, num_envs=8, cycles=40, max_episode=8, gradient_step=40, hidden=64, layers=3,
                 batch=256, seed=0, verbose=True, pbt=0, relabel="push", eval_episodes=None, max_steps=50, threshold=0.05):
    """The loop on device-resident envs: collect -> update_many -> evaluate -> exploit, the acting and the evaluation as one native call each."""
    import gcrl_amd
    from gcrl_amd.src.synthetic import agent_config as make_config, sparse_goal_reward
    from gcrl_amd.src.utils import DeviceRunningNormalizer

    group = gcrl_amd.DeviceGoalEnvGroup(device_env, members, num_envs, [seed + i for i in range(members)], max_steps=max_steps, threshold=threshold)
    held = gcrl_amd.DeviceGoalEnvGroup(device_env, members, num_envs, [seed + 10_000] * members, max_steps=max_steps, threshold=threshold)
    cfgs = [make_config(agent_name, hidden_dim=hidden, layer_count=layers, batch_size=batch, max_len=200_000, k_future=4, gamma=0.95,
                        tau=0.05, grad_clip=10.0, actor_lr=1e-3 * (1 + 0.25 * i), critic_lr=1e-3 * (1 + 0.25 * i),
                        ac_update_freq=1 if agent_name == "DDPG" else 2, policy_noise=0.2 if agent_name == "TD3" else 0.0)
            for i in range(members)]
    if relabel == "sample":
        for c in cfgs:
            c.max_len //= 1 + c.k_future
    cls = dict(DDPG=gcrl_amd.DDPGPopulation, TD3=gcrl_amd.TD3Population, SAC=gcrl_amd.SACPopulation, TQC=gcrl_amd.TQCPopulation)[agent_name]
    pop = cls(group.obs_dim + group.goal_dim, group.ac_dim, cfgs, num_envs, gradient_step, rng="engine", seeds=[seed + i for i in range(members)],
              relabel=relabel)
    for m in pop.members:
        m.buffer.obs_normalizer = DeviceRunningNormalizer(group.obs_dim)
        m.buffer.dg_normalizer = DeviceRunningNormalizer(group.goal_dim)
        m.buffer.compute_reward = sparse_goal_reward      # the built-in sparse kind at the envs' threshold
    # whole episodes per call: every staged count and every env's t is 0 between calls, so an exploit needs no env copy
    steps = -(-max_episode // num_envs) * max_steps
    eval_episodes = int(eval_episodes or 4 * num_envs)
    grad_counter, env_steps = 1, 0
    rate = [0.0] * members
    t_env = t_upd = t_eval = 0.0
    t0 = time.perf_counter()
    for cycle in range(1, cycles + 1):
        tc = time.perf_counter()
        pop.collect(group, steps)
        env_steps += steps * num_envs * members
        tu = time.perf_counter()
        t_env += tu - tc                    # (issue time: the loop does not wait for the device)
        if all(m.is_buffer_filled() for m in pop.members):
            infos = pop.update_many(grad_counter, gradient_step)
            grad_counter += gradient_step
            for info in infos:
                float(info[-1][0])          # reads one metric per member: waits for the cycle's collect and updates
        te = time.perf_counter()
        t_upd += te - tu
        due = pbt and cycle % pbt == 0 and members >= 2
        if due or cycle == cycles or (verbose and cycle % 10 == 0):
            rate = [r["success_rate"] for r in pop.evaluate(held, eval_episodes)]    # identical episodes for every member
            t_eval += time.perf_counter() - te
        if due:
            order = sorted(range(members), key=lambda i: (rate[i], i))
            q = max(1, members // 4)
            pairs = list(zip(order[::-1][:q], order[:q]))
            pop.exploit(pairs, copy_ring=True)
            gen = np.random.default_rng(seed + cycle)
            for src, dst in pairs:
                f = float(gen.choice([0.8, 1.25]))
                c = pop.members[src].config
                pop.explore(dst, actor_lr=c.actor_lr * f, critic_lr=c.critic_lr * f)
            print(f"cycle {cycle:4d}  pbt: overwritten slots " + ", ".join(f"{d} <- {s} (success {rate[d]:.2f} <- {rate[s]:.2f}, lr {pop.members[d].config.actor_lr:.2e})" for s, d in pairs))
        if verbose and cycle % 10 == 0:
            print(f"cycle {cycle:4d}  success({eval_episodes} held-out episodes) " + " ".join(f"{r:.2f}" for r in rate))
    return dict(success=[float(r) for r in rate], env_steps=env_steps, gradient_steps=(grad_counter - 1) * members, wall_s=time.perf_counter() - t0,
                acting_counts=pop.acting_counts(), collect_counts=pop.collect_counts(), eval_s=t_eval,
                env_steps_per_s=env_steps / max(t_env + t_upd, 1e-9), gradient_steps_per_s=(grad_counter - 1) * members / max(t_upd, 1e-9))


def train(agent_name="DDPG", members=4, num_envs=8, cycles=40, max_episode=8, gradient_step=40, hidden=64, layers=3, batch=256,
          seed=0, verbose=True, pbt=0, shared_ring=False, relabel="push", device_env=None, eval_episodes=None):
    if device_env is not None:
        if shared_ring:
            raise ValueError("--device-env: pop.collect is not built for a shared ring")
        return train_device(device_env, agent_name, members, num_envs, cycles, max_episode, gradient_step, hidden, layers, batch, seed, verbose, pbt,
                            relabel, eval_episodes)
    import gcrl_amd
    from gcrl_amd.src.synthetic import agent_config as make_config
    from gcrl_amd.src.utils import DeviceRunningNormalizer

    np.random.seed(seed)
    envs = [PointReachVecEnv(num_envs, seed=seed + i) for i in range(members)]
    e0 = envs[0]
    # members of one shape; here they differ in seed and learning rate (a small sweep)
    cfgs = [make_config(agent_name, hidden_dim=hidden, layer_count=layers, batch_size=batch, max_len=200_000, k_future=4, gamma=0.95,
                        tau=0.05, grad_clip=10.0, actor_lr=1e-3 * (1 + 0.25 * i), critic_lr=1e-3 * (1 + 0.25 * i),
                        ac_update_freq=1 if agent_name == "DDPG" else 2, policy_noise=0.2 if agent_name == "TD3" else 0.0)
            for i in range(members)]
    if relabel == "sample":   # the rings then count real transitions: the same episodes resident in 1 / (1 + k_future) of the rows
        for c in cfgs:
            c.max_len //= 1 + c.k_future
    cls = dict(DDPG=gcrl_amd.DDPGPopulation, TD3=gcrl_amd.TD3Population, SAC=gcrl_amd.SACPopulation, TQC=gcrl_amd.TQCPopulation)[agent_name]
    pop = cls(e0.obs_dim + e0.goal_dim, e0.ac_dim, cfgs, num_envs, gradient_step, rng="engine", seeds=[seed + i for i in range(members)],
              shared_ring=shared_ring, relabel=relabel)
    # (shared_ring: every member's .buffer is the one ring: its normalisers and reward are set once)
    for m, env in zip(pop.members[:1] if shared_ring else pop.members, envs):   # what GoalEnvHER.__init__ injects (src/env.py:93-105), device normalisers
        m.buffer.obs_normalizer = DeviceRunningNormalizer(env.obs_dim)
        m.buffer.dg_normalizer = DeviceRunningNormalizer(env.goal_dim)
        m.buffer.compute_reward = env.compute_reward

    states = [env.reset()[0] for env in envs]
    grad_counter, env_steps = 1, 0
    success = [[] for _ in range(members)]
    t_env = t_upd = 0.0
    t0 = time.perf_counter()
    for cycle in range(1, cycles + 1):
        episodes = 0
        tc = time.perf_counter()
        while episodes < max_episode:       # (episodes of member 0's env: all envs run the same fixed-length episodes)
            actions = [np.asarray(a, np.float32) for a in pop.observe_act([s["observation"] for s in states], [s["desired_goal"] for s in states])]
            stepped = [env.step(a) for env, a in zip(envs, actions)]
            pop.process_step(states, actions, [s[0] for s in stepped], [s[1] for s in stepped], [s[2] for s in stepped])
            env_steps += num_envs * members
            nxt = []
            for i, (env, (obs, _, term, trunc, _)) in enumerate(zip(envs, stepped)):
                done = np.logical_or(term, trunc)
                if done.any():
                    idx = np.nonzero(done)[0]
                    d = np.linalg.norm(obs["achieved_goal"][idx] - obs["desired_goal"][idx], axis=1)
                    success[i].extend((d < env.thr).tolist())
                    if i == 0:
                        episodes += len(idx)
                    env._reset(idx)
                    obs = env._obs()
                nxt.append(obs)
            states = nxt
        t_env += time.perf_counter() - tc
        tu = time.perf_counter()
        if all(m.is_buffer_filled() for m in pop.members):
            infos = pop.update_many(grad_counter, gradient_step)
            grad_counter += gradient_step
            for info in infos:
                float(info[-1][0])          # reads one metric per member: waits for the cycle's updates
        t_upd += time.perf_counter() - tu
        if pbt and cycle % pbt == 0 and members >= 2 and all(len(s) >= max_episode for s in success):
            # exploit: the bottom quarter takes over the top quarter's state; explore: both learning rates x0.8 or x1.25
            rate = [float(np.mean(s[-4 * max_episode:])) for s in success]
            order = sorted(range(members), key=lambda i: (rate[i], i))
            q = max(1, members // 4)
            pairs = list(zip(order[::-1][:q], order[:q]))
            pop.exploit(pairs, copy_ring=not shared_ring)
            gen = np.random.default_rng(seed + cycle)
            for src, dst in pairs:
                f = float(gen.choice([0.8, 1.25]))
                c = pop.members[src].config
                pop.explore(dst, actor_lr=c.actor_lr * f, critic_lr=c.critic_lr * f)
                success[dst] = list(success[src])
            print(f"cycle {cycle:4d}  pbt: overwritten slots " + ", ".join(f"{d} <- {s} (success {rate[d]:.2f} <- {rate[s]:.2f}, lr {pop.members[d].config.actor_lr:.2e})" for s, d in pairs))
        if verbose and cycle % 10 == 0:
            print(f"cycle {cycle:4d}  success(last {max_episode} episodes) " + " ".join(f"{np.mean(s[-max_episode:]):.2f}" for s in success))
    return dict(success=[float(np.mean(s[-10 * max_episode:])) for s in success], env_steps=env_steps,
                gradient_steps=(grad_counter - 1) * members, wall_s=time.perf_counter() - t0, acting_counts=pop.acting_counts(),
                env_steps_per_s=env_steps / max(t_env, 1e-9), gradient_steps_per_s=(grad_counter - 1) * members / max(t_upd, 1e-9))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--agent", default="DDPG", choices=["DDPG", "TD3", "SAC", "TQC"])
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--cycles", type=int, default=40)
    ap.add_argument("--nenv", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pbt", type=int, default=0, metavar="N", help="every N cycles the bottom quarter exploits the top quarter and explores (0: off)")
    ap.add_argument("--shared-ring", action="store_true", help="all members learn from one replay ring that all their envs fill")
    ap.add_argument("--relabel", default="push", choices=["push", "sample"],
                    help="push: relabelled copies stored at every flush (the reference's form); sample: rows stored once, relabelled when a batch is drawn")
    ap.add_argument("--device-env", default=None, choices=["reach", "push", "pick", "glide"],
                    help="device-resident envs: collect through pop.collect, success rates and the PBT fitness from pop.evaluate on a held-out group")
    args = ap.parse_args()
    out = train(args.agent, members=args.members, num_envs=args.nenv, cycles=args.cycles, seed=args.seed, pbt=args.pbt,
                shared_ring=args.shared_ring, relabel=args.relabel, device_env=args.device_env)
    what = "held-out success at the end" if args.device_env else "success over the last 10 cycles"
    print(f"{args.agent} x {args.members}: {what} " + " ".join(f"{s:.2f}" for s in out["success"]) +
          f"; {out['env_steps']} env steps in aggregate ({out['env_steps_per_s']:.0f}/s in the acting phase), {out['gradient_steps']} "
          f"gradient steps in aggregate ({out['gradient_steps_per_s']:.0f}/s in the update phase), {out['wall_s']:.1f} s; "
          f"acting calls / launches {out['acting_counts'][:4]}")
