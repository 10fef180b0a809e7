#!/usr/bin/env python3
"""Wall clock per `observe_act` call of the BatchNorm actors (SAC cfg 5 shapes: H 256, L 3; TQC cfg 4 shapes: H 512, L 3) in the
trainer's acting loop: 8 envs, observe_act -> process_step per vector step, so an episode of every env ends (flush + HER relabel)
on every 50th step.  Legs, alternated over `--rounds` rounds, each in a fresh child process:

  new      this tree, the one-launch form (csrc/act_bn.hip)
  staged   this tree with GCRL_ACT_STAGED=1: the chain of separate launches
  parent   another checkout of the project with its library built (--parent-tree), when given

usage: tools/acting_bench.py [--rounds 5] [--steps 3000] [--parent-tree DIR] [--out FILE.jsonl]
       tools/acting_bench.py --child KIND H L [--tree DIR] [--steps N]      (one leg; prints one JSON line)
Writes one JSON line per shape with the median and min-max of every leg (default profiles/r09_sac_acting.jsonl).  Kernel durations
come from a run of one leg under the profiler, on its own:
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/acting_bench.py --child SAC 256 3 --steps 1000
(DIR/**/run_kernel_stats.csv; the two shapes' files are concatenated into profiles/r09_sac_acting_kernel_stats.csv)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [dict(name="sac_cfg5", kind="SAC", H=256, L=3, B=512), dict(name="tqc_cfg4", kind="TQC", H=512, L=3, B=2048)]
D, G, A, ENVS = 19, 3, 3, 8


def child(kind, H, L, tree, steps):
    sys.path.insert(0, tree)
    import numpy as np
    import gcrl_amd
    from gcrl_amd.src.synthetic import agent_config, sparse_goal_reward
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    B = next(s["B"] for s in SHAPES if s["kind"] == kind)
    cfg = agent_config(kind, hidden_dim=H, layer_count=L, batch_size=B, max_len=200_000)
    cls = dict(SAC=gcrl_amd.SACAgent, TQC=gcrl_amd.TQCAgent)[kind]
    ag = cls(D + G, A, cfg, None, nenvs=ENVS, gradient_step=40, rng="engine", seed=0)
    ag.buffer.obs_normalizer, ag.buffer.dg_normalizer = DeviceRunningNormalizer(D), DeviceRunningNormalizer(G)
    ag.buffer.compute_reward = sparse_goal_reward
    gen = np.random.default_rng(0)

    def obs_dict():
        return dict(observation=gen.standard_normal((ENVS, D)).astype(np.float32), desired_goal=gen.uniform(-0.2, 0.2, (ENVS, G)).astype(np.float32),
                    achieved_goal=gen.uniform(-0.2, 0.2, (ENVS, G)).astype(np.float32))

    pool = [obs_dict() for _ in range(64)]
    rewards, dones = -np.ones(ENVS, np.float32), np.zeros(ENVS, bool)
    warm, t_act = 200, 0.0
    state = pool[0]
    for i in range(steps + warm):
        if i == warm:
            t_act = 0.0
        t0 = time.perf_counter()
        a = np.asarray(ag.observe_act(state["observation"], state["desired_goal"], eval_action=(i % 50 == 49)), dtype=np.float32)
        t_act += time.perf_counter() - t0
        nxt = pool[(i + 1) % len(pool)]
        ag.process_step(state, a, nxt, rewards, dones)
        state = nxt
    res = dict(kind=kind, H=H, L=L, envs=ENVS, steps=steps, us_per_call=round(1e6 * t_act / steps, 2),
               form="staged" if os.environ.get("GCRL_ACT_STAGED") else "default")
    if hasattr(ag, "acting_counts"):
        res["counts"] = ag.acting_counts()
    print("RESULT " + json.dumps(res), flush=True)


def run_leg(shape, tree, steps, knob):
    env = dict(os.environ)
    env.pop("GCRL_ACT_STAGED", None)
    if knob:
        env[knob] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", shape["kind"], str(shape["H"]), str(shape["L"]), "--tree", tree, "--steps", str(steps)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180 + steps // 20)
    if out.returncode != 0:
        raise SystemExit(f"leg failed ({out.returncode}): {out.stderr[-1500:]}")   # nothing more is started on the device
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3)
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent-tree")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r09_sac_acting.jsonl"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), int(a.child[2]), os.path.abspath(a.tree), a.steps)
    legs = [("new", HERE, None)] + ([("parent", os.path.abspath(a.parent_tree), None)] if a.parent_tree else []) + [("staged", HERE, "GCRL_ACT_STAGED")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for shape in SHAPES:
            runs = {name: [] for name, _, _ in legs}
            counts = {}
            for r in range(a.rounds):
                for name, tree, knob in legs:
                    res = run_leg(shape, tree, a.steps, knob)
                    runs[name].append(res["us_per_call"])
                    counts[name] = res.get("counts")
                    print(f"{shape['name']} round {r + 1} {name}: {res['us_per_call']} us", flush=True)
            line = dict(shape=shape["name"], kind=shape["kind"], H=shape["H"], L=shape["L"], state_dim=D + G, action_dim=A, envs=ENVS,
                        vector_steps=a.steps, rounds=a.rounds, unit="us per observe_act call (wall clock, Python wrapper included)",
                        legs={n: dict(median=statistics.median(v), min=min(v), max=max(v), runs=v, counts=counts[n]) for n, v in runs.items()})
            if "parent" in runs:
                line["new_range_below_parent_range"] = max(runs["new"]) < min(runs["parent"])
            f.write(json.dumps(line) + "\n")
            f.flush()
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
