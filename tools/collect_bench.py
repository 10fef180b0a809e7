"""What the on-device collect loop (agent.collect on a gcrl_amd.DeviceGoalEnv; csrc/dev_env.hip, csrc/agent.hip) gives over the host
loop it replaces, and its launches by the profiler's clock.

    python tools/collect_bench.py --cost [--out profiles/r30_collect.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/collect_bench.py --run
    python tools/collect_bench.py --parse DIR

--cost: one DDPG agent per path at the headline network (three hidden layers of 256, batch 256), `reach` dimensions (S 10, A 3, G 3),
N in {8, 32, 256} envs.  Path (i) is what the parent commit can do: observe_act + the numpy restatement of the env
(tests/dev_env_ref.py) + process_step per vector step; its env time is Python's and is reported separately, measured here.  Path
(ii) is agent.collect.  Alternating in one process, seven samples each between two device synchronisations; prints env-steps/s of
both, median and range.
--run issues, for the profiler, STEPS collect steps at every N; nothing is timed there.  --parse prints, per kernel, the launches
after the warm-up ones: number, median, range in us.  No --pmc in that run.
No GPU: --cost and --run fail."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D, G, A, T, THR = 7, 3, 3, 50, 0.05
H, L, B = 256, 3, 256
NS = (8, 32, 256)
SAMPLES, WARM = 7, 10
HOST_STEPS = {8: 100, 32: 50, 256: 10}        # vector steps of a host-loop sample (its env is a Python loop over the envs)
DEV_STEPS = 500
STEPS = 300
NAMES = ("env_step_kernel", "rowchain_act_kernel", "her_process_step_kernel", "her_flush_kernel")


def _agent(n, seed=1):
    import gcrl_amd
    from gcrl_amd.src.synthetic import agent_config
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    from oracle import her_oracle
    cfg = agent_config("DDPG", hidden_dim=H, layer_count=L, batch_size=B, max_len=400_000, k_future=4)
    ag = gcrl_amd.DDPG(D + G, A, cfg, None, nenvs=n, gradient_step=40, rng="engine", seed=seed)
    ag.buffer.obs_normalizer = DeviceRunningNormalizer(D)
    ag.buffer.dg_normalizer = DeviceRunningNormalizer(G)
    ag.buffer.compute_reward = her_oracle.sparse_reward
    return ag


def _host_steps(ag, ref, steps):
    """the parent's capability: one observe_act and one process_step per vector step around a host env; returns the env's own seconds"""
    import numpy as np
    t_env = 0.0
    zeros = np.zeros(ref.n, bool)
    for _ in range(steps):
        st = ref.state_dict()
        act = np.asarray(ag.observe_act(st["observation"], st["desired_goal"]), np.float32)
        t0 = time.perf_counter()
        raw, pay = ref.step(act)
        _, nobs, _, ndg, _, nag = ref.split(raw)
        t_env += time.perf_counter() - t0
        ag.process_step(st, act, dict(observation=nobs, desired_goal=ndg, achieved_goal=nag), pay[:, 1].copy(), zeros)
    return t_env


def cost(out):
    import torch
    import gcrl_amd
    import dev_env_ref as E
    lines = ["# env-steps/s of one vector-env collection loop, DDPG H 256 x 3, batch 256, reach dimensions; %d alternating samples" % SAMPLES,
             "# (i) observe_act + numpy ref env + process_step per step; 'engine' leaves the Python env's own time out   (ii) agent.collect"]
    for n in NS:
        host, dev = _agent(n), _agent(n)
        ref = E.RefEnv("reach", n, seed=3, max_steps=T, threshold=THR)
        env = gcrl_amd.DeviceGoalEnv("reach", n, seed=3, max_steps=T, threshold=THR)
        _host_steps(host, ref, WARM)
        dev.collect(env, WARM)
        torch.cuda.synchronize()
        hs, he, ds = [], [], []
        for _ in range(SAMPLES):
            k = HOST_STEPS[n]
            t0 = time.perf_counter(); t_env = _host_steps(host, ref, k); torch.cuda.synchronize(); dt = time.perf_counter() - t0
            hs.append(n * k / dt); he.append(n * k / max(dt - t_env, 1e-9))
            t0 = time.perf_counter(); dev.collect(env, DEV_STEPS); torch.cuda.synchronize(); dt = time.perf_counter() - t0
            ds.append(n * DEV_STEPS / dt)
        med = statistics.median
        lines.append("N %4d  (i) host loop %10.0f [%.0f .. %.0f]   (i) engine only %10.0f [%.0f .. %.0f]   (ii) collect %10.0f [%.0f .. %.0f]   "
                     "(ii)/(i engine only) %.1fx   us per vector step (ii) %.1f" %
                     (n, med(hs), min(hs), max(hs), med(he), min(he), max(he), med(ds), min(ds), max(ds), med(ds) / med(he), 1e6 * n / med(ds)))
        c = dev.collect_counts()
        lines.append("        collect counts: %s" % c)
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def run():
    import torch
    import gcrl_amd
    for n in NS:
        ag = _agent(n)
        env = gcrl_amd.DeviceGoalEnv("reach", n, seed=3, max_steps=T, threshold=THR)
        ag.collect(env, WARM)
        torch.cuda.synchronize()
        ag.collect(env, STEPS)
        torch.cuda.synchronize()


def parse(d):
    rows = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                key = next((k for k in NAMES if k in name), None)
                if key:
                    rows.setdefault(key, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    # --run goes through NS in order with the same number of steps each: a kernel's launches in time order are len(NS) equal runs
    for key, v in sorted(rows.items()):
        v = [d for _, d in sorted(v)]
        per = len(v) // len(NS)
        for k, n in enumerate(NS):
            part = v[k * per:(k + 1) * per]
            part = part[WARM:] if len(part) > 2 * WARM else part
            if part:
                print("%-26s N %4d  launches %5d  median %.2f us  [%.2f .. %.2f]" % (key, n, len(part), statistics.median(part), min(part), max(part)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--parse", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cost:
        cost(a.out)
    if a.run:
        run()
    if a.parse:
        parse(a.parse)
