"""Q-filtered behaviour cloning (bc_weight= / q_filter=; csrc/her_bc.hip) at the headline shape: what the keywords cost per step.

    python tools/bc_bench.py --time                       us/step of update_many, the configurations alternating in one process
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bc_bench.py --trace
    python tools/bc_bench.py --parse DIR                   bc_qfilter_kernel by the profiler's clock

Shape: bench.py's headline — DDPG, PickAndPlace record (S 23, A 4, G 3), batch 256, hidden 256 x 3, a main ring of 1e6 rows
(relabel="push", k_future 8, rng="engine") filled to capacity, update_many(step, 40) calls with the rings untouched in between — but
on the layer-per-launch schedule (pipeline=0), the one the term runs on.  The agents learn from ONE main ring (built once); the prior
ring holds 1e5 rows (relabel="sample", k_future 4, rng="device") of scripted episodes, prior_rows = 64.  Configurations:
  plain    pipeline=0, no prior ring (the launches of the parent commit's pipeline=0 agent)
  prior    + prior_buffer / prior_rows=64
  bc       + bc_weight=1.0, q_filter=True     (the extra critic forward inside the existing launches + one bc_qfilter_kernel launch)
  bc_nof   + bc_weight=1.0, q_filter=False    (the one launch alone)
--time: ROUNDS rounds, in each the configurations one after another, CALLS calls of 40 steps per sample between device
synchronisations; prints per configuration the samples' median and range in us/step.
--trace: WARM + ITERS calls of the two bc configurations, nothing timed (the profiler slows the host): the kernel trace is the result.
No GPU: --time and --trace fail."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, A, G = 23, 4, 3
BATCH, GSTEP, CAP, PRIOR_CAP, ROWS = 256, 40, 1_000_000, 100_000, 64
CONFIGS = ("plain", "prior", "bc", "bc_nof")
ROUNDS, CALLS = 7, 25
WARM, ITERS = 5, 10


def build(names=CONFIGS):
    import numpy as np
    import torch
    import gcrl_amd
    from gcrl_amd.src.synthetic import agent_config, synthetic_episode
    cfg = agent_config("DDPG", hidden_dim=256, layer_count=3, batch_size=BATCH, max_len=CAP, k_future=8, gamma=0.98, tau=0.05,
                       grad_clip=10.0, ac_update_freq=1, actor_lr=1e-3, actor_lr_min=1e-3, critic_lr=1e-3, critic_lr_min=1e-3)
    gen = np.random.default_rng(1898)
    eps = []
    for _ in range(64):
        s, a, ns, r, d, dg, ag = zip(*synthetic_episode(gen, 50, S, A))
        eps.append((np.array(s, np.float32), np.array(a, np.float32), np.array(ns, np.float32), np.array(r, np.float32),
                    np.zeros(50, np.float32), np.array(ag, np.float32)))
    prior = gcrl_amd.HERBuffer(PRIOR_CAP, 50, 2, k_future=4, rng="device", seed=7, relabel="sample")
    for i in range(PRIOR_CAP // 50):
        prior.push_episode(i % 2, *eps[i % 64])
    kws = dict(plain={}, prior=dict(prior_buffer=prior, prior_rows=ROWS),
               bc=dict(prior_buffer=prior, prior_rows=ROWS, bc_weight=1.0, q_filter=True),
               bc_nof=dict(prior_buffer=prior, prior_rows=ROWS, bc_weight=1.0, q_filter=False))
    agents = {}
    ring = None
    for name in names:
        ag = gcrl_amd.DDPG(S, A, cfg, None, nenvs=8, gradient_step=GSTEP, rng="engine", seed=1898, pipeline=0, **kws[name])
        if ring is None:
            ring = ag.buffer
            for i in range(-(-CAP // (50 + 8 * 49))):
                ring.push_episode(i % 8, *eps[i % 64])
            assert len(ring) == CAP
        ag.buffer = ring
        agents[name] = ag
    torch.cuda.synchronize()
    return agents


def time_it():
    import torch
    agents = build()
    step = 1
    for ag in agents.values():                               # graphs, buffers and the scratch batch exist before the clock starts
        for _ in range(WARM):
            ag.update_many(step, GSTEP)
    torch.cuda.synchronize()
    samples = {name: [] for name in agents}
    for _ in range(ROUNDS):
        for name, ag in agents.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                ag.update_many(step, GSTEP)
                step += GSTEP
            torch.cuda.synchronize()
            samples[name].append((time.perf_counter() - t0) * 1e6 / (CALLS * GSTEP))
    for name, ag in agents.items():
        v = samples[name]
        extra = ""
        if ag.bc_weight is not None:
            loss, share = ag.bc_metrics()
            extra = f"; last step: bc_loss {loss:.4g}, accepted share {share:.3f}"
        print(f"{name:7s}: {len(v)} samples of {CALLS * GSTEP} steps, median {statistics.median(v):6.2f} us/step, "
              f"range {min(v):6.2f} .. {max(v):6.2f}; series {' '.join(f'{x:.2f}' for x in v)}{extra}")


def trace():
    import torch
    agents = build(("bc", "bc_nof"))
    for name, ag in agents.items():
        for i in range(WARM + ITERS):
            ag.update_many(1 + i * GSTEP, GSTEP)
        torch.cuda.synchronize()
    print("bc_bench: done")


NAMES = ("bc_qfilter_kernel",)


def parse(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    rows, total = {}, 0
    for f in files:
        for r in csv.DictReader(open(f)):
            total += 1
            key = next((n for n in NAMES if n in r["Kernel_Name"]), None)
            if key is None:
                continue
            rows.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    print(f"{total} kernel launches in the trace")
    for key, v in sorted(rows.items()):
        v.sort()
        half = len(v) // 2
        for label, part in (("q_filter=True", v[:half]), ("q_filter=False", v[half:])):      # trace(): the bc agent first, then bc_nof
            dur = [x[1] / 1e3 for x in part[-ITERS * GSTEP:]]           # the last ITERS calls' launches: past every warm-up
            print(f"{key} ({label}): {len(part)} launches, last {len(dur)}: median {statistics.median(dur):6.2f} us, "
                  f"range {min(dur):6.2f} .. {max(dur):6.2f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--parse", metavar="DIR")
    a = ap.parse_args()
    if a.parse:
        parse(a.parse)
    elif a.time:
        time_it()
    elif a.trace:
        trace()
    else:
        ap.error("--time, --trace or --parse DIR")
