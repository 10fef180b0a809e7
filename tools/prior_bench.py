"""Prior-data replay (prior_buffer= / prior_rows=; csrc/her_prior.hip) at the headline shape: what the keywords cost per step.

    python tools/prior_bench.py --time                       us/step of update_many, three configurations alternating in one process
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/prior_bench.py --trace
    python tools/prior_bench.py --parse DIR                   her_place_rows_kernel and the prior ring's gather by the profiler's clock

Shape: bench.py's headline — DDPG, PickAndPlace record (S 23, A 4, G 3), batch 256, hidden 256 x 3, a main ring of 1e6 rows
(relabel="push", k_future 8, rng="engine") filled to capacity, update_many(step, 40) calls with the rings untouched in between.  The
three agents learn from ONE main ring (built once); the prior ring holds 1e5 rows (relabel="sample", k_future 4, rng="device") of
scripted episodes.  Configurations: no prior ring, prior_rows=64, prior_rows=128.
--time: ROUNDS rounds, in each the three configurations one after another, CALLS calls of 40 steps per sample between device
synchronisations; prints per configuration the samples' median and range in us/step and the launches prior_counts() reports per call.
--trace: WARM + ITERS calls per configuration, nothing timed (the profiler slows the host): the kernel trace is the result.
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
BATCH, GSTEP, CAP, PRIOR_CAP = 256, 40, 1_000_000, 100_000
CONFIGS = (0, 64, 128)
ROUNDS, CALLS = 7, 50
WARM, ITERS = 10, 40


def build():
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
    agents = {}
    ring = None
    for rows in CONFIGS:
        kw = dict(prior_buffer=prior, prior_rows=rows) if rows else {}
        ag = gcrl_amd.DDPG(S, A, cfg, None, nenvs=8, gradient_step=GSTEP, rng="engine", seed=1898, **kw)
        if ring is None:
            ring = ag.buffer
            for i in range(-(-CAP // (50 + 8 * 49))):
                ring.push_episode(i % 8, *eps[i % 64])
            assert len(ring) == CAP
        ag.buffer = ring
        agents[rows] = ag
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
    samples = {rows: [] for rows in CONFIGS}
    for _ in range(ROUNDS):
        for rows, ag in agents.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                ag.update_many(step, GSTEP)
                step += GSTEP
            torch.cuda.synchronize()
            samples[rows].append((time.perf_counter() - t0) * 1e6 / (CALLS * GSTEP))
    for rows, ag in agents.items():
        v = samples[rows]
        g, p = ag.prior_counts()
        calls = WARM + ROUNDS * CALLS
        print(f"prior_rows={rows:3d}: {len(v)} samples of {CALLS * GSTEP} steps, median {statistics.median(v):6.2f} us/step, "
              f"range {min(v):6.2f} .. {max(v):6.2f}; series {' '.join(f'{x:.2f}' for x in v)}; "
              f"prior gathers {g / calls:.1f} and placements {p / calls:.1f} per call")


def trace():
    import torch
    agents = build()
    for rows, ag in agents.items():
        for i in range(WARM + ITERS):
            ag.update_many(1 + i * GSTEP, GSTEP)
        torch.cuda.synchronize()
    print("prior_bench: done")


NAMES = ("her_place_rows_kernel", "her_gather_relabel_kernel", "her_gather_update_kernel")


def parse(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    rows = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            key = next((n for n in NAMES if n in r["Kernel_Name"]), None)
            if key is None:
                continue
            grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r.get("Grid_Size_X", 0))
            rows.setdefault((key, grid), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    for (key, grid), v in sorted(rows.items()):
        v.sort()
        dur = [x[1] / 1e3 for x in v[-ITERS:]]               # the last ITERS launches of each (kernel, grid): past every warm-up
        print(f"{key:30s} grid {grid:8d} threads: {len(v)} launches, last {len(dur)}: median {statistics.median(dur):7.2f} us, "
              f"range {min(dur):7.2f} .. {max(dur):7.2f} us")


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
