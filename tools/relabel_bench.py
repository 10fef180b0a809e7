"""Sample-time relabelling against the default mode, by the profiler's clock.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/relabel_bench.py --run
    python tools/relabel_bench.py --parse DIR

--run fills rings of 1e6 records at PickAndPlace dims (S 23, A 4, G 3; k_future 4, rng="device": no host draw, no index
upload) — one per relabel mode, and for the sample mode one more per n_step in NSTEPS (gamma 0.98; n_step = 1 is the sample-mode
ring itself), and one per goal strategy in GOALS at n_step 1 and at GOAL_NSTEP (csrc/her_strategy.hip) — and then, alternating the rings, issues the update engine's gather (HERBuffer.gather_update) at 9 216 and 77 824
rows, and the flush of one T = 50 episode (push_episode; the two modes and the `episode` ring, whose flush stamps `elapsed`:
n_step does not reach the flush, and a `final` ring launches the sample mode's).  Nothing is timed
here: the kernel trace is.
--parse reads the trace and prints, per kernel and launch size, the number of launches, the median and the range of the kernel
durations — the launches after the warm-up ones.  The n-step rings launch one kernel at one grid size: their launches alternate in
NSTEPS order and are told apart by that; so do the rings of the goal strategies, in GOALS order.  No GPU: --run fails; it does not fall back.
--rings NAME[,NAME ...] builds and times only those rings (push, sample, sample_n3, final, episode_n3, ...).  `sample_norm` is the
sample-mode ring with normalize="sample" (csrc/her_norm.hip; observation and goal normalisers bound): behind each of its gathers runs
her_norm_rows_kernel, whose launches are listed beside the her_gather_relabel_kernel ones they follow."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, A, G, K = 23, 4, 3, 4
CAP = 1_000_000
SIZES = ((256, 36), (256, 304))      # 9 216 and 77 824 rows: a trainer cycle's head-sized and main gather
WARM, ITERS = 10, 60
NSTEPS = (3, 8)
GOALS = ("final", "episode")
GOAL_NSTEP = 3


def run(only=None):
    import numpy as np
    import gcrl_amd
    from oracle import her_oracle
    gen = np.random.default_rng(0)
    st = her_oracle.synthetic_episode(gen, 50, S, A, G)
    ep = [np.stack([x[j] for x in st]).astype(np.float32) for j in (0, 1, 2)] + \
         [np.array([x[3] for x in st], np.float32), np.zeros(50, np.float32), np.stack([x[6] for x in st])]
    rings = {}
    want = lambda name: only is None or name in only     # (a ring that is not asked for is not built: the fill is most of the run)
    for mode in ("push", "sample"):
        if not want(mode):
            continue
        buf = gcrl_amd.HERBuffer(CAP, 50, 2, k_future=K, rng="device", seed=1, relabel=mode)
        buf.compute_reward = her_oracle.sparse_reward
        per = 50 if mode == "sample" else 50 + K * 49
        for _ in range(CAP // per + 2):                      # the same episode again and again: the gathers' addresses are what matters
            buf.push_episode(0, *ep)
        assert len(buf) == CAP
        rings[mode] = buf
    for N in NSTEPS:
        if not want(f"sample_n{N}"):
            continue
        buf = gcrl_amd.HERBuffer(CAP, 50, 2, k_future=K, rng="device", seed=1, relabel="sample", n_step=N, gamma=0.98)
        buf.compute_reward = her_oracle.sparse_reward
        for _ in range(CAP // 50 + 2):
            buf.push_episode(0, *ep)
        assert len(buf) == CAP
        rings[f"sample_n{N}"] = buf
    for N in (1, GOAL_NSTEP):
        for goal in GOALS:
            kw = dict(n_step=N, gamma=0.98) if N > 1 else {}
            if not want(goal if N == 1 else f"{goal}_n{N}"):
                continue
            buf = gcrl_amd.HERBuffer(CAP, 50, 2, k_future=K, rng="device", seed=1, relabel="sample", goal_strategy=goal, **kw)
            buf.compute_reward = her_oracle.sparse_reward
            for _ in range(CAP // 50 + 2):
                buf.push_episode(0, *ep)
            assert len(buf) == CAP
            rings[goal if N == 1 else f"{goal}_n{N}"] = buf
    if want("sample_norm"):
        from gcrl_amd.src.utils import DeviceRunningNormalizer
        buf = gcrl_amd.HERBuffer(CAP, 50, 2, k_future=K, rng="device", seed=1, relabel="sample", normalize="sample", g_normalize=True)
        buf.compute_reward = her_oracle.sparse_reward
        buf.obs_normalizer, buf.dg_normalizer = DeviceRunningNormalizer(S - G), DeviceRunningNormalizer(G)
        buf.obs_normalizer.update(ep[0][:, :S - G])
        buf.dg_normalizer.update(ep[0][:, S - G:])
        for _ in range(CAP // 50 + 2):
            buf.push_episode(0, *ep)
        assert len(buf) == CAP
        rings["sample_norm"] = buf
    if only is not None:
        unknown = [r for r in only if r not in rings]
        if unknown:
            sys.exit(f"--rings: unknown ring(s) {unknown}")
    import torch
    torch.cuda.synchronize()
    for B, M in SIZES:
        for _ in range(WARM + ITERS):
            for mode in rings:                              # push, sample (N = 1), the n-step rings in NSTEPS order, the goal rings in GOALS order
                rings[mode].gather_update(B, M)
    for _ in range(WARM + ITERS):
        for mode in ("push", "sample", "episode"):
            if mode in rings:
                rings[mode].push_episode(1, *ep)
    torch.cuda.synchronize()
    print("relabel_bench: done")


NAMES = ("her_gather_update_kernel", "her_gather_relabel_kernel", "her_gather_nstep_kernel", "her_gather_goal_kernel", "her_gather_goal_nstep_kernel",
         "her_flush_kernel", "her_flush_sample_kernel", "her_flush_episode_kernel", "her_norm_rows_kernel")


def parse(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    rows = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            key = next((n for n in NAMES if n in name), None)
            if key is None:
                continue
            grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r.get("Grid_Size_X", 0))
            rows.setdefault((key, grid), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    for (key, grid), v in list(rows.items()):
        if key == "her_gather_nstep_kernel":                 # launches alternate between the n-step rings
            v.sort()
            del rows[key, grid]
            for i, N in enumerate(NSTEPS):
                rows[f"{key} N={N}", grid] = v[i::len(NSTEPS)]
        if key in ("her_gather_goal_kernel", "her_gather_goal_nstep_kernel"):     # launches alternate between the strategies' rings
            v.sort()
            del rows[key, grid]
            for i, goal in enumerate(GOALS):
                rows[f"{key} {goal}" + (f" N={GOAL_NSTEP}" if "nstep" in key else ""), grid] = v[i::len(GOALS)]
    for (key, grid), v in sorted(rows.items()):
        v.sort()
        if len(v) < ITERS:           # the fill's flushes have their own grid sizes only in push mode; keep the timed tail of each
            continue
        dur = [x[1] / 1e3 for x in v[-ITERS:]]
        print(f"{key:42s} grid {grid:8d} threads: {len(dur)} launches, median {statistics.median(dur):7.2f} us, "
              f"range {min(dur):7.2f} .. {max(dur):7.2f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--parse", metavar="DIR")
    ap.add_argument("--rings", default=None, help="with --run: comma-separated ring names to build and time (default: all)")
    a = ap.parse_args()
    if a.parse:
        parse(a.parse)
    elif a.run:
        run(a.rings.split(",") if a.rings else None)
    else:
        ap.error("--run or --parse DIR")
