"""Sample-time relabelling against the default mode, by the profiler's clock.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/relabel_bench.py --run
    python tools/relabel_bench.py --parse DIR

--run fills rings of 1e6 records at PickAndPlace dims (S 23, A 4, G 3; k_future 4, rng="device": no host draw, no index
upload) in this order: `push` and `sample`, one per relabel mode; `sample_n3`, `sample_n8`, the sample mode with n_step in NSTEPS
(gamma 0.98); `final`, `episode`, one per goal strategy in GOALS, then `final_n3`, `episode_n3`, the same at n_step GOAL_NSTEP; and
`sample_norm` (below).  Then, the rings alternating IN THAT ORDER inside every iteration, it issues the update engine's gather
(HERBuffer.gather_update) at 9 216 and 77 824 rows, then the public sample (HERBuffer.sample) at 9 216 rows on the sample-mode rings,
then the flush of one T = 50 episode (push_episode) on `push`, `sample` and `episode` (n_step does not reach the flush; only an
`episode` ring's flush stamps `elapsed`).  Nothing is timed here: the kernel trace is.
--parse reads the trace and prints, per kernel, ring and launch size, the number of launches, the median and the range of the
kernel durations — the launches after the warm-up ones.  All sample-mode rings launch the same kernels (csrc/her_relabel.hip) at the
same grids — her_gather_relabel_kernel at n_step 1, her_gather_nstep_kernel above it, her_gather_relabel_pub_kernel for the public
sample, her_flush_sample_kernel — so a kernel's launches are told apart by the order above alone: launch i of a kernel at a grid
belongs to ring i mod R of the R rings that launch it.  No GPU: --run fails; it does not fall back.
--rings NAME[,NAME ...] builds and times only those rings; give --parse the same list.  `sample_norm` is the sample-mode ring with
normalize="sample" (csrc/her_norm.hip; observation and goal normalisers bound): behind each of its gathers runs
her_norm_rows_kernel (her_norm_dense_kernel behind its public sample), listed beside the gathers they follow."""
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
            for mode in rings:                              # in ORDER
                rings[mode].gather_update(B, M)
    for _ in range(WARM + ITERS):
        for mode in rings:
            if mode != "push":
                rings[mode].sample(*SIZES[0])
    for _ in range(WARM + ITERS):
        for mode in FLUSHED:
            if mode in rings:
                rings[mode].push_episode(1, *ep)
    torch.cuda.synchronize()
    print("relabel_bench: done")


# the rings in the order --run builds and alternates them, and which of them launch a kernel (a kernel that is not listed has one ring)
ORDER = ("push", "sample") + tuple(f"sample_n{N}" for N in NSTEPS) + GOALS + tuple(f"{g}_n{GOAL_NSTEP}" for g in GOALS) + ("sample_norm",)
FLUSHED = ("push", "sample", "episode")
ONE_STEP = ("sample",) + GOALS + ("sample_norm",)
RINGS_OF = {"her_gather_update_kernel": ("push",), "her_flush_kernel": ("push",),
            "her_gather_relabel_kernel": ONE_STEP, "her_gather_nstep_kernel": tuple(r for r in ORDER[1:] if r not in ONE_STEP),
            "her_gather_relabel_pub_kernel": ORDER[1:], "her_flush_sample_kernel": FLUSHED[1:],
            "her_norm_rows_kernel": ("sample_norm",), "her_norm_dense_kernel": ("sample_norm",)}


def parse(d, only=None):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    rows = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            key = next((n for n in RINGS_OF if n in name), None)
            if key is None:
                continue
            grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r.get("Grid_Size_X", 0))
            rows.setdefault((key, grid), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    for (key, grid), v in sorted(rows.items()):
        v.sort()
        rings = [r for r in RINGS_OF[key] if only is None or r in only]
        v = v[-len(rings) * ITERS:]  # the timed tail: the fill's flushes and the warm-up launches come first
        if not rings or len(v) < len(rings) * ITERS:
            continue
        for i, ring in enumerate(rings):
            dur = [x[1] / 1e3 for x in v[i::len(rings)]]
            print(f"{key:30s} {ring:12s} grid {grid:8d} threads: {len(dur)} launches, median {statistics.median(dur):7.2f} us, "
                  f"range {min(dur):7.2f} .. {max(dur):7.2f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--parse", metavar="DIR")
    ap.add_argument("--rings", default=None, help="comma-separated ring names to build and time, or to parse (default: all)")
    a = ap.parse_args()
    if a.parse:
        parse(a.parse, a.rings.split(",") if a.rings else None)
    elif a.run:
        run(a.rings.split(",") if a.rings else None)
    else:
        ap.error("--run or --parse DIR")
