"""The energy-prioritised replay draw of a sample-mode ring (prioritise="energy", csrc/her_prio.hip) by the profiler's clock.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/her_prio_bench.py --run
    python tools/her_prio_bench.py --parse DIR

--run fills two rings of 1e6 records at PickAndPlace dims (S 23, A 4, G 3; k_future 4, relabel="sample", eight envs): one with
rng="device" (the gather computes its indices itself) and one with prioritise="energy" (three kinds of episode alternating: a
random walk, a lifted object, an object nobody moved).  Then, alternating the two rings, it issues the update engine's gather
(HERBuffer.gather_update) at 9 216 and 77 824 rows — on the second ring that is one her_prio_draw_kernel launch and the gather fed
its indices — then flushes of ONE T = 50 episode (push_episode), then flushes of EIGHT T = 50 episodes in one launch (push_batch,
all envs ending together), each on both rings.  Nothing is timed here: the kernel trace is.
--parse prints, per kernel and launch size, the launches after the warm-up ones: their number, median and range.  The two rings
launch her_gather_relabel_kernel at the same grid sizes: their launches alternate (device ring first) and are told apart by that;
her_energy_kernel has one grid: its one-episode and eight-episode launches are told apart by their order.  No GPU: --run fails."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, A, G, K, NENV = 23, 4, 3, 4, 8
CAP = 1_000_000
SIZES = ((256, 36), (256, 304))      # 9 216 and 77 824 rows: a trainer cycle's head-sized and main gather
WARM, ITERS = 10, 60


def run():
    import numpy as np
    import torch
    import gcrl_amd
    from oracle import her_oracle
    gen = np.random.default_rng(0)
    eps = []
    for kind in ("walk", "lift", "still"):
        st = her_oracle.synthetic_episode(gen, 50, S, A, G)
        ag = np.stack([x[6] for x in st]).astype(np.float32)
        if kind == "still":
            ag[:] = ag[0]
        elif kind == "lift":
            ag[:, 2] = ag[0, 2] + np.linspace(0.0, 0.2, 50, dtype=np.float32)
        eps.append([np.stack([x[j] for x in st]).astype(np.float32) for j in (0, 1, 2)] +
                   [np.array([x[3] for x in st], np.float32), np.zeros(50, np.float32), ag])
    rings = {}
    for name, kw in (("device", dict(rng="device")), ("energy", dict(rng="engine", prioritise="energy"))):
        buf = gcrl_amd.HERBuffer(CAP, 50, NENV, k_future=K, seed=1, relabel="sample", **kw)
        buf.compute_reward = her_oracle.sparse_reward
        for i in range(CAP // 50 + 2):
            buf.push_episode(0, *eps[i % 3])
        assert len(buf) == CAP
        rings[name] = buf
    torch.cuda.synchronize()
    for B, M in SIZES:
        for _ in range(WARM + ITERS):
            for name in ("device", "energy"):
                rings[name].gather_update(B, M)
    torch.cuda.synchronize()
    for _ in range(WARM + ITERS):
        for name in ("device", "energy"):
            rings[name].push_episode(1, *eps[0])
    torch.cuda.synchronize()
    ep = eps[1]
    for _ in range(WARM + ITERS):
        for name in ("device", "energy"):
            for t in range(50):
                rows = lambda j: torch.from_numpy(np.repeat(ep[j][t:t + 1], NENV, axis=0)).cuda()
                rings[name].push_batch(rows(0), np.repeat(ep[1][t:t + 1], NENV, axis=0), rows(2), np.full(NENV, ep[3][t], np.float32),
                                       np.full(NENV, t == 49), np.repeat(ep[5][t:t + 1], NENV, axis=0))
    torch.cuda.synchronize()
    print("her_prio_bench: done")


NAMES = ("her_prio_draw_kernel", "her_energy_kernel", "her_gather_relabel_kernel", "her_flush_sample_kernel")


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
    out = {}
    for (key, grid), v in rows.items():
        v.sort()
        if key == "her_gather_relabel_kernel":               # the two rings alternate, the device ring first
            tail = v[-2 * ITERS:]
            out[f"{key} rng=device", grid], out[f"{key} tree-drawn indices", grid] = tail[0::2], tail[1::2]
        elif key == "her_energy_kernel":                     # ... the one-episode flushes, then (after their warm-up) the eight-episode ones
            out[f"{key} 8 episodes", grid] = v[-ITERS:]
            out[f"{key} 1 episode", grid] = v[-(2 * ITERS + WARM):-(ITERS + WARM)]
        elif key == "her_flush_sample_kernel":               # both rings flush: every second launch is the energy ring's
            if len(v) >= 2 * (WARM + ITERS):
                out[f"{key} (energy ring)", grid] = v[-2 * ITERS:][1::2]
        elif len(v) >= ITERS:
            out[key, grid] = v[-ITERS:]
    for (key, grid), v in sorted(out.items()):
        dur = [x[1] / 1e3 for x in v]
        if dur:
            print(f"{key:46s} grid {grid:8d} threads: {len(dur)} launches, median {statistics.median(dur):7.2f} us, "
                  f"range {min(dur):7.2f} .. {max(dur):7.2f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--parse", metavar="DIR")
    a = ap.parse_args()
    if a.parse:
        parse(a.parse)
    elif a.run:
        run()
    else:
        ap.error("--run or --parse DIR")
