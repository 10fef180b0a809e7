#!/usr/bin/env python3
"""Device-resident prioritised replay against the host-drawn parity mode (the parent's behaviour), same process.

A TD3 agent with buffer_type="PER" at H 256 / B 256 on full rings of 1e5 and 1e6 rows; `per_draw="device"` against
`per_draw="host"` in alternating rounds; steps/s per round (wall clock around `update_many(step, G)` calls, device synchronised at
the end of the round), median and min-max per side.  One JSON line per ring size, appended to --out.  A speed-up is only to be
claimed where the two ranges do not overlap.

    python tools/per_bench.py --out profiles/r15_device_per.jsonl
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/per_bench.py --trace-run     # the three new kernels, a run of its own
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gcrl_amd  # noqa: E402
from oracle.agent_oracle import make_config  # noqa: E402

S, A, H, B, G = 25, 4, 256, 256, 10


def make(mode: str, rows: int):
    cfg = make_config("TD3", buffer_type="PER", max_len=rows, hidden_dim=H, batch_size=B, alpha=0.6, beta=0.4, beta_end=100000,
                      policy_noise=0.2)
    ag = gcrl_amd.TD3Agent(S, A, cfg, None, nenvs=1, gradient_step=G, rng="engine", seed=7, per_draw=mode)
    gen = np.random.default_rng(1)
    blk = 4096
    s = torch.from_numpy(gen.standard_normal((blk, S)).astype(np.float32)).cuda()
    a = gen.uniform(-1, 1, (blk, A)).astype(np.float32)
    for i in range(rows):
        j = i % blk
        ag.push(s[j], a[j], -1.0 if i % 3 else 0.0, s[(j + 1) % blk], i % 50 == 49)
    assert len(ag.buffer) == rows
    return ag


def run(ag, step0: int, steps: int) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(0, steps, G):
        ag.update_many(step0 + k, G)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", default="100000,1000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-run", action="store_true", help="device mode only, 1e5 rows, 200 steps, nothing timed (for rocprofv3)")
    args = ap.parse_args()
    if args.trace_run:
        ag = make("device", 100000)
        for k in range(0, 200, G):
            ag.update_many(1 + k, G)
        torch.cuda.synchronize()
        print(json.dumps(dict(trace_run=True, launches=int(gcrl_amd._ffi.lib.gcrl_per_launches(ag.buffer.handle)))))
        return
    for rows in (int(x) for x in args.rings.split(",")):
        sides = {m: make(m, rows) for m in ("host", "device")}
        np.random.seed(3)
        step = {m: 1 for m in sides}
        for m, ag in sides.items():
            run(ag, step[m], args.warmup)
            step[m] += args.warmup
        rates = {m: [] for m in sides}
        for r in range(args.rounds):
            for m in (("host", "device") if r % 2 == 0 else ("device", "host")):
                rates[m].append(run(sides[m], step[m], args.steps))
                step[m] += args.steps
        rec = dict(bench="per_device_vs_host", kind="TD3", H=H, B=B, S=S, A=A, ring_rows=rows, steps_per_round=args.steps, rounds=args.rounds,
                   steps_per_call=G, device=torch.cuda.get_device_name(0))
        for m in sides:
            rec[m] = dict(steps_per_s_median=statistics.median(rates[m]), steps_per_s_min=min(rates[m]), steps_per_s_max=max(rates[m]),
                          rounds=rates[m])
        rec["ranges_overlap"] = not (rec["device"]["steps_per_s_min"] > rec["host"]["steps_per_s_max"] or
                                     rec["host"]["steps_per_s_min"] > rec["device"]["steps_per_s_max"])
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del sides


if __name__ == "__main__":
    main()
