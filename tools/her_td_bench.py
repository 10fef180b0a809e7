"""What prioritise="td_error" (csrc/her_td.hip) costs a sample-mode HER ring's agent, and its launches by the profiler's clock.

    python tools/her_td_bench.py --cost
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/her_td_bench.py --run
    python tools/her_td_bench.py --parse DIR

--cost: two DDPG agents at PickAndPlace dims (S 23 + goal in the state, A 4, G 3), B 256, three hidden layers of 256, pipeline=0 (the
layer-per-launch schedule both run on), relabel="sample" rings of 1e6 rows filled to the brim; one without the keyword, one with.
Alternating in one process, seven samples each of CALLS update_many(step, 40) calls between two device synchronisations; prints the
median and range of us/step of both and the difference of the medians: the us/step the keyword adds (per step: a draw, a weights and
an update launch, a gather launched per step instead of per call, the weighted loss).
--run issues, for the profiler, STEPS steps of the agent with the keyword and FLUSHES one-episode flushes (each followed by its seed
launch); nothing is timed there.  --parse prints, per kernel, the launches after the warm-up ones: number, median, range.
No GPU: --cost and --run fail."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, A, G = 23, 4, 3
CAP, B, H, GS = 1_000_000, 256, 256, 40
SAMPLES, CALLS, WARM_CALLS = 7, 5, 3
STEPS, FLUSHES, WARM = 400, 60, 10
NAMES = ("her_td_seed_kernel", "her_td_update_kernel", "per_draw_kernel", "per_weights_kernel", "her_flush_sample_kernel", "her_gather_relabel_kernel")


def _agent(prioritise):
    import numpy as np
    import gcrl_amd
    from gcrl_amd.src.synthetic import agent_config
    from oracle import her_oracle
    cfg = agent_config("DDPG", hidden_dim=H, layer_count=3, batch_size=B, max_len=CAP, k_future=4)
    ag = gcrl_amd.DDPG(S, A, cfg, None, nenvs=2, gradient_step=GS, rng="engine", seed=1, relabel="sample", pipeline=0, prioritise=prioritise)
    ag.buffer.compute_reward = her_oracle.sparse_reward
    gen = np.random.default_rng(0)
    st = her_oracle.synthetic_episode(gen, 50, S, A, G)
    ep = [np.stack([x[j] for x in st]).astype(np.float32) for j in (0, 1, 2)] + [np.array([x[3] for x in st], np.float32), np.zeros(50, np.float32),
                                                                                   np.stack([x[6] for x in st]).astype(np.float32)]
    for _ in range(CAP // 50 + 2):
        ag.buffer.push_episode(0, *ep)
    assert len(ag.buffer) == CAP
    return ag, ep


def cost():
    import torch
    agents = {name: _agent(p)[0] for name, p in (("plain", None), ("td_error", "td_error"))}
    step = {k: 1 for k in agents}

    def calls(name, n):
        for _ in range(n):
            agents[name].update_many(step[name], GS)
            step[name] += GS
    for name in agents:
        calls(name, WARM_CALLS)
    torch.cuda.synchronize()
    us = {k: [] for k in agents}
    for _ in range(SAMPLES):
        for name in agents:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls(name, CALLS)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / (CALLS * GS))
    out = {k: dict(median=statistics.median(v), min=min(v), max=max(v), samples=[round(x, 2) for x in v]) for k, v in us.items()}
    out["added_us_per_step"] = out["td_error"]["median"] - out["plain"]["median"]
    out["config"] = dict(S=S, A=A, G=G, B=B, H=H, layers=3, pipeline=0, ring_rows=CAP, steps_per_call=GS, calls_per_sample=CALLS, samples=SAMPLES)
    print(json.dumps(out))


def run():
    import torch
    ag, ep = _agent("td_error")
    torch.cuda.synchronize()
    step = 1
    for _ in range((WARM * GS + STEPS) // GS):
        ag.update_many(step, GS)
        step += GS
    torch.cuda.synchronize()
    for _ in range(WARM + FLUSHES):
        ag.buffer.push_episode(1, *ep)
    torch.cuda.synchronize()
    print("her_td_bench: done")


def parse(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel trace under {d}")
    rows = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            key = next((n for n in NAMES if n in r["Kernel_Name"]), None)
            if key is not None:
                rows.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    for v in rows.values():
        v.sort()
    for key, v in sorted(rows.items()):
        keep = {"her_td_seed_kernel": FLUSHES, "her_flush_sample_kernel": FLUSHES}.get(key, STEPS)
        if key == "her_td_seed_kernel" or key == "her_flush_sample_kernel":
            dur = [x[1] / 1e3 for x in v[-keep:]]                      # the flushes come last
        else:
            first = [x for x in v if x[0] < rows["her_td_seed_kernel"][-FLUSHES][0]] if "her_td_seed_kernel" in rows else v
            dur = [x[1] / 1e3 for x in first[-keep:]]
        if dur:
            print(f"{key:28s} {len(dur):4d} launches, median {statistics.median(dur):7.2f} us, range {min(dur):7.2f} .. {max(dur):7.2f} us")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--parse", metavar="DIR")
    a = ap.parse_args()
    if a.parse:
        parse(a.parse)
    elif a.cost:
        cost()
    elif a.run:
        run()
    else:
        ap.error("--cost, --run or --parse DIR")
