"""Aggregate update throughput of a DDPG, TD3, SAC or TQC population (src/population.py) against the same P agents stepped one after another
in the same process.  One JSON line per (shape, P, form):

    python tools/population_bench.py [--kind DDPG|TD3|SAC|TQC] [--shapes cfg1,headline] [--members 1,2,4,8] [--calls 50] [--warmup 5] [--out FILE]
    python tools/population_bench.py --kind SAC --shapes cfg5,sac_h64 --update-rounds 5     (both sides alive, timed in alternation: median, min-max)
    python tools/population_bench.py --kind TQC --members 1,2,4,8 --update-rounds 5           (shapes tqc_h64 and tqc_h256: five critics, two dropped)

Each agent trains from its own HER ring of synthetic episodes, `gradient_step` (40) steps per update call as the trainer does
(src/env.py:384-385).  Timing: hipEvents on the stream the updates run on, around `calls` calls after `warmup` untimed ones and
a device synchronise; steps per member = calls x 40.  Forms: "population" (one DDPGPopulation / TD3Population.update_many per
call) and "sequential" (each standalone agent's update_many per call, in member order).  TD3 (--kind TD3; its lines carry
"kind": "TD3") steps its actor every second step with target smoothing on (policy_noise 0.2, noise_clamp 0.5).

    python tools/population_bench.py --acting [--kind DDPG|TD3] [--shapes cfg1,headline] [--members 1,2,4,8,16] [--rounds 5] [--steps 3000]

times the ACTING side instead: per vector-env step of 8 envs, `pop.observe_act` + `pop.process_step` ("population") against the same
members' own `observe_act` + `process_step` made one after another ("members"), device normalisers, an episode of every env ending
every 50th step so that the flush launches are in.  Both sides run in one process, alternating round by round; wall-clock time per
round (the calls wait for their results or are host-bound), a device synchronise inside each round's bracket.  One JSON line per
configuration: median and min-max of the rounds, in microseconds per vector step, per side.

    python tools/population_bench.py --acting --kind SAC [--shapes sac_h64,cfg5] [--members 2,4,8,16] [--rounds 5] [--steps 3000]

times a SAC population's `observe_act` alone (process_step is the same merged launch on both sides): the merged launch
(gcrl_pop_observe_act_bn) against the same population with `MERGE_ACTING_FROM` forced above P (the members' own one-launch entries in
member order), each side of each round in a fresh child process, the sides alternating; wall clock per call, the Python wrapper
included.  One JSON line per (shape, P).

    python tools/population_bench.py --clone [--kinds DDPG,TD3,SAC,TQC] [--shapes cfg1,headline] [--members 4,16] [--rounds 5] [--out profiles/r13_pbt_clone.jsonl]

times `pop.exploit` of a quarter of the members (one launch for all pairs, src/population.py) against the only way the tree had before:
the members' save_state / load_state round trip through host memory (with the ring: through a file), pair by pair — both in the same
process on the same population, in alternating rounds; wall clock and device time (events around the calls) per call, median and
min-max of the rounds, with and without the replay ring, and the bytes the clone moves.  One JSON line per (kind, shape, P, ring).

    python tools/population_bench.py --gather [--kind DDPG] [--shapes cfg1,headline] [--members 2,4,8,16] [--rounds 5] [--calls 50] [--out profiles/r14_pop_gather.jsonl]

times the replay side of an update call: ONE population, `merge_gather` toggled (one population gather launch per call against the
members' own gather launches), the same process, the sides alternating round by round; wall clock per `update_many` call (a device
synchronise inside each round's bracket) at two call lengths, n = 40 and n = 1.  One JSON line per (shape, P, n): median and min-max
of the rounds per side, in microseconds per call, and whether the two ranges overlap."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gcrl_amd  # noqa: E402
from oracle import her_oracle  # noqa: E402
from oracle.agent_oracle import make_config  # noqa: E402

SHAPES = {   # bench.py WORKLOADS: ddpg_reach_b256 (cfg 1) and the ddpg_pickplace_b256 headline
    "cfg1": dict(S=10, A=3, H=64, L=3, B=256),
    "headline": dict(S=23, A=4, H=256, L=3, B=256),
    "cfg5": dict(S=28, A=4, H=256, L=3, B=512),      # sac_slide_b512
    "sac_h64": dict(S=10, A=3, H=64, L=3, B=256),
    "tqc_h64": dict(S=10, A=3, H=64, L=3, B=64),      # --kind TQC's defaults: a small shape and one at H 256 / B 256
    "tqc_h256": dict(S=28, A=4, H=256, L=3, B=256),
}
GSTEP = 40


KINDS = {"DDPG": (gcrl_amd.DDPGPopulation, gcrl_amd.DDPG, {}),
         "TD3": (gcrl_amd.TD3Population, gcrl_amd.TD3Agent, dict(ac_update_freq=2, policy_noise=0.2, noise_clamp=0.5)),
         "SAC": (gcrl_amd.SACPopulation, gcrl_amd.SACAgent, dict(ac_update_freq=2)),
         "TQC": (gcrl_amd.TQCPopulation, gcrl_amd.TQCAgent, dict(ac_update_freq=2, num_critics=5, top_quantiles_to_drop=2))}


def _cfgs(sh, P, kind="DDPG"):
    return [make_config(kind, hidden_dim=sh["H"], layer_count=sh["L"], batch_size=sh["B"], max_len=100_000, gamma=0.98,
                        tau=0.05, grad_clip=10.0, actor_lr=1e-3 * (1 + 0.1 * i), critic_lr=1e-3 * (1 + 0.1 * i), **KINDS[kind][2])
            for i in range(P)]


def _fill(ag, sh, i):
    gen = np.random.default_rng(1000 + i)
    for ep in range(12):
        for st in her_oracle.synthetic_episode(gen, 50, sh["S"], sh["A"]):
            ag.push_her(ep % 2, *st)


def _time(step_fn, calls, warmup):
    for c in range(warmup):
        step_fn(1 + c * GSTEP)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for c in range(calls):
        step_fn(1 + (warmup + c) * GSTEP)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, time.perf_counter() - t0


def run(shape, P, calls, warmup, kind="DDPG"):
    sh = SHAPES[shape]
    cfgs = _cfgs(sh, P, kind)
    seeds = list(range(7, 7 + P))
    out = []
    pop_cls, agent_cls = KINDS[kind][:2]
    pop = pop_cls(sh["S"], sh["A"], cfgs, 2, GSTEP, rng="engine", seeds=seeds)
    for i, m in enumerate(pop.members):
        _fill(m, sh, i)
    forms = [m.meetings() for m in pop.members]
    dev_s, wall_s = _time(lambda s0: pop.update_many(s0, GSTEP), calls, warmup)
    out.append(dict(form="population", dev_s=dev_s, wall_s=wall_s, member_meeting_forms=forms[0]))
    del pop
    solo = [agent_cls(sh["S"], sh["A"], c, None, nenvs=2, gradient_step=GSTEP, rng="engine", seed=s) for c, s in zip(cfgs, seeds)]
    for i, a in enumerate(solo):
        _fill(a, sh, i)

    def seq(s0):
        for a in solo:
            a.update_many(s0, GSTEP)
    dev_s, wall_s = _time(seq, calls, warmup)
    out.append(dict(form="sequential", dev_s=dev_s, wall_s=wall_s, member_meeting_forms=solo[0].meetings()))
    del solo
    steps = calls * GSTEP
    for r in out:
        r.update(shape=shape, members=P, steps_per_member=steps, calls=calls, warmup_calls=warmup,
                 agg_steps_per_s=round(P * steps / r["dev_s"], 1), us_per_step_per_member=round(r["dev_s"] / (P * steps) * 1e6, 3),
                 **{k: sh[k] for k in ("S", "A", "H", "L", "B")})
        r["dev_s"], r["wall_s"] = round(r["dev_s"], 6), round(r["wall_s"], 6)
        if kind != "DDPG":
            r["kind"] = kind
    out[0]["speedup_vs_sequential"] = round(out[1]["dev_s"] / out[0]["dev_s"], 3)
    return out


def run_rounds(shape, P, calls, warmup, kind, rounds):
    """population and sequential agents alive together, timed in alternation for `rounds` rounds: median and min-max of the aggregate rate"""
    sh = SHAPES[shape]
    cfgs = _cfgs(sh, P, kind)
    seeds = list(range(7, 7 + P))
    pop_cls, agent_cls = KINDS[kind][:2]
    pop = pop_cls(sh["S"], sh["A"], cfgs, 2, GSTEP, rng="engine", seeds=seeds)
    solo = [agent_cls(sh["S"], sh["A"], c, None, nenvs=2, gradient_step=GSTEP, rng="engine", seed=s) for c, s in zip(cfgs, seeds)]
    for i in range(P):
        _fill(pop.members[i], sh, i)
        _fill(solo[i], sh, i)

    def seq(s0):
        for a in solo:
            a.update_many(s0, GSTEP)
    steps = calls * GSTEP
    rates = dict(population=[], sequential=[])
    for r in range(rounds):
        for form, fn in (("population", lambda s0: pop.update_many(s0, GSTEP)), ("sequential", seq)):
            dev_s, _ = _time(fn, calls, warmup if r == 0 else 1)
            rates[form].append(P * steps / dev_s)
    merged, alone = pop.launch_counts()
    out = []
    for form, v in rates.items():
        v = sorted(v)
        out.append(dict(bench="update_rounds", kind=kind, shape=shape, members=P, form=form, rounds=rounds, steps_per_member_per_round=steps,
                        agg_steps_per_s_median=round(v[len(v) // 2], 1), agg_steps_per_s_min=round(v[0], 1), agg_steps_per_s_max=round(v[-1], 1),
                        forms=pop.forms() if form == "population" else solo[0].meetings(), **{k: sh[k] for k in ("S", "A", "H", "L", "B")}))
    out[0].update(launch_positions_merged=merged, launch_positions_alone=alone,
                  speedup_median=round(out[0]["agg_steps_per_s_median"] / out[1]["agg_steps_per_s_median"], 3),
                  ranges_overlap=not (out[0]["agg_steps_per_s_min"] > out[1]["agg_steps_per_s_max"] or out[0]["agg_steps_per_s_max"] < out[1]["agg_steps_per_s_min"]))
    return out


def run_acting(shape, P, rounds, steps, kind="DDPG", nenvs=8):
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    sh = SHAPES[shape]
    G = 3
    D = sh["S"] - G
    cfgs = _cfgs(sh, P, kind)
    seeds = list(range(7, 7 + P))
    pop_cls, agent_cls = KINDS[kind][:2]
    pop = pop_cls(sh["S"], sh["A"], cfgs, nenvs, GSTEP, rng="engine", seeds=seeds)
    for m in pop.members:
        m.buffer.obs_normalizer = DeviceRunningNormalizer(D)
        m.buffer.dg_normalizer = DeviceRunningNormalizer(G)
        m.buffer.compute_reward = her_oracle.sparse_reward
    gen = np.random.default_rng(5)
    K = 64    # distinct vector steps, cycled (rows differ from call to call)
    f = lambda *shp: gen.standard_normal(shp).astype(np.float32)
    data = [[(dict(observation=f(nenvs, D), achieved_goal=f(nenvs, G), desired_goal=f(nenvs, G)),
              dict(observation=f(nenvs, D), achieved_goal=f(nenvs, G), desired_goal=f(nenvs, G)),
              -(gen.random(nenvs) > 0.5).astype(np.float32)) for _ in range(P)] for _ in range(K)]
    none, alld = [np.zeros(nenvs, bool)] * P, [np.ones(nenvs, bool)] * P
    ms = pop.members

    def population(k, dn):
        d = data[k % K]
        acts = pop.observe_act([x[0]["observation"] for x in d], [x[0]["desired_goal"] for x in d])
        pop.process_step([x[0] for x in d], [a.astype(np.float32) for a in acts], [x[1] for x in d], [x[2] for x in d], dn)

    def members(k, dn):
        d = data[k % K]
        for m, x, dd in zip(ms, d, dn):
            a = m.observe_act(x[0]["observation"], x[0]["desired_goal"])
            m.process_step(x[0], a.astype(np.float32), x[1], x[2], dd)

    sides = {"population": population, "members": members}
    t = {k: [] for k in sides}
    k = 0
    for rnd in range(-1, rounds):          # round -1: warm-up, untimed
        for name, fn in sides.items():
            n = steps if rnd >= 0 else 200
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                k += 1
                fn(k, alld if k % 50 == 0 else none)
            torch.cuda.synchronize()
            if rnd >= 0:
                t[name].append((time.perf_counter() - t0) / n * 1e6)
    counts = pop.acting_counts()
    r = dict(bench="acting", kind=kind, shape=shape, members=P, nenvs=nenvs, rounds=rounds, steps_per_round=steps,
             acting_counts=counts, merged=bool(counts[1]), **{k: sh[k] for k in ("S", "A", "H", "L", "B")})
    for name, v in t.items():
        r[name + "_us_per_vector_step"] = dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2),
                                               rounds=[round(x, 2) for x in v])
    r["members_over_population"] = round(float(np.median(t["members"]) / np.median(t["population"])), 3)
    return [r]


def acting_sac_child(shape, members, steps, merged, nenvs=8):
    """One side of one round, in this (fresh) process: wall clock per `pop.observe_act` call (sampled actions, device normalisers,
    the Python wrapper included; the call returns the actions, so it has waited for them) of a SAC population with the merged launch
    on (`MERGE_ACTING_FROM = 2`) or forced off (above P: the members' own one-launch entries in member order)."""
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    sh = SHAPES[shape]
    G = 3
    D = sh["S"] - G
    out = []
    for P in members:
        pop = gcrl_amd.SACPopulation(sh["S"], sh["A"], _cfgs(sh, P, "SAC"), nenvs, GSTEP, rng="engine", seeds=list(range(7, 7 + P)))
        pop.MERGE_ACTING_FROM = 2 if merged else P + 1
        gen = np.random.default_rng(5)
        for m in pop.members:
            m.buffer.obs_normalizer = DeviceRunningNormalizer(D)
            m.buffer.dg_normalizer = DeviceRunningNormalizer(G)
            m.buffer.obs_normalizer.update(gen.standard_normal((64, D)).astype(np.float32))
        K = 64    # distinct vector steps, cycled (rows differ from call to call)
        f = lambda *shp: gen.standard_normal(shp).astype(np.float32)
        data = [([f(nenvs, D) for _ in range(P)], [f(nenvs, G) for _ in range(P)]) for _ in range(K)]
        torch.manual_seed(3)
        for k in range(300):
            pop.observe_act(*data[k % K])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            pop.observe_act(*data[k % K])
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / steps * 1e6
        counts = pop.acting_counts()
        assert bool(counts[1]) == bool(merged), counts
        out.append(dict(shape=shape, members=P, merged=bool(merged), us_per_call=round(us, 2), acting_counts=counts))
        del pop
    return out


def run_acting_sac(shapes, members, rounds, steps, write):
    """`rounds` alternating rounds of fresh child processes per shape — merged launch, then member by member — each child timing every
    population size; one JSON line per (shape, P): median and min-max of the rounds per side, and whether the merged side's whole
    range lies below the other's (the rule that sets SACPopulation.MERGE_ACTING_FROM)."""
    import subprocess
    for shape in shapes:
        t = {(side, P): [] for side in ("merged", "members") for P in members}
        for rnd in range(rounds):
            for side in ("merged", "members"):
                cmd = [sys.executable, os.path.abspath(__file__), "--kind", "SAC", "--acting", "--child", side, "--shapes", shape,
                       "--members", ",".join(str(P) for P in members), "--steps", str(steps)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
                for line in r.stdout.splitlines():
                    if line.startswith("CHILD "):
                        c = json.loads(line[6:])
                        t[(side, c["members"])].append(c["us_per_call"])
                print(f"# {shape} round {rnd} {side}: " + ", ".join(f"P={P}: {t[(side, P)][-1]}" for P in members), flush=True)
        sh = SHAPES[shape]
        for P in members:
            r = dict(bench="sac_pop_acting", kind="SAC", shape=shape, members=P, nenvs=8, rounds=rounds, steps_per_round=steps,
                     **{k: sh[k] for k in ("S", "A", "H", "L", "B")})
            for side in ("merged", "members"):
                v = t[(side, P)]
                r[side + "_us_per_call"] = dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2), rounds=v)
            r["members_over_merged"] = round(r["members_us_per_call"]["median"] / r["merged_us_per_call"]["median"], 3)
            r["merged_range_below_members"] = r["merged_us_per_call"]["max"] < r["members_us_per_call"]["min"]
            write(json.dumps(r))


class _AgentStateHeader(__import__("ctypes").Structure):
    """csrc/agent.hip AgentStateHeader: the head of a gcrl_agent_save_state blob (it says how many floats each state vector holds)"""
    _c = __import__("ctypes")
    _fields_ = ([("magic", _c.c_uint32), ("version", _c.c_uint32)] + [(k, _c.c_int32) for k in ("kind", "S", "A", "H", "L", "B", "C", "pad")] +
                [(k, _c.c_int64) for k in ("n_params", "n_grads", "bn_n", "t_actor", "t_critic", "t_alpha")] +
                [("lr_actor", _c.c_double), ("lr_critic", _c.c_double), ("rng_ctr", _c.c_uint64)])


def run_gather(shape, P, kind, rounds, calls, warmup):
    sh = SHAPES[shape]
    pop_cls = KINDS[kind][0]
    pop = pop_cls(sh["S"], sh["A"], _cfgs(sh, P, kind), 2, GSTEP, rng="engine", seeds=list(range(7, 7 + P)))
    for i, m in enumerate(pop.members):
        _fill(m, sh, i)
    out = []
    step = 1
    for n in (GSTEP, 1):
        us = {True: [], False: []}
        for r in range(rounds):
            for merged in (True, False):
                pop.merge_gather = merged
                for _ in range(warmup if r == 0 else 2):
                    pop.update_many(step, n)
                    step += n
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    pop.update_many(step, n)
                    step += n
                torch.cuda.synchronize()
                us[merged].append((time.perf_counter() - t0) / calls * 1e6)
        a, b = sorted(us[True]), sorted(us[False])
        out.append(dict(bench="gather", kind=kind, shape=shape, members=P, steps_per_call=n, rounds=rounds, calls_per_round=calls,
                        merged_us_per_call_median=round(a[len(a) // 2], 2), merged_us_per_call_min=round(a[0], 2), merged_us_per_call_max=round(a[-1], 2),
                        members_us_per_call_median=round(b[len(b) // 2], 2), members_us_per_call_min=round(b[0], 2), members_us_per_call_max=round(b[-1], 2),
                        merged_whole_range_below=a[-1] < b[0], ranges_overlap=not (a[-1] < b[0] or b[-1] < a[0]),
                        gather_counts=list(pop.gather_counts()), **{k: sh[k] for k in ("S", "A", "H", "L", "B")}))
    return out


def _ring_segment_bytes(buf):
    """bytes of a ring clone's segments (csrc/her_ring.h): [nenvs][flush_len][RG] staged floats and len x RS row floats"""
    from gcrl_amd.src.buffer import FLUSH_LEN
    r16 = lambda x, m: (x + m - 1) // m * m
    S, A, G = buf._dims
    rw = r16(S + A, 4) + r16(S, 4) + 2
    return 4 * (buf.nenvs * FLUSH_LEN * r16(rw + G, 16) + len(buf) * r16(rw, 16))


def run_clone(shape, P, kind, rounds, reps, tmp):
    import ctypes as C
    from gcrl_amd._ffi import check, lib
    sh = SHAPES[shape]
    pop_cls = KINDS[kind][0]
    pop = pop_cls(sh["S"], sh["A"], _cfgs(sh, P, kind), 2, GSTEP, rng="engine", seeds=list(range(7, 7 + P)))
    for i, m in enumerate(pop.members):
        _fill(m, sh, i)
    pop.update_many(1, GSTEP)
    q = max(1, P // 4)
    pairs = [(i, P - 1 - i) for i in range(q)]
    n = int(lib.gcrl_agent_state_size(pop.members[0]._h))
    blob = np.empty(n, np.uint8)
    check(lib.gcrl_agent_save_state(pop.members[0]._h, blob.ctypes.data, n))
    hdr = _AgentStateHeader.from_buffer_copy(blob[:C.sizeof(_AgentStateHeader)].tobytes())
    agent_bytes = 4 * (hdr.n_params + 2 * hdr.n_grads + 2 * hdr.bn_n + 1)
    assert agent_bytes == n - C.sizeof(_AgentStateHeader), (agent_bytes, n)
    out = []
    for ring in (False, True):
        def clone():
            pop.exploit(pairs, copy_ring=ring)

        def host():
            for s, d in pairs:
                if ring:
                    pop.members[s].save_state(os.path.join(tmp, "m"))
                    pop.members[d].load_state(os.path.join(tmp, "m"))
                else:
                    check(lib.gcrl_agent_save_state(pop.members[s]._h, blob.ctypes.data, n))
                    check(lib.gcrl_agent_load_state(pop.members[d]._h, blob.ctypes.data, n))
        res = {"clone": ([], []), "host": ([], [])}
        clone(); host()
        for _ in range(rounds):
            for name, fn in (("clone", clone), ("host", host)):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res[name][0].append((time.perf_counter() - t0) / reps * 1e6)
                res[name][1].append(e0.elapsed_time(e1) / reps * 1e3)
        # what the kernel's segments hold: per pair the agent's state vectors (the named vectors the blob carries: parameters with their
        # targets, both Adam moments, BatchNorm running statistics, alpha), with the ring the staged records and the filled rows
        moved = q * agent_bytes + (q * _ring_segment_bytes(pop.members[0].buffer) if ring else 0)
        r = dict(bench="clone", kind=kind, shape=shape, members=P, pairs=q, ring=ring, rounds=rounds, calls_per_round=reps, bytes_moved=int(moved),
                 **{k: sh[k] for k in ("S", "A", "H", "L", "B")})
        for name in ("clone", "host"):
            for j, what in enumerate(("wall_us", "dev_us")):
                v = sorted(res[name][j])
                r[f"{name}_{what}"] = dict(median=round(float(np.median(v)), 2), min=round(v[0], 2), max=round(v[-1], 2))
        r["ranges_overlap_wall"] = not (r["clone_wall_us"]["max"] < r["host_wall_us"]["min"] or r["host_wall_us"]["max"] < r["clone_wall_us"]["min"])
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clone", action="store_true", help="time pop.exploit against the members' save_state / load_state round trip")
    ap.add_argument("--kinds", default="DDPG,TD3,SAC,TQC", help="--clone: the kinds to time")
    ap.add_argument("--reps", type=int, default=10, help="--clone: calls per round and side")
    ap.add_argument("--child", default=None, choices=["merged", "members"], help="(internal) --kind SAC --acting: one side of one round in this process")
    ap.add_argument("--kind", default="DDPG", choices=sorted(KINDS))
    ap.add_argument("--update-rounds", type=int, default=1, help="> 1: population and sequential agents timed in alternation this many times")
    ap.add_argument("--shapes", default="cfg1,headline")
    ap.add_argument("--members", default="1,2,4,8")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--acting", action="store_true", help="time observe_act + process_step instead of the update side")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3000, help="--acting: vector steps per round and side")
    ap.add_argument("--gather", action="store_true", help="time update_many with merge_gather on against off, same population")
    a = ap.parse_args()
    if a.gather:
        assert a.rounds >= 5 or os.environ.get("POP_BENCH_SHORT"), "at least five alternating rounds"
        members = "2,4,8,16" if a.members == "1,2,4,8" else a.members
        with (open(a.out, "a") if a.out else open(os.devnull, "w")) as f:
            for shape in a.shapes.split(","):
                for P in [int(x) for x in members.split(",")]:
                    for r in run_gather(shape, P, a.kind, a.rounds, a.calls, a.warmup):
                        line = json.dumps(r)
                        print(line, flush=True)
                        f.write(line + "\n")
                        f.flush()
        return
    if a.clone:
        import tempfile
        members = "4,16" if a.members == "1,2,4,8" else a.members
        with tempfile.TemporaryDirectory() as tmp, (open(a.out, "a") if a.out else open(os.devnull, "w")) as f:
            for kind in a.kinds.split(","):
                for shape in a.shapes.split(","):
                    for P in [int(x) for x in members.split(",")]:
                        for r in run_clone(shape, P, kind, a.rounds, a.reps, tmp):
                            line = json.dumps(r)
                            print(line, flush=True)
                            f.write(line + "\n")
                            f.flush()
        return
    if a.acting:
        assert a.rounds >= 5 and a.steps >= 3000 or os.environ.get("POP_BENCH_SHORT"), "at least five rounds of 3 000 vector steps"
        members = "1,2,4,8,16" if a.members == "1,2,4,8" else a.members
        if a.kind == "SAC":
            Ps = [int(x) for x in (("2,4,8,16" if a.members == "1,2,4,8" else a.members).split(","))]
            if a.child:
                for shape in a.shapes.split(","):
                    for c in acting_sac_child(shape, Ps, a.steps, a.child == "merged"):
                        print("CHILD " + json.dumps(c), flush=True)
                return
            with open(a.out, "a") if a.out else open(os.devnull, "w") as f:
                def write(line):
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                run_acting_sac(a.shapes.split(","), Ps, a.rounds, a.steps, write)
            return
        with open(a.out, "a") if a.out else open(os.devnull, "w") as f:
            for shape in a.shapes.split(","):
                for P in [int(x) for x in members.split(",")]:
                    for r in run_acting(shape, P, a.rounds, a.steps, a.kind):
                        line = json.dumps(r)
                        print(line, flush=True)
                        f.write(line + "\n")
                        f.flush()
        return
    assert a.calls * GSTEP >= 2000 or os.environ.get("POP_BENCH_SHORT"), "at least 2 000 timed steps per member"
    if a.kind == "TQC" and a.shapes == "cfg1,headline":
        a.shapes = "tqc_h64,tqc_h256"
    f = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        for P in [int(x) for x in a.members.split(",")]:
            for r in (run_rounds(shape, P, a.calls, a.warmup, a.kind, a.update_rounds) if a.update_rounds > 1 else run(shape, P, a.calls, a.warmup, a.kind)):
                line = json.dumps(r)
                print(line, flush=True)
                if f:
                    f.write(line + "\n")
                    f.flush()
    if f:
        f.close()


if __name__ == "__main__":
    main()
