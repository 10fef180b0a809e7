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
--members P [P ...]: a DDPG population of P members at the same network on a DeviceGoalEnvGroup, N in {8, 32} envs per member: aggregate
env-steps/s of pop.collect (three launches per vector step for all members) against the same P standalone agents' own collect calls
issued one after another (3 P launches per vector step) — what the code could do before pop.collect, measured in the same run;
seven alternating samples.  With --run: the population's steps for the profiler; --parse then also lists the population kernels.
--run issues, for the profiler, STEPS collect steps at every N; nothing is timed there.  --parse prints, per kernel, the launches
after the warm-up ones: number, median, range in us.  No --pmc in that run.
--kind reach|push|pick|glide (default reach): the env kind of every mode above.  `pick` has the headline's own dimensions (S 23 = obs 20 +
goal 3, A 4), so --kind pick times the on-device loop on the network the project is measured on; its host path steps the numpy
definition tests/dev_env_pick_ref.py.  `glide` (S 19, A 3) steps tests/dev_env_glide_ref.py there.
--practice: agent.collect without and with practice=GoalProposer(...) (defaults: capacity 8192, 16 candidates) at every N, alternating in
one process, seven samples each: env-steps/s of both, and the proposer's stats.  With --run: for the profiler, N 256 and C 16 with the
archive pre-loaded to L = 8192 and then to L = 65536, six roll-overs each; --parse DIR --practice lists goal_propose_kernel and
goal_archive_append_kernel per L.
No GPU: --cost, --practice and --run fail."""
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
KIND = "reach"
DIMS = dict(reach=(7, 3), push=(13, 3), pick=(20, 4), glide=(16, 3))      # obs_dim, action_dim per kind
H, L, B = 256, 3, 256
NS = (8, 32, 256)
SAMPLES, WARM = 7, 10
HOST_STEPS = {8: 100, 32: 50, 256: 10}        # vector steps of a host-loop sample (its env is a Python loop over the envs)
DEV_STEPS = 500
STEPS = 300
NAMES = ("env_step_kernel", "rowchain_act_kernel", "her_process_step_kernel", "her_flush_kernel")
POP_NS = (8, 32)
POP_NAMES = ("env_step_pop_kernel", "rowchain_act_pop_kernel", "her_process_step_pop_kernel")


def _set_kind(kind):
    global KIND, D, A
    KIND = kind
    D, A = DIMS[kind]


def _ref_env(n):
    """the numpy definition of the kind: the host path's env"""
    if KIND == "pick":
        import dev_env_pick_ref as PK
        return PK.RefPickEnv(n, seed=3, max_steps=T, threshold=THR)
    if KIND == "glide":
        import dev_env_glide_ref as GL
        return GL.RefGlideEnv(n, seed=3, max_steps=T, threshold=THR)
    import dev_env_ref as E
    return E.RefEnv(KIND, n, seed=3, max_steps=T, threshold=THR)


def _normalizers(ag):
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    from oracle import her_oracle
    ag.buffer.obs_normalizer = DeviceRunningNormalizer(D)
    ag.buffer.dg_normalizer = DeviceRunningNormalizer(G)
    ag.buffer.compute_reward = her_oracle.sparse_reward


def _population(P, n, max_len=100_000):
    """a DDPG population on a group, and the same P agents standalone with an env each (same configs and seeds)"""
    import gcrl_amd
    from gcrl_amd.src.synthetic import agent_config
    cfgs = [agent_config("DDPG", hidden_dim=H, layer_count=L, batch_size=B, max_len=max_len, k_future=4) for _ in range(P)]
    seeds = list(range(1, P + 1))
    pop = gcrl_amd.DDPGPopulation(D + G, A, cfgs, n, 40, rng="engine", seeds=seeds)
    solo = [gcrl_amd.DDPG(D + G, A, c, None, nenvs=n, gradient_step=40, rng="engine", seed=s) for c, s in zip(cfgs, seeds)]
    for ag in pop.members + solo:
        _normalizers(ag)
    group = gcrl_amd.DeviceGoalEnvGroup(KIND, P, n, seeds, max_steps=T, threshold=THR)
    envs = [gcrl_amd.DeviceGoalEnv(KIND, n, seed=s, max_steps=T, threshold=THR) for s in seeds]
    return pop, group, solo, envs


def members_cost(ps, out):
    import torch
    lines = ["# aggregate env-steps/s of P DDPG agents (H 256 x 3, batch 256, %s dimensions: S %d, A %d), N envs each; %d alternating samples of %d vector steps" %
             (KIND, D + G, A, SAMPLES, DEV_STEPS),
             "# (i) the P standalone agents' collect calls, one after another   (ii) pop.collect on a DeviceGoalEnvGroup"]
    for P in ps:
        for n in POP_NS:
            pop, group, solo, envs = _population(P, n)
            pop.collect(group, T)
            for ag, env in zip(solo, envs):
                ag.collect(env, T)
            torch.cuda.synchronize()
            a, b = [], []
            for _ in range(SAMPLES):
                t0 = time.perf_counter()
                for ag, env in zip(solo, envs):
                    ag.collect(env, DEV_STEPS)
                torch.cuda.synchronize(); dt = time.perf_counter() - t0
                a.append(P * n * DEV_STEPS / dt)
                t0 = time.perf_counter(); pop.collect(group, DEV_STEPS); torch.cuda.synchronize(); dt = time.perf_counter() - t0
                b.append(P * n * DEV_STEPS / dt)
            med = statistics.median
            lines.append("P %2d N %3d  (i) standalone collects %10.0f [%.0f .. %.0f]   (ii) pop.collect %10.0f [%.0f .. %.0f]   (ii)/(i) %.2fx   "
                         "us per vector step (i) %.1f (ii) %.1f" % (P, n, med(a), min(a), max(a), med(b), min(b), max(b), med(b) / med(a),
                                                                    1e6 * P * n / med(a), 1e6 * P * n / med(b)))
            lines.append("            pop collect counts: %s" % pop.collect_counts())
            del pop, group, solo, envs
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def members_run(ps):
    import torch
    for P in ps:
        for n in POP_NS:
            pop, group, _, _ = _population(P, n)
            pop.collect(group, T)
            torch.cuda.synchronize()
            pop.collect(group, STEPS)
            torch.cuda.synchronize()


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
    lines = ["# env-steps/s of one vector-env collection loop, DDPG H 256 x 3, batch 256, %s dimensions (S %d, A %d); %d alternating samples" %
             (KIND, D + G, A, SAMPLES),
             "# (i) observe_act + numpy ref env + process_step per step; 'engine' leaves the Python env's own time out   (ii) agent.collect"]
    for n in NS:
        host, dev = _agent(n), _agent(n)
        ref = _ref_env(n)
        env = gcrl_amd.DeviceGoalEnv(KIND, n, seed=3, max_steps=T, threshold=THR)
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
        env = gcrl_amd.DeviceGoalEnv(KIND, n, seed=3, max_steps=T, threshold=THR)
        ag.collect(env, WARM)
        torch.cuda.synchronize()
        ag.collect(env, STEPS)
        torch.cuda.synchronize()


PRACTICE_LS = (8192, 65536)
PRACTICE_NAMES = ("goal_propose_kernel", "goal_archive_append_kernel")


def practice_cost(out):
    import torch
    import gcrl_amd
    lines = ["# env-steps/s of agent.collect without and with practice=GoalProposer() (capacity 8192, 16 candidates, radius 0.05, share 0.5, min_fill 256),",
             "# DDPG H 256 x 3, batch 256, %s dimensions (S %d, A %d); %d alternating samples of %d vector steps" % (KIND, D + G, A, SAMPLES, DEV_STEPS)]
    for n in NS:
        plain, prac = _agent(n), _agent(n)
        e0, e1 = (gcrl_amd.DeviceGoalEnv(KIND, n, seed=3, max_steps=T, threshold=THR) for _ in range(2))
        prop = gcrl_amd.GoalProposer(seed=1)
        plain.collect(e0, 2 * T)
        prac.collect(e1, 2 * T, practice=prop)
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(SAMPLES):
            t0 = time.perf_counter(); plain.collect(e0, DEV_STEPS); torch.cuda.synchronize(); dt = time.perf_counter() - t0
            a.append(n * DEV_STEPS / dt)
            t0 = time.perf_counter(); prac.collect(e1, DEV_STEPS, practice=prop); torch.cuda.synchronize(); dt = time.perf_counter() - t0
            b.append(n * DEV_STEPS / dt)
        med = statistics.median
        lines.append("N %4d  collect %10.0f [%.0f .. %.0f]   collect(practice=) %10.0f [%.0f .. %.0f]   ratio %.3f   us per vector step %.1f / %.1f" %
                     (n, med(a), min(a), max(a), med(b), min(b), max(b), med(b) / med(a), 1e6 * n / med(a), 1e6 * n / med(b)))
        lines.append("        proposer: len %d, %s; collect counts: %s" % (len(prop), prop.stats(), prac.collect_counts()))
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def practice_run():
    """for the profiler: N 256, C 16, the archive pre-loaded to L entries (a full archive of capacity L), six roll-overs per L"""
    import numpy as np
    import torch
    import gcrl_amd
    from gcrl_amd.src.goal_propose import STATE_HEADER
    n = 256
    for L in PRACTICE_LS:
        ag = _agent(n)
        env = gcrl_amd.DeviceGoalEnv(KIND, n, seed=3, max_steps=T, threshold=THR)
        prop = gcrl_amd.GoalProposer(capacity=L, candidates=16, radius=0.05, share=1.0, min_fill=L, seed=1)
        blob = prop.save_state()
        blob[:STATE_HEADER.itemsize].view(STATE_HEADER)["len"] = L
        blob[STATE_HEADER.itemsize:].view(np.float32)[:] = np.random.default_rng(L).uniform(-0.3, 0.3, 3 * L).astype(np.float32)
        prop.load_state(blob)
        ag.collect(env, 6 * T, practice=prop)
        torch.cuda.synchronize()
        assert prop.stats()["patched"] == 6 * n, prop.stats()


def practice_parse(d):
    rows = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                key = next((k for k in PRACTICE_NAMES if k in r.get("Kernel_Name", "")), None)
                if key:
                    rows.setdefault(key, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    for key, v in sorted(rows.items()):     # --run --practice goes through PRACTICE_LS in order with the same number of launches each
        v = [d for _, d in sorted(v)]
        per = len(v) // len(PRACTICE_LS)
        for k, L in enumerate(PRACTICE_LS):
            part = v[k * per:(k + 1) * per]
            part = part[1:] if len(part) > 2 else part          # the first launch of a shape loads code
            if part:
                print("%-28s N 256 C 16 L %6d  launches %5d  median %.2f us  [%.2f .. %.2f]" % (key, L, len(part), statistics.median(part), min(part), max(part)))


def parse(d, pop_ps=None):
    rows = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                key = next((k for k in POP_NAMES + NAMES if k in name), None)
                if key:
                    rows.setdefault(key, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    # --run goes through NS in order with the same number of steps each: a kernel's launches in time order are len(NS) equal runs
    for key, v in sorted(rows.items()):
        v = [d for _, d in sorted(v)]
        if key in POP_NAMES:    # --run --members P ...: per P the shapes POP_NS in order, T warm-up steps and STEPS steps each
            shapes = [(P, n) for P in (pop_ps or [0]) for n in POP_NS]
            per = len(v) // len(shapes)
            for k, (P, n) in enumerate(shapes):
                part = v[k * per:(k + 1) * per][T:]
                if part:
                    print("%-28s P %2d N %3d  launches %5d  median %.2f us  [%.2f .. %.2f]" % (key, P, n, len(part), statistics.median(part), min(part), max(part)))
            continue
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
    ap.add_argument("--members", type=int, nargs="+", default=None, metavar="P", help="population sizes: pop.collect against P standalone collect calls")
    ap.add_argument("--kind", default="reach", choices=sorted(DIMS), help="the env kind; pick has the headline's dimensions (S 23, A 4)")
    ap.add_argument("--practice", action="store_true", help="collect without and with practice=GoalProposer(); with --run / --parse: the proposer's kernels")
    a = ap.parse_args()
    _set_kind(a.kind)
    if a.practice:
        if a.run:
            practice_run()
        elif a.parse:
            practice_parse(a.parse)
        else:
            practice_cost(a.out)
        sys.exit(0)
    if a.members and not (a.run or a.parse):
        members_cost(a.members, a.out)
    if a.cost:
        cost(a.out)
    if a.run:
        members_run(a.members) if a.members else run()
    if a.parse:
        parse(a.parse, a.members)
