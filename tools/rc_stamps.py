"""Section timeline of rowchain_ddpg_kernel (development tool): needs a library built with -DGCRL_RC_STAMPS
(GCRL_HIP_LIB=<that .so>); prints the device-clock stamps (10 ns ticks) the first K-role and the first P-role workgroup
left at their section boundaries during the LAST launch of a run of headline steps.  The K role's stamps are those of the one-role
critic phase (GCRL_NO_DDPG_KSPLIT=1): the two roles of the default form run rowchain_split_body, which carries no stamps.
GCRL_RC_GLOBAL_MUL=1 stamps the global-multiplier form of the kernel, the default its LDS-multiplier form.
Since round 38 the development build also stamps the END OF EVERY LAYER PASS of each role's first workgroup (the K target role, the K
online-critic role and the P role); those tables are printed first.  GCRL_RC_NO_WARM=1 stamps the launch without its riders."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="ddpg_pickplace_b256")
a = ap.parse_args()
w = dict(bench.WORKLOADS[a.workload], cap=100_000)
args = argparse.Namespace(no_graph=False, pipeline=-1, rng="engine")
agent, _, _ = bench.build_agent(w, args, 0, 0)
for c in range(5):
    agent.update_many(1 + 40 * c, 40)
torch.cuda.synchronize()
import gcrl_amd  # noqa: E402
lib = gcrl_amd._ffi.lib
out = (C.c_uint64 * 64)()
fn = lib.gcrl_debug_rc_stamps
fn.restype = C.c_int
assert fn(out) == 0
st = np.array(list(out), dtype=np.int64).reshape(2, 32)
names_k = {0: "start", 1: "prologue", 2: "target actor hidden", 3: "its head + action", 4: "target critic hidden", 5: "its head + y", 6: "critic hidden",
           7: "head, loss, head bwd", 8: "critic dX chain"}
names_p = {0: "start", 1: "prologue", 2: "actor hidden", 3: "actor head + action", 4: "critic hidden", 6: "Q head + head bwd", 7: "critic dX chain",
           9: "da head, tanh', actor head bwd", 10: "actor dX chain"}
# the two K roles of the default form (rowchain_split_body): entry and exit, on the P role's clock
if st[0][16] and st[1][0]:
    for name, i in (("K target role", 16), ("K online-critic role", 18)):
        print(f"{name}: entry at {(st[0][i] - st[1][0]) / 100:7.2f} us, exit at {(st[0][i + 1] - st[1][0]) / 100:7.2f} us of the P role's clock")
# per pass (round 38): the end of every layer pass of each role's first workgroup, in the order the role runs them
if hasattr(lib, "gcrl_debug_rc_pass"):
    out2 = (C.c_uint64 * 96)()
    lib.gcrl_debug_rc_pass.restype = C.c_int
    assert lib.gcrl_debug_rc_pass(out2) == 0
    ps = np.array(list(out2), dtype=np.int64).reshape(3, 32)
    L = int(w.get("layer_count", w.get("L", 3)))
    fw, bw = [f"layer {l}" for l in range(L)], [f"dX {l}" for l in range(L - 1, 0, -1)]
    walks = {0: [("target actor", fw), ("target critic", fw)], 1: [("critic", fw), ("critic", bw)],
             2: [("actor", fw), ("critic", fw), ("critic", bw), ("actor", bw)]}
    for row, role in ((0, "K target role"), (1, "K online-critic role"), (2, "P role")):
        labels = [f"{net} {p}" for net, ps_ in walks[row] for p in ps_]
        if not ps[row][0] or ps[row][len(labels) - 1] <= 0:
            continue
        print(f"{role}, per pass (end of pass on the P role's clock, time since the end of the role's pass before)")
        prev = None
        for i, name in enumerate(labels):
            t = ps[row][i]
            gap = "" if prev is None else f"   (+{(t - prev) / 100:5.2f})"
            print(f"  {name:24s} at {(t - st[1][0]) / 100:7.2f} us{gap}")
            prev = t
for role, names in ((0, names_k), (1, names_p)):
    t0 = st[role][0]
    print("role", "K" if role == 0 else "P")
    prev = t0
    if st[role][11]:   # (stamp 11: the kernel's first instruction, in front of the argument warm-up)
        print(f"  {'entry, before the argument warm-up':32s} at {(st[role][11] - t0) / 100:7.2f} us")
    for i in sorted(names):
        t = st[role][i]
        print(f"  {names[i]:32s} at {(t - t0) / 100:7.2f} us   (+{(t - prev) / 100:5.2f})")
        prev = t
