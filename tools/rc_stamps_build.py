#!/usr/bin/env python3
"""Development tool: builds tools/abl/libgcrl_rcstamps.so = the library with device-clock stamps at the section boundaries of
rowchain_ddpg_kernel (first K-role and first P-role workgroup), read back by tools/rc_stamps.py.  The product build carries
no stamps: this script patches a temporary copy of csrc/rowchain.hip."""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
src = open(os.path.join(CSRC, "rowchain.hip")).read()
# the kernel's body lives in rowchain_ddpg_body.inc (shared with the population kernel): inlined into the single-agent kernel, which is
# the first to include it, so that the stamps below land in that kernel only
INC = '#include "rowchain_ddpg_body.inc"\n'
assert src.count(INC) == 2, "rowchain.hip no longer includes the DDPG body twice: follow it here"
src = src.replace(INC, open(os.path.join(CSRC, "rowchain_ddpg_body.inc")).read(), 1)


def after(anchor, stamp, nth=0):
    global src
    idx = -1
    for _ in range(nth + 1):
        idx = src.index(anchor, idx + 1)
    end = idx + len(anchor)
    src = src[:end] + f"\n    RC_STAMP({stamp});" + src[end:]


HEAD = "template <int RG, bool LM>\n__global__ __launch_bounds__(kRowThreads) void rowchain_ddpg_kernel(RowChainArgs a) {"
assert src.count(HEAD) == 1, "rowchain_ddpg_kernel's head moved: follow it here"
src = src.replace(HEAD,
                  "__device__ unsigned long long g_rc_stamps[2][32];\n"
                  "#define RC_STAMP(i) do { if (threadIdx.x == 0 && (blockIdx.x == 0 || (int)blockIdx.x == (a.k_split ? 2 : 1) * a.nblk_k)) g_rc_stamps[blockIdx.x == 0 ? 0 : 1][i] = wall_clock64(); } while (0)\n"
                  + HEAD, 1)
# P role (the plain DDPG branch)
marks_p = [
    ("    const float* src_da = a.critic[0].Wt + a.critic[0].wt[0] + (long long)S * H;   // rows S..S+A-1 of W0^T", 0, "start"),
    ("    else h = mlp_hidden<RG>(a.actor, X0, X1, X2, ldl, part + R * 16, a.hA, BH, row0, rv, XS);", 2, "actor hidden"),
    ("    if (tid < R * A) { const int r = tid / A, o = tid - r * A; X0[r * ldl + S + o] = sm[r * 16 + o]; }\n    __syncthreads();", 3, "actor head + act"),
    ("    else h = mlp_hidden<RG>(a.critic[0], X0, X1, X2, ldl, part + R * 16, a.hC2, BH, row0, rv);", 4, "critic hidden"),
    ("    else g0 = grad_chain<RG>(a.critic[0], h, X1, X2, ldl, part + R * 16, a.hC2, nullptr, BH, row0, rv);", 7, "critic dX chain"),
    ("    head_backward<RG>(XS, ldl, H, hw_a, A, sm2, a.gA + (a.actor.L - 1) * BH + row0 * H, rv);\n    __syncthreads();", 9, "da head, tanh', actor head bwd"),
    ("    else grad_chain<RG>(a.actor, XS, X1, X2, ldl, part + R * 16, a.hA, a.gA, BH, row0, rv);", 10, "actor dX chain"),
]
names_p = {}
for anchor, i, name in marks_p:
    after(anchor, i)
    names_p[i] = name
# "prologue done" and "head value + head bwd" in P
after("    if (fuse_q && tid < R) sm2[tid * 16] = (tid < rv) ? -1.0f / (float)B : 0.f;   // d(-mean Q)/dq, constant\n    __syncthreads();", 1)
after("      head_backward<RG>(h, ldl, H, hw_c, 1, sm2, nullptr, rv, sm3, hb[16]);\n      __syncthreads();", 6)
# K role
after("  if (role_k) {", 0)
after("      part[tid] = fminf(fmaxf(__fmul_rn(e, a.policy_noise), -a.noise_clamp), a.noise_clamp);\n    }\n    __syncthreads();", 1)
after("      h = mlp_hidden<RG>(a.tactor, X0, X1, X2, ldl, part + R * 16, nullptr, BH, row0, rv);", 2)
after("        X0[r * ldl + S + o] = act;\n      }\n      __syncthreads();\n    }", 3)
after("      h = mlp_hidden<RG>(a.tcritic[k], X0, X1, X2, ldl, part + R * 16, nullptr, BH, row0, rv);", 4)
after("      if (r < rv) a.y[row0 + r] = y;\n    }", 5)
after("      else h = mlp_hidden<RG>(a.critic[k], XS, X1, X2, ldl, part + R * 16, a.hC + (long long)k * a.critic[k].L * BH, BH, row0, rv);", 6)
after("      head_backward<RG>(h, ldl, H, hw_c + k * H, 1, sm2, gsave + (a.critic[k].L - 1) * BH + row0 * H, rv);\n      __syncthreads();", 7)
after("      else grad_chain<RG>(a.critic[k], h, X1, X2, ldl, part + R * 16, a.hC + (long long)k * a.critic[k].L * BH, gsave, BH, row0, rv);", 8)
src = src.replace("size_t rowchain_lds_bytes(int rg, int ldl, int A, int H, int C) {",
                  'extern "C" int gcrl_debug_rc_stamps(unsigned long long* out64) {\n'
                  "  return hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_rc_stamps), sizeof(unsigned long long) * 64) == hipSuccess ? 0 : -1;\n}\n"
                  "size_t rowchain_lds_bytes(int rg, int ldl, int A, int H, int C) {", 1)
tmp = os.path.join(CSRC, "_rowchain_stamps.hip")
open(tmp, "w").write(src)
out_dir = os.path.join(ROOT, "tools", "abl")
os.makedirs(out_dir, exist_ok=True)
try:
    subprocess.run(["make", "-C", CSRC, "-j8"], check=True, stdout=subprocess.DEVNULL)
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-ffp-contract=off"]
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-c", tmp, "-o", "/tmp/rowchain_st.o"], check=True, cwd=CSRC)
    objs = [o for o in glob.glob(os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "build", "*.o")) if not o.endswith("rowchain.o")]
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(out_dir, "libgcrl_rcstamps.so")] + objs + ["/tmp/rowchain_st.o", "-ldl"], check=True)
finally:
    os.remove(tmp)
print("built", os.path.join(out_dir, "libgcrl_rcstamps.so"))
