#!/usr/bin/env python3
"""Development tool: builds tools/abl/libgcrl_rcstamps.so = the library with device-clock stamps at the section boundaries of
rowchain_ddpg_kernel_stream (the stream form of the fused DDPG launch at 4 rows per workgroup; first K-role and first P-role workgroup),
read back by tools/rc_stamps.py.  The loop-form kernels (GCRL_RC_NO_STREAM=1) carry none: an A/B of stamps against the parent needs the
parent tree's own build of this tool.  Every role's first workgroup also stamps the end of each of its layer passes (round 38: the K
target role, the K online-critic role and the P role, per pass).  `--nosave` builds tools/abl/libgcrl_rcstamps_nosave.so, a timing-only
variant whose results are wrong by construction (see below).  The product build carries no stamps: this script patches a temporary copy
of csrc/rowchain.hip."""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
src = open(os.path.join(CSRC, "rowchain.hip")).read()
# the kernel's body lives in rowchain_ddpg_body.inc (shared by the loop-form, stream-form and population kernels): inlined into the
# single-agent stream kernel, the second to include it, so that the stamps below land in that kernel only
INC = '#include "rowchain_ddpg_body.inc"\n'
assert src.count(INC) == 4, "rowchain.hip no longer includes the DDPG body four times: follow it here"
HEAD = "template <bool LM>\n__global__ __launch_bounds__(kRowThreads) void rowchain_ddpg_kernel_stream(RowChainArgs args) {"
assert src.count(HEAD) == 1, "rowchain_ddpg_kernel_stream's head moved: follow it here"
at = src.index(INC, src.index(HEAD))
assert src.count(INC, 0, at) == 1, "the stream kernel is no longer the second to include the body"
src = src[:at] + open(os.path.join(CSRC, "rowchain_ddpg_body.inc")).read() + src[at + len(INC):]


def after(anchor, stamp, nth=0):
    global src
    idx = -1
    for _ in range(nth + 1):
        idx = src.index(anchor, idx + 1)
    end = idx + len(anchor)
    src = src[:end] + f"\n    RC_STAMP({stamp});" + src[end:]


STUB = "#ifndef RC_STAMP\n#define RC_STAMP(i)   // (tools/rc_stamps_build.py: device-clock stamps of the development build)\n#endif\n"
assert src.count(STUB) == 1, "rowchain.hip's RC_STAMP stub moved: follow it here"
COND = "threadIdx.x == 0 && (blockIdx.x == 0 || (int)blockIdx.x == (A.k_split ? 2 : 1) * A.nblk_k)"
src = src.replace(STUB,
                  "__device__ unsigned long long g_rc_stamps[2][32];\n"
                  "#define RC_STAMP_AT(A, i) do { if (" + COND + ") g_rc_stamps[blockIdx.x == 0 ? 0 : 1][i] = wall_clock64(); } while (0)\n"
                  "#define RC_STAMP(i) RC_STAMP_AT(a, i)\n", 1)
# in front of the argument warm-up (stamp 11)
src = src.replace(HEAD, HEAD + "\n  RC_STAMP_AT(args, 11);", 1)
# the P role's stamps (the stream branch of the body) stand in the text as RC_STAMP(i): 0 start, 1 prologue, 2 actor hidden, 3 actor head +
# action, 4 critic hidden, 6 Q head + head bwd, 7 critic dX chain, 9 da head / tanh' / actor head bwd, 10 actor dX chain
# the two K roles of the default form run rowchain_split_body (phase 0, part 3): entry and exit of the first target-role workgroup
# (stamps 16, 17 of row 0) and of the first online-critic workgroup (18, 19), on the same device clock as the P role's
BODY = "  const bool merged = part == 3;                 // parts 1 and 2 in this launch (rowchain.h)\n"
assert src.count(BODY) == 1, "rowchain_split_body's head moved: follow it here"
src = src.replace(BODY, BODY + "  if (tid == 0 && phase == 0 && (bid == 0 || bid == nblk)) g_rc_stamps[0][bid == 0 ? 16 : 18] = wall_clock64();\n", 1)
T_END = "      else rc_meet(meet, 2 * C, false, &s_flag, a.status);\n    }\n"
assert src.count(T_END) == 1
src = src.replace(T_END, T_END + "    if (tid == 0 && bid == 0) g_rc_stamps[0][17] = wall_clock64();\n", 1)
O_END = "    else grad_chain<RG>(a.critic[k], XS, X1, X2, ldl, part_ + R * 16, hs, gsave, BH, row0, rv);\n"
assert src.count(O_END) == 1
src = src.replace(O_END, O_END + "    if (tid == 0 && bid == nblk) g_rc_stamps[0][19] = wall_clock64();\n", 1)
# K role of the one-role form (GCRL_NO_DDPG_KSPLIT=1)
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
                  'extern "C" int gcrl_debug_rc_pass(unsigned long long* out96) {\n'
                  "  return hipMemcpyFromSymbol(out96, HIP_SYMBOL(g_rc_pass), sizeof(unsigned long long) * 96) == hipSuccess ? 0 : -1;\n}\n"
                  "size_t rowchain_lds_bytes(int rg, int ldl, int A, int H, int C) {", 1)
# ---- per-pass stamps (round 38): every layer pass of the six walks (mlp_hidden, grad_chain, their _keep and _st forms) ends with a stamp
# of thread 0 into g_rc_pass[row][n], n counting the workgroup's passes in the order it runs them.  The row and the count live in two
# words of static LDS that only thread 0 touches; the stream kernel's entry sets them for the first workgroup of each role (row 0: K
# target role, or the one-role K; 1: K online-critic role; 2: P role), every other workgroup and kernel finds a row out of range and
# stamps nothing.  The passes of a role in order: K target = target actor 0..L-1, target critic 0..L-1; K online = critic 0..L-1, its dX
# chain L-1..1; P = actor 0..L-1, critic 0..L-1, critic dX L-1..1, actor dX L-1..1.
W0 = src.index("template <int RG>\n__device__ inline float* mlp_hidden(")
W1 = src.index("// stage `n` floats of global memory into LDS (all threads)")
walks, n_pass = re.subn(r"(rows_linear(?:_stream)?<[^;]*?\);)", r"{ \1 RC_PASS(); }", src[W0:W1], flags=re.S)
assert n_pass == 9, f"{n_pass} layer-pass statements in the six walks, 9 expected: follow them here"
src = (src[:W0] +
       "__device__ unsigned long long g_rc_pass[3][32];\n"
       "__shared__ int s_rc_row, s_rc_n;\n"
       "#define RC_PASS() do { if (threadIdx.x == 0) { const unsigned r_ = (unsigned)s_rc_row, n_ = (unsigned)s_rc_n;"
       " if (r_ < 3u && n_ < 32u) { g_rc_pass[r_][n_] = wall_clock64(); s_rc_n = (int)n_ + 1; } } } while (0)\n" + walks + src[W1:])
src = src.replace(HEAD + "\n  RC_STAMP_AT(args, 11);",
                  HEAD + "\n  RC_STAMP_AT(args, 11);\n"
                  "  if (threadIdx.x == 0) { const int b_ = (int)blockIdx.x, nk_ = args.nblk_k; s_rc_n = 0;\n"
                  "    s_rc_row = args.k_split ? (b_ == 0 ? 0 : (b_ == nk_ ? 1 : (b_ == 2 * nk_ ? 2 : -1))) : (b_ == nk_ ? 2 : (b_ == 0 ? 0 : -1));\n"
                  "    if (nk_ == 0 || args.nblk_p == 0) s_rc_row = -1; }   // the overlapped launch only: a call's last launch is the actor phase alone", 1)
assert "s_rc_row = args.k_split" in src
# every OTHER kernel of the file (loop-form, population, split, acting) reaches RC_PASS through the same walks, and static LDS keeps what
# an earlier kernel on the CU left there: each of them sets the row out of range at its entry, so only the stream kernel ever stamps
KERNEL_HEAD = re.compile(r"(__global__ __launch_bounds__\(kRowThreads\) void (\w+)\([^)]*\) \{\n)")
others = [m.group(2) for m in KERNEL_HEAD.finditer(src) if m.group(2) != "rowchain_ddpg_kernel_stream"]
assert len(others) == 10, f"{others}: ten other kernels with kRowThreads expected, follow them here"
src = KERNEL_HEAD.sub(lambda m: m.group(1) if m.group(2) == "rowchain_ddpg_kernel_stream" else m.group(1) + "  if (threadIdx.x == 0) s_rc_row = -1;\n", src)
# --nosave: the TIMING-ONLY variant of round 38's part 0 — the actor's forward and backward walks of the P role run with save = nullptr
# (hA / gA are not written: the step's results are WRONG by construction; never a product build), nothing else changed
if "--nosave" in sys.argv:
    for old, new in (("part + R * 16, a.hA, BH, row0, rv, nx_c0)", "part + R * 16, nullptr, BH, row0, rv, nx_c0)"),
                     ("KP, a.gA, BH, row0, rv, nx_none)", "KP, nullptr, BH, row0, rv, nx_none)"),
                     ("a.hA, a.gA, BH, row0, rv, nx_none)", "a.hA, nullptr, BH, row0, rv, nx_none)")):
        assert src.count(old) >= 1, old
        src = src.replace(old, new)
LIBNAME = "libgcrl_rcstamps_nosave.so" if "--nosave" in sys.argv else "libgcrl_rcstamps.so"
tmp = os.path.join(CSRC, "_rowchain_stamps.hip")
open(tmp, "w").write(src)
out_dir = os.path.join(ROOT, "tools", "abl")
OBJ = os.path.join(out_dir, LIBNAME[:-3] + ".o")
os.makedirs(out_dir, exist_ok=True)
try:
    subprocess.run(["make", "-C", CSRC, "-j8"], check=True, stdout=subprocess.DEVNULL)
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-ffp-contract=off"]
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-c", tmp, "-o", OBJ], check=True, cwd=CSRC)
    objs = [o for o in glob.glob(os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "build", "*.o")) if not o.endswith("rowchain.o")]
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(out_dir, LIBNAME)] + objs + [OBJ, "-ldl"], check=True)
finally:
    os.remove(tmp)
print("built", os.path.join(out_dir, LIBNAME))
