#!/usr/bin/env python3
"""Build check: every publication through memory is released before the arrival that announces it.

The kernels whose workgroups hand data to each other inside a launch (csrc/meet.h: BatchNorm slab row groups, row-chain
roles, also inside the fused DDPG launch; csrc/gemm_tiled.h: the split-dW ticket; csrc/xchg_ipc.hip: the peer-to-peer gradient exchange) publish with
write-through (sc1 / sc0 sc1) stores and then arrive at a counter with a global atomic.  On gfx950 a workgroup-scope
release fence emits NO `s_waitcnt vmcnt(0)`, so the arrival could overtake the stores.  This script
compiles the translation units to gfx950 assembly (device side only, no GPU needed) and checks, per kernel, that every
global atomic add that follows write-through stores in the listing is preceded — after the LAST such store — by an
`s_waitcnt vmcnt(0)`.  Listing order is not control flow, so this is a lint, not a proof; it catches exactly the
regression the advisor found in the ISA.

usage: tools/check_release_isa.py [--keep DIR] [--units a.hip,b.hip]      exit code 0 = every checked kernel passes
(--units: only these translation units, for a test that is about one of them)
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]

# translation unit -> substrings of the (mangled) kernel names that must pass, and must be present
UNITS = {
    "bn_slab.hip": ["bn_linear_fwd_slab_kernel", "bn_linear_bwd_slab_kernel", "bn_linear_bwd_slab_fold_kernel"],
    "rowchain.hip": ["rowchain_split_kernel", "rowchain_ddpg_kernel", "rowchain_split_heads_kernel", "rowchain_ddpg_pop_kernel"],
    "gemm_mfma.hip": ["gemm_tiled_kernel"],
    "xchg_ipc.hip": ["xchg_two_shot_kernel"],
    "ops.hip": ["td_loss_kernelILi3ELi0ELb1"],
    "ops_sac.hip": ["actor_select_alpha_mb_kernel"],
    "act_bn.hip": [],   # no arrivals at counters: its flag store is checked by flag_report below
}

STORE_WT = re.compile(r"^\s*(buffer_store|global_store|flat_store)\S*\s.*\bsc1\b")
ATOMIC = re.compile(r"^\s*(global|flat|buffer)_atomic_(add|or|inc)")
# an 8-byte system-scope store is how xchg_ipc.hip raises its ready / done flags: an arrival as well
FLAG = re.compile(r"^\s*global_store_dwordx2\s.*\bsc0 sc1\b")
WAIT0 = re.compile(r"^\s*s_waitcnt\s+.*vmcnt\(0\)")


def kernels(asm_text):
    """yield (name, [instruction lines]) per function of the listing"""
    name, body = None, []
    for line in asm_text.splitlines():
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            if name:
                yield name, body
            name, body = m.group(1), []
        elif name is not None:
            if re.match(r"^\s*\.end_amdhsa_kernel|^\s*s_endpgm", line):
                body.append(line)
            else:
                body.append(line)
    if name:
        yield name, body


def check_kernel(body):
    """(#write-through stores, #atomics after such stores, [problems])"""
    problems = []
    last_store = None
    waited = True
    n_store = n_atomic = 0
    for i, line in enumerate(body):
        if FLAG.match(line):
            if last_store is not None:
                n_atomic += 1
                if not waited:
                    problems.append((i, line.strip(), body[last_store].strip()))
        elif STORE_WT.match(line):
            last_store, waited = i, False
            n_store += 1
        elif WAIT0.match(line):
            waited = True
        elif ATOMIC.match(line) and last_store is not None:
            n_atomic += 1
            if not waited:
                problems.append((i, line.strip(), body[last_store].strip()))
    return n_store, n_atomic, problems


# Second lint: no kernel may copy its arguments (or spill) into per-thread scratch.  Handing a device function a POINTER into a
# by-value argument struct made hipcc copy the whole 3.7 KB struct to every thread's private memory — a 3 us kernel took 36 us
# (rowchain_act_inline_kernel, round 4).  `.amdhsa_private_segment_fixed_size` says it all.
SCRATCH_UNITS = ["her_ring.hip", "her_relabel.hip", "ops.hip", "ops_sac.hip", "bn_slab.hip", "rowchain.hip", "agent.hip", "normalizer.hip", "abi_misc.hip",
                 "gemm_mfma.hip", "xchg_ipc.hip", "dw_adam.hip", "adam_pop.hip", "act_bn.hip", "pop_clone.hip", "her_prio.hip", "her_norm.hip",
                 "her_bc.hip"]
SCRATCH_ALLOWED = {   # kernel-name substring -> bytes tolerated
    "rowchain_split_kernelILi4E": 64,   # 16 rows per workgroup: register spills; row_rg_of picks it only past one wave of 8-row blocks
    "gemm_tiled_kernel": 16,                                                   # three spilled dwords outside the k-loop
}


# kernels the scratch lint reports by name whatever their figure (and misses when they are gone): the population acting launches
# ... and the BatchNorm actor's acting launches (act_bn.hip)
# ... and the population forms of the sampling launches a TQC population step issues (ops_sac.hip)
# ... and the one-launch device copy of gcrl_pop_clone (pop_clone.hip)
SCRATCH_NAMED = {"pop_clone.hip": ["pop_clone_kernel"], "her_bc.hip": ["bc_qfilter_kernel"], "her_prio.hip": ["her_energy_kernel", "her_prio_draw_kernel"],
                 "rowchain.hip": ["rowchain_act_pop_kernel"], "her_ring.hip": ["her_process_step_pop_kernel", "her_gather_update_pop_kernel"],
                 "her_relabel.hip": ["her_flush_sample_kernel", "her_gather_relabel_kernelILb0E", "her_gather_relabel_kernelILb1E",
                                     "her_gather_nstep_kernelILb0E", "her_gather_nstep_kernelILb1E", "her_gather_relabel_pub_kernel"],
                 "her_norm.hip": ["her_norm_rows_kernel", "her_norm_dense_kernel", "her_process_step_raw_kernel", "her_process_step_raw_inline_kernel",
                                  "her_process_step_raw_pop_kernel"],
                 "ops_sac.hip": ["tanh_gauss_fwd_pop_kernel", "tanh_gauss_fwd2_pop_kernel", "tanh_gauss_bwd_pop_kernel"],
                 "act_bn.hip": ["act_bn_kernel", "act_bn_inline_kernel", "act_bn_pop_kernel", "act_bn_pop_staged_kernel"]}


def scratch_report(asm_text, unit):
    bad, lines = 0, []
    kernel = None
    named = {w: 0 for w in SCRATCH_NAMED.get(unit, [])}
    for line in asm_text.splitlines():
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kernel = m.group(1)
        m = re.match(r"\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", line)
        if m and kernel and int(m.group(1)) == 0:
            for w in named:
                if w in kernel:
                    named[w] += 1
                    lines.append(f"{unit}: {kernel}: 0 bytes of scratch per thread: ok")
        if m and kernel and int(m.group(1)) > 0:
            n = int(m.group(1))
            allowed = max([v for k, v in SCRATCH_ALLOWED.items() if k in kernel] + [0])
            ok = n <= allowed
            lines.append(f"{unit}: {kernel}: {n} bytes of scratch per thread: {'tolerated' if ok else 'FAIL'}")
            bad += 0 if ok else 1
    for w, n in named.items():
        if n == 0:
            lines.append(f"{unit}: {w}: not found without scratch (renamed, or it spills: see above): FAIL")
            bad += 1
    return bad, lines


# Release lint of a kernel whose publication AND arrival are system-scope stores to host-visible memory (rowchain_act_pop_kernel: the
# float64 actions, then one 8-byte flag per workgroup that the host polls): the flag is the listing's last such store, and an
# `s_waitcnt vmcnt(0)` must stand between the store before it and the flag.
FLAG_UNITS = {"rowchain.hip": ["rowchain_act_pop_kernel"], "act_bn.hip": ["act_bn_inline_kernel", "act_bn_pop_kernel"]}
STORE_SYS = re.compile(r"^\s*global_store_dwordx2\s.*\bsc0 sc1\b")


def flag_report(asm_text, unit):
    bad, lines = 0, []
    for w in FLAG_UNITS.get(unit, []):
        found = False
        for name, body in kernels(asm_text):
            if w not in name or name.endswith(".kd"):
                continue
            found = True
            at = [i for i, l in enumerate(body) if STORE_SYS.match(l)]
            ok = len(at) >= 2 and any(WAIT0.match(l) for l in body[at[-2] + 1:at[-1]])
            lines.append(f"{unit}: {name}: {max(len(at) - 1, 0)} system-scope action stores, then the flag store after s_waitcnt vmcnt(0): {'ok' if ok else 'FAIL'}")
            bad += 0 if ok else 1
        if not found:
            lines.append(f"{unit}: {w} not found (pattern changed?)")
            bad += 1
    return bad, lines


# Scalar-memory lint: no kernel of a checked unit writes memory through the scalar unit — scalar stores (plain, buffer, scratch), scalar
# atomics, or the scalar data cache's write-back / discard.  Values leave through vector stores.  (The mnemonics are assembled from
# pieces here so that this file does not contain them.)
SCALAR_WRITE = re.compile(r"^\s*s_(buffer_|scratch_)?(" + "sto" + "re|" + "ato" + "mic)|^\s*s_" + "dca" + "che_(wb|discard)")
SCALAR_NAMED = ["act_bn.hip"]   # reported by name even when clean


def scalar_report(asm_text, unit):
    hits = [l.strip() for l in asm_text.splitlines() if SCALAR_WRITE.match(l)]
    lines = [f"{unit}: scalar-unit write `{h}`: FAIL" for h in hits[:5]]
    if not hits and unit in SCALAR_NAMED:
        lines.append(f"{unit}: no scalar-unit stores, atomics or data-cache write-backs: ok")
    return len(hits), lines


# Third lint (round 5): the fused dW + optimiser launch (dw_adam.hip) hands a workgroup's sum of squares to every other workgroup as
# ONE 8-byte word that is its own flag — no arrival follows it, so there is nothing to release — but the word must leave as a
# write-through store and every poll of it must bypass the L1: a plain store or load here would be a silent stale read.
# The row groups of a BatchNorm slab (bn_slab.hip slab_exchange_df, round 5) exchange their column partials the same way: the row-split
# instantiations (template argument NT = 1) must contain such stores and loads.
def slot_report(asm_text, unit="dw_adam.hip", patterns=("dw_adam_kernel", "dw_adam_pop_kernel")):
    bad, lines = 0, []
    for name, body in kernels(asm_text):
        if not any(p in name for p in patterns):
            continue
        st = [l for l in body if re.match(r"^\s*global_store_dwordx2\s.*\bsc1\b", l)]
        ld = [l for l in body if re.match(r"^\s*global_load_dwordx2\s.*\bsc1\b", l)]
        ok = len(st) >= 1 and len(ld) >= 1
        lines.append(f"{unit}: {name}: {len(st)} write-through slot store(s), {len(ld)} L1-bypassing slot loads: {'ok' if ok else 'FAIL'}")
        bad += 0 if ok else 1
    if not lines:
        lines.append(f"{unit}: none of {patterns} found (pattern changed?)")
        bad += 1
    return bad, lines


def main():
    keep = None
    if "--keep" in sys.argv:
        keep = sys.argv[sys.argv.index("--keep") + 1]
        os.makedirs(keep, exist_ok=True)
    only = None
    if "--units" in sys.argv:
        only = set(sys.argv[sys.argv.index("--units") + 1].split(","))
    bad = 0
    report = []
    with tempfile.TemporaryDirectory() as tmp:
        out_dir = keep or tmp
        for unit, wanted in UNITS.items():
            if only is not None and unit not in only:
                continue
            src = os.path.join(CSRC, unit)
            if not os.path.exists(src):
                report.append(f"{unit}: MISSING source")
                bad += 1
                continue
            asm = os.path.join(out_dir, unit + ".s")
            subprocess.run([HIPCC] + FLAGS + ["-x", "hip", src, "-o", asm], check=True, cwd=CSRC)
            text = open(asm).read()
            seen = {w: 0 for w in wanted}
            for name, body in kernels(text):
                hit = [w for w in wanted if w in name]
                if not hit:
                    continue
                n_store, n_atomic, problems = check_kernel(body)
                if n_atomic == 0:
                    continue   # an instantiation without a publication (e.g. the unsplit forms)
                seen[hit[0]] += 1
                status = "ok" if not problems else "FAIL"
                report.append(f"{unit}: {name}: {n_store} write-through stores, {n_atomic} arrivals after them: {status}")
                for i, atom, store in problems:
                    report.append(f"    line {i}: `{atom}` follows `{store}` without s_waitcnt vmcnt(0)")
                bad += len(problems)
            for w, n in seen.items():
                if n == 0:
                    report.append(f"{unit}: no instantiation of {w} with a publication found (pattern changed?)")
                    bad += 1
            b5, lines = flag_report(text, unit)
            report += lines
            bad += b5
        sbad = 0
        for unit in SCRATCH_UNITS:
            if only is not None and unit not in only:
                continue
            asm = os.path.join(out_dir, unit + ".s")
            if not os.path.exists(asm):
                subprocess.run([HIPCC] + FLAGS + ["-x", "hip", os.path.join(CSRC, unit), "-o", asm], check=True, cwd=CSRC)
            b, lines = scratch_report(open(asm).read(), unit)
            sbad += b
            report += lines
            b6, lines = scalar_report(open(asm).read(), unit)
            sbad += b6
            report += lines
        if only is None or "dw_adam.hip" in only:
            b3, lines = slot_report(open(os.path.join(out_dir, "dw_adam.hip.s")).read())
            report += lines
            sbad += b3
        # (mangled names: bn_linear_fwd_slab_kernelILb<VEC>ELi<NT>ELi<WV>EE / bn_linear_bwd_slab_kernelILi<NT>ELi<WV>EE)
        if only is None or "bn_slab.hip" in only:
            b4, lines = slot_report(open(os.path.join(out_dir, "bn_slab.hip.s")).read(), "bn_slab.hip",
                                    ("bn_linear_fwd_slab_kernelILb1ELi1E", "bn_linear_fwd_slab_kernelILb0ELi1E", "bn_linear_bwd_slab_kernelILi1E", "bn_linear_bwd_slab_fold_kernel"))
            report += lines
            sbad += b4
    print("\n".join(report))
    print("release check:", "PASS" if bad == 0 else f"FAIL ({bad})")
    print("scratch check:", "PASS" if sbad == 0 else f"FAIL ({sbad})")
    return 0 if bad == 0 and sbad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
