"""The gradient audit's case table, its inputs, its references and its bound: shared by tests/test_grad_ref.py (which checks,
without a GPU, that every case's seed reaches the coverage counts the case claims and keeps the near-kink cap) and
tests/test_gpu_gradient_audit.py (which runs the cases on the device).

A case is one `update(step)` from explicit parameters, batch and noise.  Shapes: the smallest that still reach each launch rule of
gcrl_agent_create (csrc/agent.hip: row_rg_of, the two-role critic phase of DDPG, td3_split_k_rule, sac_slab_rule / the slab's row
split, the row chain's H % 4, the fused dW + optimiser launch); `expect` names the form the case is there for, in the fields of
Agent.update_forms().  S, A come from SA: every S + A is off a multiple of 4 at least once, A = 1 and A = 5 exercise Apad.

Inputs: parameters 0.3 * standard_normal (as tests/test_gpu_parity.py's sweep), targets perturbed away from the online nets (a
kernel reading the wrong one shows), gamma 0.5 and rewards in {0, -1, -2} so that DDPG's target clamp [-1 / (1 - gamma), 0] is
reached at both ends at these widths, smoothing noise drawn at twice unit variance so that policy_noise 0.2 / noise_clamp 0.5
clamps on both sides.  The BatchNorm actors' heads are moderate, as in test_gpu_parity.py's wide-action case and tests/detdata.py
(log_std weights x 0.25, bias - 1, mean weights x 0.5): the reference's log(1 - tanh(x)^2 + 1e-8) amplifies one fp32 ulp of tanh by
2 |t| / (1 - t^2), and with saturated actions its own fp32 run is percents away from its fp64 run — a yardstick that holds nothing.
The log_std clamp is still reached: column 0's bias is 2.0, so about half of its rows sit above the upper clamp (std = e^2), and
that column's injected eps is scaled by 0.05 so that the action stays off saturation; where a case claims the lower clamp, column
1's bias is -20.0 and its eps scaled likewise (at std = exp(-20) the fp32 reference's log-prob loses eps^2 / 2 to cancellation:
only two cases claim it).  grad_clip 1e3: the clip is the optimiser audit's subject; inactive, the tuple's norms are the
gradients' own.

Bound (tests/fullsize.py's K_REF and RTOL, per quantity and PER PARAMETER TENSOR, W and b of every layer apart):
    max |hip - ref64|  <=  max(K_REF * e32, RTOL * scale)
e32: the largest max |ref32 - ref64| over the fp32 reference run on the batch in three row orders (as given, reversed, one fixed
permutation): one summation order is one draw of the rounding error.  scale: max |ref64| of the tensor; for the Linear bias in
front of a BatchNorm, whose fp64 gradient is analytically zero, the whole net's gradient max.
Kinks: units whose fp64 pre-activation lies within KINK_FACTOR x their layer's max |z32 - z64| of zero are listed (at most
KINK_CAP per case, none at B <= 64: the seed is changed until that holds); their flip vectors are fitted to the device's deviation
by tests/fullsize.explain_flips and subtracted before the bound is applied.
"""
from __future__ import annotations

from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

import grad_ref as gr
from fullsize import K_REF, RTOL, explain_flips

F32 = np.float32
SA = [(3, 1), (10, 3), (23, 4), (11, 5)]
KINK_FACTOR, KINK_CAP = 16.0, 12
GAMMA, GRAD_CLIP, CRITIC_LR, ACTOR_LR = 0.5, 1e3, 7e-4, 1e-3
MI355X_CUS = 256
CREATION_SWITCHES = ("GCRL_NO_DDPG_KSPLIT", "GCRL_NO_OPT_FUSE", "GCRL_RC_GLOBAL_MUL", "GCRL_NO_RC_MERGE", "GCRL_NO_BN_RSPLIT", "GCRL_NO_BN_SLAB",
                     "GCRL_NO_SPLIT_ROLES")
PROCESS_SWITCHES = ("GCRL_NO_TG_FOLD", "GCRL_NO_HEADS_FOLD", "GCRL_SLAB_MEET")

Case = namedtuple("Case", "id kind B H L S A step pipeline env proc weights ls_lo seed expect claims why")


def rows_per_workgroup(kind, B):
    """csrc/agent.hip row_rg_of, restated: 4 rows per workgroup until the phases' blocks pass 256, then 8, then 16."""
    phases, rg = (2 if kind == "DDPG" else 1), 1
    while rg < 4 and phases * ((B + 4 * rg - 1) // (4 * rg)) > 256:
        rg *= 2
    return 4 * rg


# seeds: found off-GPU (tests/test_grad_ref.py checks them): the first seed from 0 under which the case's claimed counts are all
# non-zero, no more than KINK_CAP units lie near a kink, and none does at B <= 64
SEEDS = {'ddpg-b20-h72-l4-s23a4': 2,
 'ddpg-b20-h72-l4-s23a4-no_ddpg_ksplit': 2,
 'ddpg-b20-h72-l4-s23a4-no_opt_fuse': 2,
 'ddpg-b20-h72-l4-s23a4-rc_global_mul': 2,
 'ddpg-b20-h72-l4-s23a4-p0': 2,
 'sac-b128-h16-l2-s3a1': 2,
 'sac-b512-h16-l2-s11a5': 2,
 'sac-b130-h64-l3-s10a3-p0': 1,
 'sac-b130-h64-l3-s10a3-p0-w': 1,
 'tqc-b40-h16-l2-s10a3': 1,
 'tqc-b513-h16-l2-s3a1': 1}


def table(cus=MI355X_CUS):
    """Every case of the audit.  cus: the device's compute units (the two-role critic phase of DDPG is admitted while 3 x blocks <=
    cus: its boundary shapes follow the device)."""
    out, k = [], [0]

    def add(kind, B, H, L, why, step=None, pipeline=None, env=(), proc=(), weights=False, ls_lo=False, sa=None, expect=None):
        S, A = SA[k[0] % 4] if sa is None else sa
        k[0] += 1
        step = step if step is not None else {"DDPG": 1, "TD3": 2, "SAC": 1, "TQC": 1}[kind]
        tag = "".join(f"-{e[5:].lower()}" for e in tuple(env) + tuple(proc)) + ("-p0" if pipeline == 0 else "") + ("-w" if weights else "") \
            + (f"-s{step}" if step != {"DDPG": 1, "TD3": 2, "SAC": 1, "TQC": 1}[kind] else "")
        cid = f"{kind.lower()}-b{B}-h{H}-l{L}-s{S}a{A}{tag}"
        chain = pipeline is None and H % 4 == 0 and kind != "TQC"
        rpw = rows_per_workgroup(kind, B)
        ex = dict(rowchain=int(chain))
        if chain:
            ex["rows_per_workgroup"] = rpw
            nblk = (B + rpw - 1) // rpw
            if kind == "DDPG":
                ex["ddpg_ksplit"] = int(3 * nblk <= cus and "GCRL_NO_DDPG_KSPLIT" not in env)
            if kind == "TD3":
                ex["split_k"] = int(nblk >= 256)
                ex["rc_merge_k"] = int(nblk >= 256 and "GCRL_NO_RC_MERGE" not in env)
            if kind == "SAC":
                ex["split_roles"] = int(nblk <= 256 and "GCRL_NO_SPLIT_ROLES" not in env)
                ex["rc_merge"] = int(ex["split_roles"] and "GCRL_NO_RC_MERGE" not in env)
            ex["opt_fuse"] = int("GCRL_NO_OPT_FUSE" not in env)
        if kind == "SAC":
            ex["bn_slab"] = int(chain and B <= 512 and H % 16 == 0 and "GCRL_NO_BN_SLAB" not in env) if pipeline is None else None
            if ex["bn_slab"] is None:
                del ex["bn_slab"]
            else:
                ex["bn_rsplit"] = 4 if (ex["bn_slab"] and B > 128 and "GCRL_NO_BN_RSPLIT" not in env) else 1
        ex.update(expect or {})
        gauss = kind in ("SAC", "TQC")
        claims = {"units_pos", "units_neg"}
        if B >= 20:
            claims |= {"terminal", "non_terminal"}
            claims |= {"DDPG": {"clamp_lo", "clamp_hi", "unclamped"}, "TD3": {"noise_lo", "noise_hi", "huber_saturated", "huber_quadratic", "min_is_0", "min_is_1"},
                       "SAC": {"min_is_0", "min_is_1", "log_std_hi", "log_std_inside"}, "TQC": {"log_std_hi", "log_std_inside"}}[kind]
            if kind == "SAC":
                claims |= {"actor_min_is_0", "actor_min_is_1"}
        if ls_lo:
            claims |= {"log_std_lo"}
        if chain and B % rpw:
            claims |= {"partial_block"}
        assert not ls_lo or (gauss and A >= 2)
        out.append(Case(cid, kind, B, H, L, S, A, step, pipeline, tuple(env), tuple(proc), weights, ls_lo, SEEDS.get(cid, 0), ex, frozenset(claims), why))

    n = cus // 3
    # ---- DDPG, row chain
    add("DDPG", 3, 4, 2, "fewer rows than one block", sa=(3, 1))
    add("DDPG", 6, 64, 1, "no hidden-to-hidden layer", sa=(10, 3))
    add("DDPG", 20, 72, 4, "LDS row stride off 64, more kept layers than two", sa=(23, 4))
    add("DDPG", 4 * n, 64, 2, "the two-role critic phase's last admitted shape", sa=(11, 5))
    add("DDPG", 4 * n + 1, 64, 2, "the two-role critic phase's first refused shape", sa=(11, 5))
    add("DDPG", 513, 16, 2, "8 rows per workgroup, last block 1 of 8", sa=(3, 1))
    add("DDPG", 1025, 16, 2, "16 rows per workgroup, last block 1 of 16", sa=(10, 3))
    for sw in ("GCRL_NO_DDPG_KSPLIT", "GCRL_NO_OPT_FUSE", "GCRL_RC_GLOBAL_MUL"):
        add("DDPG", 20, 72, 4, f"the (20, 72, 4) shape under {sw}", env=(sw,), sa=(23, 4))
        add("DDPG", 513, 16, 2, f"the (513, 16, 2) shape under {sw}", env=(sw,), sa=(3, 1))
    add("DDPG", 20, 72, 4, "step 40: Polyak before the actor phase", step=40, sa=(11, 5))
    # ---- DDPG, layer per launch
    add("DDPG", 20, 30, 2, "H % 4 != 0: the default schedule refuses the row chain", sa=(10, 3))
    add("DDPG", 20, 72, 4, "layer per launch", pipeline=0, sa=(23, 4))
    add("DDPG", 513, 16, 2, "layer per launch", pipeline=0, sa=(3, 1))
    add("DDPG", 130, 64, 3, "layer per launch", pipeline=0, sa=(11, 5))
    add("DDPG", 513, 16, 2, "layer per launch, importance weights", pipeline=0, weights=True, sa=(3, 1))
    add("DDPG", 130, 64, 3, "layer per launch, importance weights", pipeline=0, weights=True, sa=(11, 5))
    # ---- TD3 (ac_update_freq 2: step 1 critic-only, step 2 an actor step)
    add("TD3", 20, 64, 2, "critic-only step", step=1, sa=(10, 3))
    add("TD3", 20, 64, 2, "actor step", sa=(10, 3))
    add("TD3", 1020, 16, 1, "255 row blocks: below td3_split_k_rule", sa=(3, 1))
    add("TD3", 1021, 16, 1, "256 row blocks: the role-parallel critic phase", sa=(23, 4))
    add("TD3", 1025, 16, 1, "8 rows per workgroup, the split off again", sa=(11, 5))
    add("TD3", 1021, 16, 1, "the role-parallel critic phase as two launches", env=("GCRL_NO_RC_MERGE",), sa=(23, 4))
    add("TD3", 130, 64, 3, "layer per launch", pipeline=0, sa=(10, 3))
    add("TD3", 130, 64, 3, "layer per launch, importance weights", pipeline=0, weights=True, sa=(10, 3))
    # ---- SAC
    add("SAC", 40, 16, 2, "slab without the row split", sa=(10, 3))
    add("SAC", 128, 16, 2, "slab, the last batch without the row split", sa=(3, 1))
    add("SAC", 129, 16, 2, "slab row split, a second group of one row", sa=(23, 4))
    add("SAC", 512, 16, 2, "the last batch with the slab", sa=(11, 5))
    add("SAC", 513, 16, 2, "the first batch without the slab", sa=(10, 3))
    add("SAC", 40, 24, 2, "H % 16 != 0: GEMM + BatchNorm launches for the actor, row chain for the critics", ls_lo=True, sa=(23, 4))
    for sw in ("GCRL_NO_BN_RSPLIT", "GCRL_NO_BN_SLAB", "GCRL_NO_SPLIT_ROLES"):
        add("SAC", 129, 48, 3, f"under {sw}", env=(sw,), sa=(11, 5))
    for sw in PROCESS_SWITCHES:
        add("SAC", 129, 16, 2, f"under {sw} (read once per process: a child process)", proc=(sw,), sa=(23, 4))
        add("SAC", 40, 16, 2, f"under {sw} (read once per process: a child process)", proc=(sw,), sa=(10, 3))
    add("SAC", 130, 64, 3, "layer per launch", pipeline=0, sa=(10, 3))
    add("SAC", 130, 64, 3, "layer per launch, importance weights", pipeline=0, weights=True, sa=(10, 3))
    # ---- TQC, scalar critics (C = 5, drop 2)
    add("TQC", 40, 16, 2, "five critics", sa=(10, 3))
    add("TQC", 129, 24, 2, "five critics, A = 5", ls_lo=True, sa=(11, 5))
    add("TQC", 513, 16, 2, "five critics", sa=(3, 1))
    add("TQC", 129, 24, 2, "five critics, importance weights", weights=True, sa=(23, 4))
    assert len({c.id for c in out}) == len(out)
    return out


def by_id(cus=MI355X_CUS):
    return {c.id: c for c in table(cus)}


def hyper(case):
    kind = case.kind
    return dict(gamma=GAMMA, grad_clip=GRAD_CLIP, critic_lr=CRITIC_LR, policy_noise=0.2, noise_clamp=0.5, top_drop=2 if kind == "TQC" else 0,
                target_entropy={"SAC": -0.5 * case.A, "TQC": -float(case.A)}.get(kind, 0.0))


def config_overrides(case):
    """make_config(kind, **this): the engine's side of `hyper`."""
    over = dict(hidden_dim=case.H, layer_count=case.L, batch_size=case.B, max_len=2000, grad_clip=GRAD_CLIP, policy_noise=0.2, noise_clamp=0.5,
                ac_update_freq=2 if case.kind == "TD3" else 1, tau=0.05, actor_lr=ACTOR_LR, actor_lr_min=ACTOR_LR, critic_lr=CRITIC_LR,
                critic_lr_min=CRITIC_LR, gamma=GAMMA)
    if case.kind in ("SAC", "TQC"):
        over.update(alpha_min_steps=0.0, alpha_lr=1e-2)
    return over


def inputs(case, seed=None):
    """-> SimpleNamespace(nets, batch, noise, eps_next, eps_cur, weights, log_alpha, actor_step, alpha_step), numpy float32."""
    gen = np.random.default_rng(1000 + (case.seed if seed is None else seed))
    kind, B, S, A, H, L = case.kind, case.B, case.S, case.A, case.H, case.L
    gauss = kind in ("SAC", "TQC")
    C = gr.n_critics(kind)
    lay_a, lay_c = gr.layout("gauss" if gauss else "mlp", S, H, L, A), gr.layout("mlp", S + A, H, L, 1)
    nets = {"actor": (0.3 * gen.standard_normal(gr.numel(lay_a))).astype(F32)}
    if gauss:
        p = gr.split(nets["actor"], lay_a)                      # views: writes go to the flat vector
        p["log_std.weight"] *= F32(0.25)
        p["mean.weight"] *= F32(0.5)
        p["log_std.bias"] -= F32(1.0)
        p["log_std.bias"][0] = 2.0
        if case.ls_lo:
            p["log_std.bias"][1] = -20.0
    else:
        nets["target_actor"] = (nets["actor"] + 0.05 * gen.standard_normal(nets["actor"].size)).astype(F32)
    for i in range(C):
        nets[f"critic_{i}"] = (0.3 * gen.standard_normal(gr.numel(lay_c))).astype(F32)
        nets[f"target_critic_{i}"] = (nets[f"critic_{i}"] + 0.05 * gen.standard_normal(gr.numel(lay_c))).astype(F32)
    s, ns = gen.standard_normal((B, S)).astype(F32), gen.standard_normal((B, S)).astype(F32)
    a = np.tanh(gen.standard_normal((B, A))).astype(F32)
    r = -gen.choice([0.0, 1.0, 2.0], size=(B, 1), p=[0.3, 0.5, 0.2]).astype(F32)
    d = (gen.random((B, 1)) < 0.2).astype(F32)
    actor_step = kind != "TD3" or case.step % 2 == 0
    eps = [gen.standard_normal((B, A)).astype(F32) for _ in range(2)] if gauss else [None, None]
    for e in eps if gauss else ():
        e[:, :2 if case.ls_lo else 1] *= F32(0.05)
    return SimpleNamespace(nets=nets, batch=(s, a, r, ns, d),
                           noise=(2.0 * gen.standard_normal((B, A))).astype(F32) if kind == "TD3" else None,
                           eps_next=eps[0], eps_cur=eps[1],
                           weights=gen.uniform(0.2, 1.0, B).astype(F32) if case.weights else None,
                           log_alpha=-0.3 if gauss else 0.0, actor_step=actor_step, alpha_step=gauss and actor_step)


def step_of(case, inp):
    return gr.Step(case.kind, case.S, case.A, case.H, case.L, hyper(case), inp.nets, inp.batch, log_alpha=inp.log_alpha, weights=inp.weights,
                   noise=inp.noise, eps_next=inp.eps_next, eps_cur=inp.eps_cur, actor_step=inp.actor_step, alpha_step=inp.alpha_step)


def row_orders(B):
    return [None, np.arange(B)[::-1].copy(), np.random.default_rng(77).permutation(B)]


def references(case, inp, critics_after=None, flips=True):
    """-> SimpleNamespace(step, r64, r32 (three row orders), units (near-kink, listed), vectors (their flip vectors), cover)."""
    st = step_of(case, inp)
    if critics_after is None:
        # off-GPU: the fp32 reference's own stepped critics (tests/adam_ref.py) stand in for the engine's, for every run alike
        critics_after = st.run(torch.float32).critics_after
    r64 = st.run(torch.float64, critics_after=critics_after)
    r32 = [st.run(torch.float32, critics_after=critics_after, order=o) for o in row_orders(case.B)]
    units = gr.near_kink_units(r32[0], r64, KINK_FACTOR)
    cover = dict(r64.cover)
    if case.expect.get("rowchain"):
        cover["partial_block"] = case.B % case.expect["rows_per_workgroup"]
    vectors = st.flip_vectors(units, r64, critics_after=critics_after) if flips and len(units) <= KINK_CAP else []
    return SimpleNamespace(step=st, r64=r64, r32=r32, units=units, vectors=vectors, cover=cover)


def quantities(st, R):
    """name -> flat float64 array, every audited quantity of a Result except the gradients."""
    q = {"td_abs": R.td_abs}
    if R.pi is not None:
        q["pi"] = R.pi.reshape(-1)
    for j, v in enumerate(R.tuple):
        q[f"tuple[{j}]"] = np.array([v], np.float64)
    if R.g_log_alpha is not None:
        q["grad:log_alpha"] = np.array([R.g_log_alpha])
    if st.gauss:
        q["bn_running_mean"] = np.concatenate([m for m, _ in R.bn_running])
        q["bn_running_var"] = np.concatenate([v for _, v in R.bn_running])
    return q


def norm_positions(kind, n):
    """tuple position -> the nets whose (mean) gradient norm it holds."""
    if kind == "DDPG":
        return {3: ["critic_0"]} if n == 4 else {4: ["critic_0"], 5: ["actor"]}
    if kind in ("TD3", "SAC"):
        return {4: ["critic_0"], 5: ["critic_1"]} if n == 6 else {5: ["critic_0"], 6: ["critic_1"], 7: ["actor"]}
    cr = [f"critic_{i}" for i in range(5)]
    return {4: cr, 5: cr} if n == 6 else {5: cr, 6: cr, 7: ["actor"]}


def judge(case, ref, got, out=print):
    """got: grads {net: flat}, and the `quantities` names -> arrays, as the device gave them.  -> (rows, fitted): one row per quantity
    (quantity, err, e32, scale, bound, ratio, ok), the number of listed kink units whose flip the fit applied."""
    st, r64 = ref.step, ref.r64
    assert len(ref.units) <= KINK_CAP, f"{case.id}: {len(ref.units)} units near a kink (cap {KINK_CAP})"
    assert case.B > 64 or not ref.units, f"{case.id}: {len(ref.units)} units near a kink at B <= 64"
    nets = list(r64.grads)
    assert sorted(got["grads"]) == sorted(nets), (sorted(got["grads"]), nets)
    g64 = {n: st.flat(r64, n) for n in nets}
    c, shift, dnorm = explain_flips(SimpleNamespace(g=gr.FlipData(g64, ref.vectors)), {n: np.asarray(got["grads"][n], np.float64) for n in nets})
    fitted = int(np.sum(c))
    rows = []

    def held(q, x, x64, x32s, scale=None, extra=0.0):
        x, x64 = np.asarray(x, np.float64).reshape(-1), np.asarray(x64, np.float64).reshape(-1)
        assert x.shape == x64.shape, (q, x.shape, x64.shape)
        e32 = max(float(np.max(np.abs(np.asarray(y, np.float64).reshape(-1) - x64))) for y in x32s)
        scale = float(np.max(np.abs(x64))) if scale is None else scale
        err = float(np.max(np.abs(x - x64)))
        bound = max(K_REF * e32, RTOL * scale) + extra
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        ok = bool(np.isfinite(err) and err <= bound)
        out(f"  {q:<34} err {err:.3e}  e32 {e32:.3e}  scale {scale:.3e}  err/bound {ratio:.3f}" + ("" if ok else "  <-- FAIL"))
        rows.append(dict(quantity=q, err=err, e32=e32, scale=scale, bound=bound, ratio=ratio, ok=ok))

    for n in nets:
        lay = st.lay(n)
        dev = gr.split(np.asarray(got["grads"][n], np.float64) - shift[n], lay)
        net_max = float(np.max(np.abs(g64[n])))
        for key, _ in lay:
            zero = st.gauss and n == "actor" and key.endswith(".bias") and key[0].isdigit()    # Linear bias in front of BatchNorm
            held(f"grad:{n} {key}", dev[key], r64.grads[n][key], [r.grads[n][key] for r in ref.r32], scale=net_max if zero else None)
    q64, q32 = quantities(st, r64), [quantities(st, r) for r in ref.r32]
    slack = {n: abs(float(dnorm[n]) - float(np.sqrt(np.square(g64[n]).sum()))) for n in nets}
    pos = norm_positions(case.kind, len(r64.tuple))
    for q in q64:
        if q not in got:
            continue                     # (td_abs and pi on the row chain: not outputs there; the caller checks the set of names)
        extra = 0.0
        if q.startswith("tuple["):
            ns = pos.get(int(q[6:-1]), [])
            extra = float(np.mean([slack[n] for n in ns])) if ns else 0.0
        held(q, got[q], q64[q], [x[q] for x in q32], extra=extra)
    return rows, fitted
