"""The optimiser step of an update (global-norm clip, Adam / AdamW, Polyak, the log-alpha step: csrc/adam_math.h,
csrc/adam_device.inc, csrc/dw_adam_body.inc, csrc/adam_pop.hip, `alpha_step` in csrc/ops.h) as torch computes it, and the bound
an implementation of it is held to.  No GPU.  The reference is torch itself: `torch.optim.Adam` (DDPG, src/agent.py:1201) /
`torch.optim.AdamW` (the other agents) with `foreach=False`, the optimiser state injected, `torch.nn.utils.clip_grad_norm_` in
front; on the CPU, on one thread, once in fp32 and once in fp64 on the same fp32 inputs.

GIVEN the gradient, a step is a deterministic function of (p, m, v, g, t, lr): none of the fp32 reordering noise that a gradient
carries enters, so the bound can be tight.  `held_step` applies tests/fullsize.py's criterion

    max |x - ref64|  <=  max(K_REF * max |ref32 - ref64|,  RTOL * max |ref64|)

to
  * the parameter STEP  d = p_after - p_before  (formed in fp64 from the fp32 words), not the parameter: a step has scale ~ lr,
    a parameter ~ 0.3, so a bound on the parameter would let 0.3 % of a step through; on the step, the floor is the fp32
    rounding of p;
  * the target's step (Polyak: tau * p_new + (1 - tau) * target, in the dtype), the same way;
  * m and v;
  * m and v per ELEMENT, in units of ulp32(max(|m_old|, |g_eff|)) and ulp32(max(v_old, w2 * g_eff^2)), g_eff = g * grad_scale *
    coef with the fp64 reference's clip coefficient: allowed is K_REF x the worst such figure of torch's own fp32 run on the same
    case (measured, not fixed in advance: under an active clip its own coefficient moves it to tens of units), floored at 4
    units — five roundings of at most half a unit each separate the inputs from v_new, and the one on g_eff enters squared,
    which makes about 3.  Under an ACTIVE clip the figure is mostly the rounding of the clip coefficient, one random draw per
    net and step for either side, and a single draw of torch's can come out near zero: the device audit's rows of one net's
    active-clip steps are therefore judged by `judge_units` against torch's worst figure over those steps of that net (never
    across nets: a small net is not granted a large net's fp32 norm error); every other row against its own step's figure;
  * the post-clip norm, against min(1, clip / (norm + 1e-6)) * norm of the fp64 reference.

The comparison cannot be bitwise: torch's CPU `lerp_` and `addcmul_` fuse the multiply-add, adam_elem rounds every product
(about 12 % of moment words differ in the last place).  "Same op order as torch" is about the order, not the bits.
tests/test_adam_ref.py proves on the CPU that this checker rejects the mistakes it is there for.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from fullsize import K_REF, RTOL

F32 = np.float32
BETA1, BETA2, EPS, WEIGHT_DECAY = 0.9, 0.999, 1e-8, 0.01      # torch's defaults; AdamW's decay, Adam has none
UNIT_FLOOR = 4.0

Ref = namedtuple("Ref", "p m v post_norm coef norm")


def weight_decay_of(kind: str) -> float:
    return 0.0 if kind == "DDPG" else WEIGHT_DECAY


def cosine_lrs(lr0: float, lr_min: float, t_max: int, n: int):
    """lr of optimiser steps 1..n under the reference's schedule: CosineAnnealingLR stepped once after every optimiser step."""
    dummy = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=lr0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(dummy, T_max=int(t_max), eta_min=lr_min)
    out = []
    for _ in range(n):
        out.append(float(dummy.param_groups[0]["lr"]))
        dummy.step()
        sched.step()
    return out


def reference_step(dtype, kind, p, m, v, g, t, lr, weight_decay, clip, grad_scale):
    """Optimiser step number t (1-based: the injected state holds step = t - 1) of one net.  p, m, v, g: fp32 vectors (the whole
    net: the clip norm is global); clip < 0: no clipping.  -> Ref(p, m, v, post_norm, coef, norm), arrays as float64."""
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        def T(x):
            return torch.tensor(np.ascontiguousarray(x, dtype=F32).reshape(-1), dtype=dtype)
        param = torch.nn.Parameter(T(p))
        param.grad = T(g) * grad_scale
        norm = float(torch.linalg.vector_norm(param.grad))
        coef = 1.0
        if clip >= 0:
            torch.nn.utils.clip_grad_norm_([param], clip)
            c = torch.tensor(clip, dtype=dtype) / (torch.tensor(norm, dtype=dtype) + 1e-6)
            coef = float(torch.clamp(c, max=1.0))
        post = float(torch.tensor(coef, dtype=dtype) * torch.tensor(norm, dtype=dtype))
        Opt = torch.optim.Adam if kind == "DDPG" else torch.optim.AdamW
        opt = Opt([param], lr=float(lr), betas=(BETA1, BETA2), eps=EPS, weight_decay=weight_decay, foreach=False)
        opt.state[param] = dict(step=torch.tensor(float(t - 1)), exp_avg=T(m), exp_avg_sq=T(v))
        opt.step()
        st = opt.state[param]
        assert int(st["step"]) == t
        return Ref(param.detach().double().numpy().copy(), st["exp_avg"].double().numpy().copy(), st["exp_avg_sq"].double().numpy().copy(),
                   post, coef, norm)
    finally:
        torch.set_num_threads(old)


def reference_polyak(dtype, tau, p_new, target):
    """src/agent.py:1260-1271: tau * p + (1 - tau) * target in the dtype.  p_new: the reference's own new parameter (float64 array
    holding dtype values); target: fp32."""
    pn = torch.tensor(np.asarray(p_new, np.float64), dtype=dtype)
    tg = torch.tensor(np.ascontiguousarray(target, dtype=F32), dtype=dtype)
    return (tau * pn + (1 - tau) * tg).double().numpy()


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)


def unit_figures(before, m_new, v_new, ref64):
    """-> (worst |m - m64| / unit_m, worst |v - v64| / unit_v) over the elements."""
    g_eff = np.asarray(before["g"], np.float64) * float(before["grad_scale"]) * ref64.coef
    um = ulp32(np.maximum(np.abs(np.asarray(before["m"], np.float64)), np.abs(g_eff)))
    uv = ulp32(np.maximum(np.asarray(before["v"], np.float64), float(F32(1.0 - BETA2)) * g_eff * g_eff))
    fm = float(np.max(np.abs(np.asarray(m_new, np.float64) - ref64.m) / um))
    fv = float(np.max(np.abs(np.asarray(v_new, np.float64) - ref64.v) / uv))
    return fm, fv


def references(kind, before, t, lr, clip, tau=None):
    """(ref32, ref64[, target32, target64]) of one net's step.  before: dict p, m, v, g, grad_scale (+ target)."""
    out = []
    for dt in (torch.float32, torch.float64):
        out.append(reference_step(dt, kind, before["p"], before["m"], before["v"], before["g"], t, lr, weight_decay_of(kind), clip,
                                  before["grad_scale"]))
    tg = [None, None]
    if tau is not None:
        tg = [reference_polyak(dt, tau, r.p, before["target"]) for dt, r in zip((torch.float32, torch.float64), out)]
    return out[0], out[1], tg[0], tg[1]


def held(what, q, got, r32, r64, out=print):
    """tests/fullsize.py's bound for one quantity, every element taking part: prints one line, -> the row."""
    got, r32, r64 = (np.asarray(x, np.float64).reshape(-1) for x in (got, r32, r64))
    assert got.shape == r32.shape == r64.shape, (what, q)
    scale = float(np.max(np.abs(r64)))
    e_got, e_ref = float(np.max(np.abs(got - r64))), float(np.max(np.abs(r32 - r64)))
    bound = max(K_REF * e_ref, RTOL * scale)
    ratio = e_got / bound if bound > 0 else (0.0 if e_got == 0 else float("inf"))
    ok = bool(np.isfinite(e_got) and e_got <= bound)
    out(f"  {what + ' ' + q:<34} err {e_got:.3e}  ref32 err {e_ref:.3e}  scale {scale:.3e}  err/bound {ratio:.3f}" + ("" if ok else "  <-- FAIL"))
    return dict(quantity=q, err=e_got, ref32_err=e_ref, scale=scale, ratio=ratio, ok=ok)


def judge_units(rows, out=print):
    """The per-element rows of one case (rows carry `net` and `active`: the clip was active on that step): the active-clip steps
    of a net are judged together — allowed is K_REF x torch fp32's worst figure over them, floored at UNIT_FLOOR.  Rows of
    inactive-clip steps keep held_step's verdict, each against its own step's figure.  Rewrites ratio / ok in place."""
    for q in ("m/unit", "v/unit"):
        for net in sorted({r["net"] for r in rows if r["quantity"] == q and r.get("active")}):
            mine = [r for r in rows if r["quantity"] == q and r.get("active") and r["net"] == net]
            torch_worst = max(r["units_torch32"] for r in mine)
            allowed = max(K_REF * torch_worst, UNIT_FLOOR)
            for r in mine:
                r["ratio"], r["ok"] = r["units"] / allowed, bool(np.isfinite(r["units"]) and r["units"] <= allowed)
            worst = max(r["units"] for r in mine)
            out(f"  active clip, {net + ' ' + q:<21} worst {worst:.2f} units  torch fp32 {torch_worst:.2f} units  allowed {allowed:.2f}  "
                f"err/bound {worst / allowed:.3f}" + ("" if worst <= allowed else "  <-- FAIL"))


def held_step(what, before, after, ref32, ref64, target32=None, target64=None, check=True, out=print):
    """before: dict p, m, v, g, grad_scale (+ target when the step has a Polyak); after: dict p, m, v (+ target, + post_norm: the
    logged post-clip norm, when the implementation reports one).  Prints one line per quantity; -> list of rows (quantity, err,
    ref32_err, scale, ratio, ok, + unit figures for the per-element rows).  check: assert that every row is ok."""
    rows = []
    p0 = np.asarray(before["p"], np.float64)
    rows.append(held(what, "dp", np.asarray(after["p"], np.float64) - p0, ref32.p - p0, ref64.p - p0, out))
    if target64 is not None:
        t0 = np.asarray(before["target"], np.float64)
        rows.append(held(what, "dtarget", np.asarray(after["target"], np.float64) - t0, target32 - t0, target64 - t0, out))
    rows.append(held(what, "m", after["m"], ref32.m, ref64.m, out))
    rows.append(held(what, "v", after["v"], ref32.v, ref64.v, out))
    got_u = unit_figures(before, after["m"], after["v"], ref64)
    ref_u = unit_figures(before, ref32.m, ref32.v, ref64)
    for q, gu, ru in zip(("m/unit", "v/unit"), got_u, ref_u):
        allowed = max(K_REF * ru, UNIT_FLOOR)
        ok = bool(np.isfinite(gu) and gu <= allowed)
        out(f"  {what + ' ' + q:<34} worst {gu:.2f} units  torch fp32 {ru:.2f} units  allowed {allowed:.2f}  err/bound {gu / allowed:.3f}"
            + ("" if ok else "  <-- FAIL"))
        rows.append(dict(quantity=q, err=gu, ref32_err=ru, scale=1.0, ratio=gu / allowed, ok=ok, units=gu, units_torch32=ru))
    if after.get("post_norm") is not None:
        rows.append(held(what, "post_norm", [after["post_norm"]], [ref32.post_norm], [ref64.post_norm], out))
    if check:
        bad = [(what, r["quantity"], r["err"], r["ref32_err"], r["scale"]) for r in rows if not r["ok"]]
        assert not bad, bad
    return rows


# ---- exact expectations (on top of the bound)
def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def unfused_moments(m, v, g, grad_scale=1.0, coef=1.0):
    """m_new, v_new of adam_elem in fp32, every product rounded before it is added (numpy's float32 arithmetic fuses nothing):
    what an implementation must give BITWISE when its clip coefficient is exactly `coef`."""
    m, v, g = (np.ascontiguousarray(x, dtype=F32) for x in (m, v, g))
    w1, w2, b2 = F32(1.0 - BETA1), F32(1.0 - BETA2), F32(BETA2)
    gi = g * (F32(grad_scale) * F32(coef))
    return m + w1 * (gi - m), v * b2 + (w2 * gi) * gi


def still_entries(before):
    """Entries whose gradient is exactly zero and whose moments are zero: they move by the decay alone."""
    return (np.asarray(before["g"]) == 0) & (np.asarray(before["m"]) == 0) & (np.asarray(before["v"]) == 0)


def decayed(p, kind, lr):
    """fl(p * decay) — and p itself under Adam."""
    p = np.ascontiguousarray(p, dtype=F32)
    return p.copy() if kind == "DDPG" else p * F32(1.0 - lr * WEIGHT_DECAY)
