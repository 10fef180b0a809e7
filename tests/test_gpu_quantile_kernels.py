"""GPU: the loss kernels of the distributional TQC variant (n_quantiles > 1) as single problems, through gcrl_quantile_td_f32
(quantile_td_kernel + quantile_metrics_kernel) and gcrl_quantile_actor_f32 (quantile_actor_kernel) — the kernels the agent
launches, at the edges the agent-level test never reaches: a full wavefront (C*Q = 64), one padding lane (63), drop = 0 and
drop = Q - 1, rows saturated on both Huber sides, u exactly 0 and +-1, ties across the truncation boundary, batches that leave
1 or 3 rows in the last 4-row workgroup, 257 / 1025 rows for the 256-thread strided sums, and the launcher's own refusals.

The variant has no reference counterpart: the specification is oracle/quantile_tqc_oracle.py.  The reference here is a plain
torch restatement of its loss lines, run on the CPU with autograd twice on the same fp32 inputs (fp32 on one thread, fp64), and
the bound is tests/fullsize.py's, per quantity, as in tests/test_gpu_stage_kernels.py (whose helpers this file uses):

    max |hip - ref64|  <=  max(K_REF * max |ref32 - ref64|,  RTOL * max |ref64|)

On top of it: y is the fp32 restatement bit for bit (adds and multiplies only, in the oracle's order), +0 beyond the K kept
atoms; the actor's dz is -1 / (B*C*Q) in every word; nothing but the launch's own words is written.

Mutations of the kernels, and the cases that fail under each (the table is proved without a GPU by
test_quantile_case_table_covers_what_it_claims):
  `lane < K` -> `lane <= K` in the target line: y[:, K] != +0 and the td metric moves, in every case with K < 64;
  `norm` without K: dz is K times too large, in every case with K > 1;
  the actor's `gz` without C: dz is C times too large, in every actor case with C > 1;
  `u < 0.f` -> `u <= 0.f`: NOT observable in any output — at u = 0 the weight multiplies huber(0) = 0 in the loss and
  clamp(0) = 0 in the gradient, and 0 - (+-0) = +0 either way; the kink cases pin what is observable there (dz exactly 0)."""
import functools

import numpy as np
import pytest
import torch

from fullsize import K_REF, RTOL  # noqa: F401  (the bound `held` applies)
from test_gpu_stage_kernels import _reference_on_one_thread  # noqa: F401  (autouse here too: the fp32 run on one thread)
from test_gpu_stage_kernels import F32, GAMMA, MET_ACTOR_LOSS, MET_FLOATS, MET_LOSS, MET_TD, WORST, T, bits, covers, dev, held, host, ptr

pytestmark = pytest.mark.gpu

EDGE = [(2, 25, 2), (2, 32, 0), (2, 32, 31), (8, 8, 7), (4, 16, 15), (3, 21, 5), (2, 2, 1), (4, 13, 0), (1, 64, 63)]
FULL = [e for e in EDGE if e[0] * e[1] == 64]                # N = 64: no padding lane
BS = [1, 3, 4, 5, 63, 257, 1025]
REGIMES = ["plain", "saturated", "kink", "ties"]
ALPHAS = [0.2, 1e-3]
OFF = np.array([0.0, 1.0, -1.0, 2.0, -2.0], F32)             # z - r on a crafted row: u = 0, -1, +1, -2, +2
PAD = 64                                                     # filler words behind every output: an overrun shows
FILL = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_quantile():
    yield
    for k in sorted(k for k in WORST if k.startswith("quantile")):
        print(f"\nworst |hip - ref64| / bound  {k:<22} {WORST[k]:.3f}", end="")
    print()


def filler(n):
    return torch.full((n + PAD,), -1, dtype=torch.int32, device="cuda").view(torch.float32)


def read(t, n):
    out = host(t)
    assert (bits(out[n:]) == FILL).all(), "words behind the output were written"
    return out[:n]


# ------------------------------------------------------------------------------------------------------------- reference
def ref_qtd(dt, r, d, zt, z, lp, alpha, C, Q, drop):
    """oracle/quantile_tqc_oracle.py:78-103, the loss lines: zt, z [C][B][Q] are the critics' outputs."""
    B, K = r.shape[0], C * (Q - drop)
    r, d, lp = T(r, dt)[:, None], T(d, dt)[:, None], T(lp, dt)[:, None]
    zg = T(z, dt, grad=True)
    with torch.no_grad():
        pooled = torch.cat([T(zt[c], dt) for c in range(C)], dim=1)                      # [B, C*Q]
        srt, _ = torch.sort(pooled, dim=1)
        y = r + GAMMA * (1 - d) * (srt[:, :K] - alpha * lp)                              # [B, K]
    tau = ((2 * torch.arange(Q, dtype=dt) + 1) / (2 * Q)).view(1, Q, 1)
    losses, tds, us = [], [], []
    for c in range(C):
        q = zg[c]
        u = y[:, None, :] - q[:, :, None]                                                # [B, Q, K]
        hub = torch.where(u.abs() <= 1.0, 0.5 * u * u, u.abs() - 0.5)
        losses.append((torch.abs(tau - (u.detach() < 0).to(dt)) * hub).mean())
        tds.append((y.mean(dim=1) - q.detach().mean(dim=1)).abs())
        us.append(u.detach())
    torch.stack(losses).sum().backward()
    td = torch.stack(tds).max(dim=0)[0].mean()
    return dict(y=y.numpy(), sorted=srt.numpy(), dz=zg.grad.numpy(), loss=np.array([float(x.detach()) for x in losses]), td=float(td),
                u=torch.stack(us).numpy())


def ref_qactor(dt, z, lp, alpha, C):
    """oracle/quantile_tqc_oracle.py:112-113."""
    zg, lp = T(z, dt, grad=True), T(lp, dt)[:, None]
    zz = torch.cat([zg[c] for c in range(C)], dim=1)
    loss = (alpha * lp - zz.mean(dim=1, keepdim=True)).mean()
    loss.backward()
    return dict(dz=zg.grad.numpy(), loss=float(loss.detach()))


def qtd_inputs(seed, B, C, Q, drop, regime):
    g = np.random.default_rng(seed)
    N, K, b = C * Q, C * (Q - drop), np.arange(B)
    s_atoms, s_r = (6.0, 4.0) if regime == "saturated" else (1.0, 1.0)
    r = (s_r * g.normal(0, 1, B)).astype(F32)
    d = (b % 3 == 2).astype(F32)
    zt = (s_atoms * g.normal(0, 1, (C, B, Q))).astype(F32)
    z = (s_atoms * g.normal(0, 1, (C, B, Q))).astype(F32)
    lp = (g.uniform(0.1, 1.0, B) * np.where(b % 2 == 0, 8.0, -3.0)).astype(F32)    # both signs from B = 2 on
    kink = np.zeros(B, bool)
    if regime == "kink":            # every other terminal row: y = r exactly in fp32 and in fp64, the atoms sit on the kinks
        kink = (d == 1) & ((b // 3) % 2 == 0)
        r[kink] = (np.round(r[kink] * 4) / 4 + 0.0).astype(F32)                          # r, r +- 1, r +- 2 exact; no -0.0
        for c in range(C):
            z[c][kink] = r[kink, None] + OFF[(np.arange(Q) + c) % 5][None, :]
    if regime == "ties":
        pooled = np.concatenate([zt[c] for c in range(C)], axis=1)                       # [B, N], lane = c * Q + q
        for row in range(B):
            order = np.argsort(pooled[row], kind="stable")
            if row % 3 == 0 and drop > 0:     # sorted[K-1] == sorted[K]: the first dropped atom of ANOTHER critic, if there is one
                other = [p for p in order[K:] if p // Q != order[K - 1] // Q]
                pooled[row, other[0] if other else order[K]] = pooled[row, order[K - 1]]
            elif K >= 2:                      # a duplicate inside the kept set
                pooled[row, order[1]] = pooled[row, order[0]]
        zt = np.ascontiguousarray(pooled.reshape(B, C, Q).transpose(1, 0, 2))
    return r, d, zt, z, lp, kink


@functools.lru_cache(maxsize=None)
def qtd_reference(B, C, Q, drop, regime, alpha):
    """Inputs, both reference runs and the coverage the case claims: computed once per case, shared by the table test and the
    launch test, never modified."""
    alpha = float(F32(alpha))
    K = C * (Q - drop)
    r, d, zt, z, lp, kink = qtd_inputs(1000 * B + 100 * C + 10 * Q + drop + REGIMES.index(regime), B, C, Q, drop, regime)
    r32, r64 = (ref_qtd(dt, r, d, zt, z, lp, alpha, C, Q, drop) for dt in (torch.float32, torch.float64))
    u, au = r32["u"], np.abs(r32["u"])
    claim = B >= 3 and K >= 2 and B * C * Q * K >= 64       # else too small to hold every side
    counts = dict(quadratic=(au < 1).sum(), linear_pos=(u > 1).sum(), linear_neg=(u < -1).sum(), u_neg=(u < 0).sum(), u_nonneg=(u >= 0).sum(),
                  done=(d == 1).sum(), live=(d == 0).sum(), logp_pos=(lp > 0).sum(), logp_neg=(lp < 0).sum())
    if regime == "saturated":
        counts.update(mostly_linear=int(2 * (au > 1).sum() > au.size))
    if regime == "kink":
        counts.update(u_zero=(u[:, kink] == 0).sum(), u_plus_one=(u[:, kink] == 1).sum(), u_minus_one=(u[:, kink] == -1).sum())
        assert np.array_equal(u[:, kink], r64["u"][:, kink]), "a crafted row's u differs between fp32 and fp64"
        assert np.isin(u[:, kink], OFF).all()
    if regime == "ties":
        srt = r32["sorted"]
        if drop > 0:
            counts.update(tied_at_the_cut=(srt[:, K - 1] == srt[:, K]).sum(), untied_at_the_cut=(srt[:, K - 1] != srt[:, K]).sum())
        counts.update(tied_inside=(srt[:, :K - 1] == srt[:, 1:K]).any(axis=1).sum())
    print(f"B{B} C{C} Q{Q} drop{drop} {regime}:")
    covers(claim, **counts)
    assert np.array_equal(r32["y"][d == 1], np.broadcast_to(r[d == 1, None], (int((d == 1).sum()), K))), "y != r on a terminal row"
    r32["u_kink"] = r32.pop("u")[:, kink][..., 0]            # [C, rows, Q]: on a crafted row every target is r, u the same for all K
    del r64["u"]
    return dict(r=r, d=d, zt=zt, z=z, lp=lp, kink=kink, r32=r32, r64=r64, alpha=alpha, K=K, claim=claim)


def _qtd_cases():
    out = []
    for j, B in enumerate(BS):                               # every B meets the benchmark's shape and one full wavefront
        out.append(((2, 25, 2), B, REGIMES[j % 4], ALPHAS[j % 2]))
        out.append((FULL[j % len(FULL)], B, REGIMES[(j + 1) % 4], ALPHAS[(j + 1) % 2]))
    for i, e in enumerate(EDGE):                             # every edge meets two regimes at two sizes
        for k in range(2):
            out.append((e, BS[(3 * i + 4 * k + 2) % 7], REGIMES[(i + 2 * k + 2) % 4], ALPHAS[(i + k) % 2]))
    out += [((2, 25, 2), 63, "kink", 0.2), ((2, 32, 0), 257, "kink", 1e-3), ((3, 21, 5), 63, "ties", 0.2), ((2, 2, 1), 63, "kink", 0.2),
            ((2, 25, 2), 257, "ties", 1e-3), ((2, 32, 0), 63, "saturated", 0.2)]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return [pytest.param(B, C, Q, drop, regime, alpha, id=f"B{B}-C{C}-Q{Q}-drop{drop}-{regime}-a{alpha}") for (C, Q, drop), B, regime, alpha in uniq]


def test_quantile_case_table_covers_what_it_claims():
    """No launch: the reference alone over the whole table.  Every B meets the benchmark's (2, 25, 2) and a full wavefront, every
    edge is there, every regime meets the benchmark's shape and a full wavefront at a size that claims its sides, and every
    claim holds (qtd_reference fails on a zero count)."""
    cases = [c.values for c in _qtd_cases()]
    assert {c[1:4] for c in cases} == set(EDGE)
    for B in BS:
        assert any(c[0] == B and c[1:4] == (2, 25, 2) for c in cases) and any(c[0] == B and c[1] * c[2] == 64 for c in cases), B
    assert {c[0] for c in cases} == set(BS)
    assert {c[5] for c in cases} == set(ALPHAS)
    claimed = {(regime, "bench" if (C, Q, drop) == (2, 25, 2) else "full" if C * Q == 64 else "other")
               for B, C, Q, drop, regime, alpha in cases if qtd_reference(B, C, Q, drop, regime, alpha)["claim"]}
    for regime in REGIMES:
        assert (regime, "bench") in claimed and (regime, "full") in claimed, regime
    # partial last workgroups of 1 and 3 rows (4 rows per workgroup), one past a multiple of the 256-thread stride
    assert {B % 4 for B in BS} >= {1, 3} and {257, 1025} <= set(BS)
    # a tie at the cut needs something dropped, and is claimed where that is so
    assert any(c[4] == "ties" and c[3] > 0 and c[0] >= 3 for c in cases)
    for B, C, Q in _qactor_cases():
        assert C * Q <= 64
    assert {(C, Q) for _, C, Q in _qactor_cases()} == {e[:2] for e in EDGE} and {B for B, _, _ in _qactor_cases()} == set(BS)


@pytest.mark.parametrize("B,C,Q,drop,regime,alpha", _qtd_cases())
def test_quantile_td(lib, B, C, Q, drop, regime, alpha):
    ref = qtd_reference(B, C, Q, drop, regime, alpha)
    r32, r64, K, kink, d = ref["r32"], ref["r64"], ref["K"], ref["kink"], ref["d"]
    ins = [dev(ref[k]) for k in ("r", "d", "zt", "z", "lp")]
    y, dz, row_loss, row_td, met = filler(B * 64), filler(C * B * Q), filler(C * B), filler(B), filler(MET_FLOATS)
    rc = lib.gcrl_quantile_td_f32(*(ptr(t) for t in ins), ref["alpha"], B, C, Q, drop, GAMMA, ptr(y), ptr(dz), ptr(row_loss), ptr(row_td), ptr(met), 1)
    assert rc == 0, rc
    y, dz, row_loss, row_td, met = read(y, B * 64).reshape(B, 64), read(dz, C * B * Q).reshape(C, B, Q), read(row_loss, C * B), read(row_td, B), \
        read(met, MET_FLOATS)
    # written: all of y, dz, row_loss, row_td; of the metrics record the C losses and td, nothing else
    for what, a in (("y", y), ("dz", dz), ("row_loss", row_loss), ("row_td", row_td)):
        assert not np.isnan(a).any(), f"{what}: words left unwritten (or NaN)"
    mine = np.zeros(MET_FLOATS, bool)
    mine[[MET_TD] + [MET_LOSS + c for c in range(C)]] = True
    assert (bits(met[~mine]) == FILL).all() and not np.isnan(met[mine]).any(), "the launch wrote metrics that are not its own, or not all of its own"
    # exact: the kept targets are the fp32 restatement (torch.sort's order; adds and multiplies in the oracle's order); +0 beyond
    assert np.array_equal(bits(y[:, :K]), bits(r32["y"])), "y differs from the fp32 restatement"
    assert (bits(y[:, K:]) == 0).all(), "y beyond the K kept atoms is not +0.0"
    assert np.array_equal(bits(y[d == 1, :K]), bits(np.broadcast_to(ref["r"][d == 1, None], (int((d == 1).sum()), K)))), "y != r on a terminal row"
    # the bound
    for c in range(C):
        held(f"quantile dz[{c}]", dz[c], r32["dz"][c], r64["dz"][c])
        held(f"quantile loss[{c}]", [met[MET_LOSS + c]], [r32["loss"][c]], [r64["loss"][c]])
    held("quantile td", [met[MET_TD]], [r32["td"]], [r64["td"]])
    if kink.any():
        u = r32["u_kink"]
        got, want = dz[:, kink], r32["dz"][:, kink]
        assert (got[u == 0] == 0).all() and (want[u == 0] == 0).all(), "a gradient at u = 0"
        assert np.array_equal(np.sign(got[u != 0]), np.sign(want[u != 0])) and np.array_equal(np.sign(got[u != 0]), -np.sign(u[u != 0]))
        # ... and its value: K equal terms, added one by one in fp32 (at most 63 * 2^-24 = 3.8e-6 relative, inside RTOL)
        tau = ((2 * np.arange(Q, dtype=np.float64) + 1) / (2 * Q))[None, None, :]
        exact = -np.where(u < 0, 1 - tau, tau) * np.clip(u, -1, 1) * K / (float(B) * Q * K)
        assert np.allclose(got, exact, rtol=RTOL, atol=0), "a crafted row's gradient is not -|tau - 1(u<0)| clamp(u) / (B Q)"


def _qactor_cases():
    return [(BS[(2 * i + 3 * k) % 7], C, Q) for i, (C, Q, _) in enumerate(EDGE) for k in range(2)]


@pytest.mark.parametrize("B,C,Q", [pytest.param(B, C, Q, id=f"B{B}-C{C}-Q{Q}") for B, C, Q in _qactor_cases()])
def test_quantile_actor(lib, B, C, Q):
    g = np.random.default_rng(7 * B + 3 * C + Q)
    alpha = float(F32(ALPHAS[(B + C) % 2]))
    z = g.normal(0, 2.0, (C, B, Q)).astype(F32)
    lp = g.uniform(-3.0, 8.0, B).astype(F32)
    r32, r64 = (ref_qactor(dt, z, lp, alpha, C) for dt in (torch.float32, torch.float64))
    zd, ld = dev(z), dev(lp)
    dz, met = filler(C * B * Q), filler(MET_FLOATS)
    assert lib.gcrl_quantile_actor_f32(ptr(zd), ptr(ld), alpha, B, C, Q, ptr(dz), ptr(met), 1) == 0
    dz, met = read(dz, C * B * Q).reshape(C, B, Q), read(met, MET_FLOATS)
    held("quantile actor dz", dz, r32["dz"], r64["dz"])
    assert np.array_equal(bits(dz), bits(np.full((C, B, Q), F32(-1) / (F32(B) * F32(C * Q)))))
    held("quantile actor_loss", [met[MET_ACTOR_LOSS]], [r32["loss"]], [r64["loss"]])
    mine = np.zeros(MET_FLOATS, bool)
    mine[MET_ACTOR_LOSS] = True
    assert (bits(met[~mine]) == FILL).all(), "the launch wrote metrics that are not its own"


@pytest.mark.parametrize("C,Q,drop", [(5, 13, 2), (2, 25, 25), (2, 25, -1)], ids=["CQ65", "drop-eq-Q", "drop-negative"])
def test_quantile_td_refusals_come_from_the_launcher(gcrl, lib, C, Q, drop):
    B = 5
    g = np.random.default_rng(C * Q)
    ins = [dev(g.normal(0, 1, n)) for n in (B, B, C * B * Q, C * B * Q, B)]
    outs = [filler(n) for n in (B * 64, C * B * Q, C * B, B, MET_FLOATS)]
    rc = lib.gcrl_quantile_td_f32(*(ptr(t) for t in ins), 0.2, B, C, Q, drop, GAMMA, *(ptr(t) for t in outs), 1)
    assert rc != 0
    assert "quantile_td:" in gcrl._ffi.last_error(), gcrl._ffi.last_error()
    for t in outs:
        assert (bits(host(t)) == FILL).all(), "a refused call wrote to an output"
