"""CPU: tests/adam_ref.py's checker against an fp32 NumPy restatement of adam_elem / clip_coef / polyak_elem (csrc/adam_math.h):
it accepts the right restatement on every table below, and rejects each of the mistakes that bitwise equality between the launch
forms cannot see (they all include adam_math.h) on at least one NAMED table.  This is what proves that
tests/test_gpu_optimiser_audit.py can fail.

Tables (name: what it holds):
  wide37_adam_t1         37 entries, |g| log-uniform from 1e-10 to 1 in one vector, zero moments, first step, Adam, no clip
  wide4099_adamw_t5      4 099 entries, the same spread, live moments, AdamW, clip inactive, grad_scale 0.5, Polyak
  wide140000_adamw_t3    140 000 entries, the same spread, AdamW, clip ACTIVE (norm ~ 40 x the clip), Polyak
  zeros4099_adamw_t1     4 099 entries, every third gradient exactly zero, zero moments, AdamW
  small4099_adam_t2      4 099 entries, gradient norm 5e-4 (< 1e-3), clip 1e-4 below it: the 1e-6 of the coefficient is 0.2 %
  small37_adamw_t4       37 entries, norm 3e-4, clip 2e-5, AdamW, Polyak
  crafted4099_adamw_t2   v from 1e-30 to 1e4, m set against the gradient so that m_new cancels, AdamW
"""
import numpy as np
import pytest
import torch

import adam_ref as ar
from adam_ref import F32

MUTANTS = ["eps_inside_division", "t_off_by_one", "decay_omitted", "beta2_wrong", "w2_wrong", "clip_without_1e-6", "grad_scale_ignored",
           "polyak_swapped", "bc2s_as_bc2"]
# the table on which each mistake must be caught (others may catch it too)
CAUGHT_ON = {
    "eps_inside_division": "wide37_adam_t1",
    "t_off_by_one": "wide4099_adamw_t5",
    "decay_omitted": "zeros4099_adamw_t1",
    "beta2_wrong": "wide4099_adamw_t5",
    "w2_wrong": "wide140000_adamw_t3",
    "clip_without_1e-6": "small4099_adam_t2",
    "grad_scale_ignored": "wide4099_adamw_t5",
    "polyak_swapped": "wide140000_adamw_t3",
    "bc2s_as_bc2": "wide4099_adamw_t5",
}


def _wide(gen, n):
    return (gen.choice([-1.0, 1.0], n) * 10.0 ** gen.uniform(-10.0, 0.0, n)).astype(F32)


def _table(name):
    gen = np.random.default_rng(sum(map(ord, name)))
    c = dict(name=name, kind="DDPG", t=1, lr=1e-3, clip=-1.0, grad_scale=1.0, tau=None)
    if name == "wide37_adam_t1":
        n = 37
        c.update(g=_wide(gen, n), m=np.zeros(n, F32), v=np.zeros(n, F32))
    elif name == "wide4099_adamw_t5":
        n = 4099
        g = _wide(gen, n)
        c.update(kind="TD3", t=5, lr=7e-4, clip=100.0, grad_scale=0.5, tau=0.05, g=g,
                 m=(0.3 * g * gen.uniform(0.5, 1.5, n)).astype(F32), v=(0.004 * g.astype(np.float64) ** 2 * gen.uniform(0.5, 2.0, n)).astype(F32))
    elif name == "wide140000_adamw_t3":
        n = 140000
        g = _wide(gen, n)
        c.update(kind="SAC", t=3, lr=1e-3, clip=2.0, tau=0.005, g=g,
                 m=(0.2 * g * gen.uniform(0.5, 1.5, n)).astype(F32), v=(0.002 * g.astype(np.float64) ** 2 * gen.uniform(0.5, 2.0, n)).astype(F32))
    elif name == "zeros4099_adamw_t1":
        n = 4099
        g = (0.01 * gen.standard_normal(n)).astype(F32)
        g[::3] = 0.0
        c.update(kind="TQC", g=g, m=np.zeros(n, F32), v=np.zeros(n, F32), clip=10.0)
    elif name == "small4099_adam_t2":
        n = 4099
        g = gen.standard_normal(n)
        g = (g * (5e-4 / np.linalg.norm(g))).astype(F32)
        c.update(t=2, clip=1e-4, g=g, m=(0.1 * g).astype(F32), v=(0.001 * g.astype(np.float64) ** 2).astype(F32))
    elif name == "small37_adamw_t4":
        n = 37
        g = gen.standard_normal(n)
        g = (g * (3e-4 / np.linalg.norm(g))).astype(F32)
        c.update(kind="TD3", t=4, clip=2e-5, tau=0.05, g=g, m=(0.2 * g).astype(F32), v=(0.003 * g.astype(np.float64) ** 2).astype(F32))
    elif name == "crafted4099_adamw_t2":
        n = 4099
        g = (0.05 * gen.standard_normal(n)).astype(F32)
        c.update(kind="SAC", t=2, clip=10.0, g=g, m=(-g / 9.0).astype(F32),       # m + w1 * (g - m) = 0.9 m + 0.1 g ~ 0
                 v=(10.0 ** gen.uniform(-30.0, 4.0, n)).astype(F32))
    else:
        raise KeyError(name)
    c["p"] = (0.3 * gen.standard_normal(n)).astype(F32)
    if c["tau"] is not None:
        c["target"] = (c["p"] + 0.01 * gen.standard_normal(n)).astype(F32)
    return c


TABLES = ["wide37_adam_t1", "wide4099_adamw_t5", "wide140000_adamw_t3", "zeros4099_adamw_t1", "small4099_adam_t2", "small37_adamw_t4",
          "crafted4099_adamw_t2"]
_CACHE = {}


def _case(name):
    """(table, references): computed once, shared, never changed."""
    if name not in _CACHE:
        c = _table(name)
        _CACHE[name] = (c, ar.references(c["kind"], c, c["t"], c["lr"], c["clip"], c["tau"]))
    return _CACHE[name]


def restate(c, mutant=None):
    """adam_elem / clip_coef / polyak_elem in numpy float32: every operation rounded on its own, in the header's order."""
    g, p, m, v = (np.ascontiguousarray(c[k], dtype=F32) for k in ("g", "p", "m", "v"))
    t, lr = c["t"] + (1 if mutant == "t_off_by_one" else 0), c["lr"]
    beta2 = 0.99 if mutant == "beta2_wrong" else ar.BETA2
    w1, w2, b2, eps = F32(1.0 - ar.BETA1), F32(1.0 - (0.99 if mutant == "w2_wrong" else beta2)), F32(beta2), F32(ar.EPS)
    step_size = F32(lr / (1.0 - ar.BETA1 ** t))
    bc2 = 1.0 - beta2 ** t
    bc2s = F32(bc2 if mutant == "bc2s_as_bc2" else np.sqrt(bc2))
    decay = F32(1.0 - lr * ar.weight_decay_of(c["kind"]))
    if mutant == "decay_omitted":
        decay = F32(1.0)
    gscale = F32(1.0 if mutant == "grad_scale_ignored" else c["grad_scale"])
    norm = gscale * F32(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    coef = F32(1.0)
    if c["clip"] >= 0:
        coef = np.minimum(F32(c["clip"]) / (norm if mutant == "clip_without_1e-6" else norm + F32(1e-6)), F32(1.0))
    post = norm * coef
    gi = g * (gscale * coef)
    if decay != F32(1.0):
        p = p * decay
    m = m + w1 * (gi - m)
    v = v * b2 + (w2 * gi) * gi
    if mutant == "eps_inside_division":
        denom = (np.sqrt(v) + eps) / bc2s
    else:
        denom = np.sqrt(v) / bc2s + eps
    p = p + (-step_size * m) / denom
    out = dict(p=p, m=m, v=v, post_norm=float(post))
    if c["tau"] is not None:
        tau, omt = F32(c["tau"]), F32(1.0 - c["tau"])
        if mutant == "polyak_swapped":
            tau, omt = omt, tau
        out["target"] = tau * p + omt * np.ascontiguousarray(c["target"], dtype=F32)
    return out


def test_tables_are_what_they_claim():
    for name in TABLES:
        c, (r32, r64, _, _) = _case(name)
        assert all(np.asarray(c[k]).dtype == F32 for k in ("p", "m", "v", "g"))
        a = np.abs(c["g"][c["g"] != 0])
        if name.startswith("wide"):
            assert a.min() < 1e-9 and a.max() > 0.5 if c["g"].size > 1000 else a.min() < 1e-8 and a.max() > 0.1
        if name.startswith("small"):
            assert c["clip"] < r64.norm < 1e-3 and r64.coef < 1.0
        if name.startswith("zeros"):
            assert int(ar.still_entries(c).sum()) > 1000
    assert {_case(n)[0]["g"].size for n in TABLES} >= {37, 4099, 140000}
    assert _case("wide140000_adamw_t3")[1][1].coef < 1.0 and _case("wide4099_adamw_t5")[1][1].coef == 1.0


@pytest.mark.parametrize("name", TABLES)
def test_checker_accepts_the_right_restatement(name):
    c, (r32, r64, t32, t64) = _case(name)
    got = restate(c)
    rows = ar.held_step(name, c, got, r32, r64, t32, t64)
    worst = max(r["ratio"] for r in rows)
    print(f"{name}: worst err/bound {worst:.3f}")
    assert worst < 1.0
    # the exact expectations the device test holds on top of the bound
    still = ar.still_entries(c)
    assert np.array_equal(ar.bits(got["p"][still]), ar.bits(ar.decayed(c["p"], c["kind"], c["lr"])[still]))
    if r64.coef == 1.0:
        mm, vv = ar.unfused_moments(c["m"], c["v"], c["g"], c["grad_scale"])
        assert np.array_equal(ar.bits(got["m"]), ar.bits(mm)) and np.array_equal(ar.bits(got["v"]), ar.bits(vv))


@pytest.mark.parametrize("mutant", MUTANTS)
def test_checker_rejects_the_mutant(mutant):
    name = CAUGHT_ON[mutant]
    c, (r32, r64, t32, t64) = _case(name)
    lines = []
    rows = ar.held_step(f"{name}[{mutant}]", c, restate(c, mutant), r32, r64, t32, t64, check=False, out=lines.append)
    failed = [r for r in rows if not r["ok"]]
    print(f"{mutant} on {name}: rejected by {[r['quantity'] for r in failed]}, worst err/bound {max(r['ratio'] for r in rows):.3g}")
    assert failed, "\n".join(lines)
    with pytest.raises(AssertionError):
        ar.held_step(name, c, restate(c, mutant), r32, r64, t32, t64, out=lambda s: None)


def test_decay_after_the_step_is_not_observable():
    """Applying the weight decay after the step instead of before differs by less than an ulp of the parameter: the checker
    cannot (and need not) tell; 'decay omitted' is the mutant that stands for the decay."""
    c, (r32, r64, t32, t64) = _case("zeros4099_adamw_t1")
    right = restate(c)
    undecayed = restate(c, "decay_omitted")
    late = dict(right, p=(undecayed["p"] * F32(1.0 - c["lr"] * ar.WEIGHT_DECAY)).astype(F32))
    rows = ar.held_step("decay after the step", c, late, r32, r64, t32, t64)
    assert max(r["ratio"] for r in rows) < 1.0


def test_cosine_lrs_follow_the_scheduler():
    lrs = ar.cosine_lrs(1e-3, 2e-4, 3, 7)
    assert lrs[0] == 1e-3 and abs(lrs[3] - 2e-4) < 1e-18 and abs(lrs[6] - 1e-3) < 1e-12 and lrs[1] > lrs[2] > lrs[3]
    assert ar.cosine_lrs(1e-3, 1e-3, 1, 4) == [1e-3] * 4


def test_reference_leaves_the_thread_count_alone():
    n = torch.get_num_threads()
    _case("wide37_adam_t1")
    assert torch.get_num_threads() == n
