"""GPU: the small kernels between the GEMM stages of an update step, each as a single problem through its stand-alone entry
(gcrl_td_loss_f32, gcrl_actor_select_f32, gcrl_tanh_gauss_fwd_f32 / _bwd_f32, gcrl_td3_smooth_f32), at the edges the golden
fixtures never reach: saturated Huber rows, clamped targets, terminal rows, importance weights, tied critics, the clamped and
saturated tanh-Gaussian head, batch sizes around every guard and launch-form switch.

The reference is a plain torch restatement of the reference's lines (below), run on the CPU with autograd twice on the same fp32
inputs: in fp32 on one thread and in fp64.  The bound is tests/fullsize.py's, per quantity:

    max |hip - ref64|  <=  max(K_REF * max |ref32 - ref64|,  RTOL * max |ref64|)

That bound widens where fp32 itself departs from fp64 (the clamped / saturated region), so those rows are also held to exact
expectations against the fp32 run.  Every case counts, on the reference's own intermediate values, the rows that land on each
side it claims to cover, and fails when a count is zero.  Cases too small to hold every branch (B = 1 ...) are there for the
bounds guards and claim no branch."""
import numpy as np
import pytest
import torch

from fullsize import K_REF, RTOL

pytestmark = pytest.mark.gpu

MET_LOSS, MET_TD, MET_Q, MET_ACTOR_LOSS, MET_ALPHA_LOSS, MET_ALPHA, MET_FLOATS = 0, 16, 17, 18, 20, 21, 32
TGT_DDPG, TGT_MIN, TGT_MIN_ENT, TGT_TRUNC_ENT = 0, 1, 2, 3
LOSS_MSE, LOSS_HUBER = 0, 1
F32 = np.float32
GAMMA = float(F32(0.98))
CLAMP_LO = float(F32(-1.0 / (1.0 - 0.98)))   # src/agent.py:1318, as the fp32 tensor op sees it
TRUNC = [(2, 0), (3, 1), (5, 2), (8, 0), (8, 7)]
SMALL, MID, BIG = [1, 63, 64, 65, 255], [256, 257, 1023], [1024, 1025, 2049]
MB_TD, MB_SEL = [1024, 1025, 1087, 1279, 1280, 2049], [1024, 1025, 1279, 2049]
WORST = {}


@pytest.fixture(autouse=True)
def _reference_on_one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k in sorted(WORST):
        print(f"\nworst |hip - ref64| / bound  {k:<22} {WORST[k]:.3f}", end="")
    print()


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def same_written(a, b):
    """Bitwise equal wherever a launch wrote; what no launch wrote is still a NaN filler (check() has verified which words those are)."""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(a)])


def held(what, got, ref32, ref64):
    """tests/fullsize.py's bound for one quantity; every element takes part."""
    got, ref32, ref64 = (np.asarray(x, np.float64).reshape(-1) for x in (got, ref32, ref64))
    assert got.shape == ref32.shape == ref64.shape, what
    scale = float(np.max(np.abs(ref64)))
    e_got, e_ref = float(np.max(np.abs(got - ref64))), float(np.max(np.abs(ref32 - ref64)))
    bound = max(K_REF * e_ref, RTOL * scale)
    ratio = e_got / bound if bound > 0 else (0.0 if e_got == 0 else float("inf"))
    print(f"  {what:<22} err {e_got:.3e}  ref32 err {e_ref:.3e}  scale {scale:.3e}  err/bound {ratio:.3f}")
    key = what.split("[")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio if ratio == ratio else float("inf"))
    assert e_got <= bound, (what, e_got, e_ref, scale)


def covers(claim, **counts):
    print("  covers " + " ".join(f"{k}={int(v)}" for k, v in counts.items()) + ("" if claim else "  (too small: claims none)"))
    if claim:
        zero = [k for k, v in counts.items() if int(v) == 0]
        assert not zero, f"the inputs miss {zero}"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).cuda()


def nan_dev(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def ptr(t):
    return t.data_ptr() if t is not None else None


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def T(x, dt, grad=False):
    return torch.tensor(np.asarray(x, F32), dtype=dt, requires_grad=grad)


# ------------------------------------------------------------------------------------------------------------- TD target + loss
def ref_td(dt, kind, loss, r, d, qt, q, lp, alpha, w, drop):
    """src/agent.py:174-184 (TD3), :566-569 (SAC), :971-974 (TQC), :1317 (DDPG); the weighted loss of :1320-1325."""
    r, d, qt = T(r, dt), T(d, dt), T(qt, dt)
    q = T(q, dt, grad=True)
    with torch.no_grad():
        if kind == TGT_DDPG:
            tq = qt[0]
        elif kind in (TGT_MIN, TGT_MIN_ENT):
            tq = torch.min(qt[0], qt[1])
        elif drop > 0:
            srt, _ = torch.sort(qt, dim=0)
            tq = srt[:-drop].mean(dim=0)
        else:
            tq = qt.mean(dim=0)
        if kind in (TGT_MIN_ENT, TGT_TRUNC_ENT):
            tq = tq - alpha * T(lp, dt)
        y_raw = r + GAMMA * (1 - d) * tq
        y = torch.clamp(y_raw, min=CLAMP_LO, max=0.0) if kind == TGT_DDPG else y_raw
    fn = torch.nn.functional.mse_loss if loss == LOSS_MSE else torch.nn.functional.smooth_l1_loss
    losses = []
    for c in range(q.shape[0]):
        if w is not None:
            losses.append((T(w, dt) * fn(q[c], y, reduction="none")).mean())
        else:
            losses.append(fn(q[c], y))
    torch.stack(losses).sum().backward()
    diff = (q.detach() - y)
    td_abs = diff.abs().max(dim=0).values
    return dict(dq=q.grad.numpy(), td_abs=td_abs.numpy(), loss=np.array([float(x.detach()) for x in losses]), td=float(td_abs.mean()),
                qmean=float(q.detach().mean()), y_raw=y_raw.numpy(), diff=diff.numpy())


def td_inputs(seed, kind, B, C, with_w):
    g = np.random.default_rng(seed)
    b = np.arange(B)
    r = np.where(g.random(B) < 0.6, -1.0, 0.0).astype(F32)
    d = (b % 4 == 3).astype(F32)
    if kind == TGT_DDPG:     # every fifth row's target falls below -1/(1-gamma), every fifth above 0
        lo, hi = np.array([-65.0, 5.0, -30.0, -20.0, -10.0])[b % 5], np.array([-55.0, 15.0, -20.0, -10.0, -1.0])[b % 5]
        qt = g.uniform(lo, hi)[None, :].astype(F32)
    else:
        qt = g.normal(-10.0, 5.0, (C, B)).astype(F32)
        qt[1, b % 7 == 0] = qt[0, b % 7 == 0]          # equal target critics
    lp = g.uniform(-3.0, 8.0, B).astype(F32)
    w = g.uniform(0.1, 1.0, B).astype(F32) if with_w else None
    return r, d, qt, lp, w


def td_case(lib, kind, loss, B, C, drop, with_w, seed):
    alpha = float(F32(0.2)) if kind != TGT_TRUNC_ENT else float(F32(0.37))
    r, d, qt, lp, w = td_inputs(seed, kind, B, C, with_w)
    # q = y + delta with |delta| < 0.4, in (0.55, 0.95), in (1.5, 4): both Huber sides, both signs, and the band a moved threshold would flip
    g = np.random.default_rng(seed + 1)
    y64 = ref_td(torch.float64, kind, loss, r, d, qt, np.zeros((C, B), F32), lp, alpha, w, drop)
    y64 = -y64["diff"][0]
    lo, hi = np.array([0.0, 0.55, 0.55, 1.5, 1.5, 0.0]), np.array([0.4, 0.95, 0.95, 4.0, 4.0, 0.4])
    sign = np.array([1.0, 1.0, -1.0, 1.0, -1.0, -1.0])
    cls = (np.arange(B)[None, :] + np.arange(C)[:, None]) % 6
    q = (y64[None, :] + sign[cls] * g.uniform(lo[cls], hi[cls])).astype(F32)
    r32 = ref_td(torch.float32, kind, loss, r, d, qt, q, lp, alpha, w, drop)
    r64 = ref_td(torch.float64, kind, loss, r, d, qt, q, lp, alpha, w, drop)
    ad = np.abs(r32["diff"])
    counts = dict(huber_hi=(r32["diff"] > 1).sum(), huber_lo=(r32["diff"] < -1).sum(), mid=((ad > 0.5) & (ad < 1)).sum(), small=(ad < 0.5).sum(),
                  done=(d == 1).sum(), live=(d == 0).sum())
    if kind == TGT_DDPG:
        counts.update(y_clamped_low=(r32["y_raw"] < CLAMP_LO).sum(), y_clamped_zero=(r32["y_raw"] > 0).sum(),
                      y_inside=((r32["y_raw"] > CLAMP_LO) & (r32["y_raw"] < 0)).sum())
    # the same decisions in both precisions
    assert np.array_equal(r32["diff"] > 1, r64["diff"] > 1) and np.array_equal(r32["diff"] < -1, r64["diff"] < -1)
    covers(B >= 63, **counts)
    args = dict(r=dev(r), d=dev(d), qt=dev(qt), q=dev(q), lp=dev(lp), w=dev(w) if with_w else None)

    def run(multi_block):
        dq, td_abs, met = nan_dev(C, B), (nan_dev(B) if with_w else None), nan_dev(MET_FLOATS)
        rc = lib.gcrl_td_loss_f32(ptr(args["r"]), ptr(args["d"]), ptr(args["qt"]), ptr(args["q"]), ptr(args["lp"]), alpha, ptr(args["w"]), B, C, drop,
                                  kind, loss, GAMMA, CLAMP_LO, multi_block, ptr(dq), ptr(td_abs), ptr(met), 1)
        assert rc == 0, rc
        return host(dq), (host(td_abs) if with_w else None), host(met)

    def check(out):
        dq, td_abs, met = out
        held("td_loss dq", dq, r32["dq"], r64["dq"])
        if td_abs is not None:
            held("td_loss td_abs", td_abs, r32["td_abs"], r64["td_abs"])
        for c in range(C):
            held(f"td_loss loss[{c}]", [met[MET_LOSS + c]], [r32["loss"][c]], [r64["loss"][c]])
        held("td_loss td", [met[MET_TD]], [r32["td"]], [r64["td"]])
        held("td_loss q", [met[MET_Q]], [r32["qmean"]], [r64["qmean"]])
        untouched = np.ones(MET_FLOATS, bool)
        untouched[[MET_TD, MET_Q] + list(range(C))] = False
        assert np.isnan(met[untouched]).all(), "the launch wrote metrics that are not its own"
    return run, check


INSTANCES = [(k, l) for k in (TGT_DDPG, TGT_MIN, TGT_MIN_ENT, TGT_TRUNC_ENT) for l in (LOSS_MSE, LOSS_HUBER)]


def _td_single_cases():
    out = []
    for i, (kind, loss) in enumerate(INSTANCES):
        for j, B in enumerate([SMALL[i % 5], SMALL[(i + 3) % 5], MID[i % 3], BIG[i % 3], BIG[(i + 1) % 3]]):
            C, drop = {TGT_DDPG: (1, 0), TGT_MIN: (2, 0), TGT_MIN_ENT: (2, 0)}.get(kind, TRUNC[(i + j) % 5])
            out.append(pytest.param(kind, loss, B, C, drop, (i + j) % 2, id=f"tgt{kind}-loss{loss}-B{B}-C{C}-drop{drop}-w{(i + j) % 2}"))
    return out


def _td_multi_cases():
    out = []
    for i, (kind, loss) in enumerate(INSTANCES):
        for j in range(3):
            B = MB_TD[(i + 2 * j) % 6]
            C, drop = {TGT_DDPG: (1, 0), TGT_MIN: (2, 0), TGT_MIN_ENT: (2, 0)}.get(kind, TRUNC[(i + 2 * j + 1) % 5])
            out.append(pytest.param(kind, loss, B, C, drop, (i + j + 1) % 2, id=f"tgt{kind}-loss{loss}-B{B}-C{C}-drop{drop}-w{(i + j + 1) % 2}"))
    return out


def test_td_case_tables_meet_every_size_class():
    for cases, sizes in ((_td_single_cases(), SMALL + MID + BIG), (_td_multi_cases(), MB_TD)):
        single = sizes is not MB_TD
        assert {c.values[2] for c in cases} == set(sizes)
        for kind, loss in INSTANCES:
            mine = [c.values[2] for c in cases if c.values[:2] == (kind, loss)]
            assert any(b >= 1024 for b in mine) and any(b % 64 for b in mine)
            assert not single or any(b < 256 for b in mine)
        assert {c.values[3:5] for c in cases if c.values[0] == TGT_TRUNC_ENT} == set(TRUNC)


@pytest.mark.parametrize("kind,loss,B,C,drop,with_w", _td_single_cases())
def test_td_loss_single_workgroup(lib, kind, loss, B, C, drop, with_w):
    run, check = td_case(lib, kind, loss, B, C, drop, bool(with_w), seed=1000 * kind + 100 * loss + B)
    check(run(0))


@pytest.mark.parametrize("kind,loss,B,C,drop,with_w", _td_multi_cases())
def test_td_loss_multi_workgroup(lib, kind, loss, B, C, drop, with_w):
    """The multi-workgroup form: its ticket returns to zero (a second launch into NaN-filled outputs writes the same bits), its
    per-row results are the single-workgroup form's bits, its metric sums hold the fp64 bound on their own."""
    run, check = td_case(lib, kind, loss, B, C, drop, bool(with_w), seed=7000 + 1000 * kind + 100 * loss + B)
    once, twice, single = run(1), run(2), run(0)
    check(once)
    for a, b, what in zip(once, twice, ("dq", "td_abs", "metrics")):
        if a is not None:
            assert same_written(a, b), f"{what}: the second launch differs from the first"
    for a, b, what in zip(once[:2], single[:2], ("dq", "td_abs")):
        if a is not None:
            assert np.array_equal(bits(a), bits(b)), f"{what}: multi-workgroup form differs from the single-workgroup form"


# ------------------------------------------------------------------------------------------------------------- actor selection
def ref_select(dt, q, logp, alpha, drop, min2, target_entropy, log_alpha):
    """src/agent.py:516-521 (SAC), :916-925 (TQC); the alpha loss of :532-546."""
    q, lp = T(q, dt, grad=True), T(logp, dt)
    if min2:
        sel = torch.min(q[0], q[1])
    elif drop > 0:
        srt, _ = torch.sort(q, dim=0)
        sel = srt[:-drop].mean(dim=0)
    else:
        sel = q.mean(dim=0)
    loss = (alpha * lp - sel).mean()
    loss.backward()
    la = torch.tensor(log_alpha, dtype=dt, requires_grad=True)
    al = -(la * (lp + target_entropy).detach()).mean()
    al.backward()
    return dict(dq=q.grad.numpy(), loss=float(loss.detach()), alpha_loss=float(al.detach()), grad=float(la.grad), qmean=float(q.detach().mean()))


SEL = [(2, 0, 1), (2, 0, 0), (3, 1, 0), (5, 2, 0), (8, 0, 0), (8, 7, 0)]


def sel_case(lib, B, C, drop, min2, do_alpha, seed):
    g = np.random.default_rng(seed)
    alpha, te, log_alpha = float(F32(0.2 if min2 else 0.37)), float(F32(-1.5)), float(F32(-0.9))
    q = g.normal(0.0, 2.0, (C, B)).astype(F32)
    tied = np.arange(B) % 3 == 0            # a third of the rows: exact ties, wherever the kept / dropped boundary falls
    q[:, tied] = g.integers(0, 3, (C, int(tied.sum()))).astype(F32)
    if min2:
        q[:, tied] = g.normal(0.0, 2.0, int(tied.sum())).astype(F32)[None, :]
    if B >= 5 and C == 5:
        q[:, 0] = [1, 1, 0, 1, 2]
    logp = g.uniform(-3.0, 8.0, B).astype(F32)
    r32 = ref_select(torch.float32, q, logp, alpha, drop, min2, te, log_alpha)
    r64 = ref_select(torch.float64, q, logp, alpha, drop, min2, te, log_alpha)
    keep = C - drop
    srt = np.sort(q, axis=0)
    straddle = srt[keep - 1] == srt[keep] if drop > 0 else np.zeros(B, bool)     # a tie across the kept / dropped boundary
    if min2:
        covers(B >= 63, tied_rows=(q[0] == q[1]).sum(), first_smaller=(q[0] < q[1]).sum(), second_smaller=(q[0] > q[1]).sum())
        assert (q[0] == q[1]).sum() * 4 >= B
    else:
        covers(B >= 63 and drop > 0, ties_across_the_cut=straddle.sum(), no_tie_at_the_cut=(~straddle).sum())
    qd, ld = dev(q), dev(logp)

    def run(form):
        dq, met, grad = nan_dev(C, B), nan_dev(MET_FLOATS), torch.full((1,), 123.0, dtype=torch.float32, device="cuda")
        rc = lib.gcrl_actor_select_f32(ptr(qd), ptr(ld), alpha, B, C, drop, min2, do_alpha, te, log_alpha, form, ptr(dq), ptr(met), ptr(grad), 1)
        assert rc == 0, rc
        return host(dq), host(met), host(grad)

    def check(out, form):
        dq, met, grad = out
        held("select dq", dq, r32["dq"], r64["dq"])
        # exact: torch.min's 1/2 : 1/2 split on ties; with tied critics the kept ones are those of lower index — what CPU
        # torch.sort does here (observed behaviour of the CPU sort, which is stable in practice; not a documented guarantee)
        # (a critic without gradient gets -1/B * 0 = -0.0 from the kernel and +0.0 from autograd: zeros compare by value)
        assert np.array_equal(bits(dq + F32(0)), bits(r32["dq"] + F32(0))), "dq differs from the fp32 autograd gradient"
        if min2:
            t = q[0] == q[1]
            assert np.array_equal(bits(dq[:, t]), bits(np.full((2, int(t.sum())), F32(-1.0) / F32(B) * F32(0.5))))
        else:
            assert ((dq != 0).sum(axis=0) == keep).all(), "kept count per row"
            if B >= 5 and C == 5 and drop == 2:
                assert (dq[:, 0] != 0).tolist() == [True, True, True, False, False]   # [1, 1, 0, 1, 2]: keeps indices 2, 0, 1
        held("select actor_loss", [met[MET_ACTOR_LOSS]], [r32["loss"]], [r64["loss"]])
        written = [MET_ACTOR_LOSS]
        if form >= 1:
            held("select q rider", [met[MET_Q]], [r32["qmean"]], [r64["qmean"]])
            written += [MET_Q, MET_ALPHA_LOSS]
            if do_alpha:
                held("select alpha_loss", [met[MET_ALPHA_LOSS]], [r32["alpha_loss"]], [r64["alpha_loss"]])
                held("select grad_log_alpha", grad, [r32["grad"]], [r64["grad"]])
            else:      # `gradient_step <= alpha_min_steps: return 0.0`
                assert met[MET_ALPHA_LOSS] == 0.0 and bits(met[MET_ALPHA]) == bits(F32(alpha)) and grad[0] == 123.0
                written.append(MET_ALPHA)
        else:
            assert grad[0] == 123.0
        untouched = np.ones(MET_FLOATS, bool)
        untouched[written] = False
        assert np.isnan(met[untouched]).all(), "the launch wrote metrics that are not its own"
    return run, check


def _sel_cases():
    out = []
    for i, (C, drop, min2) in enumerate(SEL):
        for j, B in enumerate([SMALL[i % 5], MID[i % 3], BIG[i % 3], SMALL[(i + 2) % 5], BIG[(i + 1) % 3]]):
            form, do_alpha = (i + j) % 2, ((i + j) // 2) % 2
            out.append(pytest.param(B, C, drop, min2, form, do_alpha, id=f"B{B}-C{C}-drop{drop}-min{min2}-form{form}-alpha{do_alpha}"))
    return out


@pytest.mark.parametrize("B,C,drop,min2,form,do_alpha", _sel_cases())
def test_actor_select_single_workgroup(lib, B, C, drop, min2, form, do_alpha):
    run, check = sel_case(lib, B, C, drop, min2, do_alpha, seed=31 * B + 7 * C + drop + min2)
    check(run(form), form)


@pytest.mark.parametrize("B,C,drop,min2,do_alpha", [pytest.param(MB_SEL[(i + 2 * j) % 4], C, drop, min2, (i + j) % 2,
                                                                 id=f"B{MB_SEL[(i + 2 * j) % 4]}-C{C}-drop{drop}-min{min2}-alpha{(i + j) % 2}")
                                                    for i, (C, drop, min2) in enumerate(SEL) for j in range(2)])
def test_actor_select_multi_workgroup(lib, B, C, drop, min2, do_alpha):
    """As test_td_loss_multi_workgroup: the ticket returns to zero, the rows' bits are the single-workgroup form's."""
    run, check = sel_case(lib, B, C, drop, min2, do_alpha, seed=99 + 31 * B + 7 * C + drop + min2)
    once, twice, single = run(3), run(2), run(1)
    check(once, 3)
    for a, b, what in zip(once, twice, ("dq", "metrics", "grad_log_alpha")):
        assert same_written(a, b), f"{what}: the second launch differs from the first"
    assert np.array_equal(bits(once[0]), bits(single[0])), "dq: multi-workgroup form differs from the single-workgroup form"


# ------------------------------------------------------------------------------------------------------------- tanh-Gaussian head
def ref_sample(dt, mu, ls_raw, eps, alpha, dact):
    """src/model.py:118-141 under the actor loss mean(alpha * logp - Q): `dact` [C][B][A] stands for the critics' action gradients."""
    mu, ls_raw, eps = T(mu, dt, grad=True), T(ls_raw, dt, grad=True), T(eps, dt)
    log_std = torch.clamp(ls_raw, -20.0, 2.0)
    std = log_std.exp()
    normal = torch.distributions.Normal(mu, std, validate_args=False)
    x_t = mu + eps * std                      # Normal.rsample with its standard-normal draw given
    action = torch.tanh(x_t)
    log_prob = normal.log_prob(x_t)
    log_prob = log_prob - torch.log(1 - action.pow(2) + 1e-8)
    log_prob = log_prob.sum(dim=-1)
    loss = (alpha * log_prob).mean() + (T(dact, dt).sum(dim=0) * action).sum()
    loss.backward()
    return dict(act=action.detach().numpy(), logp=log_prob.detach().numpy(), std=std.detach().numpy(), x=x_t.detach().numpy(),
                dx0=(x_t - mu).detach().numpy(), gmu=mu.grad.numpy(), gls=ls_raw.grad.numpy(), mean_act=torch.tanh(mu).detach().numpy())


LS_BELOW, LS_ABOVE = np.nextafter(F32(-20), F32(-np.inf)), np.nextafter(F32(2), F32(np.inf))


def sample_inputs(seed, regime, B, A):
    g = np.random.default_rng(seed)
    n = B * A
    mu, ls, eps = g.uniform(-1, 1, n), g.uniform(-2.0, 0.5, n), np.clip(g.normal(0, 1, n), -1, 1)
    e = np.arange(n)
    if regime == "band":           # 3 < |x| < 9: log(1 - t^2 + 1e-8) amplifies one ulp of t
        band = e % 2 == 0
        mu[band] = (g.uniform(3.5, 8.4, n) * np.where(g.random(n) < 0.5, -1, 1))[band]
        ls[band] = g.uniform(-3.0, -1.0, n)[band]
    if regime == "edge":
        table = [(12.0, 0.0, 0.3), (-11.0, -1.0, -0.5), (9.5, -20.0, 0.5), (0.3, -25.0, 2.0), (0.5, LS_BELOW, 1.0), (-0.4, LS_ABOVE, 0.2),
                 (0.1, 2.0, -0.1), (14.0, 5.0, 0.1), (-15.0, 2.0, 0.0), (13.0, -20.0, 1.0)]
        for k, (m, l, ee) in enumerate(table):
            sel = e % 16 == k
            mu[sel], ls[sel], eps[sel] = m, l, ee
    return mu.reshape(B, A).astype(F32), ls.reshape(B, A).astype(F32), eps.reshape(B, A).astype(F32)


SHAPES = [(B, A) for B in (1, 255, 256, 257, 513) for A in (1, 3, 4, 16)]


@pytest.mark.parametrize("B,A,regime,C,alpha", [pytest.param(B, A, ("plain", "band", "edge")[(i + i // 4) % 3], (1, 2, 5)[i % 3], (0.2, 1e-3)[(i // 2) % 2],
                                                             id=f"B{B}-A{A}-{('plain', 'band', 'edge')[(i + i // 4) % 3]}-C{(1, 2, 5)[i % 3]}-a{(0.2, 1e-3)[(i // 2) % 2]}")
                                                for i, (B, A) in enumerate(SHAPES)])
def test_tanh_gauss_sample_and_backward(lib, B, A, regime, C, alpha):
    alpha = float(F32(alpha))
    mu, ls, eps = sample_inputs(17 * B + A, regime, B, A)
    g = np.random.default_rng(B + A)
    dact = (g.normal(0, 1, (C, B, A)) / B).astype(F32)
    r32, r64 = (ref_sample(dt, mu, ls, eps, alpha, dact) for dt in (torch.float32, torch.float64))
    x, claim = np.abs(r32["x"]), B * A >= 64
    sat, in_range = x >= 10, (ls >= -20) & (ls <= 2)
    if regime == "plain":
        covers(claim, moderate=(x < 3).sum())
        assert (x < 3).all()
    elif regime == "band":
        covers(claim, band=((x > 3) & (x < 9)).sum(), moderate=(x < 3).sum())
        assert (x < 9).all()
    else:
        covers(claim, saturated=sat.sum(), ls_below=(ls < -20).sum(), ls_above=(ls > 2).sum(), one_ulp_below=(ls == LS_BELOW).sum(),
               one_ulp_above=(ls == LS_ABOVE).sum(), at_low_end=(ls == -20).sum(), at_high_end=(ls == 2).sum(), saturated_in_range=(sat & in_range).sum(),
               x_minus_mu_rounds_to_0=((r32["dx0"] == 0) & (eps != 0)).sum(), fp32_departs=(np.abs(r32["logp"] - r64["logp"]) > 1.0).sum())
        assert not ((x > 3) & (x < 9.4)).any()
    ld_head, ld_act, ld_dact, ld_g = A + 3, A + 5, A + 2, A + 1

    def padded(a, ld, fill=7.0):
        out = np.full(a.shape[:-1] + (ld,), fill, F32)
        out[..., :A] = a
        return dev(out)
    mu_d, ls_d, eps_d = padded(mu, ld_head), padded(ls, ld_head), dev(eps)
    act, logp, s_eps, s_std = padded(np.full((B, A), np.nan, F32), ld_act), nan_dev(B), nan_dev(B, A), nan_dev(B, A)
    assert lib.gcrl_tanh_gauss_fwd_f32(ptr(mu_d), ptr(ls_d), ld_head, ptr(eps_d), B, A, 0, ptr(act), ld_act, ptr(logp), ptr(s_eps), ptr(s_std), 1) == 0
    act_h, logp_h, eps_h, std_h = host(act), host(logp), host(s_eps), host(s_std)
    assert (act_h[:, A:] == 7.0).all(), "columns beyond A were written"
    held("sample act", act_h[:, :A], r32["act"], r64["act"])
    held("sample logp", logp_h, r32["logp"], r64["logp"])
    held("sample std", std_h, r32["std"], r64["std"])
    assert np.array_equal(bits(eps_h), bits(eps))
    want_std = np.exp(np.clip(ls, F32(-20), F32(2)).astype(np.float64)).astype(F32)
    assert np.abs(bits(std_h).astype(np.int64) - bits(want_std).astype(np.int64)).max() <= 1, "save_std: more than 1 ulp from exp(clamp(ls_raw))"

    gmu, gls = padded(np.full((B, A), np.nan, F32), ld_g), padded(np.full((B, A), np.nan, F32), ld_g)
    dact_d = padded(dact, ld_dact)
    assert lib.gcrl_tanh_gauss_bwd_f32(ptr(dact_d), C, ld_dact, ptr(act), ld_act, ptr(s_eps), ptr(s_std), ptr(ls_d), ld_head, alpha, B, A,
                                       ptr(gmu), ptr(gls), ld_g, 1) == 0
    gmu_h, gls_h = host(gmu), host(gls)
    assert (gmu_h[:, A:] == 7.0).all() and (gls_h[:, A:] == 7.0).all(), "columns beyond A were written"
    gmu_h, gls_h = gmu_h[:, :A], gls_h[:, :A]
    held("sample gmu", gmu_h, r32["gmu"], r64["gmu"])
    held("sample gls", gls_h, r32["gls"], r64["gls"])
    # the clamp's backward, exactly: no gradient one ulp outside [-20, 2] (nor further out), a gradient at both end points
    assert (gls_h[~in_range] == 0).all() and (r32["gls"][~in_range] == 0).all()
    if regime == "edge":
        # the saturated / clamped rows follow the fp32 run, not the fp64 one (there x - mu rounds to 0 and tanh to +-1)
        assert np.array_equal(bits(act_h[:, :A][sat]), bits(np.sign(r32["x"][sat]).astype(F32))) and (np.abs(r32["act"][sat]) == 1).all()
        assert (gmu_h[sat] == 0).all() and (r32["gmu"][sat] == 0).all()
        minus_wlp = -(F32(alpha) / F32(B))
        assert np.array_equal(bits(gls_h[sat & in_range]), bits(np.full(int((sat & in_range).sum()), minus_wlp)))
        assert (gls_h[in_range] != 0).all()
        scale = float(np.abs(r64["logp"]).max())
        err32 = float(np.abs(logp_h.astype(np.float64) - r32["logp"]).max())
        print(f"  sample logp vs the fp32 run: {err32:.3e}  (floor {RTOL * scale:.3e})")
        assert err32 <= RTOL * scale, "logp does not follow the fp32 run where fp32 departs from fp64"

    # deterministic: tanh of the mean head, nothing else written
    act2, logp2 = padded(np.full((B, A), np.nan, F32), ld_act), nan_dev(B)
    assert lib.gcrl_tanh_gauss_fwd_f32(ptr(mu_d), None, ld_head, None, B, A, 1, ptr(act2), ld_act, ptr(logp2), None, None, 1) == 0
    act2_h = host(act2)
    held("sample mean action", act2_h[:, :A], r32["mean_act"], r64["mean_act"])
    assert (act2_h[:, A:] == 7.0).all() and np.isnan(host(logp2)).all()
    big = np.abs(mu) >= 10
    assert np.array_equal(bits(act2_h[:, :A][big]), bits(np.sign(mu[big])))


# ------------------------------------------------------------------------------------------------------------- TD3 smoothing
@pytest.mark.parametrize("B,A,ld", [(1, 1, 1), (37, 7, 9), (256, 4, 27), (300, 3, 3)])
def test_td3_smooth_is_the_fp32_expression(lib, B, A, ld):
    """src/agent.py:174-179: adds, multiplies and clamps only, so the kernel equals the fp32 torch expression bit for bit."""
    g = np.random.default_rng(B * A + ld)
    pn, nc = float(F32(0.2)), float(F32(0.5))
    act = g.uniform(-1, 1, (B, A)).astype(F32)
    act[g.random((B, A)) < 0.1] = 1.0
    act[g.random((B, A)) < 0.1] = -1.0
    eps = (g.normal(0, 1, (B, A)) * 2.5).astype(F32)
    a, e = torch.from_numpy(act), torch.from_numpy(eps)
    noise_raw = e * pn
    noise = torch.clamp(noise_raw, -nc, nc)
    want = torch.clamp(a + noise, -1, 1).numpy()
    covers(B * A >= 64, noise_clipped_high=(noise_raw > nc).sum(), noise_clipped_low=(noise_raw < -nc).sum(), noise_inside=(noise_raw.abs() < nc).sum(),
           action_clamped_high=((a + noise) > 1).sum(), action_clamped_low=((a + noise) < -1).sum(), action_inside=((a + noise).abs() < 1).sum())
    buf = np.full((B, ld), 7.0, F32)
    buf[:, :A] = act
    buf_d, eps_d = dev(buf), dev(eps)
    assert lib.gcrl_td3_smooth_f32(ptr(buf_d), ld, B, A, ptr(eps_d), pn, nc, 1) == 0
    got = host(buf_d)
    assert np.array_equal(bits(got[:, :A]), bits(want))
    assert (got[:, A:] == 7.0).all(), "columns beyond A were written"
