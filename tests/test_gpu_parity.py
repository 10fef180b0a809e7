"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the golden vectors
of the real reference and against the oracle on the same seeded inputs.

Bars (north_star): HER index selection, stored rows and gathered batches BIT-EXACT; fp32 losses
and gradients within 1e-5 relative (abs floor 1e-6 on the vector's scale)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from conftest import hparams_from_golden, load_golden
from oracle import her_oracle
from oracle.agent_oracle import OracleAgent, make_config

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _oracle_on_one_thread():
    """The oracle is eager torch on the CPU: its fp32 sums depend on the thread count (the reference itself moves 9.8e-4 between
    thread counts over a few Adam steps), and a trajectory test must not depend on which test ran before it."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)
RTOL, ATOL = 1e-5, 1e-6


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def vec_close(got, want, rtol=RTOL, atol=ATOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want))) <= atol + rtol * float(np.max(np.abs(want))) if want.size else True


# ------------------------------------------------------------------ GEMM kernel (all tile shapes)
@pytest.mark.parametrize("shape", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (64, 64, 27), (33, 7, 13), (256, 1, 256), (17, 300, 70), (2048, 512, 512)])
def test_gemm_forms_against_fp64(lib, M, N, K, shape):
    gen = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    X = torch.randn(M, K, generator=gen)
    W = torch.randn(N, K, generator=gen) / K ** 0.5
    b = torch.randn(N, generator=gen)
    Xd, Wd, bd = X.cuda(), W.cuda(), b.cuda()
    st = 1
    # forward (NT): Y = leaky(X W^T + b)
    Y = torch.full((M, N), float("nan"), device="cuda")
    assert lib.gcrl_gemm_f32(Xd.data_ptr(), K, 1, Wd.data_ptr(), 1, K, Y.data_ptr(), N, bd.data_ptr(), M, N, K, 1, shape, st) == 0
    ref = torch.nn.functional.leaky_relu(X.double() @ W.double().T + b.double(), 0.01)
    assert vec_close(Y.cpu().numpy(), ref.numpy(), rtol=2e-6)
    # dX (NN): dX = G W
    G = torch.randn(M, N, generator=gen)
    Gd = G.cuda()
    dX = torch.full((M, K), float("nan"), device="cuda")
    assert lib.gcrl_gemm_f32(Gd.data_ptr(), N, 1, Wd.data_ptr(), K, 1, dX.data_ptr(), K, None, M, K, N, 0, shape, st) == 0
    assert vec_close(dX.cpu().numpy(), (G.double() @ W.double()).numpy(), rtol=2e-6)
    # dW (TN): dW = G^T X   (reduction over the batch rows)
    dW = torch.full((N, K), float("nan"), device="cuda")
    assert lib.gcrl_gemm_f32(Gd.data_ptr(), 1, N, Xd.data_ptr(), K, 1, dW.data_ptr(), K, None, N, K, M, 0, shape, st) == 0
    assert vec_close(dW.cpu().numpy(), (G.double().T @ X.double()).numpy(), rtol=2e-6)
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N", [(2048, 512), (1024, 256), (77, 36), (5, 4)])
def test_gemm_outer_form_equals_the_mfma_form(lib, M, N):
    """K = 1 (the input gradient of a one-output head): the streaming form (5) writes what the matrix-core form (3) writes,
    with and without bias / activation; a misaligned problem is refused."""
    gen = torch.Generator().manual_seed(M + N)
    g = torch.randn(M, 1, generator=gen).cuda()
    w = torch.randn(1, N, generator=gen).cuda()
    b = torch.randn(N, generator=gen).cuda()
    for act, bias in ((0, None), (1, b.data_ptr()), (3, b.data_ptr())):
        out = [torch.full((M, N), float("nan"), device="cuda") for _ in range(2)]
        for o, shape in zip(out, (3, 5)):
            assert lib.gcrl_gemm_f32(g.data_ptr(), 1, 1, w.data_ptr(), N, 1, o.data_ptr(), N, bias, M, N, 1, act, shape, 1) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[0], out[1])          # (-0 == +0: the MFMA path adds its padded k, exact zeros)
        ref = g.double() @ w.double() + (b.double() if bias else 0)
        ref = torch.nn.functional.leaky_relu(ref, 0.01) if act == 1 else (torch.tanh(ref) if act == 3 else ref)
        assert vec_close(out[1].cpu().numpy(), ref.cpu().numpy(), rtol=2e-6)
    o = torch.empty(M, N + 1, device="cuda")
    assert lib.gcrl_gemm_f32(g.data_ptr(), 1, 1, w.data_ptr(), N, 1, o.data_ptr(), N + 1, None, M, N, 1, 0, 5, 1) != 0   # c_rs % 4 != 0
    assert lib.gcrl_gemm_f32(g.data_ptr(), 1, 1, w.data_ptr(), N, 1, o.data_ptr(), N, None, M, N, 2, 0, 5, 1) != 0       # K != 1


def test_gemm_asymmetric_identity(lib):
    """A = I with an asymmetric B catches a transposed C write (guide §3)."""
    n = 48
    A = torch.eye(n).cuda()
    B = (torch.arange(n * n, dtype=torch.float32).reshape(n, n) * 0.5 + 1).cuda()  # B[k][j]
    Cc = torch.empty(n, n, device="cuda")
    for shape in (1, 2, 3, 4):
        assert lib.gcrl_gemm_f32(A.data_ptr(), n, 1, B.data_ptr(), n, 1, Cc.data_ptr(), n, None, n, n, n, 0, shape, 1) == 0
        assert torch.equal(Cc, B)


# ------------------------------------------------------------------ dW | db on the split LDS-tiled form
@pytest.mark.parametrize("out,inn,batch,S,ldg,ldx", [
    (512, 512, 2048, 2, 512, 512),      # TQC's ensemble batch: two splits per tile
    (256, 256, 2048, 8, 256, 256),      # TD3's hidden layers
    (256, 27, 2048, 8, 256, 28),        # a first layer: 27 input columns inside rows of 28 (element-wise B operand, pipelined loop)
    (1, 256, 2048, 8, 1, 256),          # a critic's head: one output row (element-wise A operand)
    (4, 256, 2048, 8, 4, 256),          # an actor's head
    (70, 100, 300, 4, 72, 100),         # nothing a multiple of anything: partial tiles, a reduction of 18.75 k-steps
    (130, 65, 1024, 3, 132, 68),        # three splits; tile columns 64 | 1
    (256, 256, 2048, 1, 256, 256),      # no split: the row-sum bias gradient alone
    (64, 64, 64, 4, 64, 64)])           # more splits than k-steps per split can fill: empty splits
def test_dw_split_reduction_matches_fp64(lib, out, inn, batch, S, ldg, ldx):
    """dW = G^T X, db = colsum(G) on csrc/gemm_tiled.h with the reduction split over S workgroups per tile (partials + ticket,
    last arriver sums in index order) and the bias gradient taken from the A operand's row sums: against an fp64 product, at the
    accuracy of a plain fp32 sum of `batch` terms; run twice inside the entry point (the tickets must reset themselves); the
    sum-of-squares partials must add up to ||dW|db||^2; and the result must be bitwise reproducible."""
    gen = torch.Generator().manual_seed(out * 3 + inn * 5 + batch)
    G = torch.randn(batch, ldg, generator=gen)
    X = torch.randn(batch, ldx, generator=gen)
    Gd, Xd = G.cuda(), X.cuda()
    runs = []
    for _ in range(2):
        dW = torch.full((out, inn), float("nan"), device="cuda")
        db = torch.full((out,), float("nan"), device="cuda")
        ss = torch.zeros(1, device="cuda")
        assert lib.gcrl_gemm_dw_split_f32(Gd.data_ptr(), ldg, Xd.data_ptr(), ldx, dW.data_ptr(), db.data_ptr(), out, inn, batch, S, ss.data_ptr(), 1) == 0
        torch.cuda.synchronize()
        runs.append((dW.cpu(), db.cpu(), float(ss)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    G64, X64 = G[:, :out].double(), X[:, :inn].double()
    ref_w, ref_b = G64.T @ X64, G64.sum(0)
    mag_w = (G64.abs().T @ X64.abs())          # the size of what is being summed, term by term
    mag_b = G64.abs().sum(0)
    dW, db, ss = runs[0]
    assert float(((dW.double() - ref_w).abs() / mag_w).max()) < 2e-6
    assert float(((db.double() - ref_b).abs() / mag_b).max()) < 2e-6
    want_ss = float((ref_w ** 2).sum() + (ref_b ** 2).sum())
    assert abs(ss - want_ss) <= 1e-5 * want_ss


# ------------------------------------------------------------------ BatchNorm1d(train) + ReLU kernels vs torch (fp32 op, fp64 yardstick)
@pytest.mark.parametrize("B,H", [(512, 256), (64, 64), (100, 48), (33, 4), (2048, 512), (2100, 68), (1, 8)])
def test_batchnorm_relu_forward_backward_against_torch(lib, B, H):
    """nn.BatchNorm1d in training mode followed by ReLU (src/model.py:106-108), forward and backward, at shapes that hit
    every partial block: B not a multiple of 16 / 64, H not a multiple of 64, several 16-row slabs per block (B >= 2048)."""
    gen = torch.Generator().manual_seed(B * 131 + H)
    z = torch.randn(B, H, generator=gen) * 1.7 + 0.3
    gamma = torch.rand(H, generator=gen) + 0.5
    beta = torch.randn(H, generator=gen) * 0.2
    dh = torch.randn(B, H, generator=gen)
    rm0, rv0 = torch.randn(H, generator=gen) * 0.1, torch.rand(H, generator=gen) + 0.5

    def reference(dtype):
        zz = z.detach().clone().to(dtype).requires_grad_(True)
        g, b = gamma.detach().clone().to(dtype).requires_grad_(True), beta.detach().clone().to(dtype).requires_grad_(True)
        rm, rv = rm0.to(dtype).clone(), rv0.to(dtype).clone()
        if B > 1:
            y = torch.nn.functional.batch_norm(zz, rm, rv, g, b, training=True, momentum=0.1, eps=1e-5)
        else:   # torch refuses one row in training mode; the formula still holds (variance 0)
            y = (zz - zz.mean(0)) / torch.sqrt(zz.var(0, unbiased=False) + 1e-5) * g + b
        h = torch.relu(y)
        h.backward(dh.to(dtype))
        return h.detach(), zz.grad, g.grad, b.grad, rm, rv

    h32, dz32, dg32, db32, rm32, rv32 = reference(torch.float32)
    h64, dz64, dg64, db64, rm64, rv64 = reference(torch.float64)
    dev = dict(device="cuda", dtype=torch.float32)
    zd, gd, bd, dhd = z.cuda(), gamma.cuda(), beta.cuda(), dh.cuda()
    rmd, rvd = rm0.cuda().clone(), rv0.cuda().clone()
    h, xhat, dz = torch.empty(B, H, **dev), torch.empty(B, H, **dev), torch.empty(B, H, **dev)
    invstd, dgamma, dbeta = torch.empty(H, **dev), torch.empty(H, **dev), torch.empty(H, **dev)
    scratch = torch.zeros(2 * ((B + 63) // 64) * H, **dev)
    assert lib.gcrl_bn_relu_fwd_f32(zd.data_ptr(), B, H, gd.data_ptr(), bd.data_ptr(), h.data_ptr(), xhat.data_ptr(), invstd.data_ptr(),
                                    rmd.data_ptr(), rvd.data_ptr(), scratch.data_ptr(), 1) == 0
    assert lib.gcrl_bn_relu_bwd_f32(dhd.data_ptr(), xhat.data_ptr(), invstd.data_ptr(), gd.data_ptr(), bd.data_ptr(), B, H, dz.data_ptr(),
                                    dgamma.data_ptr(), dbeta.data_ptr(), scratch.data_ptr(), 1) == 0
    torch.cuda.synchronize()

    def check(name, got, r32, r64):
        got, r32, r64 = got.cpu().double(), r32.double(), r64
        scale = float(r64.abs().max()) + 1e-30
        e_got, e_ref = float((got - r64).abs().max()) / scale, float((r32 - r64).abs().max()) / scale
        # no worse than 3x torch's own fp32 error against fp64, or 1e-5 relative (the north star's tolerance)
        assert e_got <= max(3.0 * e_ref, 1e-5), (name, B, H, e_got, e_ref)

    check("h", h, h32, h64)
    if B > 1:   # (with one row every gradient w.r.t. z is exactly 0 up to rounding noise of size eps)
        check("dz", dz, dz32, dz64)
    check("dgamma", dgamma, dg32, dg64)
    check("dbeta", dbeta, db32, db64)
    if B > 1:
        check("running_mean", rmd, rm32, rm64)
        check("running_var", rvd, rv32, rv64)


@pytest.mark.parametrize("rsplit", [1, 4])
@pytest.mark.parametrize("B,H,K,ldx,Kup,ldg", [(512, 256, 256, 256, 256, 256), (512, 256, 24, 28, 3, 8), (300, 64, 21, 24, 64, 64),
                                             (17, 32, 5, 5, 4, 8), (512, 16, 256, 256, 16, 16), (1, 16, 8, 8, 16, 16), (129, 48, 128, 128, 48, 48)])
def test_linear_batchnorm_relu_slab_launches_against_torch(lib, B, H, K, ldx, Kup, ldg, rsplit):
    """[Linear -> BatchNorm1d(train) -> ReLU] (src/model.py:104-108) as the one-launch-per-direction slab form (csrc/bn_slab.hip):
    forward from x, backward from the consuming layer's output gradient g_up (dh = g_up . w_up), against torch autograd in
    fp32 with the fp64 run as the yardstick.  Shapes: the cfg 5 hidden layer, a first layer (K = 24 inside rows of 28 floats),
    the heads as consumers (K_up = 3 inside rows of 8), element-wise operand loads (K = 21, ldx = 5), partial row tiles, one row.
    rsplit = 4: the rows of a slab split over ceil(B / 128) workgroups that exchange their partials inside the launch (129 rows:
    a second group of ONE row); run twice so that the barrier words of the first launch are what the second one finds."""
    gen = torch.Generator().manual_seed(B * 7 + H * 3 + K)
    x_full = torch.randn(B, ldx, generator=gen)
    W = torch.randn(H, K, generator=gen) / K ** 0.5
    bias = torch.randn(H, generator=gen) * 0.1
    gamma = torch.rand(H, generator=gen) + 0.5
    beta = torch.randn(H, generator=gen) * 0.2
    g_full = torch.randn(B, ldg, generator=gen)
    w_up = torch.randn(Kup, H, generator=gen) / Kup ** 0.5

    def reference(dtype):
        xx = x_full[:, :K].to(dtype)
        Wd, bd = W.to(dtype), bias.to(dtype)
        g, b = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
        z = (xx @ Wd.T + bd).requires_grad_(True)
        mean, var = z.mean(0), z.var(0, unbiased=False)
        xhat = (z - mean) / torch.sqrt(var + 1e-5)
        h = torch.relu(xhat * g + b)
        dh = g_full[:, :Kup].to(dtype) @ w_up.to(dtype)
        h.backward(dh)
        return h.detach(), xhat.detach(), mean.detach(), var.detach(), z.grad, g.grad, b.grad

    r32, r64 = reference(torch.float32), reference(torch.float64)
    dev = dict(device="cuda", dtype=torch.float32)
    h, xhat = torch.empty(B, H, **dev), torch.empty(B, H, **dev)
    invstd, bstat = torch.empty(H, **dev), torch.empty(2, H, **dev)
    dgamma, dbeta = torch.empty(H, **dev), torch.empty(H, **dev)
    xd, Wd, bd, gd, btd, gud, wud = (t.cuda().contiguous() for t in (x_full, W, bias, gamma, beta, g_full, w_up))
    for _ in range(2):
        assert lib.gcrl_bn_linear_slab_fwd_f32(xd.data_ptr(), ldx, Wd.data_ptr(), bd.data_ptr(), gd.data_ptr(), btd.data_ptr(), B, H, K,
                                               h.data_ptr(), xhat.data_ptr(), invstd.data_ptr(), bstat.data_ptr(), rsplit, 1) == 0
        torch.cuda.synchronize()
        xhat_fwd = xhat.clone()
        assert lib.gcrl_bn_linear_slab_bwd_f32(gud.data_ptr(), ldg, Kup, wud.data_ptr(), xhat.data_ptr(), invstd.data_ptr(), gd.data_ptr(),
                                               btd.data_ptr(), B, H, dgamma.data_ptr(), dbeta.data_ptr(), rsplit, 1) == 0
        torch.cuda.synchronize()

    def check(name, got, a32, a64):
        got, a32 = got.cpu().double(), a32.double()
        scale = float(a64.abs().max()) + 1e-30
        e_got, e_ref = float((got - a64).abs().max()) / scale, float((a32 - a64).abs().max()) / scale
        assert e_got <= max(3.0 * e_ref, 1e-5), (name, B, H, K, e_got, e_ref)

    check("h", h, r32[0], r64[0])
    check("mean", bstat[0], r32[2], r64[2])
    if B > 1:
        check("xhat", xhat_fwd, r32[1], r64[1])
        check("var", bstat[1], r32[3], r64[3])
        check("dz", xhat, r32[4], r64[4])     # (written over xhat)
    check("dgamma", dgamma, r32[5], r64[5])
    check("dbeta", dbeta, r32[6], r64[6])
    assert torch.allclose(invstd.cpu(), 1.0 / torch.sqrt(r32[3] + 1e-5), rtol=1e-5)


# ------------------------------------------------------------------ HER rows / batches vs the reference's goldens
CASES = ["full50", "done12", "single", "wrap300", "k8_two_envs", "tiny_cap100"]


def push_case(g, name, buf, how):
    e = 0
    while f"{name}_ep{e}_s" in g.files:
        env = int(g[f"{name}_ep{e}_env"][0])
        done_last = bool(g[f"{name}_ep{e}_done_last"][0])
        s, a, ns = g[f"{name}_ep{e}_s"], g[f"{name}_ep{e}_a"], g[f"{name}_ep{e}_ns"]
        r, dg, ag = g[f"{name}_ep{e}_r"], g[f"{name}_ep{e}_dg"], g[f"{name}_ep{e}_ag"]
        T = s.shape[0]
        if how == "episode":
            d = np.zeros(T, np.float32)
            d[-1] = float(done_last)
            buf.push_episode(env, s, a, ns, r, d, ag)
        else:
            for t in range(T):
                st = torch.from_numpy(s[t]).cuda() if how == "device" else s[t]
                nst = torch.from_numpy(ns[t]).cuda() if how == "device" else torch.from_numpy(ns[t])
                buf.push(env, st, a[t], nst, r[t], bool(done_last and t == T - 1), dg[t], ag[t])
        e += 1


@pytest.mark.parametrize("how", ["device", "host", "episode"])
@pytest.mark.parametrize("name", CASES)
def test_her_rows_and_batch_bit_exact_vs_reference(gcrl, name, how):
    g = load_golden("her_rows.npz")
    cap, k = (int(x) for x in g[f"{name}_cap_k"])
    if how == "episode" and name in ("done12", "single", "k8_two_envs"):
        pass  # episode path handles short / done-terminated episodes too
    random.seed(1898)  # rng="python": the ring shares Python's global MT stream like the reference
    buf = gcrl.HERBuffer(cap, 50, 2, k_future=k, rng="python")
    buf.compute_reward = her_oracle.sparse_reward
    push_case(g, name, buf, how)
    got = buf.rows()
    for key, arr in zip("s a ns r d".split(), got):
        want = g[f"{name}_rows_{key}"]
        assert arr.shape == want.shape, (name, key, arr.shape, want.shape)
        assert np.array_equal(bits(arr), bits(want)), (name, key)
    assert np.array_equal(np.array(random.getstate()[1], dtype=np.uint32), g[f"{name}_state_after_push"])
    if f"{name}_batch_s" in g.files:
        batch = buf.sample(32)
        for key, t in zip("s a r ns d".split(), batch):
            assert np.array_equal(bits(t.cpu().numpy()), bits(g[f"{name}_batch_{key}"])), (name, key)
        assert np.array_equal(np.array(random.getstate()[1], dtype=np.uint32), g[f"{name}_state_after_sample"])


def test_her_engine_rng_equals_python_rng_and_oracle(gcrl):
    """Private engine stream == shared python stream == oracle, over many episodes with eviction."""
    gen = np.random.default_rng(3)
    S, A = 23, 4
    eng = gcrl.HERBuffer(3000, 50, 4, k_future=8, rng="engine", seed=77)
    orc = her_oracle.HERBufferOracle(3000, 50, 4, k_future=8, rng=random.Random(77))
    for ep in range(12):
        T = [50, 50, 13, 50, 1, 50][ep % 6]
        steps = her_oracle.synthetic_episode(gen, T, S, A)
        for t, st in enumerate(steps):
            done = (t == T - 1) and T < 50
            eng.push(ep % 4, torch.from_numpy(st[0]).cuda(), st[1], torch.from_numpy(st[2]).cuda(), st[3], done, st[5], st[6])
            orc.push(ep % 4, st[0], st[1], st[2], st[3], done, st[5], st[6])
    assert len(eng) == len(orc) == 3000
    for got, want in zip(eng.rows(), orc.as_arrays()):
        assert np.array_equal(bits(got), bits(want))
    for _ in range(3):
        got = eng.sample(256)
        want = orc.sample(256)
        for gt, w in zip(got, want):
            assert np.array_equal(bits(gt.cpu().numpy()), bits(w))


@pytest.mark.parametrize("seed", range(10))
def test_her_randomized_differential_vs_oracle(gcrl, seed):
    """Property-style sweep: random state / action / goal widths (records of 1 and 2 column passes), ring
    capacities small enough to wrap several times, 1-4 env streams pushed interleaved, k_future 0-8, ragged episodes
    (1, 2, ... 50 steps; ended by `done` or by the 50-step flush) — stored rows, sampled batches and the index stream
    must equal the oracle's (itself pinned to the reference's goldens) bit for bit."""
    cfg = random.Random(1000 + seed)
    G = cfg.choice([1, 2, 3, 3, 4])
    S = cfg.randint(G + 2, 44)
    A = cfg.randint(1, 8)
    nenvs = cfg.randint(1, 4)
    k = cfg.choice([0, 1, 4, 4, 8])
    cap = cfg.choice([60, 130, 500, 1700, 4000])
    n_eps = cfg.randint(6, 16)
    gen = np.random.default_rng(seed)
    eng = gcrl.HERBuffer(cap, 50, nenvs, k_future=k, rng="engine", seed=500 + seed)
    orc = her_oracle.HERBufferOracle(cap, 50, nenvs, k_future=k, rng=random.Random(500 + seed))
    # one episode queue per env stream, pushed round-robin one transition at a time (the vector-env order, env.py:343-375)
    queues = [[] for _ in range(nenvs)]
    for e in range(n_eps):
        T = cfg.choice([1, 2, 3, 7, 13, 31, 49, 50, 50, 50])
        steps = her_oracle.synthetic_episode(gen, T, S, A, G)
        for t, st in enumerate(steps):
            queues[e % nenvs].append(st[:4] + ((t == T - 1) and T < 50,) + st[5:])
    while any(queues):
        for env in range(nenvs):
            if queues[env]:
                st = queues[env].pop(0)
                eng.push(env, torch.from_numpy(st[0]).cuda(), st[1], torch.from_numpy(st[2]).cuda(), st[3], st[4], st[5], st[6])
                orc.push(env, *st)
    assert len(eng) == len(orc), (len(eng), len(orc))
    if len(orc) == 0:
        return
    for key, got, want in zip("s a ns r d".split(), eng.rows(), orc.as_arrays()):
        assert np.array_equal(bits(got), bits(want)), (seed, key, S, A, G, nenvs, k, cap)
    B = min(len(orc), cfg.choice([1, 7, 32, 64]))
    for _ in range(2):
        for got, want in zip(eng.sample(B), orc.sample(B)):
            assert np.array_equal(bits(got.cpu().numpy()), bits(np.asarray(want, dtype=np.float32).reshape(got.shape))), (seed, B)


def test_device_rng_mode_equals_its_restatement(gcrl):
    """rng="device": future picks by a counter hash inside the flush kernel, batch draws by the same hash
    with duplicates rejected.  Not the reference's stream — pinned against oracle/her_oracle.py HashRng:
    stored rows, sampled batches and the batches update_many consumes, bit-exact."""
    S, A, B = 10, 3, 48
    seed = 77
    buf = gcrl.HERBuffer(5000, 50, 3, k_future=4, rng="device", seed=seed)
    orc = her_oracle.HERBufferOracle(5000, 50, 3, k_future=4, rng=her_oracle.HashRng(seed))
    buf.compute_reward = her_oracle.sparse_reward
    gen = np.random.default_rng(8)
    eps = [her_oracle.synthetic_episode(gen, T, S, A) for T in (50, 50, 50, 50, 50)]
    # envs 0 and 1 finish together (flushed in env order), then three more episodes
    for t in range(50):
        for env in (0, 1):
            buf.push(env, *eps[env][t]); orc.push(env, *eps[env][t])
    for k, env in ((2, 2), (3, 0), (4, 1)):
        for st in eps[k]:
            buf.push(env, *st); orc.push(env, *st)
    assert len(buf) == len(orc) == 5 * 246
    for g, w in zip(buf.rows(), orc.as_arrays()):
        assert np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32))
    for _ in range(3):
        got = buf.sample(B)
        want = orc.sample(B)
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), np.asarray(w, dtype=np.float32).reshape(g.shape))
    # the update engine draws with the same hash stream (its own draw counter continues the ring's)
    cfg = make_config("DDPG", hidden_dim=32, layer_count=2, batch_size=B, max_len=5000)
    ag = gcrl.DDPG(S, A, cfg, None, nenvs=2, gradient_step=3, rng="device", seed=seed)
    orc2 = OracleAgent("DDPG", S, A, cfg, nenvs=2, gradient_step=3, rng=her_oracle.HashRng(seed))
    for k in range(4):
        for st in eps[k]:
            ag.push_her(k % 2, torch.from_numpy(st[0]).cuda(), *st[1:]); orc2.push_her(k % 2, *st)
    ag.actor.set_flat(orc2.flat_params(orc2.actor))
    ag.critic.set_flat(orc2.flat_params(orc2.critics[0]))
    ag.update_target_network(); orc2.hard_update()
    for step, info in zip((1, 2, 3), ag.update_many(1, 3)):
        ref = orc2.update(step)
        assert np.allclose([float(x) for x in info], [float(np.asarray(x)) for x in ref], rtol=5e-5, atol=5e-6)


def test_sample_errors_and_multi_batch(gcrl):
    buf = gcrl.HERBuffer(1000, 50, 1, rng="engine", seed=1)
    gen = np.random.default_rng(0)
    for st in her_oracle.synthetic_episode(gen, 50, 10, 3):
        buf.push(0, st[0], st[1], st[2], st[3], False, st[5], st[6])
    assert len(buf) == 246
    with pytest.raises(AssertionError):
        buf.sample(247)
    out = buf.sample(64, num_batches=3, return_indices=True)
    idx = out[-1].reshape(3, 64)
    for m in range(3):
        assert len(set(idx[m].tolist())) == 64          # without replacement inside a batch
    s_all = buf.rows()[0]
    assert np.array_equal(out[0].cpu().numpy(), s_all[idx.reshape(-1)])


# ------------------------------------------------------------------ sort / truncate op
@pytest.mark.parametrize("width,drop", [(5, 2), (50, 4), (64, 0), (1, 0), (25, 2)])
def test_sort_truncate_mean(lib, width, drop):
    x = torch.randn(777, width)
    xd = x.cuda()
    srt = torch.empty_like(xd)
    mean = torch.empty(777, device="cuda")
    assert lib.gcrl_sort_truncate_mean(xd.data_ptr(), 777, width, drop, srt.data_ptr(), mean.data_ptr(), 1) == 0
    want, _ = torch.sort(x, dim=1)
    assert torch.equal(srt.cpu(), want)
    wm = want[:, : width - drop].double().mean(dim=1)
    assert vec_close(mean.cpu().numpy(), wm.numpy(), rtol=1e-6)


# ------------------------------------------------------------------ update steps vs the reference's goldens
def make_agent(gcrl, g, use_graph):
    kind = str(g["kind"][0])
    S, A, B, gstep = (int(x) for x in g["dims"])
    cfg = hparams_from_golden(g)
    cls = dict(DDPG=gcrl.DDPG, TD3=gcrl.TD3Agent, SAC=gcrl.SACAgent, TQC=gcrl.TQCAgent)[kind]
    ag = cls(S, A, cfg, None, nenvs=1, gradient_step=gstep, use_graph=use_graph, rng="engine", seed=0)
    views = {"actor": ag.actor}
    if kind in ("DDPG", "TD3"):
        views["target_actor"] = ag.target_actor
    for i, (c, t) in enumerate(zip(ag.critics, ag.target_critics)):
        views[f"critic_{i}"] = c
        views[f"target_critic_{i}"] = t
    for name, v in views.items():
        key = f"init_{name}"
        v.set_flat(g[key] if key in g.files else g[f"init_{name.replace('target_', '')}"])
    return ag, views


@pytest.mark.parametrize("use_graph", [False, 2])   # plain launches / hipGraph replay everywhere
@pytest.mark.parametrize("tag", ["ddpg_reach", "ddpg_cosine", "ddpg_pickplace_h256", "td3", "sac", "tqc"])
def test_update_matches_reference(gcrl, tag, use_graph):
    g = load_golden(f"update_{tag}.npz")
    ag, views = make_agent(gcrl, g, use_graph)
    kind = str(g["kind"][0])
    cfg = hparams_from_golden(g)
    # Every agent is held to the north star's 1e-5 against the reference's fp32 run.  SAC / TQC quantities that miss it must
    # pass THROUGH THE REFERENCE'S FP64 RUN of the same fixture (tests/golden/update_<tag>_fp64.npz, make_golden_act.py):
    # |hip - ref64| <= max(3 |ref32 - ref64|, 1e-5 scale) — the criterion of the full-size fixtures (tests/fullsize.py).  The
    # reference's log(1 - tanh(x)^2 + 1e-8) amplifies a 1-ulp tanh difference by 2|t|/(1-t^2) (> 1e3 at |x| > 4, where these
    # fresh-Xavier fixtures sit): its own fp32 run is up to 2.7e-2 (SAC) / 6.7e-3 (TQC) away from its fp64 run on them.
    rtol = 1e-5
    g64 = load_golden(f"update_{tag}_fp64.npz") if kind in ("SAC", "TQC") else None
    via64 = 0
    lr = max(cfg.actor_lr, cfg.critic_lr)
    bad = []
    worst = dict(tuple_rel=0.0, grad_rel_to_max=0.0)     # measured, written to gpurun_out/parity_small.json
    for i, step in enumerate(g["steps"]):
        batch = tuple(torch.from_numpy(g[f"step{i}_{k}"]).cuda() for k in ("s", "a", "r", "ns", "d"))
        kw = {}
        if f"step{i}_noise" in g.files:
            kw["noise"] = torch.from_numpy(g[f"step{i}_noise"])
        if f"step{i}_eps_next" in g.files:
            kw["eps_next"] = torch.from_numpy(g[f"step{i}_eps_next"])
            kw["eps_cur"] = torch.from_numpy(g[f"step{i}_eps_cur"])
        info = ag.update(int(step), batch=batch, **kw)
        want = g[f"step{i}_tuple"]
        assert len(info) == len(want), (tag, i, len(info), len(want))
        got = np.array([float(x) for x in info])
        for j, (a, b) in enumerate(zip(got, want)):
            if b != 0.0:
                worst["tuple_rel"] = max(worst["tuple_rel"], abs(a - b) / abs(b))
            if abs(a - b) > 1e-6 + rtol * abs(b):
                b64 = float(g64[f"step{i}_tuple"][j]) if g64 is not None else None
                if b64 is not None and abs(a - b64) <= 1e-6 + max(3.0 * abs(b - b64), rtol * abs(b64)):
                    via64 += 1
                else:
                    bad.append((f"step{i} tuple[{j}]", a, b, b64))
        # pre-clip gradients (the engine keeps them unscaled; clipping is fused into the optimiser)
        for name, v in views.items():
            k = f"step{i}_gradpre_{name}"
            if k in g.files:
                worst["grad_rel_to_max"] = max(worst["grad_rel_to_max"], float(np.max(np.abs(v.grad_flat() - g[k])) / np.max(np.abs(g[k]))))
            if k in g.files and not vec_close(v.grad_flat(), g[k], rtol=rtol):
                ok64 = False
                if g64 is not None and k in g64.files:
                    r64, r32, x = g64[k], g[k].astype(np.float64), v.grad_flat().astype(np.float64)
                    ok64 = bool(np.all(np.abs(x - r64) <= 1e-7 + np.maximum(3.0 * np.abs(r32 - r64), rtol * np.max(np.abs(r64)))))
                if ok64:
                    via64 += 1
                else:
                    bad.append((k, float(np.max(np.abs(v.grad_flat() - g[k]))), float(np.max(np.abs(g[k])))))
            # parameters after the optimiser / Polyak step.  Adam's update is lr*m/(sqrt(v)+eps):
            # where a gradient is ~0, 1e-7 noise decides its sign and the parameter moves by up
            # to lr either way (SURVEY.md hard part 3; the reference itself differs by 9.8e-4
            # between thread counts; a Linear bias in front of a BatchNorm has an analytically
            # ZERO gradient, i.e. pure noise).  So: entries whose reference gradient is
            # significant must be tight, every entry must be within 2.2*lr.
            k = f"step{i}_param_{name}"
            if k in g.files:
                err = np.abs(v.flat().astype(np.float64) - g[k])
                gk = f"step{i}_gradpre_{name}"
                sig = np.ones(err.shape, bool)
                if gk in g.files:
                    sig = np.abs(g[gk]) > 1e-3 * np.max(np.abs(g[gk]))
                if float(err[sig].max()) > 2e-5 or float(err.max()) > 2.2 * lr:
                    bad.append((k, float(err[sig].max()), float(err.max())))
                v.set_flat(g[k])          # continue the next step from the reference's state
        if f"step{i}_log_alpha" in g.files:
            la = float(ag.log_alpha.detach())
            if abs(la - float(g[f"step{i}_log_alpha"][0])) > 1e-6:
                bad.append((f"step{i}_log_alpha", la, float(g[f"step{i}_log_alpha"][0])))
            if abs(ag.alpha.item() - float(g[f"step{i}_alpha"][0])) > 1e-6:
                bad.append((f"step{i}_alpha", ag.alpha.item()))
            sd = ag.actor.state_dict()
            L = ag.actor.layer_stack
            rm = np.concatenate([sd[f"base_net.{3 * l + 1}.running_mean"].numpy() for l in range(L)])
            rv = np.concatenate([sd[f"base_net.{3 * l + 1}.running_var"].numpy() for l in range(L)])
            if not vec_close(rm, g[f"step{i}_bn_mean"], rtol=1e-5) or not vec_close(rv, g[f"step{i}_bn_var"], rtol=1e-5):
                bad.append((f"step{i}_bn_stats", float(np.max(np.abs(rm - g[f"step{i}_bn_mean"]))),
                            float(np.max(np.abs(rv - g[f"step{i}_bn_var"])))))
            ag.actor._set("bn_running_mean", g[f"step{i}_bn_mean"])
            ag.actor._set("bn_running_var", g[f"step{i}_bn_var"])
            ag.actor._set("log_alpha", g[f"step{i}_log_alpha"])
    worst["quantities_passed_through_the_fp64_run"] = via64
    _record_small(tag, use_graph, rtol, worst)
    assert not bad, bad[:10]


_small = {}


def _record_small(tag, use_graph, rtol, worst):
    import json
    import os
    from conftest import ROOT
    _small[f"{tag}/graph={use_graph}"] = dict(rtol_asserted=rtol, **worst)
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "parity_small.json"), "w") as f:
        json.dump(dict(note="HIP vs the reference's fp32 goldens (tests/golden/update_*.npz): worst relative error of a returned "
                            "tuple entry, worst gradient error relative to the vector's max", rows=_small), f, indent=1)


def test_adam_moments_match_reference(gcrl):
    g = load_golden("update_ddpg_reach.npz")
    ag, views = make_agent(gcrl, g, True)
    for i, step in enumerate(g["steps"]):
        batch = tuple(torch.from_numpy(g[f"step{i}_{k}"]).cuda() for k in ("s", "a", "r", "ns", "d"))
        ag.update(int(step), batch=batch)
    for name in ("actor", "critic_0"):
        m = views[name]._get(f"adam_m:{name}")
        v = views[name]._get(f"adam_v:{name}")
        assert vec_close(m, g[f"final_adam_m_{name}"], rtol=2e-5)
        assert vec_close(v, g[f"final_adam_v_{name}"], rtol=2e-5)


# ------------------------------------------------------------------ end to end vs the oracle, sampling path
@pytest.mark.parametrize("kind,S,A", [("DDPG", 10, 3), ("TD3", 10, 3), ("DDPG", 41, 7), ("TD3", 62, 2)])
def test_sampled_updates_track_oracle(gcrl, kind, S, A):
    """push -> flush -> sample -> update, three steps, engine RNG == oracle RNG; deterministic
    agents only (SAC/TQC draw device noise when nothing is injected).  The wide state dims put the
    ring record past 64 floats (second column pass of the engine's batch gather)."""
    B = 64
    cfg = make_config(kind, hidden_dim=32, layer_count=2, batch_size=B, max_len=5000, ac_update_freq=1,
                      policy_noise=0.0, noise_clamp=0.5, grad_clip=5.0)
    cls = dict(DDPG=gcrl.DDPG, TD3=gcrl.TD3Agent)[kind]
    ag = cls(S, A, cfg, None, nenvs=2, gradient_step=3, rng="engine", seed=5)
    orc = OracleAgent(kind, S, A, cfg, nenvs=2, gradient_step=3, rng=random.Random(5))
    gen = np.random.default_rng(1)
    for ep in range(4):
        for st in her_oracle.synthetic_episode(gen, 50, S, A):
            ag.push_her(ep % 2, torch.from_numpy(st[0]).cuda(), *st[1:])
            orc.push_her(ep % 2, *st)
    ag.actor.set_flat(orc.flat_params(orc.actor))
    for i, c in enumerate(orc.critics):
        ag.critics[i].set_flat(orc.flat_params(c))
    ag.update_target_network()
    orc.hard_update()
    outs = ag.update_many(1, 3)            # one gather launch for the three batches
    for step, info in zip((1, 2, 3), outs):
        ref = orc.update(step)             # policy_noise = 0 -> TD3's randn draw is multiplied away
        got = np.array([float(x) for x in info])
        want = np.array([float(np.asarray(x)) for x in ref])
        assert got.shape == want.shape
        assert np.allclose(got, want, rtol=5e-5, atol=5e-6), (kind, step, got, want)


def test_update_many_equals_repeated_update(gcrl):
    S, A, B = 10, 3, 32
    cfg = make_config("DDPG", hidden_dim=32, layer_count=2, batch_size=B, max_len=2000)
    gen = np.random.default_rng(2)
    eps = [her_oracle.synthetic_episode(gen, 50, S, A) for _ in range(2)]

    def build():
        ag = gcrl.DDPG(S, A, cfg, None, nenvs=1, gradient_step=8, rng="engine", seed=9)
        for ep in eps:
            for st in ep:
                ag.push_her(0, *st)
        ag.actor.set_flat(np.linspace(-0.1, 0.1, ag.actor.numel(), dtype=np.float32))
        ag.critic.set_flat(np.linspace(0.1, -0.1, ag.critic.numel(), dtype=np.float32))
        ag.update_target_network()
        return ag

    a1, a2 = build(), build()
    t1 = [tuple(float(x) for x in a1.update(s)) for s in range(1, 9)]
    t2 = [tuple(float(x) for x in t) for t in a2.update_many(1, 8)]
    assert t1 == t2                                   # same kernels, same order: bitwise equal
    assert np.array_equal(a1.actor.flat(), a2.actor.flat())


def _ddpg_for_schedules(gcrl, H, L, pipeline, B=32, S=10, A=3, use_graph=True):
    cfg = make_config("DDPG", hidden_dim=H, layer_count=L, batch_size=B, max_len=3000, grad_clip=0.5)
    gen = np.random.default_rng(4)
    eps = [her_oracle.synthetic_episode(gen, 50, S, A) for _ in range(3)]
    ag = gcrl.DDPG(S, A, cfg, None, nenvs=1, gradient_step=40, rng="engine", seed=11, pipeline=pipeline, use_graph=use_graph)
    for ep in eps:
        for st in ep:
            ag.push_her(0, *st)
    gen2 = np.random.default_rng(5)
    ag.actor.set_flat((0.1 * gen2.standard_normal(ag.actor.numel())).astype(np.float32))
    ag.critic.set_flat((0.1 * gen2.standard_normal(ag.critic.numel())).astype(np.float32))
    ag.update_target_network()
    return ag


def _run_many(ag):
    out = []
    for s0, n in [(1, 40), (41, 7), (48, 33), (81, 10)]:
        out += [tuple(float(x) for x in t) for t in ag.update_many(s0, n)]
    return out


# (sequential agent, overlapped agent): layer-per-launch path vs its co-scheduled form, and the
# row-block path's update() (K then P) vs its overlapped update_many
@pytest.mark.parametrize("levels", [(0, 1, True), (2, 2, True), (2, 2, 2)])   # (sequential, overlapped, use_graph of the latter)
@pytest.mark.parametrize("H,L", [(32, 2), (64, 3)])
def test_pipelined_ddpg_is_bitwise_the_sequential_path(gcrl, H, L, levels):
    """Software-pipelined update_many (actor phase of step i co-scheduled with the critic phase of
    step i+1) vs one update() per step, across two Polyak boundaries (steps 40 and 80) and an
    update_many call that starts mid-stream: every returned tuple and every parameter bitwise equal."""
    a_seq, a_pipe = _ddpg_for_schedules(gcrl, H, L, levels[0]), _ddpg_for_schedules(gcrl, H, L, levels[1], use_graph=levels[2])
    seq = [tuple(float(x) for x in a_seq.update(s)) for s in range(1, 91)]
    pipe = _run_many(a_pipe)
    assert len(seq) == len(pipe) == 90
    for i, (x, y) in enumerate(zip(seq, pipe)):
        assert x == y, (i + 1, x, y)
    for v1, v2 in [(a_seq.actor, a_pipe.actor), (a_seq.critic, a_pipe.critic), (a_seq.target_actor, a_pipe.target_actor),
                   (a_seq.target_critic, a_pipe.target_critic)]:
        assert np.array_equal(v1.flat(), v2.flat())


@pytest.mark.parametrize("H,L,B", [(32, 2, 32), (64, 3, 30), (256, 3, 256), (512, 1, 64), (36, 4, 70)])
def test_row_block_ddpg_tracks_the_layer_per_launch_path(gcrl, H, L, B):
    """The row-block kernels (whole forward / input-gradient chain of a phase in one launch, weights
    streamed from [in][out] copies the optimiser keeps in step) against the per-layer GEMM path over
    90 steps without any parameter read-back in between: same math, different summation order."""
    a_old, a_new = _ddpg_for_schedules(gcrl, H, L, 0, B=B), _ddpg_for_schedules(gcrl, H, L, 2, B=B)
    old = np.array([tuple(float(x) for x in a_old.update(s)) for s in range(1, 91)])
    new = np.array(_run_many(a_new))
    # tight while the two trajectories are the same trajectory; later a sign flip of a ~0 Adam
    # gradient or a LeakyReLU kink sends them apart like any fp32 reordering does
    assert np.allclose(old[:5], new[:5], rtol=2e-5, atol=1e-6), np.abs(old[:5] - new[:5]).max()
    assert np.all(np.isfinite(new))
    # the copies kept by the optimiser == copies rebuilt from the parameters before every step
    a_chk = _ddpg_for_schedules(gcrl, H, L, 2, B=B)
    chk = []
    for s in range(1, 91):
        chk.append(tuple(float(x) for x in a_chk.update(s)))
        a_chk.actor.set_flat(a_chk.actor.flat())     # marks the [in][out] copies stale
    assert np.array_equal(np.array(chk), new)
    for v1, v2 in [(a_chk.actor, a_new.actor), (a_chk.critic, a_new.critic), (a_chk.target_critic, a_new.target_critic)]:
        assert np.array_equal(v1.flat(), v2.flat())


@pytest.mark.parametrize("kind,H,L,B,S,A", [("TD3", 32, 2, 32, 10, 3), ("TD3", 128, 3, 1030, 23, 4), ("TD3", 64, 1, 7, 5, 16),
                                              ("DDPG", 4, 2, 3, 3, 1), ("DDPG", 128, 8, 17, 30, 6), ("DDPG", 520, 2, 40, 12, 2),
                                              ("TD3-devnoise", 64, 2, 50, 9, 3), ("SAC", 64, 2, 40, 11, 3), ("SAC", 256, 3, 130, 22, 4),
                                              # 2A > 16: heads_sample_rows' two-pass branch and the wide side of sac_heads.h
                                              ("SAC", 64, 2, 40, 11, 9), ("SAC", 64, 2, 40, 11, 16)])
def test_row_block_path_against_the_layer_per_launch_path_one_step(gcrl, kind, H, L, B, S, A):
    """Shape sweep of the row-block kernels (ragged last row block, 1..8 hidden layers, 1..16
    action dims, hidden width below / across the 256-column chunk, 4-/8-/16-row blocks): one update
    with injected batches and noise from identical parameters must give the layer-per-launch
    path's gradients, parameters and metrics to fp32 reordering accuracy."""
    inject_noise = kind != "TD3-devnoise"     # else: the smoothing noise comes from the device counter hash in both paths
    kind = kind.split("-")[0]
    cls = dict(DDPG=gcrl.DDPG, TD3=gcrl.TD3Agent, SAC=gcrl.SACAgent)[kind]
    cfg = make_config(kind, hidden_dim=H, layer_count=L, batch_size=B, max_len=2000, grad_clip=0.7, ac_update_freq=1,
                      policy_noise=0.2, noise_clamp=0.5)
    gen = np.random.default_rng(H + L + B)
    batch = (gen.standard_normal((B, S)).astype(np.float32), gen.uniform(-1, 1, (B, A)).astype(np.float32),
             -(gen.uniform(size=(B, 1)) > 0.3).astype(np.float32), gen.standard_normal((B, S)).astype(np.float32),
             (gen.uniform(size=(B, 1)) > 0.9).astype(np.float32))
    noise = gen.standard_normal((B, A)).astype(np.float32)
    agents = []
    for level in (0, 2):
        ag = cls(S, A, cfg, None, nenvs=1, gradient_step=40, rng="engine", seed=3, pipeline=level)
        g2 = np.random.default_rng(9)
        ag.actor.set_flat((0.3 * g2.standard_normal(ag.actor.numel())).astype(np.float32))
        for c in ag.critics:
            c.set_flat((0.3 * g2.standard_normal(c.numel())).astype(np.float32))
        ag.update_target_network()
        agents.append(ag)
    outs = []
    for ag in agents:
        kw = dict(noise=torch.from_numpy(noise).cuda()) if (kind == "TD3" and inject_noise) else {}
        if kind == "SAC":   # the two reparameterisation draws (next-state action, current action) injected
            kw = dict(eps_next=torch.from_numpy(noise).cuda(), eps_cur=torch.from_numpy(noise[::-1].copy()).cuda())
        tup = ag.update(1, batch=tuple(torch.from_numpy(x).cuda() for x in batch), **kw)
        outs.append(np.array([float(x) for x in tup]))
    assert np.allclose(outs[0], outs[1], rtol=1e-4, atol=1e-6), (outs[0], outs[1])
    a0, a1 = agents
    views = lambda ag: [("actor", ag.actor)] + [(f"critic_{i}", c) for i, c in enumerate(ag.critics)]
    for (nm, v0), (_, v1) in zip(views(a0), views(a1)):
        g0, g1 = v0.grad_flat(), v1.grad_flat()
        scale = max(1e-6, float(np.abs(g0).max()))
        assert float(np.abs(g0 - g1).max()) <= 2e-5 * scale + 1e-7, (nm, float(np.abs(g0 - g1).max()), scale)
    pairs = [(a0.actor, a1.actor), (a0.critics[0], a1.critics[0]), (a0.target_critics[0], a1.target_critics[0])]
    if kind != "SAC":
        pairs.append((a0.target_actor, a1.target_actor))
    for v0, v1 in pairs:
        d = np.abs(v0.flat() - v1.flat())
        assert float(np.mean(d > 2e-5)) < 0.02 and float(d.max()) < 3e-3      # Adam turns ~0 gradients into +-lr


@pytest.mark.parametrize("A", [9, 16])
def test_sac_first_update_with_wide_actions_matches_the_oracle(gcrl, A):
    """SAC with more than 8 actions (2A > 16: the two-pass branch of heads_sample_rows, the wide side of csrc/sac_heads.h), which no
    other test of the suite reaches: the first update() against OracleAgent from identical parameters, batch and injected eps -
    returned tuple and pre-clip gradients of the actor and both critics at RTOL / ATOL."""
    H, L, B, S = 64, 2, 40, 11
    cfg = make_config("SAC", hidden_dim=H, layer_count=L, batch_size=B, max_len=2000, grad_clip=0.7, ac_update_freq=1)
    torch.manual_seed(40 + A)
    orc = OracleAgent("SAC", S, A, cfg, nenvs=1, gradient_step=40, rng=random.Random(1))
    ag = gcrl.SACAgent(S, A, cfg, None, nenvs=1, gradient_step=40, rng="engine", seed=3)
    gen = np.random.default_rng(100 + A)
    with torch.no_grad():   # moderate tanh-Gaussian heads (see tests/detdata.py), asymmetric everything else
        for net in [orc.actor] + orc.critics:
            for p in net.parameters():
                p.add_(torch.from_numpy((0.02 * gen.standard_normal(tuple(p.shape))).astype(np.float32)))
        orc.actor.log_std_head.weight.mul_(0.25); orc.actor.log_std_head.bias.fill_(-1.0); orc.actor.mean_head.weight.mul_(0.5)
    orc.hard_update()
    ag.actor.set_flat(orc.flat_params(orc.actor))
    for v, c in zip(ag.critics, orc.critics):
        v.set_flat(orc.flat_params(c))
    ag.update_target_network()
    batch = (gen.standard_normal((B, S)).astype(np.float32), gen.uniform(-1, 1, (B, A)).astype(np.float32),
             -(gen.uniform(size=(B, 1)) > 0.3).astype(np.float32), gen.standard_normal((B, S)).astype(np.float32),
             (gen.uniform(size=(B, 1)) > 0.9).astype(np.float32))
    e1, e2 = gen.standard_normal((B, A)).astype(np.float32), gen.standard_normal((B, A)).astype(np.float32)
    want = orc.update(1, tuple(torch.from_numpy(x) for x in batch), eps_next=torch.from_numpy(e1), eps_cur=torch.from_numpy(e2))
    got = ag.update(1, batch=tuple(torch.from_numpy(x).cuda() for x in batch), eps_next=torch.from_numpy(e1), eps_cur=torch.from_numpy(e2))
    g = np.array([float(x) for x in got]); w = np.array([float(np.asarray(x)) for x in want])
    assert g.shape == w.shape == (9,)
    print(f"SAC A={A}: tuple worst |diff| {np.abs(g - w).max():.3e} of scale {np.abs(w).max():.3e}")
    assert vec_close(g, w), (g, w)
    for v, pre in zip(ag.critics, orc.last["critic_grads_pre"]):
        print(f"SAC A={A}: {v.name} pre-clip gradient worst |diff| {np.abs(v.grad_flat() - pre).max():.3e} of scale {np.abs(pre).max():.3e}")
        assert vec_close(v.grad_flat(), pre), (v.name, float(np.abs(v.grad_flat() - pre).max()), float(np.abs(pre).max()))
    pre = orc.last["actor_grads_pre"]
    print(f"SAC A={A}: actor pre-clip gradient worst |diff| {np.abs(ag.actor.grad_flat() - pre).max():.3e} of scale {np.abs(pre).max():.3e}")
    assert vec_close(ag.actor.grad_flat(), pre), (float(np.abs(ag.actor.grad_flat() - pre).max()), float(np.abs(pre).max()))


def test_tuple_contract_and_td_error_array(gcrl):
    cfg = make_config("TD3", hidden_dim=32, layer_count=2, batch_size=16, ac_update_freq=2)
    ag = gcrl.TD3Agent(10, 3, cfg, None, nenvs=1, gradient_step=4, sync_metrics=True, rng="engine", seed=1)
    gen = np.random.default_rng(0)
    for st in her_oracle.synthetic_episode(gen, 50, 10, 3):
        ag.push_her(0, *st)
    t1 = ag.update(1)
    t2 = ag.update(2)
    assert len(t1) == 6 and len(t2) == 8                         # src/env.py:448-506 dispatches on these
    assert isinstance(t1[2], np.ndarray) and t1[2].ndim == 0      # td_error is a 0-d array (src/agent.py:243)
    assert isinstance(t2[3], np.ndarray) and isinstance(t2[0], float)


# ------------------------------------------------------------------ full-size properties (BASELINE configs)
def test_full_size_ring_properties(gcrl):
    """cfg 2 size: capacity 1e6, B = 1024.  Size-independent properties: FIFO length/eviction,
    gathered rows == ring rows at the drawn indices, no repeats inside a batch, relabelled rows
    keep obs and carry done = 0 / reward in {-1, -0}."""
    S, A, k = 10, 3, 4
    cap = 1_000_000
    buf = gcrl.HERBuffer(cap, 50, 8, k_future=k, rng="engine", seed=1898)
    gen = np.random.default_rng(7)
    n_eps = 400
    pool = [her_oracle.synthetic_episode(gen, 50, S, A) for _ in range(16)]
    for ep in range(n_eps):
        steps = pool[ep % 16]
        s, a, ns, r, d, dg, agl = zip(*steps)
        buf.push_episode(ep % 8, np.array(s), np.array(a), np.array(ns), np.array(r, np.float32), np.zeros(50, np.float32), np.array(agl))
    assert len(buf) == n_eps * 246
    out = buf.sample(1024, num_batches=4, return_indices=True)
    idx = out[-1].reshape(4, 1024)
    for m in range(4):
        assert len(np.unique(idx[m])) == 1024
    rows = buf.rows()
    flat_idx = idx.reshape(-1)
    for t, arr in zip(out[:5], (rows[0], rows[1], rows[3][:, None], rows[2], rows[4][:, None])):
        assert np.array_equal(bits(t.cpu().numpy()), bits(arr[flat_idx]))
    s_rows, _, _, r_rows, d_rows = rows[0], rows[1], rows[2], rows[3], rows[4]
    ep0 = s_rows[:246]
    for i in range(49):
        for j in range(1, k + 1):
            assert np.array_equal(ep0[i * 5 + j][:-3], ep0[i * 5][:-3])
            assert d_rows[i * 5 + j] == 0.0 and r_rows[i * 5 + j] in (-1.0, 0.0)
    # overflow: FIFO eviction keeps exactly `cap` newest rows
    small = gcrl.HERBuffer(1000, 50, 1, k_future=k, rng="engine", seed=3)
    orc = her_oracle.HERBufferOracle(1000, 50, 1, k_future=k, rng=random.Random(3))
    for ep in range(7):
        for st in pool[ep]:
            small.push(0, *st)
            orc.push(0, *st)
    assert len(small) == 1000
    for got, want in zip(small.rows(), orc.as_arrays()):
        assert np.array_equal(bits(got), bits(want))


def test_large_k_future_flush_bit_exact(gcrl):
    """k_future * (T - 1) beyond the flush kernel's inline argument space (2048 indices): the future indices travel
    through an uploaded buffer instead; rows and RNG state still equal the oracle's, several envs finishing together."""
    S, A, k = 10, 3, 48
    eng = gcrl.HERBuffer(60000, 50, 3, k_future=k, rng="engine", seed=21)
    orc = her_oracle.HERBufferOracle(60000, 50, 3, k_future=k, rng=random.Random(21))
    gen = np.random.default_rng(6)
    eps = [her_oracle.synthetic_episode(gen, 50, S, A) for _ in range(3)]
    for t in range(50):
        s = torch.from_numpy(np.stack([eps[e][t][0] for e in range(3)])).cuda()
        ns = torch.from_numpy(np.stack([eps[e][t][2] for e in range(3)])).cuda()
        eng.push_batch(s, np.stack([eps[e][t][1] for e in range(3)]), ns, np.array([eps[e][t][3] for e in range(3)], np.float32),
                       np.zeros(3, bool), np.stack([eps[e][t][6] for e in range(3)]))
        for e in range(3):
            orc.push(e, *eps[e][t])
    assert len(eng) == len(orc) == 3 * (50 + k * 49)
    for got, want in zip(eng.rows(), orc.as_arrays()):
        assert np.array_equal(bits(got), bits(want))
    for st in her_oracle.synthetic_episode(gen, 50, S, A):     # and the single-push path
        eng.push(1, *st); orc.push(1, *st)
    for got, want in zip(eng.rows(), orc.as_arrays()):
        assert np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------ distributional TQC (BASELINE.json configs[3]; no reference parity)
# the small-net cases: Q-wide head GEMM, its backward and the [C][B][Q] stores at Q = 2, 13, 21 (rows not 16-byte aligned) and
# Q = 32, a full wavefront of pooled atoms (C*Q = 64) and one padding lane (63), drop = 0 and Q - 1, ragged last row groups
@pytest.mark.parametrize("H,L,B,Q,C,drop", [(32, 2, 64, 25, 2, 2), (64, 3, 130, 8, 3, 1), (512, 3, 2048, 25, 2, 2),
                                            (32, 2, 7, 32, 2, 0), (32, 2, 66, 8, 8, 7), (32, 2, 30, 21, 3, 5), (32, 2, 5, 2, 2, 1), (32, 2, 33, 13, 4, 12)])
def test_quantile_tqc_matches_its_oracle(gcrl, H, L, B, Q, C, drop):
    """The 25-quantile x 2-critic TQC variant (n_quantiles > 1: pooled-atom wavefront sort, truncation, quantile-Huber
    loss) against oracle/quantile_tqc_oracle.py — the reference has no quantile critic, so the oracle is the specification
    (built from the reference's own networks / optimiser / cadence).  Two steps from identical parameters: returned tuples,
    pre-clip gradients of every network, including the full BASELINE shape (H=512, B=2048)."""
    _quantile_tqc_against_its_oracle(gcrl, H, L, B, Q, C, drop, steps=(1, 2))


def test_quantile_tqc_matches_its_oracle_across_the_actor_cadence(gcrl):
    """The same with ac_update_freq = 2 and the log-alpha branch switching on inside the run (alpha_min_steps as in
    tests/test_gpu_multistep.py): critic-only steps (6-tuples), actor steps (9-tuples) with alpha frozen, then live."""
    lens, alpha_losses = _quantile_tqc_against_its_oracle(gcrl, 32, 2, 64, 25, 2, 2, steps=range(1, 11), ac_update_freq=2, alpha_min_steps=6.0,
                                                          alpha_lr=1e-2)
    assert lens == [6, 9] * 5
    # steps 2, 4, 6: off; step 8 > alpha_min_steps: the first live update, whose loss -(log_alpha * ...).mean() is 0 at log_alpha = 0
    # and whose step moves log_alpha; step 10: the loss of the moved log_alpha
    assert alpha_losses[:4] == [0.0] * 4 and alpha_losses[4] != 0.0


def _quantile_tqc_against_its_oracle(gcrl, H, L, B, Q, C, drop, steps, ac_update_freq=1, **over):
    from oracle.quantile_tqc_oracle import QuantileTQCOracle
    S, A = 22, 3
    cfg = make_config("TQC", **dict(dict(hidden_dim=H, layer_count=L, batch_size=B, max_len=5000, grad_clip=5.0, gamma=0.95, tau=0.05,
                                         alpha_min_steps=0.0, ac_update_freq=ac_update_freq), **over))
    lens, alpha_losses = [], []
    torch.manual_seed(3)
    torch.set_num_threads(4)
    orc = QuantileTQCOracle(S, A, cfg, n_quantiles=Q, num_critics=C, top_drop=drop)
    ag = gcrl.TQCAgent(S, A, cfg, None, nenvs=1, gradient_step=40, rng="engine", seed=0, n_quantiles=Q, num_critics=C,
                       top_quantiles_to_drop=drop)
    gen = np.random.default_rng(H + B)
    with torch.no_grad():   # moderate tanh-Gaussian heads (see tests/detdata.py), asymmetric everything else
        for net in [orc.actor] + orc.critics:
            for p in net.parameters():
                p.add_(torch.from_numpy((0.02 * gen.standard_normal(tuple(p.shape))).astype(np.float32)))
        orc.actor.log_std_head.weight.mul_(0.25); orc.actor.log_std_head.bias.fill_(-1.0); orc.actor.mean_head.weight.mul_(0.5)
    orc.hard_update()
    ag.actor.set_flat(orc.flat_params(orc.actor))
    for v, c in zip(ag.critics, orc.critics):
        v.set_flat(orc.flat_params(c))
    ag.update_target_network()
    for step in steps:
        batch = (gen.standard_normal((B, S)).astype(np.float32), gen.uniform(-1, 1, (B, A)).astype(np.float32),
                 -(gen.uniform(size=(B, 1)) > 0.3).astype(np.float32), gen.standard_normal((B, S)).astype(np.float32),
                 (gen.uniform(size=(B, 1)) > 0.9).astype(np.float32))
        e1, e2 = gen.standard_normal((B, A)).astype(np.float32), gen.standard_normal((B, A)).astype(np.float32)
        want = orc.update(step, tuple(torch.from_numpy(x) for x in batch), torch.from_numpy(e1), torch.from_numpy(e2))
        got = ag.update(step, batch=tuple(torch.from_numpy(x).cuda() for x in batch), eps_next=torch.from_numpy(e1),
                        eps_cur=torch.from_numpy(e2))
        g = np.array([float(x) for x in got]); w = np.array([float(x) for x in want])
        actor_step = step % ac_update_freq == 0
        assert g.shape == w.shape == ((9,) if actor_step else (6,))
        assert np.allclose(g, w, rtol=5e-5, atol=2e-6), (step, g, w)
        for v, pre in zip(ag.critics, orc.last["critic_grads_pre"]):
            assert vec_close(v.grad_flat(), pre, rtol=5e-5), (step, v.name, float(np.abs(v.grad_flat() - pre).max()), float(np.abs(pre).max()))
        if actor_step:
            assert vec_close(ag.actor.grad_flat(), orc.last["actor_grads_pre"], rtol=5e-5), step
            alpha_losses.append(float(g[-1]))
        lens.append(len(g))
        # continue both from the oracle's state
        ag.actor.set_flat(orc.flat_params(orc.actor))
        for v, t, c, tc in zip(ag.critics, ag.target_critics, orc.critics, orc.target_critics):
            v.set_flat(orc.flat_params(c)); t.set_flat(orc.flat_params(tc))
        bns = [m for m in orc.actor.base_net if isinstance(m, torch.nn.BatchNorm1d)]
        ag.actor._set("bn_running_mean", np.concatenate([m.running_mean.numpy() for m in bns]))
        ag.actor._set("bn_running_var", np.concatenate([m.running_var.numpy() for m in bns]))
        ag.actor._set("log_alpha", orc.log_alpha.detach().numpy())
    return lens, alpha_losses
