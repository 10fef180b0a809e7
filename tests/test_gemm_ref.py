"""CPU tests of tests/gemm_ref.py, the float64 definition the batched GEMM is held to on the GPU (tests/test_gpu_gemm_batch.py):
the definition against torch matmul and autograd in float64, the restated form rule against a hand-made table, and the accuracy
bar against the worst summation order the kernels use — one fp32 accumulator walking K alone."""
import numpy as np
import pytest
import torch

import gemm_ref as R


@pytest.mark.parametrize("M,N,K", [(33, 7, 13), (17, 40, 70), (1, 1, 1), (5, 4, 65)])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_reference_forward_and_input_gradient_against_torch(M, N, K, act):
    """Y = act(X W^T + b) is torch's; dX = (G W) * act'(H) with H = the saved activation is autograd's gradient of sum(G * act(Z))
    through the activation, for all three derivatives taken from the SAVED value."""
    X, Wt, b, _ = R.make_operands(M, N, K, "rounding", 1)
    fn = {0: lambda z: z, 1: lambda z: torch.nn.functional.leaky_relu(z, R.SLOPE), 2: torch.relu, 3: torch.tanh}[act]
    x = torch.from_numpy(X).double().requires_grad_(True)
    w, bb = torch.from_numpy(Wt.T.copy()).double(), torch.from_numpy(b).double()
    y = fn(x @ w.T + bb)
    r = R.gemm_ref(X, Wt, b, None, act, 0)
    assert np.allclose(r["out"], y.detach().numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(r["S"], (x.detach().abs() @ w.abs().T + bb.abs()).numpy(), rtol=1e-13)
    if act == 0:
        return
    # backward through a hidden layer: h = act(x), loss = sum(G * (h W2^T)) -> dx = (G W2) * act'(h)
    G, W2, _, _ = R.make_operands(M, K, N, "rounding", 2)          # G [M, N] as the A operand, W2 [N, K] as B
    h = fn(x)
    (h @ torch.from_numpy(W2).double().T * torch.from_numpy(G).double()).sum().backward()
    back = R.gemm_ref(G, W2, None, h.detach().numpy(), 0, act)
    assert np.allclose(back["out"], x.grad.numpy(), rtol=1e-12, atol=1e-13)


def test_reference_weight_and_bias_gradient_against_torch():
    M, N, K = 20, 34, 70      # dW [out = 20, in = 33] | db, reduced over a batch of 70
    Gt, X, _, _ = R.make_operands(M, N, K, "rounding", 3, ones_col=True)      # A(m, k) = G[k][m]
    x = torch.from_numpy(X).double()
    w = torch.zeros(M, N - 1, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(M, dtype=torch.float64, requires_grad=True)
    ((x @ w.T + bias) * torch.from_numpy(Gt.T.copy()).double()).sum().backward()
    r = R.gemm_ref(Gt, X, ones_col=True)
    assert np.allclose(r["C"], w.grad.numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(r["col"], bias.grad.numpy(), rtol=1e-13, atol=1e-13)


def test_derivative_at_the_zeros_and_exact_data():
    h = np.array([-1.0, -0.0, 0.0, 0.5, 2.0])
    assert R.act_deriv(h, R.MUL_DRELU).tolist() == [0, 0, 0, 1, 1]
    assert R.act_deriv(h, R.MUL_DLEAKY).tolist() == [R.SLOPE, R.SLOPE, R.SLOPE, 1, 1]
    assert R.act_deriv(h, R.MUL_DTANH).tolist() == [0, 1, 1, 0.75, -3]
    # exact data: the fp32 step-by-step result is the float64 reference rounded once, except where two roundings meet
    A, B, b, H = R.make_operands(33, 20, 70, "exact", 4)
    for act, mul in [(0, 0), (1, 0), (2, 2), (0, 1), (2, 1)]:
        r = R.gemm_ref(A, B, b, H, act, mul)
        assert np.array_equal(R.out_exact_f32(r["pre"], H, act, mul), r["out"].astype(np.float32))
    r = R.gemm_ref(A, B, b, H, 1, 1)
    assert np.allclose(R.out_exact_f32(r["pre"], H, 1, 1), r["out"], rtol=2 ** -23)
    assert np.array_equal(R.sequential_f32(A, B, b, H, 1, 1), R.out_exact_f32(r["pre"], H, 1, 1))


def test_batchnorm_partials_of_row_tiles():
    x = np.random.default_rng(5).standard_normal((100, 6))
    for tile in (16, 64):
        mean, m2 = R.bn_part_ref(x, tile)
        T = (100 + tile - 1) // tile
        assert mean.shape == m2.shape == (T, 6)
        xt = torch.from_numpy(x)
        for t in range(T):
            blk = xt[t * tile:(t + 1) * tile]
            assert np.allclose(mean[t], blk.mean(0).numpy(), rtol=1e-13, atol=1e-15)
            assert np.allclose(m2[t], (blk.var(0, unbiased=False) * blk.shape[0]).numpy(), rtol=1e-12)
        m32, q32 = R.bn_part_two_pass_f32(x, tile)
        assert np.allclose(m32, mean, atol=1e-6) and np.allclose(q32, m2, rtol=1e-5)


# (M, N, K, outer_ok) -> form: worked out by hand from the comments of shape_of
FORM_TABLE = [
    ((256, 256, 256, False), 1),      # 256 tiles of 16x16
    ((512, 512, 24, False), 1),       # exactly 1024
    ((528, 528, 24, False), 2),       # 1089 tiles of 16, 81 of 64: one 16x16 tile per wave
    ((528, 528, 16, False), 3),       # a single 16-k chunk
    ((528, 528, 17, False), 2),
    ((832, 832, 24, False), 2),       # 169 tiles of 64x64
    ((896, 896, 24, False), 4),       # 196
    ((896, 896, 16, False), 3),
    ((528, 528, 1024, False), 1),     # a long reduction into 81 tiles of 64x64
    ((528, 528, 1023, False), 2),
    ((896, 896, 1024, False), 4),     # 196 tiles: not "mid-sized"
    ((2048, 512, 512, False), 4),     # 256 tiles of 64x64
    ((2048, 256, 256, False), 2),     # TD3 at B = 2048: 128 tiles of 64x64
    ((512, 512, 1, True), 1),         # 2^18 elements but 1024 tiles
    ((1040, 256, 1, True), 5),
    ((1040, 256, 1, False), 3),
    ((1040, 252, 1, True), 3),        # below 2^18 elements
    ((10240, 512, 1, True), 5),
    ((1, 1, 1, False), 1),
]


@pytest.mark.parametrize("args,form", FORM_TABLE)
def test_form_rule_restated(args, form):
    assert R.shape_of(*args) == form


def test_outer_form_conditions():
    ok = dict(M=1040, N=256, K=1)
    assert R.outer_ok(**ok)
    for bad in (dict(K=2), dict(N=254), dict(ones_col=True), dict(sumsq=True), dict(bn_part=True), dict(ksplit=2), dict(b_cs=260),
                dict(c_rs=257), dict(b_addr=4), dict(c_addr=8), dict(bias_addr=4), dict(mul=1, h_rs=257), dict(mul=2, h_addr=4),
                dict(slot=True, c_slot=6), dict(slot=True, b_slot=1), dict(slot=True, h_slot=2)):
        assert not R.outer_ok(**{**ok, **bad}), bad
    assert R.outer_ok(**ok, ksplit=1, bias_addr=32, mul=1, h_rs=260, h_addr=16, slot=True, b_slot=4, c_slot=8, h_slot=12)


def test_tolerance_values():
    assert R.tol_k(1) == 4 * 2.0 ** -24 and R.tol_k(27) == 30 * 2.0 ** -24
    assert R.tol_k(30) == 33 * 2.0 ** -24 < 2e-6 < 34 * 2.0 ** -24      # the cap takes over at K = 31
    assert R.tol_k(31) == R.tol_k(512) == 2e-6
    assert R.derived_tol_k(512) == 515 * 2.0 ** -24


@pytest.mark.parametrize("M,N,K", R.ROUNDING_SHAPES)
def test_sequential_fp32_meets_the_bar_with_a_factor_two(M, N, K):
    """The bar is not one that only a lucky order meets: a plain fp32 accumulation in the WORST order the kernels use — one wave
    walking K alone — stays inside half of it at every rounding-data case (same operands as the GPU test draws), for every
    epilogue of the sweep."""
    for seed in (1, 2, 3, 4):
        A, B, b, H = R.make_operands(M, N, K, "rounding", seed)
        for act, mul in R.ROUNDING_EPILOGUES:
            r = R.gemm_ref(A, B, b, H if mul else None, act, mul)
            got = R.sequential_f32(A, B, b, H if mul else None, act, mul)
            ratio = float(R.error_ratio(got, r).max())
            assert ratio <= 0.5 * R.tol_k(K), (M, N, K, act, mul, ratio, R.tol_k(K))
            assert (np.abs(got - r["out"]) <= R.bar(r, K)).all()
        A, B, _, _ = R.make_operands(M, max(N, 2), K, "rounding", seed, ones_col=True)
        r = R.gemm_ref(A, B, ones_col=True)
        got = R.sequential_f32(A, np.concatenate([B, np.ones((K, 1), np.float32)], axis=1))
        assert float(R.error_ratio(got, r).max()) <= 0.5 * R.tol_k(K)
