"""The batched GEMM's definition in plain numpy float64 (no torch, no project import): what one problem record of
gcrl_gemm_batch_f32 (include/gcrl.h) computes, the size of what it sums, the accuracy bar its kernels are held to, the BatchNorm
partials of its row tiles, and the launcher's form rule restated from the comments of shape_of (csrc/gemm_mfma.hip).

A problem here is its LOGICAL operands: A [M, K], B [K, N] (with ones_col: [K, N-1], the ones column is implied), bias [N] or None,
H [M, N] or None.  How they lie in memory (strides, slots, alignment) is the test's business, not the definition's."""
import numpy as np

ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_TANH = 0, 1, 2, 3
MUL_NONE, MUL_DLEAKY, MUL_DRELU, MUL_DTANH = 0, 1, 2, 3
SLOPE = float(np.float32(0.01))      # nn.LeakyReLU()'s default slope as the kernels hold it: the fp32 number nearest 0.01
EPS32 = 2.0 ** -24                   # unit roundoff of fp32


def act_apply(v, act):
    v = np.asarray(v, np.float64)
    if act == ACT_LEAKY:
        return np.where(v > 0, v, SLOPE * v)
    if act == ACT_RELU:
        return np.where(v > 0, v, 0.0)
    if act == ACT_TANH:
        return np.tanh(v)
    return v.copy()


def act_deriv(h, mul):
    """act'(.) from the SAVED post-activation value h: h > 0 decides (so both zeros take the non-positive branch)."""
    h = np.asarray(h, np.float64)
    if mul == MUL_DLEAKY:
        return np.where(h > 0, 1.0, SLOPE)
    if mul == MUL_DRELU:
        return np.where(h > 0, 1.0, 0.0)
    if mul == MUL_DTANH:
        return 1.0 - h * h
    return np.ones_like(h)


def gemm_ref(A, B, bias=None, H=None, act=ACT_NONE, mul=MUL_NONE, ones_col=False):
    """-> dict: pre [M,N] = A.B (+ bias), out = act(pre) * act'(H), S = |A|.|B| + |bias| (the size of what was summed),
    dact = |act'(H)|.  With ones_col, B gains a last column of ones; `col` is column N-1 of out (what goes to col_out) and
    `C` the other columns (what goes to C); without it C is out."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if ones_col:
        B = np.concatenate([B, np.ones((B.shape[0], 1))], axis=1)
    pre = A @ B + 0.0                                  # (+ 0.0: a sum of zeros is +0, as an accumulator that starts at +0 gives)
    S = np.abs(A) @ np.abs(B)
    if bias is not None:
        bias = np.asarray(bias, np.float64)
        pre = pre + bias[None, :]
        S = S + np.abs(bias)[None, :]
    d = act_deriv(H, mul) if mul != MUL_NONE else np.ones_like(pre)
    out = act_apply(pre, act) * d
    r = dict(pre=pre, out=out, S=S, dact=np.abs(d))
    if ones_col:
        r["C"], r["col"] = out[:, :-1], out[:, -1]
    else:
        r["C"] = out
    return r


def out_exact_f32(pre, H, act, mul):
    """The result on EXACT data (pre holds integers, exactly representable): every step rounded to fp32 as the kernels round it —
    the one product by 0.01f, then the product by the derivative.  For act in {none, ReLU, LeakyReLU}, mul in {none, DRELU, DLEAKY}."""
    assert act != ACT_TANH and mul != MUL_DTANH
    v = np.asarray(pre, np.float64).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), pre), "not exact data"
    s = np.float32(0.01)
    if act == ACT_LEAKY:
        v = np.where(v > 0, v, s * v).astype(np.float32)
    elif act == ACT_RELU:
        v = np.where(v > 0, v, np.float32(0.0)).astype(np.float32)
    if mul != MUL_NONE:
        h = np.asarray(H, np.float32)
        d = np.where(h > 0, np.float32(1.0), s if mul == MUL_DLEAKY else np.float32(0.0)).astype(np.float32)
        v = (v * d).astype(np.float32)
    return v


def tol_k(K):
    """Relative to S: (K + 3) roundings of an fp32 evaluation in any order — K additions (the products inside an fma chain are
    exact), the bias, the 0.01 product, the derivative product — capped by the project's own 2e-6."""
    return min(2e-6, (K + 3) * EPS32)


def derived_tol_k(K):
    return (K + 3) * EPS32


def bar(ref, K, tol=None):
    """Per-element allowance |got - out| <= tol_K * S * |act'(H)| + 2^-24 * |out| (the last term: the tanh path's single final
    rounding from double)."""
    t = tol_k(K) if tol is None else tol
    return t * ref["S"] * ref["dact"] + EPS32 * np.abs(ref["out"])


def error_ratio(got, ref):
    """|got - out| less the final-rounding allowance, over S * |act'(H)|: the figure held against tol_K (0 where nothing was summed)."""
    err = np.maximum(np.abs(np.asarray(got, np.float64) - ref["out"]) - EPS32 * np.abs(ref["out"]), 0.0)
    den = ref["S"] * ref["dact"]
    return np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))


def sequential_f32(A, B, bias=None, H=None, act=ACT_NONE, mul=MUL_NONE):
    """A plain fp32 evaluation in the worst order the kernels use — one accumulator walking K alone, each product exact and
    each addition rounded (an fma chain) — then bias, activation and derivative, each rounded to fp32."""
    A64, B64 = np.asarray(A, np.float32).astype(np.float64), np.asarray(B, np.float32).astype(np.float64)
    acc = np.zeros((A64.shape[0], B64.shape[1]), np.float32)
    for k in range(A64.shape[1]):
        acc = (acc.astype(np.float64) + A64[:, k:k + 1] * B64[k:k + 1, :]).astype(np.float32)   # (24 x 24 bits: exact in fp64)
    if bias is not None:
        acc = (acc + np.asarray(bias, np.float32)[None, :]).astype(np.float32)
    s = np.float32(0.01)
    if act == ACT_LEAKY:
        acc = np.where(acc > 0, acc, s * acc).astype(np.float32)
    elif act == ACT_RELU:
        acc = np.where(acc > 0, acc, np.float32(0)).astype(np.float32)
    elif act == ACT_TANH:
        acc = np.tanh(acc.astype(np.float64)).astype(np.float32)
    if mul != MUL_NONE:
        h = np.asarray(H, np.float32)
        if mul == MUL_DTANH:
            d = (np.float32(1.0) - (h * h).astype(np.float32)).astype(np.float32)
        else:
            d = np.where(h > 0, np.float32(1.0), s if mul == MUL_DLEAKY else np.float32(0.0)).astype(np.float32)
        acc = (acc * d).astype(np.float32)
    return acc


def bn_part_ref(x, tile):
    """Per-row-tile, per-column (mean, M2 = sum of squared deviations from the tile's own mean) of x [M, N]; tiles of `tile` rows
    (16 on form 1, 64 on form 4), the last one partial.  -> (mean [T, N], m2 [T, N]) as they lie in bn_part: mean rows first."""
    x = np.asarray(x, np.float64)
    T = (x.shape[0] + tile - 1) // tile
    mean, m2 = np.empty((T, x.shape[1])), np.empty((T, x.shape[1]))
    for t in range(T):
        blk = x[t * tile:(t + 1) * tile]
        mean[t] = blk.mean(0)
        m2[t] = ((blk - mean[t]) ** 2).sum(0)
    return mean, m2


def bn_part_two_pass_f32(x, tile):
    """The same by a plain fp32 two-pass: the yardstick a partial tile's error is measured with."""
    x = np.asarray(x, np.float32)
    T = (x.shape[0] + tile - 1) // tile
    mean, m2 = np.empty((T, x.shape[1]), np.float32), np.empty((T, x.shape[1]), np.float32)
    for t in range(T):
        blk = x[t * tile:(t + 1) * tile]
        mean[t] = blk.sum(0, dtype=np.float32) / np.float32(blk.shape[0])
        m2[t] = ((blk - mean[t]) ** 2).sum(0, dtype=np.float32)
    return mean, m2


def _al16(addr):
    return addr % 16 == 0


def outer_ok(M, N, K, *, ones_col=False, sumsq=False, bn_part=False, ksplit=0, b_cs=1, c_rs=None, b_addr=0, c_addr=0, bias_addr=None,
             mul=MUL_NONE, h_rs=None, h_addr=0, slot=False, b_slot=0, c_slot=0, h_slot=0):
    """Form 5's conditions: K = 1, no ones column / sum of squares / BatchNorm partials / split, whole aligned 16-byte quads of B,
    C, bias and (with a multiplier) H, slot strides that keep them aligned.  Addresses in bytes."""
    c_rs = N if c_rs is None else c_rs
    h_rs = N if h_rs is None else h_rs
    return bool(K == 1 and not ones_col and not sumsq and not bn_part and ksplit <= 1 and N % 4 == 0 and b_cs == 1 and c_rs % 4 == 0
                and _al16(b_addr) and _al16(c_addr) and (bias_addr is None or _al16(bias_addr))
                and (mul == MUL_NONE or (h_rs % 4 == 0 and _al16(h_addr)))
                and (not slot or (b_slot % 4 == 0 and c_slot % 4 == 0 and h_slot % 4 == 0)))


def shape_of(M, N, K, outer=False):
    """The launcher's form rule (`outer`: outer_ok of the problem):
       <= 1024 tiles of 16x16                                   -> 1 (one tile per workgroup, K split over its 4 waves)
       K >= 1024 into fewer than 192 tiles of 64x64             -> 1 (a long reduction into a mid-sized output)
       an aligned K = 1 outer product of >= 2^18 elements       -> 5 (streaming)
       K <= 16 (a single 16-k chunk)                            -> 3 (32x32 per wave)
       >= 192 tiles of 64x64, or K >= 1024                      -> 4 (LDS-tiled), else 2 (16x16 per wave)"""
    tiles16 = ((M + 15) // 16) * ((N + 15) // 16)
    tiles64 = ((M + 63) // 64) * ((N + 63) // 64)
    if tiles16 <= 1024:
        return 1
    if K >= 1024 and tiles64 < 192:
        return 1
    if outer and M * N >= (1 << 18):
        return 5
    if K <= 16:
        return 3
    return 4 if (tiles64 >= 192 or K >= 1024) else 2


# ---- the data both test files draw (tests/test_gemm_ref.py on the CPU, tests/test_gpu_gemm_batch.py on the GPU) ----------------
H_EXACT = np.array([-1.0, -0.0, 0.0, 0.5, 2.0], np.float32)
SHAPES = [(33, 7, 13), (17, 300, 70), (64, 64, 27), (1, 1, 1), (16, 16, 16), (16, 16, 17), (16, 16, 15), (5, 4, 65)]
# (act, mul) pairs of the rounding-data sweep: every activation with a bias, every multiplier, tanh on both sides
ROUNDING_EPILOGUES = [(0, 0), (1, 1), (2, 2), (3, 3), (3, 0), (0, 3), (1, 2)]
# every (M, N, K) at which a rounding-data case runs: the sweep's shapes, the split cases, the company batch's long reductions
ROUNDING_SHAPES = SHAPES + [(70, 65, 64), (70, 65, 300), (33, 20, 300), (130, 40, 300), (130, 40, 512), (48, 33, 200), (16, 16, 40), (16, 32, 33),
                            (48, 16, 16), (80, 10, 70), (129, 48, 24), (300, 300, 1), (20, 34, 70), (33, 18, 16), (70, 65, 70)]


def make_operands(M, N, K, data, seed, ones_col=False):
    """Logical operands of one problem.  data = "exact": integers in [-3, 3] (bias in [-2, 2], H from H_EXACT) — every partial sum in
    any order is an exact fp32 number; "rounding": seeded normals, the weight scaled by K^-1/2, H = tanh of a normal on a grid of 2^-8."""
    g = np.random.default_rng([seed, M, N, K, 1 if data == "exact" else 2])
    nm = N - 1 if ones_col else N
    if data == "exact":
        A = g.integers(-3, 4, (M, K)).astype(np.float32)
        B = g.integers(-3, 4, (K, nm)).astype(np.float32)
        bias = g.integers(-2, 3, N).astype(np.float32)
        H = H_EXACT[g.integers(0, len(H_EXACT), (M, N))]
    else:
        A = g.standard_normal((M, K)).astype(np.float32)
        B = (g.standard_normal((K, nm)) / np.sqrt(K)).astype(np.float32)
        bias = g.standard_normal(N).astype(np.float32)
        # (multiples of 2^-8 inside [-1, 1]: h^2 and 1 - h^2 are exact in fp32, so the bar's ONE rounding for the derivative product
        # is all a tanh derivative costs; an arbitrary h near 1 would add the rounding of 1 - h^2 itself, which |act'(H)| does not scale)
        H = (np.round(np.tanh(g.standard_normal((M, N))) * 256) / 256).astype(np.float32)
    return A, B, bias, H
