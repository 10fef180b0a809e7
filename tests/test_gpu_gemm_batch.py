"""GPU tests (-m gpu) of the batched GEMM's whole problem record (csrc/gemm_mfma.hip launch_gemm_batch, through
gcrl_gemm_batch_f32) against tests/gemm_ref.py, the float64 definition.

Two kinds of data.  EXACT data (small integers; H from {-1, -0, +0, 0.5, 2}): every partial sum in any order is an exact fp32 number,
so the kernel must equal the reference BIT FOR BIT — these cases carry the structural checks.  ROUNDING data (seeded normals, the
weight scaled by K^-1/2) is held per element to  |got - ref| <= tol_K * S * |act'(H)| + 2^-24 |ref|,  tol_K = min(2e-6, (K+3) 2^-24)
(gemm_ref.bar; tests/test_gemm_ref.py shows on the CPU that a one-accumulator fp32 walk of K meets it with a factor 2 to spare).

Poison everywhere: every operand lies in an allocation larger than the problem (row strides beyond the extent, rows and words past
the end, other slots) whose other words hold a NaN pattern.  Outputs must keep the pattern bit for bit in every word the problem
does not own; a kernel that lets an input word it does not own reach a result shows NaN there.  Every pointer handed to the entry
is backed by an allocation that covers the problem's stated extent: no case provokes a fault."""
import json
import os

import numpy as np
import pytest
import torch

import gemm_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

POISON = 0x7FC0BEEF          # a quiet NaN with a recognisable payload
TAIL = 64                    # poisoned words behind every operand


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _poison(n):
    return np.full(n, POISON, np.uint32).view(np.float32)


def _ld(extent, odd=False):
    """A row stride beyond the extent: a multiple of 4 floats (the 16-byte paths stay eligible), or one that is not."""
    return (extent + 3) // 4 * 4 + (5 if odd else 4)


class Buf:
    """One operand in device memory: `rows` x `cols` logical words at base + r * ld + c of slot `slot` (of `nslots`, `slot_stride`
    words apart), `off` words past a 16-byte boundary; everything else poison."""

    def __init__(self, rows, cols, ld, off=0, nslots=1, slot=0, data=None):
        self.rows, self.cols, self.ld, self.off, self.slot = rows, cols, ld, off, slot
        self.slot_stride = ((rows + 1) * ld + TAIL + 3) // 4 * 4
        self.host = _poison(off + nslots * self.slot_stride + TAIL).copy()
        self.own = off + slot * self.slot_stride + (np.arange(rows)[:, None] * ld + np.arange(cols)[None, :])
        if data is not None:
            self.host[self.own] = np.asarray(data, np.float32).reshape(rows, cols)
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self, slotted=True):
        """Base of slot 0 (`slotted`: the entry adds slot * stride on the device) or of the data's own slot."""
        return self.dev.data_ptr() + 4 * (self.off + (0 if slotted else self.slot * self.slot_stride))

    def fetch(self):
        """The owned words [rows, cols]; asserts that every other word still holds the poison."""
        got = self.dev.cpu().numpy()
        other = np.ones(got.size, bool)
        other[self.own.ravel()] = False
        assert np.array_equal(_bits(got)[other], _bits(self.host)[other]), "a word the problem does not own was written"
        return got[self.own]

    def untouched(self):
        return np.array_equal(_bits(self.dev.cpu().numpy()), _bits(self.host))


class Prob:
    """One problem on one of the three operand layouts the engine builds (agent.hip):
       fwd     Y = act(X W^T + b)            A = X [M, ld] k-contiguous,  B(k, n) = W[n][k]
       bwd_dx  dX = (G W[:, col0:col0+N]) * act'(H)     A = G k-contiguous,  B(k, n) = W[k][col0 + n]
       bwd_dw  dW | db = G^T [X | 1]         A(m, k) = G[k][m],  B(k, n) = X[k][n]"""

    def __init__(self, M, N, K, layout="fwd", act=0, mul=0, bias=False, ones=False, data="exact", seed=0, off=(), odd=False, col0=0,
                 slot=None, indirect=True, ksplit=0, hint=0, bn_tile=0, sumsq=False):
        self.M, self.N, self.K, self.layout, self.act, self.mul, self.ones = M, N, K, layout, act, mul, ones
        self.ksplit, self.hint, self.bn_tile, self.indirect = ksplit, hint, bn_tile, indirect
        self.A, self.B, b, H = R.make_operands(M, N, K, data, seed, ones)
        self.bias = b if bias else None
        self.H = H if mul else None
        nm = N - 1 if ones else N
        off = {k: 1 for k in off} if not isinstance(off, dict) else off
        ns, sv = (4, slot) if slot is not None else (1, 0)
        o = lambda k: off.get(k, 0)
        if layout == "bwd_dw":
            self.a = Buf(K, M, _ld(M, odd), o("a"), ns, sv, self.A.T)
            self.a_rs, self.a_cs = 1, self.a.ld
        else:
            self.a = Buf(M, K, _ld(K, odd), o("a"), ns, sv, self.A)
            self.a_rs, self.a_cs = self.a.ld, 1
        if layout == "fwd":
            self.b = Buf(nm, K, _ld(K, odd), o("b"), ns, sv, self.B.T)
            self.b_rs, self.b_cs = 1, self.b.ld
        else:   # K rows of col0 + nm columns, the problem's window starting at column col0 (poison before it)
            ldb = _ld(col0 + nm, odd)
            self.b = Buf(K, nm, ldb, o("b") + col0, ns, sv, self.B)
            self.b_rs, self.b_cs = ldb, 1
        self.c = Buf(M, nm, _ld(nm, odd), o("c"), ns, sv)
        self.h = Buf(M, N, _ld(N, odd), o("h"), ns, sv, self.H) if mul else None
        self.bv = Buf(1, N, N, o("bias"), data=self.bias) if bias else None
        self.col = Buf(1, M, M) if ones else None
        self.tiles_m = (M + bn_tile - 1) // bn_tile if bn_tile else 0
        self.bn = Buf(2 * self.tiles_m, N, N) if bn_tile else None
        self.ss = torch.from_numpy(_poison(1).copy()).cuda() if sumsq else None
        self.slot_word = torch.tensor([sv], dtype=torch.int32).cuda() if (slot is not None and indirect) else None
        self.form = None

    def record(self, rec):
        s = self.indirect
        rec.a_dev, rec.a_rs, rec.a_cs = self.a.ptr(s), self.a_rs, self.a_cs
        rec.b_dev, rec.b_rs, rec.b_cs = self.b.ptr(s), self.b_rs, self.b_cs
        rec.c_dev, rec.c_rs = self.c.ptr(s), self.c.ld
        rec.bias_dev = self.bv.ptr() if self.bv else None
        rec.h_dev, rec.h_rs = (self.h.ptr(s), self.h.ld) if self.h else (None, 0)
        rec.col_out_dev = self.col.ptr() if self.col else None
        rec.M, rec.N, rec.K, rec.act, rec.mul, rec.ones_col = self.M, self.N, self.K, self.act, self.mul, int(self.ones)
        if self.slot_word is not None:
            rec.slot_dev = self.slot_word.data_ptr()
            rec.a_slot, rec.b_slot, rec.c_slot = self.a.slot_stride, self.b.slot_stride, self.c.slot_stride
            rec.h_slot = self.h.slot_stride if self.h else 0
        rec.shape_hint, rec.ksplit = self.hint, self.ksplit
        rec.bn_part_dev = self.bn.ptr() if self.bn else None
        rec.sumsq_dev = self.ss.data_ptr() if self.ss is not None else None
        rec.form_out = -1

    def outputs(self):
        """What the problem wrote (C, col, bn, ss), after checking the poison around each of them."""
        out = dict(C=self.c.fetch())
        if self.col:
            out["col"] = self.col.fetch()[0]
        if self.bn:
            out["bn"] = self.bn.fetch()
        if self.ss is not None:
            out["ss"] = self.ss.cpu().numpy().copy()
        return out

    def outputs_untouched(self):
        return all(b.untouched() for b in (self.c, self.col, self.bn) if b) and \
            (self.ss is None or int(_bits(self.ss.cpu().numpy())[0]) == POISON)

    def ref(self):
        return R.gemm_ref(self.A, self.B, self.bias, self.H, self.act, self.mul, self.ones)

    def exact(self):
        """The expected fp32 words on exact data: (C, col)."""
        r = self.ref()
        H = self.H if self.mul else None
        full = R.out_exact_f32(r["pre"], H, self.act, self.mul)
        return (full[:, :-1], full[:, -1]) if self.ones else (full, None)


def launch(gcrl, lib, probs, shape=0):
    recs = (gcrl._ffi.GemmProblem * max(len(probs), 1))()
    for p, r in zip(probs, recs):
        p.record(r)
    rc = lib.gcrl_gemm_batch_f32(recs, len(probs), shape, 1)
    torch.cuda.synchronize()
    for p, r in zip(probs, recs):
        p.form = r.form_out
    return rc


def run1(gcrl, lib, shape, *a, **kw):
    p = Prob(*a, **kw)
    assert launch(gcrl, lib, [p], shape) == 0, lib.gcrl_last_error()
    assert p.form == (shape or p.form)
    return p, p.outputs()


def same_bits(x, y):
    return np.array_equal(_bits(x), _bits(y))


def assert_exact(p, out):
    C_want, col_want = p.exact()
    bad = np.argwhere(_bits(out["C"]) != _bits(C_want))
    assert bad.size == 0, (p.layout, p.M, p.N, p.K, p.act, p.mul, "first differing (m, n):", bad[:4].tolist(),
                           out["C"][tuple(bad[0])], C_want[tuple(bad[0])])
    if p.ones:
        assert same_bits(out["col"], col_want), (p.layout, p.M, p.N, p.K, out["col"][:8], col_want[:8])


_worst = {}


def _record(form, K, ratio):
    key = f"form{form}/K={K}"
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))
    os.makedirs(os.path.join(ROOT, "test_records"), exist_ok=True)
    with open(os.path.join(ROOT, "test_records", "gemm_batch.json"), "w") as f:
        json.dump(dict(note="batched GEMM on rounding data: worst (|got - ref| - 2^-24 |ref|) / (S |act'(H)|) per tile form and K; "
                            "asserted bar: min(2e-6, (K + 3) 2^-24)", rows=dict(sorted(_worst.items()))), f, indent=1)


def assert_bar(p, out, form):
    r = p.ref()
    got = np.concatenate([out["C"], out["col"][:, None]], axis=1) if p.ones else out["C"]
    assert not np.isnan(got).any(), (p.layout, p.M, p.N, p.K, "a poisoned input word reached a result")
    ratio = float(R.error_ratio(got, r).max())
    _record(form, p.K, ratio)
    print(f"form {form} {p.layout} M={p.M} N={p.N} K={p.K} act={p.act} mul={p.mul}: worst ratio {ratio:.3e} (bar {R.tol_k(p.K):.3e})")
    assert ratio <= R.tol_k(p.K), (form, p.layout, p.M, p.N, p.K, p.act, p.mul, ratio, R.tol_k(p.K))


EXACT_EPILOGUES = [(0, 0), (1, 1), (2, 2), (1, 2), (2, 1), (0, 1), (0, 2)]


def _kw(layout, act, mul):
    """The sweep's problem on a layout: a bias wherever there is an activation (and on the plain forward), H at h_rs > N wherever
    there is a multiplier; the input gradient on a column window of W."""
    return dict(layout=layout, act=act, mul=mul, bias=(act != 0 or layout == "fwd"), col0=(4 if layout == "bwd_dx" else 0))


# ------------------------------------------------------------------ 1. forms x epilogues
@pytest.mark.parametrize("layout", ["fwd", "bwd_dx", "bwd_dw"])
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_forms_and_epilogues_exact(gcrl, lib, shape, layout):
    for M, N, K in R.SHAPES:
        for act, mul in EXACT_EPILOGUES:
            p, out = run1(gcrl, lib, shape, M, N, K, seed=shape, **_kw(layout, act, mul))
            assert_exact(p, out)


@pytest.mark.parametrize("layout", ["fwd", "bwd_dx", "bwd_dw"])
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_forms_and_epilogues_rounding(gcrl, lib, shape, layout):
    for M, N, K in R.SHAPES:
        for act, mul in R.ROUNDING_EPILOGUES:
            p, out = run1(gcrl, lib, shape, M, N, K, data="rounding", seed=shape, **_kw(layout, act, mul))
            assert_bar(p, out, shape)


@pytest.mark.parametrize("M,N", [(77, 36), (5, 4), (1, 8), (300, 300)])
def test_outer_form_equals_form_3(gcrl, lib, M, N):
    """Form 5 (K = 1) with every multiplier and with a bias: the bits of form 3, and the reference's on exact data."""
    for data in ("exact", "rounding"):
        for act, mul, bias in [(0, 0, False), (0, 1, False), (0, 2, True), (0, 3, False), (1, 1, True), (2, 0, True), (3, 3, True)]:
            kw = dict(layout="bwd_dx", act=act, mul=mul, bias=bias, data=data, seed=5)
            p5, o5 = run1(gcrl, lib, 5, M, N, 1, **kw)
            p3, o3 = run1(gcrl, lib, 3, M, N, 1, **kw)
            diff = np.argwhere(_bits(o5["C"]) != _bits(o3["C"]))
            assert diff.size == 0, (M, N, act, mul, bias, data, len(diff), [(hex(_bits(o5["C"])[tuple(i)]), hex(_bits(o3["C"])[tuple(i)])) for i in diff[:4]])
            if data == "exact" and act != 3 and mul != 3:
                assert_exact(p5, o5)
            else:
                assert_bar(p5, o5, 5)


def test_outer_form_refusals(gcrl, lib):
    M, N = 8, 8
    for why, kw, K in [("K != 1", {}, 2), ("N % 4", dict(), 1), ("ones_col", dict(ones=True), 1), ("sumsq", dict(sumsq=True), 1),
                       ("B misaligned", dict(off=("b",)), 1), ("C misaligned", dict(off=("c",)), 1), ("bias misaligned", dict(bias=True, off=("bias",)), 1),
                       ("H misaligned", dict(mul=1, off=("h",)), 1), ("c_rs % 4", dict(odd=True), 1), ("b_cs != 1", dict(layout="fwd"), 1),
                       ("split", dict(ksplit=2), 1)]:
        p = Prob(M, 7 if why == "N % 4" else N, K, **{**dict(layout="bwd_dx"), **kw})
        assert launch(gcrl, lib, [p], 5) != 0, why
        assert b"problem 0" in lib.gcrl_last_error(), (why, lib.gcrl_last_error())
        assert p.outputs_untouched(), why


# ------------------------------------------------------------------ 2. the bias gradient on every form
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_bias_gradient_on_every_form(gcrl, lib, shape):
    """ones_col: B(k, N-1) = 1 out of an out-of-range offset OR-ed with 1.0f (interior chunks), by a second rule in the K-tail chunk
    (forms 1-3) and from the A operand's row sums (form 4); column N-1 goes to col_out and is never written to C (Buf.fetch)."""
    for M, N, K in [(33, 17, 15), (33, 18, 16), (33, 33, 17), (20, 34, 70), (5, 2, 16), (5, 2, 70), (1, 17, 17), (1, 2, 15), (70, 65, 70), (64, 49, 16)]:
        for layout in ("bwd_dw", "bwd_dx"):
            p, out = run1(gcrl, lib, shape, M, N, K, layout=layout, ones=True, seed=7)
            assert_exact(p, out)
            p, out = run1(gcrl, lib, shape, M, N, K, layout=layout, ones=True, data="rounding", seed=7)
            assert_bar(p, out, shape)


# ------------------------------------------------------------------ 3. alignment
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_misaligned_bases_and_odd_strides(gcrl, lib, shape):
    """A base 4 bytes past a 16-byte boundary switches that operand's 16-byte path (a_vec, b_vec, epi_vec) to the element path at an
    otherwise aligned stride: the same bits as the aligned run.  Strides that are no multiple of 4 likewise."""
    for M, N, K in [(33, 20, 32), (17, 300, 70), (64, 64, 64), (5, 4, 65)]:
        for layout, act, mul in [("fwd", 1, 0), ("bwd_dx", 0, 1), ("bwd_dw", 0, 0), ("fwd", 2, 2)]:
            kw = dict(layout=layout, act=act, mul=mul, bias=True, seed=9)
            p0, o0 = run1(gcrl, lib, shape, M, N, K, **kw)
            assert_exact(p0, o0)
            for off in [("a",), ("b",), ("c",), ("bias",), ("h",), ("a", "b", "c", "bias", "h")]:
                if "h" in off and len(off) == 1 and not mul:
                    continue
                p, o = run1(gcrl, lib, shape, M, N, K, off=off, **kw)
                assert same_bits(o["C"], o0["C"]), (layout, M, N, K, off)
            p, o = run1(gcrl, lib, shape, M, N, K, odd=True, **kw)
            assert same_bits(o["C"], o0["C"]), (layout, M, N, K, "odd strides")
            p, o = run1(gcrl, lib, shape, M, N, K, odd=True, off=("a", "b", "c", "bias", "h"), **kw)
            assert same_bits(o["C"], o0["C"]), (layout, M, N, K, "odd strides, misaligned")


# ------------------------------------------------------------------ 4. company
def _company(data, hints=None):
    """12 heterogeneous problems: 1, 2, 3, 5 and more tiles of every form's size, one with ones_col, some with a multiplier, one
    behind a slot."""
    spec = [
        dict(M=16, N=16, K=40, layout="fwd", act=1, bias=True),                       # 1 tile of 16x16
        dict(M=16, N=32, K=33, layout="bwd_dx", mul=1, col0=2),                       # 2
        dict(M=48, N=16, K=16, layout="bwd_dw"),                                      # 3
        dict(M=80, N=10, K=70, layout="fwd", act=2, bias=True),                       # 5
        dict(M=48, N=33, K=200, layout="bwd_dw", ones=True),                          # 9, the bias gradient
        dict(M=33, N=7, K=13, layout="bwd_dx", mul=2, slot=3),                        # 3, behind a slot
        dict(M=130, N=40, K=512, layout="fwd", act=1, bias=True),                     # 27 (2 tiles of 64x64 in a column: 3)
        dict(M=1, N=1, K=1, layout="fwd", bias=True),
        dict(M=70, N=65, K=64, layout="bwd_dw", ones=True),
        dict(M=17, N=300, K=70, layout="bwd_dx", mul=1, act=1, bias=True),
        dict(M=64, N=64, K=27, layout="fwd", act=2, mul=2, bias=True),
        dict(M=5, N=4, K=65, layout="bwd_dx"),
    ]
    out = []
    for i, s in enumerate(spec):
        s = dict(s)
        M, N, K = s.pop("M"), s.pop("N"), s.pop("K")
        out.append(Prob(M, N, K, data=data, seed=100 + i, hint=(hints[i] if hints else 0), **s))
    return out


def _equal_outputs(a, b):
    return all(same_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("data", ["exact", "rounding"])
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_company_does_not_change_a_problem(gcrl, lib, shape, data):
    """The launcher's invariant: a problem's outputs are a function of the problem alone, never of a launch's composition — the
    bits of a batch of 12 are the bits of each problem alone, in either order."""
    alone = []
    for p in _company(data):
        assert launch(gcrl, lib, [p], shape) == 0, lib.gcrl_last_error()
        alone.append(p.outputs())
        if data == "exact":
            assert_exact(p, alone[-1])
        else:
            assert_bar(p, alone[-1], shape)      # (the long reductions of every form: K = 200 and 512)
    for order in (list(range(12)), list(range(11, -1, -1))):
        batch = _company(data)
        assert launch(gcrl, lib, [batch[i] for i in order], shape) == 0, lib.gcrl_last_error()
        for i in range(12):
            assert batch[i].form == shape
            assert _equal_outputs(batch[i].outputs(), alone[i]), (shape, data, "problem", i, "order", order[:2])


def test_company_of_mixed_forms_in_one_call(gcrl, lib):
    """shape = 0 with mixed shape_hints: one call, one launch per form present; every problem reports its form and keeps its bits."""
    hints = [1, 2, 3, 4, 4, 1, 2, 3, 4, 2, 3, 0]
    batch, singles = _company("rounding", hints), _company("rounding")
    assert launch(gcrl, lib, batch, 0) == 0, lib.gcrl_last_error()
    for i, p in enumerate(batch):
        want = hints[i] or R.shape_of(p.M, p.N, p.K)
        assert p.form == want, (i, p.form, want)
        q = singles[i]
        assert launch(gcrl, lib, [q], want) == 0
        assert _equal_outputs(p.outputs(), q.outputs()), i


def test_problem_count_limits(gcrl, lib):
    probs = [Prob(5, 4, 3, seed=i) for i in range(13)]
    for n in (13, 0):
        assert launch(gcrl, lib, probs[:n], 1) != 0
        assert (b"%d problems" % n) in lib.gcrl_last_error(), lib.gcrl_last_error()
    assert all(p.outputs_untouched() for p in probs)
    assert launch(gcrl, lib, probs[:12], 1) == 0
    for p in probs[:12]:
        assert_exact(p, p.outputs())


# ------------------------------------------------------------------ 5. slots
@pytest.mark.parametrize("shape", [1, 2, 3, 4, 5])
def test_slot_indirection(gcrl, lib, shape):
    """base + (*slot) * stride on A, B, C and H: the bits of the un-indirected call on the offset pointers; the other slots of C
    keep their poison (Buf.fetch), the other slots of the inputs hold NaN."""
    M, N, K = (40, 36, 1) if shape == 5 else (40, 36, 50)
    for layout, act, mul in [("bwd_dx", 0, 1), ("bwd_dx", 1, 2), ("fwd", 1, 0)] if shape != 5 else [("bwd_dx", 0, 1), ("bwd_dx", 1, 2)]:
        kw = dict(layout=layout, act=act, mul=mul, bias=(act != 0), seed=11)
        for s in (0, 1, 3):
            p, o = run1(gcrl, lib, shape, M, N, K, slot=s, **kw)
            assert_exact(p, o)
            q, oq = run1(gcrl, lib, shape, M, N, K, slot=s, indirect=False, **kw)
            assert same_bits(o["C"], oq["C"]), (shape, layout, s)


# ------------------------------------------------------------------ 6. the sum of squares
@pytest.mark.parametrize("ones", [False, True])
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_sum_of_squares_partials(gcrl, lib, shape, ones):
    for M, N, K in [(33, 18, 13), (70, 65, 70), (16, 16, 16), (1, 2, 5), (130, 40, 64)]:
        for data in ("exact", "rounding"):
            p = Prob(M, N, K, layout="bwd_dw", ones=ones, data=data, seed=13, sumsq=True)
            assert launch(gcrl, lib, [p], shape) == 0, lib.gcrl_last_error()
            o = p.outputs()
            if data == "exact":
                assert_exact(p, o)
            want = float((o["C"].astype(np.float64) ** 2).sum() + ((o["col"].astype(np.float64) ** 2).sum() if ones else 0.0))
            got = float(o["ss"][0])
            assert abs(got - want) <= 1e-5 * want, (shape, M, N, K, data, got, want)
            assert launch(gcrl, lib, [p], shape) == 0          # again into the same record: the same bits
            assert same_bits(p.outputs()["ss"], o["ss"])


# ------------------------------------------------------------------ 7. BatchNorm partials
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("B", [16, 64, 100, 129])
@pytest.mark.parametrize("shape", [1, 4])
def test_batchnorm_partials(gcrl, lib, shape, B, N, bias):
    """Per-row-tile (mean, M2) of the result out of the epilogue: 16-row tiles on form 1, 64-row tiles on the unsplit form 4.  Full
    tiles on exact data are bitwise: the row count T is a power of two, so the mean and every deviation are exact multiples of 1/T,
    and wherever T^2 * M2 < 2^24 every square and every partial sum of them, in any order, is an exact fp32 number too (the
    reduction is short here — K = 24 on form 1, K = 2 on form 4 — to keep the results that small).  Everything else is held against
    float64 at three times the error of a float32 numpy two-pass on the same tile, or 1e-5 of the scale."""
    tile = 16 if shape == 1 else 64
    bitwise_tiles = 0
    for data in ("exact", "rounding"):
        K = 24 if (shape == 1 or data == "rounding") else 2
        p = Prob(B, N, K, layout="fwd", bias=bias, data=data, seed=17, bn_tile=tile)
        assert launch(gcrl, lib, [p], shape) == 0, lib.gcrl_last_error()
        o = p.outputs()
        if data == "exact":
            assert_exact(p, o)
        else:
            assert_bar(p, o, shape)
        T = p.tiles_m
        ref_mean, ref_m2 = R.bn_part_ref(o["C"], tile)
        f32_mean, f32_m2 = R.bn_part_two_pass_f32(o["C"], tile)
        for t in range(T):
            rows = min(tile, B - t * tile)
            exact = (tile * tile * ref_m2[t] < 2 ** 24) if (data == "exact" and rows == tile) else np.zeros(N, bool)
            if exact.any():
                bitwise_tiles += 1
                assert same_bits(o["bn"][t][exact], ref_mean[t].astype(np.float32)[exact]), (shape, B, N, t)
                assert same_bits(o["bn"][T + t][exact], ref_m2[t].astype(np.float32)[exact]), (shape, B, N, t)
            if exact.all():
                continue
            for name, got, r32, r64 in (("mean", o["bn"][t], f32_mean[t], ref_mean[t]), ("m2", o["bn"][T + t], f32_m2[t], ref_m2[t])):
                got, r32, r64 = got.astype(np.float64)[~exact], r32.astype(np.float64)[~exact], r64[~exact]
                scale = float(np.abs(r64).max()) + 1e-30
                e_got, e_ref = float(np.abs(got - r64).max()) / scale, float(np.abs(r32 - r64).max()) / scale
                assert e_got <= max(3.0 * e_ref, 1e-5), (name, shape, B, N, t, e_got, e_ref)
    assert bitwise_tiles >= B // tile, "the exact-data full tiles were meant to be compared bit for bit"


def test_batchnorm_partials_refusals(gcrl, lib):
    for why, shape, kw in [("ones_col", 1, dict(ones=True, layout="bwd_dw")), ("form 2", 2, {}), ("form 3", 3, {}),
                           ("form 4, C misaligned", 4, dict(off=("c",))), ("form 4, N % 4", 4, dict(N=18)),
                           ("form 4, bias misaligned", 4, dict(bias=True, off=("bias",))), ("form 4, c_rs % 4", 4, dict(odd=True)),
                           ("form 4 with a multiplier", 4, dict(mul=1)), ("form 4 with a split", 4, dict(ksplit=2))]:
        kw = dict(kw)
        N = kw.pop("N", 16)
        p = Prob(20, N, 24, bn_tile=(64 if shape == 4 else 16), **kw)
        assert launch(gcrl, lib, [p], shape) != 0, why
        assert b"problem 0" in lib.gcrl_last_error() and b"bn_part" in lib.gcrl_last_error(), (why, lib.gcrl_last_error())
        assert p.outputs_untouched(), why


# ------------------------------------------------------------------ 8. the split reduction with an epilogue
@pytest.mark.parametrize("K", [64, 300])
@pytest.mark.parametrize("S", [2, 3, 4])
def test_split_reduction_with_an_epilogue(gcrl, lib, S, K):
    """Form 4 with the reduction split over S workgroups per tile and bias + LeakyReLU + the LeakyReLU derivative in the last
    arriver's epilogue; launched twice inside the entry (the tickets reset themselves; the outputs are poisoned in between)."""
    for M, N, layout in [(70, 65, "bwd_dw"), (33, 20, "fwd"), (130, 40, "bwd_dx")]:
        kw = dict(layout=layout, act=1, mul=1, bias=True, seed=19)
        p1, o1 = run1(gcrl, lib, 4, M, N, K, **kw)
        pS, oS = run1(gcrl, lib, 4, M, N, K, ksplit=S, **kw)
        assert_exact(pS, oS)
        assert same_bits(oS["C"], o1["C"])
        pS, oS = run1(gcrl, lib, 4, M, N, K, ksplit=S, data="rounding", **kw)
        assert_bar(pS, oS, 4)
    p, o = run1(gcrl, lib, 4, 70, 65, K, layout="bwd_dw", ones=True, ksplit=S, seed=19, sumsq=True)
    assert_exact(p, o)


def test_split_reduction_with_more_splits_than_k_steps(gcrl, lib):
    for K, S in [(16, 4), (40, 8), (64, 64)]:
        p, o = run1(gcrl, lib, 4, 70, 65, K, layout="fwd", act=1, mul=1, bias=True, ksplit=S, seed=23)
        assert_exact(p, o)
        p, o = run1(gcrl, lib, 4, 70, 33, K, layout="bwd_dw", ones=True, ksplit=S, seed=23)
        assert_exact(p, o)


# ------------------------------------------------------------------ 9. the form rule
FORM_RULE = [   # (M, N, K, layout, extra): both sides of every threshold of shape_of
    (512, 512, 24, "fwd", {}),          # 1024 tiles of 16x16
    (528, 528, 24, "fwd", {}),          # 1089; 81 tiles of 64x64, K > 16 -> one 16x16 tile per wave
    (528, 528, 16, "fwd", {}),          # K = 16: a single chunk -> 32x32 per wave
    (528, 528, 17, "fwd", {}),
    (832, 832, 24, "fwd", {}),          # 169 tiles of 64x64
    (896, 896, 24, "fwd", {}),          # 196 -> LDS-tiled
    (896, 896, 16, "fwd", {}),          # ... but not for a single chunk
    (528, 528, 1024, "fwd", {}),        # K >= 1024 into 81 tiles of 64x64 -> back to the k-split form
    (512, 512, 1, "bwd_dx", {}),        # M N = 2^18 but <= 1024 tiles of 16: never form 5
    (1024, 256, 1, "bwd_dx", {}),       # M N = 2^18, 1024 tiles
    (1040, 256, 1, "bwd_dx", {}),       # the outer product, streaming
    (1040, 256, 1, "bwd_dx", dict(off=("c",))),      # misaligned: not an outer-form problem
    (1040, 256, 1, "bwd_dx", dict(sumsq=True)),
    (1040, 252, 1, "bwd_dx", {}),       # M N < 2^18
    (1040, 256, 2, "bwd_dx", {}),       # K != 1
]


@pytest.mark.parametrize("M,N,K,layout,extra", FORM_RULE)
def test_form_rule(gcrl, lib, M, N, K, layout, extra):
    """shape = 0: the reported form is the Python restatement's and the output is bitwise the explicit form's."""
    kw = dict(layout=layout, seed=29, **extra)
    p, o = run1(gcrl, lib, 0, M, N, K, **kw)
    outer = R.outer_ok(M, N, K, sumsq=bool(extra.get("sumsq")), b_cs=p.b_cs, c_rs=p.c.ld, c_addr=p.c.ptr(), b_addr=p.b.ptr())
    want = R.shape_of(M, N, K, outer)
    assert p.form == want, (M, N, K, p.form, want)
    assert_exact(p, o)
    q, oq = run1(gcrl, lib, want, M, N, K, **kw)
    assert same_bits(o["C"], oq["C"])


# ------------------------------------------------------------------ 10. refusals
def test_refusals_leave_the_outputs_alone(gcrl, lib):
    """Every argument check of launch_gemm_batch the entry can reach, and the entry's own, on real device allocations: a nonzero
    status, a message that names the problem, every output still poisoned (the good neighbour's too)."""
    def broken(edit, **kw):
        good, bad = Prob(20, 12, 9, seed=31, sumsq=True), Prob(20, 12, 9, seed=32, **kw)
        recs = (gcrl._ffi.GemmProblem * 2)()
        good.record(recs[0]); bad.record(recs[1])
        edit(recs[1])
        rc = lib.gcrl_gemm_batch_f32(recs, 2, 1, 1)
        torch.cuda.synchronize()
        assert rc != 0 and b"problem 1" in lib.gcrl_last_error(), lib.gcrl_last_error()
        assert good.outputs_untouched() and bad.outputs_untouched()

    for field in ("M", "N", "K"):
        broken(lambda r, f=field: setattr(r, f, 0))
    for field in ("a_dev", "b_dev", "c_dev"):
        broken(lambda r, f=field: setattr(r, f, None))
    broken(lambda r: setattr(r, "col_out_dev", None), ones=True, layout="bwd_dw")
    broken(lambda r: setattr(r, "N", 1), ones=True, layout="bwd_dw")
    broken(lambda r: setattr(r, "act", 4))
    broken(lambda r: setattr(r, "mul", 7), mul=1)
    broken(lambda r: setattr(r, "h_dev", None), mul=1)
    broken(lambda r: setattr(r, "shape_hint", 6))
    broken(lambda r: setattr(r, "ksplit", -1))
    p = Prob(20, 12, 9, seed=33)
    assert launch(gcrl, lib, [p], 6) != 0 and p.outputs_untouched()
