"""Host tests (no GPU) of tests/her_td_ref.py, the numpy definition of TD-error prioritised replay on a sample-mode HER ring
(HERBuffer(relabel="sample", prioritise="td_error"); csrc/her_td.hip): the restated seed and update on hand-made trees of one, two
and three levels, the p_max rule, the frequencies the descent gives on leaves of the kind the mode produces — the condition the GPU
draw inherits by being bitwise this code — the weights, the boundary, and that the two new kernels use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import her_td_ref as T
import per_tree_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CAPS = (60, 150, 4160)          # one, two and three levels


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F32)).view(np.uint32)


def _filled(cap, seed=0, wrapped=False):
    """a hand-made ring: filled by flushes of 50 and 3 rows; `wrapped`: past its end, head != 0"""
    ring = T.RefHerTd(cap, alpha=0.6, eps=1e-6, seed=seed)
    rows = cap + 57 if wrapped else cap - 7
    while rows > 0:
        n = 50 if rows >= 50 else min(rows, 3)
        ring.flush(n)
        rows -= n
    return ring


def _rebuilt(ring):
    """every level from the leaves alone: what the incremental recomputation must equal"""
    return R.build(ring.levels[0])


def _same_levels(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize("cap", CAPS)
def test_seed_and_update_keep_the_tree_a_function_of_its_leaves(cap):
    ring = _filled(cap, wrapped=cap == 4160)
    assert len(ring.levels) == {60: 1, 150: 2, 4160: 3}[cap]
    if cap == 4160:
        assert ring.head != 0 and ring.len == cap
    R.check_invariant(ring.levels)
    filled = np.zeros(ring.levels[0].size, bool)
    filled[(ring.head + np.arange(ring.len)) % cap] = True
    assert np.all(ring.levels[0][filled] == T.P_MAX_INIT) and not ring.levels[0][~filled].any()
    gen = np.random.default_rng(cap)
    for B in (1, 64, 300):
        idx = gen.integers(0, ring.len, B)
        td = (gen.standard_normal(B) * 20).astype(F32)
        before = ring.levels[0].copy()
        ring.update(idx, td)
        _same_levels(ring.levels, _rebuilt(ring))
        keep = R.last_occurrence(idx)
        slots = (ring.head + idx) % cap
        want = R.priority64(td[keep], 1e-6, 0.6)
        assert np.max(np.abs(ring.levels[0][slots[keep]].astype(np.float64) - want) / want) <= 1e-6
        untouched = np.ones(before.size, bool)
        untouched[slots] = False
        assert np.array_equal(bits(ring.levels[0][untouched]), bits(before[untouched]))
    # the next flush seeds the raised p_max, over the ring's end on the wrapped tree
    assert ring.p_max > 1.0
    segs = ring.flush(50)
    for a, b in segs:
        assert np.all(bits(ring.levels[0][a:b]) == bits(ring.p_max))
    _same_levels(ring.levels, _rebuilt(ring))


def test_last_occurrence_wins_and_alpha_one_is_the_single_add():
    ring = T.RefHerTd(150, alpha=1.0, eps=1e-6)
    ring.flush(50); ring.flush(50)
    idx = np.array([5, 40, 5, 95, 0, 40, 5, 17])
    td = np.array([0.5, -2.0, 0.25, 1e-3, -0.0, 3.0, -0.125, 7.5], F32)
    ring.update(idx, td)
    lv = ring.levels[0]
    assert bits(lv[5]) == bits(F32(0.125) + F32(1e-6)) and bits(lv[40]) == bits(F32(3.0) + F32(1e-6))
    assert bits(lv[0]) == bits(F32(1e-6)) and bits(lv[17]) == bits(F32(7.5) + F32(1e-6))       # -0.0: |td| = +0
    assert bits(ring.p_max) == bits(F32(7.5) + F32(1e-6))
    # an overwritten occurrence still counts towards p_max: it is a priority the batch has seen
    ring.update(np.array([9, 9]), np.array([30.0, 0.5], F32))
    assert bits(ring.levels[0][9]) == bits(F32(0.5) + F32(1e-6)) and bits(ring.p_max) == bits(F32(30.0) + F32(1e-6))
    # an index >= cap is skipped: no leaf, no share in p_max, nothing out of place
    before = [x.copy() for x in ring.levels]
    ring.update(np.array([150, 2 ** 32 - 1, 4000]), np.array([1e9, 1e9, 1e9], F32))
    _same_levels(ring.levels, before)
    assert bits(ring.p_max) == bits(F32(30.0) + F32(1e-6))


@pytest.mark.parametrize("alpha", [1.0, 0.6])
def test_p_max_is_monotone_and_nan_or_inf_never_raise_it(alpha):
    ring = T.RefHerTd(150, alpha=alpha, eps=1e-6)
    ring.flush(50); ring.flush(50); ring.flush(3)
    gen = np.random.default_rng(7)
    seen = [ring.p_max]
    for step in range(12):
        B = (1, 64, 300)[step % 3]
        td = (gen.standard_normal(B) * (0.01 if step % 4 == 3 else 5.0)).astype(F32)
        if step % 2:
            td[gen.integers(0, B)] = np.nan
            td[gen.integers(0, B)] = np.inf if step % 3 else -np.inf
        idx = gen.integers(0, ring.len, B)
        ring.update(idx, td)
        assert np.isfinite(ring.p_max) and ring.p_max >= seen[-1]
        finite = T.new_values(td, 1e-6, alpha)
        finite = finite[np.isfinite(finite)]
        assert bits(ring.p_max) == bits(max([seen[-1]] + finite.tolist()))
        seen.append(ring.p_max)
    # the non-finite values went to their leaves, as the PER update writes them
    ring.update(np.array([1, 2]), np.array([np.nan, np.inf], F32))
    assert np.isnan(ring.levels[0][1]) and np.isinf(ring.levels[0][2]) and bits(ring.p_max) == bits(seen[-1])
    # the reduction order does not matter to the value, only to being restated: a batch longer than one pass of the 1024 threads
    v = np.abs(gen.standard_normal(2500)).astype(F32)
    assert bits(T.pmax_reduce(v, np.ones(2500, bool))) == bits(v.max())


def test_seed_over_two_segments_and_with_skipped_rows():
    ring = T.RefHerTd(60, alpha=1.0, eps=1e-6)
    ring.flush(50)
    ring.update(np.arange(50), np.full(50, 4.0, F32))
    segs = ring.flush(3 * 8)                              # eight episodes of three rows in one launch: slots 50..59 and 0..13
    assert segs == [(50, 60), (0, 14)] and ring.head == 14 and ring.len == 60
    pm = F32(4.0) + F32(1e-6)
    assert np.all(bits(ring.levels[0][50:60]) == bits(pm)) and np.all(bits(ring.levels[0][:14]) == bits(pm))
    assert np.all(bits(ring.levels[0][14:50]) == bits(pm))           # (the updated rows: the same value here)
    assert not ring.levels[0][60:].any()
    small = T.RefHerTd(40, alpha=1.0, eps=1e-6)
    small.flush(3)
    small.update(np.array([0]), np.array([9.0], F32))
    head, length, skip = T.book_append(small.head, small.len, 40, 50)
    assert skip == 10 and length == 40
    segs = small.flush(50)                                # a ring smaller than the flush: only its 40 slots are written, once each
    assert sorted(segs) == [(0, 13), (13, 40)] or segs == [(0, 40)]
    assert small.head == head == 13 and np.all(bits(small.levels[0][:40]) == bits(F32(9.0) + F32(1e-6))) and not small.levels[0][40:].any()
    R.check_invariant(R.build(small.levels[0]))


def test_draw_frequencies_follow_the_leaves():
    """2^16 draws of the reference on the wrapped 4 160-slot tree, leaves spanning three decades with 30 % never-updated rows at
    p_max: counts against p_i / sum(p) within 5 binomial standard errors (the device draw's bound).  The bound is a normal
    approximation, so (as the energy draw's host test does) it is asked of bins with an expected count of at least 25: every row
    that has one on its own — all rows at p_max among them — and the lighter rows pooled by the decade of their leaf, so that every
    row is in exactly one bin.  Observed here: worst |z| = 2.95 over 1 443 bins."""
    cap = 4160
    ring = _filled(cap, seed=20261020, wrapped=True)
    gen = np.random.default_rng(5)
    upd = gen.permutation(cap)[: int(0.7 * cap)]
    # |td| such that the leaves (|td| + eps)^0.6 span 1e-3 .. 1 times the largest; the largest first, so that p_max is final
    td = (F32(50.0) * np.exp(gen.uniform(np.log(1e-3), 0.0, upd.size) / 0.6)).astype(F32)
    td[0] = F32(50.0)
    ring.update(upd[:1], td[:1])
    never = np.ones(cap, bool)
    never[upd] = False
    ring.levels[0][(ring.head + np.nonzero(never)[0]) % cap] = ring.p_max        # the rows of flushes that came after that update
    ring.levels = R.build(ring.levels[0])
    for o in range(0, upd.size, 256):
        ring.update(upd[o:o + 256], td[o:o + 256])
    leaves = ring.priorities()
    assert leaves.max() / leaves.min() >= 0.9e3 and np.all(bits(leaves[never]) == bits(ring.p_max)) and bits(leaves.max()) == bits(ring.p_max)
    n, B = 1 << 16, 256
    got = np.concatenate([ring.draw(B)[0] for _ in range(n // B)]).astype(np.int64)
    p = leaves.astype(np.float64) / leaves.astype(np.float64).sum()
    count = np.bincount(got, minlength=cap)
    own = n * p >= 25
    assert own[never].all() and own.sum() >= 0.3 * cap
    decade = np.floor(np.log10(leaves / leaves.max()) - 1e-9).astype(int)
    q = list(p[own]) + [p[~own & (decade == d)].sum() for d in np.unique(decade[~own])]
    c = list(count[own]) + [count[~own & (decade == d)].sum() for d in np.unique(decade[~own])]
    q, c = np.array(q), np.array(c)
    assert abs(q.sum() - 1.0) < 1e-9 and c.sum() == n and (n * q >= 25).all()
    z = (c - n * q) / np.sqrt(n * q * (1 - q))
    worst = float(np.max(np.abs(z)))
    print(f"worst |z| {worst:.2f} over {q.size} bins")
    assert worst < 5.0


def test_weights_are_the_fp64_formula_within_1e6():
    ring = _filled(4160, seed=3, wrapped=True)
    gen = np.random.default_rng(8)
    ring.update(gen.integers(0, 4160, 300), (gen.standard_normal(300) * 30).astype(F32))
    total = R.reduce64(ring.levels[-1])[0]
    for B, beta in ((1, 0.4), (64, 0.7), (72, 1.0)):
        idx, p = ring.draw(B)
        w = ring.weights(p, beta)
        want = R.weights64(p, total, ring.len, beta)
        assert np.max(np.abs(w.astype(np.float64) - want) / want) <= 1e-6 and w.max() == 1.0


def test_abi_and_ctypes_entries_exist(gcrl):
    lib = gcrl._ffi.lib
    hdr = open(os.path.join(ROOT, "include", "gcrl.h")).read()
    for e in ("gcrl_her_td_attach", "gcrl_her_td_get_pmax", "gcrl_her_td_set_pmax"):
        assert e in gcrl._ffi.PROTOTYPES and hasattr(lib, e) and re.search(rf"\b{e}\s*\(", hdr), e
    assert re.search(r"GCRL_PRIO_TD\s*=\s*2", hdr)
    assert lib.gcrl_her_td_attach(None, 0.6, 1e-6) < 0 and "prioritise" in gcrl._ffi.last_error()
    out = C.c_float(0)
    assert lib.gcrl_her_td_get_pmax(None, C.byref(out)) < 0 and "prioritise" in gcrl._ffi.last_error()
    assert lib.gcrl_her_td_set_pmax(None, 2.0) < 0 and "prioritise" in gcrl._ffi.last_error()
    assert lib.gcrl_her_prio_mode(None) == 0


def test_python_refusals_come_before_any_device_work(gcrl):
    """every spelling but 'td_error' stays refused, and what 'td_error' does not combine with is refused by name — on a machine
    without a GPU too, so before any device work"""
    err = gcrl._ffi.GcrlError
    for bad in ("td", "tde", "TD_ERROR", "per"):
        with pytest.raises(err, match="prioritise"):
            gcrl.HERBuffer(1000, 50, 1, relabel="sample", prioritise=bad)
    with pytest.raises(err, match="prioritise"):
        gcrl.HERBuffer(1000, 50, 1, relabel="push", prioritise="td_error")
    with pytest.raises(err, match="prioritise"):
        gcrl.HERBuffer(1000, 50, 1, relabel="sample", td=dict(alpha=0.5))
    with pytest.raises(err, match="prioritise"):
        gcrl.HERBuffer(1000, 50, 1, relabel="sample", prioritise="td_error", energy=dict(clip=1.0))
    with pytest.raises(err, match="prioritise"):
        gcrl.HERBuffer(1000, 50, 1, relabel="sample", prioritise="energy", td=dict(alpha=0.5))
    for td in (dict(beta=1.0), dict(alpha=-0.1), dict(eps=0.0), dict(alpha=float("nan")), dict(eps=float("inf")), dict(alpha=True), [0.6]):
        with pytest.raises(err, match="prioritise"):
            gcrl.HERBuffer(1000, 50, 1, relabel="sample", prioritise="td_error", td=td)


def test_new_kernels_use_no_scratch(tmp_path):
    """her_td.hip compiled to gfx950 assembly with the Makefile's flags: .private_segment_fixed_size is 0 for both kernels"""
    csrc = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)).split()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1)
    assert "her_td.hip" in re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    asm = tmp_path / "her_td.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "her_td.hip"), "-o", str(asm)], check=True, cwd=csrc)
    found = re.findall(r"\.name:\s+(\S*(?:her_td_seed_kernel|her_td_update_kernel)\S*)\n((?:(?!\.name:).)*?)\.private_segment_fixed_size:\s+(\d+)", asm.read_text(), re.S)
    sizes = {n: int(sz) for n, _, sz in found}
    assert len(sizes) == 2 and sum("her_td_seed_kernel" in n for n in sizes) == 1, sizes
    assert all(v == 0 for v in sizes.values()), sizes
