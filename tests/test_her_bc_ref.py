"""Host tests (no GPU) of tests/her_bc_ref.py, the numpy definition of Q-filtered behaviour cloning on the prior rows of a batch
(bc_weight= / q_filter=; csrc/her_bc.hip): the restatement against torch autograd of the stated loss in float64, what it leaves
untouched, the mask's edge cases, every keyword refusal that precedes device work, the ABI entries, and the new unit's metadata."""
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle.agent_oracle import make_config

import her_bc_ref as BC

F32 = np.float32


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F32)).view(np.uint32)


# ---------------------------------------------------------------- 1. the restatement against autograd of the stated loss
def _problem(seed, B=8, Bd=3, A=4, S=6, H=16):
    """a random 2-layer tanh actor (hidden tanh, tanh output) and a fixed linear critic, float64; actions of the batch in [-1, 1]"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    return dict(B=B, Bd=Bd, A=A, s=r(B, S), a=torch.tanh(r(B, A)), W1=r(H, S) / S ** 0.5, b1=r(H) * 0.1, W2=r(A, H) / H ** 0.5, b2=r(A) * 0.1,
                ws=r(S) * 0.3, wa=r(A) * 0.3, qb=r(1) * 0.1)


def _autograd(p, bc_weight, q_filter):
    """z = the pre-tanh action as a leaf of the full loss -> (dL/dz, the BC term, mask, pi, q_a, q_pi), float64"""
    B, Bd = p["B"], p["Bd"]
    z = (torch.tanh(p["s"] @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"]).detach().requires_grad_(True)
    pi = torch.tanh(z)
    Q = lambda act: p["s"] @ p["ws"] + act @ p["wa"] + p["qb"]
    q_pi, q_a = Q(pi), Q(p["a"])
    mask = torch.zeros(B, dtype=torch.float64)
    mask[B - Bd:] = (q_a > q_pi)[B - Bd:].double().detach() if q_filter else 1.0
    term = bc_weight * (1.0 / Bd) * (mask[:, None] * (pi - p["a"]) ** 2).sum()
    loss = -q_pi.mean() + term
    loss.backward()
    return z.grad.numpy(), float(term.detach()), mask.numpy(), pi.detach().numpy(), q_a.detach().numpy(), q_pi.detach().numpy()


@pytest.mark.parametrize("q_filter", [True, False])
def test_ref_gradient_and_loss_equal_autograd_in_float64(q_filter):
    """B = 8, Bd = 3, A = 4.  The ref gets fp32 roundings of pi, a, of the critic's part of dL/dz and of the two Q vectors; its
    output against autograd in float64: 1e-6 relative on the max-norm (DESIGN.md §4h's bound for fp32-vs-fp64 evaluations)."""
    W = 0.7
    for seed in range(40):                      # the first seed whose Q-filter both accepts and rejects a row
        p = _problem(seed)
        grad, term, mask, pi, q_a, q_pi = _autograd(p, W, q_filter)
        tail = mask[p["B"] - p["Bd"]:]
        if not q_filter or (tail.min() == 0 and tail.max() == 1):
            break
    assert not q_filter or (tail.min() == 0 and tail.max() == 1)
    B, Bd, A = p["B"], p["Bd"], p["A"]
    critic_part = (-p["wa"].numpy()[None, :] / B) * (1.0 - pi * pi)             # d(-mean Q)/dz for the linear critic
    m32 = BC.mask_of(q_a.astype(F32), q_pi.astype(F32), B, Bd, q_filter)
    assert np.array_equal(m32, mask.astype(F32))
    dact = np.zeros((B, 4), F32)
    dact[:, :A] = critic_part.astype(F32)
    out, loss, share = BC.step(pi.astype(F32), p["a"].numpy().astype(F32), dact, m32, W, Bd)
    assert out.dtype == F32 and loss.dtype == F32 and share.dtype == F32
    err = np.abs(out[:, :A].astype(np.float64) - grad).max() / np.abs(grad).max()
    print(f"q_filter={q_filter}: gradient max-norm relative error {err:.3e}, loss {float(loss)!r} vs {term!r}")
    assert err <= 1e-6, err
    assert abs(float(loss) - term) <= 1e-6 * abs(term) and term > 0
    assert float(share) == float(F32(F32(mask.sum()) / F32(Bd)))
    assert abs(BC.loss_f64(pi, p["a"].numpy(), mask, W, Bd) - term) <= 1e-12 * term


# ---------------------------------------------------------------- 2. what the launch leaves alone
def test_head_rows_rejected_rows_and_pad_columns_keep_their_bits():
    gen = np.random.default_rng(5)
    B, Bd, A, Apad = 8, 5, 3, 4
    pi, a = np.tanh(gen.standard_normal((B, A))).astype(F32), np.tanh(gen.standard_normal((B, A))).astype(F32)
    dact = gen.standard_normal((B, Apad)).astype(F32)
    dact[1, 0] = dact[4, 1] = dact[6, 2] = F32(-0.0)                          # a head row, a rejected row, an accepted row
    dact[:, A:] = np.nan
    mask = np.array([1, 1, 1, 0, 0, 1, 1, 0], F32)                            # (rows 0..2 are head rows: their 1s must not count)
    out, loss, share = BC.step(pi, a, dact, mask, 2.0, Bd)
    untouched = [0, 1, 2, 3, 4, 7]
    assert np.array_equal(bits(out[untouched]), bits(dact[untouched]))
    assert np.signbit(out[1, 0]) and np.signbit(out[4, 1]) and out[4, 1] == 0
    assert np.array_equal(bits(out[:, A:]), bits(dact[:, A:]))
    for b in (5, 6):
        assert not np.array_equal(bits(out[b, :A]), bits(dact[b, :A]))
    assert float(share) == float(F32(2) / F32(5))
    c, w_bd = BC.scales(2.0, Bd)
    assert c == F32(0.8) and w_bd == F32(0.4)
    want = F32(w_bd * F32(sum_rows(pi, a, [5, 6])))
    assert loss == want
    same, l2, _ = BC.step(pi, a, dact, np.zeros(B, F32), 2.0, Bd)                # nothing accepted: nothing moves, the term is 0
    assert np.array_equal(bits(same), bits(dact)) and l2 == 0


def sum_rows(pi, a, rows):
    """rows < 256 sit in one wave, one per lane: the butterfly adds them as a tree whose other leaves are exact zeros"""
    acc = np.zeros(BC.WAVE, F32)
    for k, b in enumerate(rows):
        s = F32(0)
        for j in range(pi.shape[1]):
            d = F32(pi[b, j] - a[b, j])
            s = F32(s + F32(d * d))
        acc[(b - (pi.shape[0] - 5)) % BC.WAVE] = s
    return BC.butterfly(acc)


def test_more_rows_than_threads_sum_in_the_stated_order():
    """Bd > 256: a thread meets several rows; four waves' words are added in wave order"""
    gen = np.random.default_rng(11)
    B, Bd, A = 700, 650, 2
    pi, a = np.tanh(gen.standard_normal((B, A))).astype(F32), np.tanh(gen.standard_normal((B, A))).astype(F32)
    mask = BC.mask_of(None, None, B, Bd, q_filter=False)
    _, loss, share = BC.step(pi, a, np.zeros((B, 4), F32), mask, 1.0, Bd)
    rows = ((pi - a).astype(F32) ** 2).astype(F32)
    rows = (rows[:, 0] + rows[:, 1]).astype(F32)[B - Bd:]
    acc = np.zeros(256, F32)
    for i, s in enumerate(rows):
        acc[i % 256] = F32(acc[i % 256] + s)
    waves = [BC.butterfly(acc[w * 64:(w + 1) * 64]) for w in range(4)]
    total = F32(F32(F32(waves[0] + waves[1]) + waves[2]) + waves[3])
    assert loss == F32(F32(1.0 / 650) * total) and share == 1
    assert abs(float(loss) - BC.loss_f64(pi, a, mask, 1.0, Bd)) <= 1e-5 * float(loss)


# ---------------------------------------------------------------- 3. the mask's edges
def test_nan_and_equal_q_give_mask_zero():
    B, Bd = 6, 5
    q_a = np.array([9, 1.0, np.nan, 2.0, -0.0, 3.0], F32)
    q_pi = np.array([0, 1.0, 0.0, np.nan, 0.0, 2.9999998], F32)
    m = BC.mask_of(q_a, q_pi, B, Bd)
    assert m.dtype == F32 and m.tolist() == [0, 0, 0, 0, 0, 1]                  # head row; tie; NaN; NaN; -0.0 == 0.0; strictly above
    assert BC.mask_of(q_a, q_pi, B, Bd, q_filter=False).tolist() == [0, 1, 1, 1, 1, 1]
    assert BC.mask_of(np.full(B, np.inf, F32), np.full(B, np.inf, F32), B, B).sum() == 0
    assert BC.rows_ok(8, 8) and BC.rows_ok(8, 1) and not BC.rows_ok(8, 0) and not BC.rows_ok(8, 9) and not BC.rows_ok(8, True)
    for bad in (0, -1.0, float("nan"), float("inf"), True, None, "1"):
        assert not BC.weight_ok(bad), bad
    assert BC.weight_ok(1) and BC.weight_ok(0.004) and BC.weight_ok(np.float32(2))


# ---------------------------------------------------------------- 4. keyword refusals before any device work, ABI
def _prior_stub(HERBuffer):
    b = HERBuffer.__new__(HERBuffer)
    b.rng, b.prioritise, b.normalize, b._h = SimpleNamespace(mode="device"), None, "push", None
    b.obs_normalize, b.g_normalize = True, False
    return b


def test_python_refusals_name_bc_weight(gcrl):
    err = gcrl._ffi.GcrlError
    from gcrl_amd.src.agent import _check_bc
    from gcrl_amd.src.buffer import HERBuffer
    good = _prior_stub(HERBuffer)
    assert _check_bc("x", "DDPG", None, True, None) is None and _check_bc("x", "SAC", None, True, None) is None
    assert _check_bc("x", "TD3", 2, False, good) == 2.0 and _check_bc("x", "DDPG", np.float32(0.5), True, good) == 0.5
    kw = dict(hidden_dim=64, layer_count=3, batch_size=64)
    prior = dict(prior_buffer=good, prior_rows=20)
    for name, cls in (("DDPG", gcrl.DDPG), ("TD3", gcrl.TD3Agent)):
        cfg = make_config(name, **kw)
        for bad in (0, 0.0, -1.0, float("nan"), float("inf"), True, "1"):                  # finite and > 0; "off" is None
            with pytest.raises(err, match=f"{cls.__name__}: bc_weight"):
                cls(10, 3, cfg, None, 2, 4, bc_weight=bad, **prior)
        with pytest.raises(err, match=f"{cls.__name__}: bc_weight.*prior_buffer"):        # the term needs the prior rows
            cls(10, 3, cfg, None, 2, 4, bc_weight=1.0)
        with pytest.raises(err, match=f"{cls.__name__}: q_filter"):
            cls(10, 3, cfg, None, 2, 4, bc_weight=1.0, q_filter="yes", **prior)
    for name, cls in (("SAC", gcrl.SACAgent), ("TQC", gcrl.TQCAgent)):                     # accepted only to be refused
        with pytest.raises(err, match=f"{cls.__name__}: bc_weight"):
            cls(10, 3, make_config(name, **kw), None, 2, 4, bc_weight=1.0, **prior)
    for name, pop in (("DDPG", gcrl.DDPGPopulation), ("TD3", gcrl.TD3Population), ("SAC", gcrl.SACPopulation), ("TQC", gcrl.TQCPopulation)):
        with pytest.raises(err, match=f"{pop.__name__}: bc_weight"):
            pop(10, 3, [make_config(name, **kw) for _ in range(2)], 2, 4, bc_weight=1.0, **prior)
    from gcrl_amd.src.dp import DataParallelUpdater
    with pytest.raises(err, match="bc_weight"):
        DataParallelUpdater(SimpleNamespace(per_draw="host", prior_buffer=good, bc_weight=1.0))


def test_abi_declares_the_new_entries(gcrl):
    lib = gcrl._ffi.lib
    names = ("gcrl_agent_set_bc", "gcrl_agent_get_bc", "gcrl_agent_bc_metrics", "gcrl_bc_qfilter_f32")
    hdr = open(os.path.join(ROOT, "include", "gcrl.h")).read()
    for name in names:
        assert hasattr(lib, name) and name + "(" in hdr and name in gcrl._ffi.PROTOTYPES, name
    # null handles and bad arguments: refused by name, no device touched
    assert lib.gcrl_agent_set_bc(None, 1.0, 1, 3) == -1 and b"gcrl_agent_set_bc" in lib.gcrl_last_error()
    assert lib.gcrl_agent_get_bc(None, None, None, None, None) == -1 and b"gcrl_agent_get_bc" in lib.gcrl_last_error()
    assert lib.gcrl_agent_bc_metrics(None, 0, None) == -1 and b"gcrl_agent_bc_metrics" in lib.gcrl_last_error()
    assert lib.gcrl_bc_qfilter_f32(None, None, 8, 4, 1, 0, None, None, 8, 3, 4, 1.0, None, 4, None, None, None) == -1
    assert b"gcrl_bc_qfilter_f32" in lib.gcrl_last_error()
    csrc = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
    ops = open(os.path.join(csrc, "ops.h")).read()
    assert re.search(r"MET_BC_LOSS\s*=\s*22\b", ops) and re.search(r"MET_BC_PASS\s*=\s*23\b", ops)
    assert re.search(r"\bV_BC\s*=\s*2048\b", open(os.path.join(csrc, "agent.hip")).read())


# ---------------------------------------------------------------- 5. the new unit's kernel metadata
def test_new_kernel_uses_no_scratch_and_does_not_spill(tmp_path):
    """her_bc.hip compiled to gfx950 assembly with the Makefile's flags: by the kernel's metadata 0 bytes of scratch and no spills;
    its LDS is the eight words of the wave-order sums"""
    csrc = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)).split()
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1))
    assert "her_bc.hip" in re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split() and "-ffp-contract=off" in flags and "-O3" in flags
    asm = tmp_path / "her_bc.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "her_bc.hip"), "-o", str(asm)], check=True, cwd=csrc)
    text = asm.read_text()
    seen = []
    for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        field = lambda f: int(re.search(rf"\.{f}:\s+(\d+)", blk).group(1))
        seen.append(name)
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0, name
        assert field("group_segment_fixed_size") == 32, name
    assert len(seen) == 1 and "bc_qfilter_kernel" in seen[0], seen
    assert "atomic" not in text and "s_sleep" not in text      # no atomics, no waits for other workgroups
