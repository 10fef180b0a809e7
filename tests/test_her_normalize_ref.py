"""Host tests (no GPU) of tests/her_normalize_ref.py, the numpy definition of sample-time normalisation of a HER ring
(HERBuffer(normalize="sample"); csrc/her_norm.hip): its normaliser arithmetic is the reference's bit for bit in the three regimes the
goldens pin (created, loaded as float32, float64 rows), it composes with her_strategy_ref without touching anything but the state
columns, the keyword's Python refusals come before any device work, the ABI declares the new entries, and the new unit's kernels use
no scratch memory and the registers and LDS that DESIGN.md §4m states."""
import os
import re
import subprocess

import numpy as np
import pytest
import yaml

import her_normalize_ref as NR
import her_relabel_ref as R
import her_strategy_ref as GS
from oracle.agent_oracle import make_config
from oracle.normalizer_oracle import RunningNormalizerOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F32)).view(np.uint32)


# ---------------------------------------------------------------- 1. the arithmetic is the reference's, regime by regime
def test_created_normaliser_matches_the_golden(golden):
    g = golden("normalizer.npz")
    o = RunningNormalizerOracle(int(g["D"][0]))
    for i in range(len(g["sizes"])):
        o.update(g[f"x{i}"])
        assert np.array_equal(bits(NR.apply(o, g["probe"])), bits(g[f"norm32_{i}"])), i


def test_loaded_normaliser_matches_the_golden(golden):
    g = golden("normalizer_loaded.npz")
    y = yaml.safe_load(str(g["yaml_text"]))
    o = RunningNormalizerOracle(int(g["D"][0]))
    o.load_state(y["mean"], y["var"], y["count"], y["clip_range"])
    got = NR.apply(o, g["probe"])
    assert got.dtype == F32 and np.array_equal(bits(got), bits(g["load_norm"]))
    for i in range(len(g["sizes"])):                                     # float32 rows keep the float32 regime through updates
        o.update(g[f"x{i}"])
        assert np.array_equal(bits(NR.apply(o, g["probe"])), bits(g[f"norm{i}"])), i


def test_float64_rows_match_the_golden(golden):
    g = golden("normalizer_f64.npz")
    probe = g["probe"]
    assert np.array_equal(probe.astype(F32).astype(np.float64), probe)   # float32-valued: they cross the ABI exactly
    o = RunningNormalizerOracle(int(g["D"][0]))
    for i in range(len(g["a_sizes"])):
        o.update(g[f"a_x{i}"])
        assert np.array_equal(bits(NR.apply(o, probe.astype(F32), rows64=True)), bits(g[f"a_norm{i}"].astype(F32))), i
    y = yaml.safe_load(str(g["yaml_text"]))
    o = RunningNormalizerOracle(int(g["D"][0]))
    o.load_state(y["mean"], y["var"], y["count"], y["clip_range"])       # float32 statistics, float64 rows
    assert np.array_equal(bits(NR.apply(o, probe.astype(F32), rows64=True)), bits(g["b_load_norm"].astype(F32)))


def test_zero_variance_and_clip():
    o = RunningNormalizerOracle(3, clip_range=5.0)
    o.mean, o.var = np.array([1.0, 0.0, -2.0]), np.array([0.0, 4.0, 1.0])
    x = np.array([[1.0, 100.0, -2.5], [1.5, -100.0, 0.0]], F32)
    got = NR.apply(o, x)
    assert got.tolist() == [[0.0, 5.0, -0.5], [5.0, -5.0, 2.0]]          # var = 0: (x - mean) / 1e-8, clipped — and exactly 0 at the mean


# ---------------------------------------------------------------- 2. composition: only the state columns move
def _ring(cap=60, seed=3):
    import test_her_strategy_ref as T
    return T.make_ring(cap, [50, 50], dims=(7, 2, 3), seed=seed), T.ring_args


@pytest.mark.parametrize("strategy,N", [(GS.FUTURE, 1), (GS.FUTURE, 3), (GS.FINAL, 1), (GS.EPISODE, 3)])
@pytest.mark.parametrize("flags", [(True, False), (True, True), (False, True)])
def test_gather_composes_strategy_and_normaliser(strategy, N, flags):
    q, ring_args = _ring()
    D = 4
    gen = np.random.default_rng(8)
    no, ng = RunningNormalizerOracle(D), RunningNormalizerOracle(3, clip_range=2.0)
    no.update(gen.standard_normal((40, D)).astype(F32) * 3 + 1)
    ng.update(gen.standard_normal((40, 3)).astype(F32) * 0.2)
    idx = gen.integers(0, q["len"], 300)
    raw = GS.gather(*ring_args(q), q["el"], q["head"], q["cap"], idx, 17, 5, 4, R.SPARSE, 0.05, strategy, N, 0.98)
    got = NR.gather(*ring_args(q), q["el"], q["head"], q["cap"], idx, 17, 5, 4, R.SPARSE, 0.05, D, no if flags[0] else None,
                    ng if flags[1] else None, strategy=strategy, n_step=N, gamma=0.98)
    for key in ("a", "r", "d"):
        assert np.array_equal(bits(got[key]), bits(raw[key])), key       # rewards: those of the raw achieved goals
    for key in ("s", "ns"):
        assert np.array_equal(bits(got["raw_" + key]), bits(raw[key]))
        want_o = NR.apply(no, raw[key][:, :D]) if flags[0] else raw[key][:, :D]
        want_g = NR.apply(ng, raw[key][:, D:]) if flags[1] else raw[key][:, D:]
        assert np.array_equal(bits(got[key][:, :D]), bits(want_o)) and np.array_equal(bits(got[key][:, D:]), bits(want_g))
    assert (got["o"] != 0).any()
    if flags[1]:
        assert (np.abs(got["s"][:, D:]) <= 2.0).all()                    # the goal normaliser's own clip
    sa, nsa, spa = NR.engine_matrices(got, 2, spa=True)
    assert sa.shape[1] == 12 and np.array_equal(bits(sa[:, 7:9]), bits(got["a"])) and not sa[:, 9:].any() and not nsa[:, 7:].any()
    assert np.array_equal(bits(spa[:, :8]), bits(sa[:, :8])) and np.isnan(spa[:, 8:]).all()


def test_sparse_reward_is_decided_in_metres_not_in_normalised_units():
    """what the mode exists for: a relabelled row whose achieved goal lies 0.04 from the goal is a success at threshold 0.05, although
    the normalised distance (statistics with std 0.01) is 4; and one 0.06 away is a failure although a wide normaliser makes it 0.006"""
    thr = 0.05
    a, near, far = np.zeros(3, F32), np.array([0.04, 0, 0], F32), np.array([0.06, 0, 0], F32)
    assert R.reward(near, a, R.SPARSE, thr) == 0.0 and R.reward(far, a, R.SPARSE, thr) == -1.0
    tight, wide = RunningNormalizerOracle(3), RunningNormalizerOracle(3)
    tight.var, wide.var = np.full(3, 1e-4), np.full(3, 100.0)
    assert R.reward(NR.apply(tight, near[None])[0], NR.apply(tight, a[None])[0], R.SPARSE, thr) == -1.0
    assert R.reward(NR.apply(wide, far[None])[0], NR.apply(wide, a[None])[0], R.SPARSE, thr) == 0.0


# ---------------------------------------------------------------- 3. refusals before any device work, the ABI, the unit's metadata
def test_python_refusals_name_normalize(gcrl):
    err = gcrl._ffi.GcrlError
    from gcrl_amd.src.buffer import HERBuffer, _RingState
    from gcrl_amd.src.utils import RunningNormalizer
    for bad in ("gather", None, 1):
        with pytest.raises(err, match="normalize"):
            HERBuffer(1000, 50, 2, normalize=bad)
    with pytest.raises(err, match="normalize"):
        HERBuffer(1000, 50, 2, normalize="sample", obs_normalize=False, g_normalize=False)
    kw = dict(hidden_dim=64, layer_count=3, batch_size=64)
    for name, cls, pop in (("DDPG", gcrl.DDPG, gcrl.DDPGPopulation), ("TD3", gcrl.TD3Agent, gcrl.TD3Population),
                           ("SAC", gcrl.SACAgent, gcrl.SACPopulation), ("TQC", gcrl.TQCAgent, gcrl.TQCPopulation)):
        cfg = make_config(name, **kw)
        with pytest.raises(err, match=f"{cls.__name__}: normalize"):
            cls(10, 3, cfg, None, 2, 4, normalize="always")
        with pytest.raises(err, match=f"{cls.__name__}: normalize"):
            cls(10, 3, cfg, None, 2, 4, normalize="sample", obs_normalize=False)
        for bt in ("PER", "REPLAY"):
            c2 = make_config(name, **kw)
            c2.buffer_type = bt
            with pytest.raises(err, match=f"{cls.__name__}: normalize"):
                cls(10, 3, c2, None, 2, 4, normalize="sample")
        for shared in (False, True):
            cfgs = [make_config(name, **kw) for _ in range(2)]
            with pytest.raises(err, match=f"{pop.__name__}: normalize"):
                pop(10, 3, cfgs, 2, 4, normalize="never", shared_ring=shared)
            with pytest.raises(err, match=f"{pop.__name__}: normalize"):
                pop(10, 3, cfgs, 2, 4, normalize="sample", obs_normalize=False, g_normalize=False, shared_ring=shared)
    # a buffer as its constructor leaves it, without the device its last lines ask for
    b = HERBuffer.__new__(HERBuffer)
    b.normalize, b.obs_normalize, b.g_normalize, b._h, b._obs_normalizer, b._dg_normalizer = "sample", True, False, None, None, None
    with pytest.raises(err, match="normalize"):
        b.obs_normalizer = RunningNormalizer(7)                          # a host normaliser where a device one is needed
    assert b.obs_normalizer is None
    b.dg_normalizer = RunningNormalizer(3)                               # g_normalize is off: not needed, any object may sit there
    b.relabel, b.goal_strategy, b.prioritise = "push", "future", None
    for meta in (dict(normalize="push"), dict(), dict(normalize="sample", obs_normalize=False, g_normalize=False),
                 dict(normalize="sample", obs_normalize=True, g_normalize=True)):
        with pytest.raises(err, match="normalize"):
            _RingState.load_state(b, "/nonexistent", dict(meta, bytes=0))
    b.normalize = "push"
    with pytest.raises(err, match="normalize"):
        _RingState.load_state(b, "/nonexistent", dict(normalize="sample", obs_normalize=True, g_normalize=False, bytes=0))


def test_abi_declares_the_new_entries(gcrl):
    for name in ("gcrl_her_set_normalize", "gcrl_her_require_normalize", "gcrl_her_normalize_mode"):
        assert hasattr(gcrl._ffi.lib, name), name
    lib = gcrl._ffi.lib
    assert lib.gcrl_her_normalize_mode(None) == -1
    assert lib.gcrl_her_set_normalize(None, None, None, 3) == -1 and b"gcrl_her_set_normalize" in lib.gcrl_last_error()   # null handle: refused, no device touched
    hdr = open(os.path.join(ROOT, "include", "gcrl.h")).read()
    for name in ("gcrl_her_set_normalize", "gcrl_her_require_normalize", "gcrl_her_normalize_mode", "GCRL_NORMALIZE_SAMPLE"):
        assert name in hdr, name


# what DESIGN.md §4m states for the unit: kernel -> (VGPRs, bytes of static LDS)
# (the process_step kernels: 42 / 42 / 44 VGPRs before norm_update_col's pairwise order for one-feature normalisers, whose running
# sums and waiting left halves are kept in registers; still 0 bytes of scratch and LDS)
KERNELS = {"her_norm_rows_kernel": (36, 2176), "her_norm_dense_kernel": (32, 2176), "her_process_step_raw_kernel": (72, 0),
           "her_process_step_raw_inline_kernel": (90, 0), "her_process_step_raw_pop_kernel": (90, 0)}


def test_new_kernels_use_no_scratch_and_the_stated_registers(tmp_path):
    """her_norm.hip compiled to gfx950 assembly with the Makefile's flags: 0 bytes of scratch, no spills, and the VGPR and LDS figures
    of DESIGN.md §4m for each of its five kernels"""
    csrc = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)).split()
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1))
    assert "her_norm.hip" in re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split() and "-ffp-contract=off" in flags and "-O3" in flags
    asm = tmp_path / "her_norm.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "her_norm.hip"), "-o", str(asm)], check=True, cwd=csrc)
    text = asm.read_text()
    seen = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        field = lambda f: int(re.search(rf"\.{f}:\s+(\d+)", blk).group(1))
        short = next((k for k in sorted(KERNELS, key=len, reverse=True) if k in name), None)
        assert short is not None and short not in seen, name
        seen[short] = (field("vgpr_count"), field("group_segment_fixed_size"))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0, name
    assert seen == KERNELS, seen
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4m."):]
    for k, (v, lds) in KERNELS.items():
        assert re.search(rf"`{k}`[^|\n]*\|\s*{v}\s*\|[^|\n]*\|\s*{lds}\s*\|", sec), k
