"""Not gpu: the comparison of tests/test_gpu_acting_edges.py must be able to fail.  On the CPU the helper of tests/acting_edges.py is
fed the oracle's own fp32 output, which must pass at every case of the tables (the condition on the choice of inputs), and three
corruptions of it, each of which must trip the bound at every case it applies to:
  one row's last 16 input columns left un-normalised; one head output computed without its bias; DDPG's tanh applied once, not twice."""
import copy

import numpy as np
import pytest
import torch

import acting_edges as ae

ROW = [(k, c) for k in ("DDPG", "TD3") for c in ae.ROWCHAIN_CASES]
BN = [(k, c) for k in ("SAC", "TQC") for c in ae.BN_CASES]
ALL = ROW + BN
NORMALISED = [(k, c) for k, c in ALL if c not in ae.ROWCHAIN_NO_NORMALISER]      # (s300-raw has no normalised columns to leave out)


def setup(kind, case, seed=7):
    from gcrl_amd.src.utils import RunningNormalizer
    D, G, A, H, L, n = (ae.ROWCHAIN_CASES if kind in ("DDPG", "TD3") else ae.BN_CASES)[case]
    S = D + G
    bn = ae.bn_statistics(seed, H, L) if kind in ("SAC", "TQC") else (None, None)
    mod = ae.oracle_actor(kind, S, A, H, L, ae.initial_flat(kind, S, A, H, L, seed), *bn)
    obs, dg = ae.raw_rows(seed, n, D, G)
    if case in ae.ROWCHAIN_NO_NORMALISER:
        onz = gnz = None
    else:
        onz, gnz = RunningNormalizer(D), RunningNormalizer(G)
        wo, wg = ae.warm_batches(seed, D, G)
        onz.update(wo); gnz.update(wg)
    x = ae.host_state(onz, gnz, obs, dg)
    gen = np.random.default_rng(seed + 1)
    noise = gen.standard_normal((n, A)).astype(np.float32).astype(np.float64) * (1.0 if kind in ("SAC", "TQC") else 0.1)
    return mod, x, np.concatenate([obs, dg], axis=-1), noise, (onz is not None)


@pytest.mark.parametrize("kind,case", ALL)
def test_the_clean_fp32_run_is_inside_the_bound(kind, case):
    mod, x, _, noise, _ = setup(kind, case)
    for ev in (True, False):
        r64, r32 = ae.references(kind, mod, x, ev, noise)
        e_got, e_ref, bound = ae.errors(r32, r64, r32)
        assert e_got == e_ref <= bound and e_ref < 1e-5, (ev, e_ref)
        assert ae.within_bound(r32, r64, r32)
        # the inputs leave the actions off the rails: an error in the network is visible in them
        if ev:
            assert np.mean(np.abs(r64) < 0.999) > 0.5, r64
        else:
            assert np.any(np.abs(r64) < 1.0), r64      # (exploring: not every element clipped)


@pytest.mark.parametrize("kind,case", NORMALISED)
def test_a_row_with_its_last_columns_left_raw_trips_the_bound(kind, case):
    mod, x, raw, noise, normalised = setup(kind, case)
    assert normalised
    bad = x.copy()
    r, w = x.shape[0] - 1, min(16, x.shape[1])
    bad[r, -w:] = raw[r, -w:]
    for ev in (True, False):
        r64, r32 = ae.references(kind, mod, x, ev, noise)
        got = ae.reference_action(kind, mod, bad, ev, noise, torch.float32)
        assert not ae.within_bound(got, r64, r32), (ev, ae.errors(got, r64, r32))


@pytest.mark.parametrize("kind,case", ALL)
def test_a_head_output_without_its_bias_trips_the_bound(kind, case):
    mod, x, _, noise, _ = setup(kind, case)
    bad = copy.deepcopy(mod)
    head = bad.mean_head if kind in ("SAC", "TQC") else [m for m in bad.base_net if isinstance(m, torch.nn.Linear)][-1]
    with torch.no_grad():
        head.bias[head.bias.numel() - 1] = 0.0
    for ev in (True, False):
        r64, r32 = ae.references(kind, mod, x, ev, noise)
        got = ae.reference_action(kind, bad, x, ev, noise, torch.float32)
        assert not ae.within_bound(got, r64, r32), (ev, ae.errors(got, r64, r32))


@pytest.mark.parametrize("case", list(ae.ROWCHAIN_CASES))
def test_ddpg_with_one_tanh_trips_the_bound(case):
    mod, x, _, noise, _ = setup("DDPG", case)
    for ev in (True, False):
        r64, r32 = ae.references("DDPG", mod, x, ev, noise)
        got = ae.reference_action("DDPG", mod, x, ev, noise, torch.float32, corrupt="single_tanh")
        assert not ae.within_bound(got, r64, r32), (ev, ae.errors(got, r64, r32))
