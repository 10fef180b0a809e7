"""Not gpu: tests/numpy_pairwise_ref.py against numpy itself, bit for bit.  It is the definition of the order csrc/norm_math.h sums a
one-feature normaliser's batch in; if numpy ever changes that order, this is where it shows."""
import numpy as np
import pytest

from numpy_pairwise_ref import mean_var_one_feature, pairwise_sum, sequential_sum

SIZES = [1, 7, 8, 9, 17, 127, 128, 129, 136, 257, 1000, 5000, 8192, 8193, 20000]


def draw(n, dtype, seed):
    gen = np.random.default_rng(seed)
    return (gen.standard_normal((n, 1)) * 3 + 0.7).astype(np.float32).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", SIZES)
def test_restatement_equals_numpy_mean_and_var_of_one_feature(n, dtype):
    x = draw(n, dtype, n)
    if dtype is np.float64:
        x = x * 1.0000001            # (float32-valued doubles would add without rounding at the small sizes)
    mean, var = mean_var_one_feature(x)
    want_m, want_v = np.mean(x, axis=0), np.var(x, axis=0)
    assert mean.dtype == want_m.dtype == dtype and var.dtype == want_v.dtype == dtype
    assert mean.tobytes() == want_m.tobytes(), (n, mean, want_m)
    assert var.tobytes() == want_v.tobytes(), (n, var, want_v)
    assert np.asarray(pairwise_sum(x[:, 0])).tobytes() == np.asarray(x.sum(axis=0)[0]).tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_features_or_more_are_summed_row_after_row(dtype):
    """The other half of the rule: from two features upward every feature's sum is sequential in the rows."""
    for D in (2, 3, 7):
        for n in (8, 129, 1000):
            x = np.ascontiguousarray(np.repeat(draw(n, dtype, 31 * n + D), D, axis=1) * np.arange(1, D + 1, dtype=dtype))
            got = x.sum(axis=0)
            for j in range(D):
                assert np.asarray(sequential_sum(x[:, j])).tobytes() == np.asarray(got[j]).tobytes(), (D, n, j)


def test_the_two_orders_differ_where_the_issue_is():
    """The reason the rule matters: at 8 float32 rows (a 1-D goal with two envs: 4 * nenvs rows per step) the pairwise and the
    sequential sum already round differently for ordinary data."""
    differ = 0
    for seed in range(20):
        x = draw(8, np.float32, 1000 + seed)[:, 0]
        differ += np.asarray(pairwise_sum(x)).tobytes() != np.asarray(sequential_sum(x)).tobytes()
    assert differ > 0


@pytest.mark.parametrize("regime", ["c32", "l32", "c64"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_the_normaliser_oracle_follows_both_orders(golden, D, regime):
    """oracle/normalizer_oracle.py (explicit sums: pairwise at one feature, row after row from two) against the reference's
    statistics at 1, 2 and 3 features, tests/golden/normalizer_widths.npz: every update, bit for bit."""
    from oracle.normalizer_oracle import RunningNormalizerOracle
    g = golden("normalizer_widths.npz")
    k, cast = f"d{D}_{regime}_", np.float64 if regime == "c64" else np.float32
    nz = RunningNormalizerOracle(D)
    if regime == "l32":
        nz.load_state(g[f"d{D}_load_mean"], g[f"d{D}_load_var"], g[f"d{D}_load_count"][0], 5.0)
    at = 0
    for i, n in enumerate(int(v) for v in g["sizes"]):
        nz.update(g[f"d{D}_x"][at:at + n].astype(cast))
        at += n
        assert nz.mean.dtype == g[k + "mean"].dtype
        assert np.array_equal(nz.mean, g[k + "mean"][i]) and np.array_equal(nz.var, g[k + "var"][i]) and nz.count == g[k + "count"][i], (D, regime, n)
        assert np.array_equal(nz.normalize(g[f"d{D}_probe"].astype(cast)), g[k + "norm"][i]), (D, regime, n)
