"""Generate tests/golden/normalizer_widths.npz from the REAL reference (build container only; see make_golden.py).

    GCRL_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_norm_widths.py

The reference's RunningNormalizer (src/utils.py:68-117) at ONE, two and three features.  np.mean / np.var over axis 0 add the rows
of an (n, D) array one after another for D >= 2; a contiguous (n, 1) array is reduced by numpy's pairwise sum instead (from 8 rows
on; tests/numpy_pairwise_ref.py restates the order), so a one-feature normaliser - a 1-D goal under g_normalize - gets other bits
than a column of a wider one.  The other normaliser goldens are all D = 7.  Captured for every D in (1, 2, 3), with batches of
1, 2, 7, 8, 9, 16, 33, 128, 129, 136 and 1000 rows in sequence (below, at and past numpy's thresholds 8 and 128), in three regimes:
  c32   a created normaliser fed float32 rows (float32 moments, float64 merge);
  l32   a normaliser loaded from the reference's yaml (float32 statistics, everything float32 from then on) fed float32 rows;
  c64   a created normaliser fed the same rows as float64 arrays (float32 VALUES, as the vector env hands observations over).
After every update: mean, var, count and the normalised probe rows (stacked along axis 0).  Data only; the rows are stored once
per D as float32, the batches one below the other."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
gym = types.ModuleType("gymnasium")


class _W:
    def __init__(self, env=None):
        self.env = env


gym.Wrapper = _W
gym.ObservationWrapper = _W
gym.vector = types.SimpleNamespace(AsyncVectorEnv=object)
gym.spaces = types.SimpleNamespace(Dict=dict, Box=object)
sys.modules["gymnasium"] = gym
sys.path.insert(0, os.environ["GCRL_REFERENCE"])

from src.utils import RunningNormalizer  # noqa: E402  (the reference)

WIDTHS = [1, 2, 3]
SIZES = [1, 2, 7, 8, 9, 16, 33, 128, 129, 136, 1000]


def main():
    gen = np.random.default_rng(2718)
    out = dict(widths=np.array(WIDTHS), sizes=np.array(SIZES), numpy=np.array(np.__version__))
    scale, shift = np.array([0.15, 10.0, 1e-3]), np.array([0.05, 5.0, 0.0])      # (goal-like first column: the one-feature case)
    for D in WIDTHS:
        draw = lambda n: (gen.standard_normal((n, D)) * scale[:D] + shift[:D]).astype(np.float32)
        xs = [draw(n) for n in SIZES]
        probe = draw(9)
        probe[0] += 100 * scale[:D].astype(np.float32)                          # one row far enough out for the clip
        out[f"d{D}_probe"] = probe
        out[f"d{D}_x"] = np.concatenate(xs)                                      # the batches one below the other: split by `sizes`
        # a warmed normaliser, saved: what the loaded regime starts from
        warm = RunningNormalizer(D)
        for n in (16, 40):
            warm.update(draw(n))
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "sub", "n.yaml")
            warm.save(path)
            with open(path) as fh:
                out[f"d{D}_yaml_text"] = np.array(fh.read())
            loaded = RunningNormalizer(D)
            loaded.load(path)
        assert loaded.mean.dtype == np.float32
        out[f"d{D}_load_mean"], out[f"d{D}_load_var"], out[f"d{D}_load_count"] = loaded.mean.copy(), loaded.var.copy(), np.array([loaded.count])
        for tag, nz, cast in (("c32", RunningNormalizer(D), np.float32), ("l32", loaded, np.float32), ("c64", RunningNormalizer(D), np.float64)):
            means, vars_, counts, norms = [], [], [], []
            for x in xs:
                rows = np.ascontiguousarray(x.astype(cast))
                nz.update(rows)
                z = nz.normalize(probe.astype(cast))
                means.append(nz.mean.copy()); vars_.append(nz.var.copy()); counts.append(nz.count); norms.append(z)
            k = f"d{D}_{tag}_"                                                   # one entry per update along axis 0
            out[k + "mean"], out[k + "var"], out[k + "count"], out[k + "norm"] = np.stack(means), np.stack(vars_), np.array(counts), np.stack(norms)
            want = np.float32 if tag == "l32" else np.float64
            assert nz.mean.dtype == want and z.dtype == want, (D, tag, nz.mean.dtype, z.dtype)
    np.savez_compressed(os.path.join(HERE, "normalizer_widths.npz"), **out)
    print("normalizer_widths ok", os.path.getsize(os.path.join(HERE, "normalizer_widths.npz")), "bytes, numpy", np.__version__)


if __name__ == "__main__":
    main()
