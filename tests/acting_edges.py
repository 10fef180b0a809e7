"""Shared by tests/test_gpu_acting_edges.py (gpu) and tests/test_acting_edges_host.py: the case tables, the inputs, the fp64 / fp32
CPU reference of an acting call and the comparison that holds the HIP acting kernels to it.

Reference: the oracle's DetActor / GaussActor (oracle/agent_oracle.py, pinned against the reference by tests/test_oracle_golden.py)
holding the agent's own flat weights, run on one thread in float64, and once more in float32 as the yardstick.  The inputs are
normalised by the host RunningNormalizer (numpy) and cast to float32 as the trainer does (src/env.py:189-190); the post-processing
restates select_action (src/agent.py:1345-1366, :253-270, :641-647).

Bound, for every returned action array:  e_got = max|HIP - fp64|,  e_ref = max|fp32 CPU - fp64|,  e_got <= max(3 * e_ref, 2e-6).
The factor 3 over torch's own fp32 error is the rule of test_batchnorm_relu_forward_backward_against_torch; the floor is the project's
acting bound (ATOL of tests/test_gpu_acting_bn.py).  Actions lie in [-1, 1], so the bound is absolute."""
import copy
import json
import os

import numpy as np
import torch

from oracle.agent_oracle import DetActor, GaussActor

FLOOR, FACTOR = 2e-6, 3.0

# (D, G, A, H, L, n): observation width, goal width, action width, hidden width, hidden layers, rows
ROWCHAIN_CASES = {
    "minimal": (1, 1, 1, 4, 1, 1),            # everything minimal: three of the four waves have an empty j-share
    "headline-n7": (20, 3, 4, 256, 3, 7),     # the headline shape, ragged last workgroup (3 of 4 rows), past the prefetch bound
    "headline-n8": (20, 3, 4, 256, 3, 8),     # the same with two full workgroups
    "prefetch-edge": (20, 3, 4, 256, 2, 4),   # (L - 1) * H^2 = 65 536 exactly: the prefetch loop runs
    "h260": (7, 3, 3, 260, 2, 5),             # one column chunk of 256 and four more columns: the unchained rows_linear
    "h512-l3": (7, 3, 3, 512, 3, 3),          # two full chunks, three layers
    "h520": (9, 3, 2, 520, 2, 6),             # two chunks and eight columns, S 12
    "l8": (7, 3, 3, 32, 8, 3),                # kRowMaxLayers
    "s128-inline": (125, 3, 2, 64, 2, 5),     # S 128 with fused normalisation: 4 * jpad0 = 512 (both staged elements of every thread used); n * S = 640, the inline limit
    "s128-staged": (125, 3, 2, 64, 2, 6),     # one row past the limit: the staged kernel
    "a16-inline": (7, 3, 16, 64, 2, 6),       # n * A = 96: the inline noise limit exactly
    "a16-staged": (7, 3, 16, 64, 2, 7),       # n * A = 112: past it
    "s300-raw": (297, 3, 2, 64, 2, 3),        # rows of 300 floats through the trailing loop, J > 256 in the first layer; no fused normalisation at this width
}
ROWCHAIN_NO_NORMALISER = {"s300-raw"}
ROWCHAIN_REGIME_SHAPE = (7, 3, 3, 64, 2, 5)   # the normaliser regimes, the constant column and the clip are run at this shape
ROWCHAIN_REFUSED = (126, 3, 2, 64, 2, 3)      # S 129 with device normalisers: refused by name (state_dim)
POPULATION_CASES = ["s128-inline", "a16-inline"]

BN_CASES = {
    "s12": (9, 3, 3, 32, 2, 5),               # S 12: the 16-byte first layer (hidden_layer<4>)
    "cfg5-width": (25, 3, 3, 256, 3, 8),      # cfg 5's row width, S 28
    "a1": (7, 3, 1, 32, 2, 1),                # one action, one row
    "a8": (7, 3, 8, 32, 2, 3),                # 2A = 16
    "a9": (7, 3, 9, 32, 2, 3),                # 2A = 18: the first width past 16
    "a16-inline": (7, 3, 16, 32, 2, 6),       # 2A = 32 fills kHeadLd; n * A = 96, the inline limit
    "a16-staged": (7, 3, 16, 32, 2, 7),       # n * A = 112: the staged form
    "h260": (7, 3, 3, 260, 2, 2),             # a second round of four columns in hidden_layer
    "l1": (7, 3, 3, 36, 1, 3),                # one hidden layer
    "l5": (7, 3, 3, 36, 5, 3),                # five
}


def record(**line):
    """Append the measured figures to the file GCRL_ACTING_EDGES_RECORD names (how profiles/r27_acting_edges.jsonl is made)."""
    path = os.environ.get("GCRL_ACTING_EDGES_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(line) + "\n")


# ---------------------------------------------------------------- inputs
def raw_rows(seed, n, D, G, far=False):
    """Raw observation and goal rows as an env hands them over (float32); far: some elements far enough out for the clip."""
    gen = np.random.default_rng(seed)
    obs = (gen.standard_normal((n, D)) * 3 + 1).astype(np.float32)
    dg = gen.uniform(-0.2, 0.2, (n, G)).astype(np.float32)
    if far:
        obs[0, 0], obs[n - 1, D - 1], dg[0, G - 1] = 40.0, -55.0, 3.0
    return obs, dg


def warm_batches(seed, D, G, rows=40):
    """The batches both sides' normalisers are updated with before the calls."""
    gen = np.random.default_rng(10_000 + seed)
    return (gen.standard_normal((rows, D)) * 3 + 1).astype(np.float32), gen.uniform(-0.2, 0.2, (rows, G)).astype(np.float32)


def host_state(obs_nz, dg_nz, obs, dg):
    """normalize_state_batch on the host, cast as the trainer casts it: the float32 rows the network sees."""
    o = obs_nz.normalize(obs) if obs_nz is not None else obs
    g = dg_nz.normalize(dg) if dg_nz is not None else dg
    return np.concatenate([o, g], axis=-1).astype(np.float32)


# ---------------------------------------------------------------- the oracle actor with the agent's weights
def oracle_actor(kind, S, A, H, L, flat, bn_mean=None, bn_var=None):
    """DetActor / GaussActor (eval mode) holding `flat` (the agent's flat parameter vector: the module's parameters in order) and,
    for the BatchNorm actors, the agent's running statistics ([L * H] each)."""
    stochastic = kind in ("SAC", "TQC")
    mod = (GaussActor if stochastic else DetActor)(S, H, A, L)
    flat = np.asarray(flat, np.float32)
    at = 0
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.from_numpy(flat[at:at + p.numel()].reshape(tuple(p.shape)).copy()))
            at += p.numel()
        assert at == flat.size, (at, flat.size)
        if stochastic:
            bns = [m for m in mod.base_net if isinstance(m, torch.nn.BatchNorm1d)]
            assert len(bns) == L
            for l, bn in enumerate(bns):
                bn.running_mean.copy_(torch.from_numpy(np.asarray(bn_mean, np.float32)[l * H:(l + 1) * H].copy()))
                bn.running_var.copy_(torch.from_numpy(np.asarray(bn_var, np.float32)[l * H:(l + 1) * H].copy()))
    return mod.eval()


def initial_flat(kind, S, A, H, L, seed):
    """Without an agent (the host self-check): the oracle's own initialisation, perturbed so that no two biases are equal."""
    gen = torch.Generator().manual_seed(seed)
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    mod = (GaussActor if kind in ("SAC", "TQC") else DetActor)(S, H, A, L)
    torch.set_rng_state(state)
    flat = np.concatenate([p.detach().numpy().reshape(-1) for p in mod.parameters()]).astype(np.float32)
    return (flat + 0.02 * torch.randn(flat.size, generator=gen).numpy()).astype(np.float32)


def bn_statistics(seed, H, L):
    gen = np.random.default_rng(seed)
    return (gen.standard_normal(L * H) * 0.3).astype(np.float32), gen.uniform(0.3, 2.0, L * H).astype(np.float32)


# ---------------------------------------------------------------- the reference of one acting call
def reference_action(kind, mod, x32, eval_action, noise=None, dtype=torch.float64, corrupt=None):
    """What select_action returns for the float32 rows x32, computed in `dtype` on one thread, as a float64 array.
    noise: DDPG / TD3: the np.random.normal draw of the exploring branch; SAC / TQC: rsample's eps (float32 values).
    corrupt (the host self-check only): "single_tanh": DDPG's second tanh left out."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        m = copy.deepcopy(mod).to(dtype).eval()
        x = torch.from_numpy(np.ascontiguousarray(x32, np.float32)).to(dtype)
        with torch.no_grad():
            if kind in ("SAC", "TQC"):
                mean, log_std = m(x)
                out = torch.tanh(mean) if eval_action else torch.tanh(mean + torch.from_numpy(np.asarray(noise)).to(dtype) * log_std.exp())
                return out.double().numpy()
            y = m(x)                                              # (the module ends in Tanh)
            if kind == "TD3" and eval_action:
                return y.double().numpy()                         # the network output as it is (src/agent.py:265-270)
            a = (y if corrupt == "single_tanh" else torch.tanh(y)).double().numpy()     # the double tanh of the reference
            if not eval_action:
                a = a + np.asarray(noise, np.float64)
            return np.clip(a, -1, 1)
    finally:
        torch.set_num_threads(threads)


def references(kind, mod, x32, eval_action, noise=None):
    """(fp64 reference, fp32 yardstick) of one call."""
    return (reference_action(kind, mod, x32, eval_action, noise, torch.float64),
            reference_action(kind, mod, x32, eval_action, noise, torch.float32))


def errors(got, ref64, ref32):
    """(e_got, e_ref, bound) of one returned action array."""
    got, ref64, ref32 = (np.asarray(v, np.float64) for v in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (got.shape, ref64.shape, ref32.shape)
    assert np.all(np.isfinite(got)), "non-finite action"
    e_got, e_ref = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    return e_got, e_ref, max(FACTOR * e_ref, FLOOR)


def within_bound(got, ref64, ref32):
    e_got, e_ref, bound = errors(got, ref64, ref32)
    return e_got <= bound


def check(got, ref64, ref32, **what):
    """The comparison: records the figures, then asserts the bound."""
    e_got, e_ref, bound = errors(got, ref64, ref32)
    print(f"acting edges {what}: e_got {e_got:.3e} e_ref {e_ref:.3e} bound {bound:.3e}")
    record(e_got=e_got, e_ref=e_ref, bound=bound, ratio=e_got / bound, **what)
    assert e_got <= bound, (what, e_got, e_ref, bound)
    return e_got, e_ref
