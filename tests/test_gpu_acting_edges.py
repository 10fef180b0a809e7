"""GPU (-m gpu): the acting kernels against an fp64 CPU reference, at the edges of their launch forms.

csrc/rowchain.hip (rowchain_act_kernel, rowchain_act_inline_kernel, rowchain_act_pop_kernel) and csrc/act_bn.hip (act_bn_kernel,
act_bn_inline_kernel and the population forms) are elsewhere compared with one another: inline against staged, a population against
its members, observe_act against select_action - forms that run the same body text, so a defect in the body passes those bitwise.
Here every returned action array is held to the oracle's DetActor / GaussActor carrying the agent's own weights, run in float64 on
the CPU from host-normalised float32 rows: e_got = max|HIP - fp64| <= max(3 * e_ref, 2e-6) with e_ref torch's own fp32 error
(tests/acting_edges.py; tests/test_acting_edges_host.py shows the comparison failing on three planted defects).  Every figure is
appended to the file GCRL_ACTING_EDGES_RECORD names (profiles/r27_acting_edges.jsonl is one MI355X run)."""
import random

import numpy as np
import pytest
import torch

import acting_edges as ae
from oracle.agent_oracle import make_config

pytestmark = pytest.mark.gpu


def seed_all(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def build(gcrl, kind, shape, normalisers=True, seed=11):
    """(agent, oracle actor with the agent's weights, host normalisers or None).  rng="python": DDPG's epsilon branch draws from
    `random`, which the test replays.  The weights are perturbed so that no two biases are equal."""
    from gcrl_amd.src.utils import DeviceRunningNormalizer, RunningNormalizer
    D, G, A, H, L, n = shape
    cfg = make_config(kind, hidden_dim=H, layer_count=L, batch_size=64, max_len=2000, noise_std=0.1)
    cls = dict(SAC=gcrl.SACAgent, TQC=gcrl.TQCAgent, DDPG=gcrl.DDPG, TD3=gcrl.TD3Agent)[kind]
    ag = cls(D + G, A, cfg, None, nenvs=n, gradient_step=10, rng="python")
    gen = np.random.default_rng(seed)
    flat = ag.actor.flat()
    ag.actor.set_flat((flat + 0.02 * gen.standard_normal(flat.shape)).astype(np.float32))
    bn = (None, None)
    if kind in ("SAC", "TQC"):
        bn = ae.bn_statistics(seed, H, L)
        ag.actor._set("bn_running_mean", bn[0])
        ag.actor._set("bn_running_var", bn[1])
    mod = ae.oracle_actor(kind, D + G, A, H, L, ag.actor.flat(), *bn)
    host = None
    if normalisers:
        host = (RunningNormalizer(D), RunningNormalizer(G))
        ag.buffer.obs_normalizer, ag.buffer.dg_normalizer = DeviceRunningNormalizer(D), DeviceRunningNormalizer(G)
        wo, wg = ae.warm_batches(seed, D, G)
        for nz, dev, rows in ((host[0], ag.buffer.obs_normalizer, wo), (host[1], ag.buffer.dg_normalizer, wg)):
            nz.update(rows)
            dev.update(rows)
            assert np.array_equal(dev.mean, nz.mean) and np.array_equal(dev.var, nz.var) and dev.count == nz.count
    return ag, mod, host


def call(kind, ag, shape, f, ev, seed):
    """f() under seeded host generators -> (the returned actions, the noise / eps that call drew: replayed from the same states).
    DDPG's epsilon-random action involves no network: it is checked exactly and the call repeated under the next seed."""
    D, G, A, H, L, n = shape
    if ev:
        return np.asarray(f()), None
    for attempt in range(40):
        seed_all(seed + 1000 * attempt)
        got = np.asarray(f())
        seed_all(seed + 1000 * attempt)
        if kind == "DDPG" and random.random() < 0.2:          # src/agent.py:1348
            assert np.array_equal(got, np.clip(np.random.randn(n, A), -1, 1))
            continue
        if kind in ("DDPG", "TD3"):
            return got, np.random.normal(0, ag.noise_std, size=(n, A))
        return got, torch.randn((n, A), dtype=torch.float32).numpy().astype(np.float64)
    raise AssertionError("forty epsilon branches in a row")


def run_paths(kind, case, ag, mod, shape, x32, paths):
    """every path x (eval, exploring): one comparison each"""
    worst = 0.0
    for name, f in paths:
        for ev in (True, False):
            c0 = ag.acting_counts()
            got, noise = call(kind, ag, shape, lambda: f(ev), ev, 77)
            c1 = ag.acting_counts()
            assert got.shape == (shape[5], shape[2]), got.shape
            r64, r32 = ae.references(kind, mod, x32, ev, noise)
            e_got, e_ref = ae.check(got, r64, r32, kind=kind, case=case, shape=list(shape), path=name, eval_action=ev,
                                    launches=c1["launches"] - c0["launches"], copies=c1["copies"] - c0["copies"])
            worst = max(worst, e_got)
    return worst


@pytest.mark.parametrize("case", list(ae.ROWCHAIN_CASES))
@pytest.mark.parametrize("kind", ["DDPG", "TD3"])
def test_rowchain_acting_against_fp64(gcrl, kind, case):
    """select_action, observe_act with device normalisers and observe_act without normalisation, eval and exploring, at the
    row-chain edges (the table in tests/acting_edges.py names what each shape hits)."""
    shape = ae.ROWCHAIN_CASES[case]
    D, G, A, H, L, n = shape
    normalised = case not in ae.ROWCHAIN_NO_NORMALISER
    ag, mod, host = build(gcrl, kind, shape, normalisers=normalised)
    obs, dg = ae.raw_rows(5, n, D, G)
    x32 = ae.host_state(host[0] if host else None, host[1] if host else None, obs, dg)
    paths = [("select_action", lambda ev: ag.select_action(x32, eval_action=ev)),
             ("observe_act_raw", lambda ev: ag.observe_act(x32[:, :D], x32[:, D:], eval_action=ev, obs_normalize=False, g_normalize=False))]
    if normalised:
        paths.insert(1, ("observe_act", lambda ev: ag.observe_act(obs, dg, eval_action=ev, obs_normalize=True, g_normalize=True)))
    before = ag.acting_counts()["calls"]
    run_paths(kind, case, ag, mod, shape, x32, paths)
    assert ag.acting_counts()["calls"] - before >= 2 * (len(paths) - 1)      # the fused entry was reached, not the host fallback


@pytest.mark.parametrize("regime", ["created", "loaded", "rows64", "constant-column", "clip"])
@pytest.mark.parametrize("kind", ["DDPG", "TD3"])
def test_rowchain_fused_normalisation_regimes_against_fp64(gcrl, kind, regime):
    """The prologue's normaliser arithmetic in its regimes (bit-exactness of the arithmetic itself is pinned by the normaliser
    goldens; here its result is held within the bound): a created normaliser, a loaded (float32) one, float64 observation rows,
    statistics holding a constant column (variance 0) and rows far enough out that the clip engages."""
    shape = ae.ROWCHAIN_REGIME_SHAPE
    D, G, A, H, L, n = shape
    ag, mod, host = build(gcrl, kind, shape)
    obs, dg = ae.raw_rows(6, n, D, G, far=regime == "clip")
    dev = (ag.buffer.obs_normalizer, ag.buffer.dg_normalizer)
    if regime == "loaded":          # float32 statistics on both sides: everything float32 from then on (src/utils.py:108-117)
        for nz, d in zip(host, dev):
            nz.mean, nz.var = nz.mean.astype(np.float32), nz.var.astype(np.float32)
            d.set_state(nz.mean, nz.var, nz.count)
            assert d.float32
    if regime == "rows64":
        obs = obs.astype(np.float64)
    if regime == "constant-column":
        host[0].var[2] = 0.0
        dev[0].set_state(host[0].mean, host[0].var, host[0].count)
        obs[:, 2] = np.float32(host[0].mean[2])       # on the mean's float32 neighbour: (x - mean) / 1e-8, a few units or the clip
        obs[0, 2] += np.float32(1e-3)                 # and one element off it: clipped
    x32 = ae.host_state(host[0], host[1], obs, dg)
    if regime in ("clip", "constant-column"):
        assert np.abs(x32).max() == 5.0
    run_paths(kind, "regime-" + regime, ag, mod, shape, x32,
              [("observe_act", lambda ev: ag.observe_act(obs, dg, eval_action=ev, obs_normalize=True, g_normalize=True))])


@pytest.mark.parametrize("kind", ["DDPG", "TD3"])
def test_rowchain_fused_normalisation_refuses_129_state_columns(gcrl, kind):
    """S 129 with device normalisers: the prologue stages two elements per thread, 128 columns of four rows; a wider state is refused
    by name, never read out of bounds."""
    shape = ae.ROWCHAIN_REFUSED
    D, G, A, H, L, n = shape
    ag, _, _ = build(gcrl, kind, shape)
    obs, dg = ae.raw_rows(7, n, D, G)
    with pytest.raises(ValueError, match="state_dim"):
        ag.observe_act(obs, dg, eval_action=True, obs_normalize=True, g_normalize=True)


@pytest.mark.parametrize("case", ae.POPULATION_CASES)
@pytest.mark.parametrize("kind", ["DDPG", "TD3"])
def test_rowchain_population_is_bitwise_its_members(gcrl, kind, case):
    """A population of 2 launching rowchain_act_pop_kernel (MERGE_ACTING_FROM = 2) at the two inline limits: bitwise the members'
    own observe_act, which test_rowchain_acting_against_fp64 anchors at the same shapes."""
    import test_gpu_population_acting as tpa
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    D, G, A, H, L, n = ae.ROWCHAIN_CASES[case]
    P, S = 2, D + G
    cfgs = [make_config(kind, hidden_dim=H, layer_count=L, batch_size=64, max_len=2000, noise_std=0.1) for _ in range(P)]
    seeds = [31, 32]
    pop = (gcrl.DDPGPopulation if kind == "DDPG" else gcrl.TD3Population)(S, A, cfgs, n, 8, rng="engine", seeds=seeds)
    pop.MERGE_ACTING_FROM = 2
    cls = gcrl.DDPG if kind == "DDPG" else gcrl.TD3Agent
    solo = [cls(S, A, c, None, nenvs=n, gradient_step=8, rng="engine", seed=s) for c, s in zip(cfgs, seeds)]
    wo, wg = ae.warm_batches(3, D, G)
    for i in range(P):
        gen = np.random.default_rng(40 + i)
        flat = solo[i].actor.flat()
        flat = (flat + 0.02 * gen.standard_normal(flat.shape)).astype(np.float32)
        for ag in (pop.members[i], solo[i]):
            ag.actor.set_flat(flat)
            ag.buffer.obs_normalizer, ag.buffer.dg_normalizer = DeviceRunningNormalizer(D), DeviceRunningNormalizer(G)
            ag.buffer.obs_normalizer.update(wo * (1 + i)); ag.buffer.dg_normalizer.update(wg)
    before = pop.acting_counts()
    step = 0
    for ev in (True, False, False, False):
        rows = [ae.raw_rows(100 * i + step, n, D, G) for i in range(P)]
        obs, dg = [r[0] for r in rows], [r[1] for r in rows]
        kw = dict(eval_action=ev, obs_normalize=True, g_normalize=True)
        got, want = tpa._both(900 + step, lambda: pop.observe_act(obs, dg, **kw), lambda: [a.observe_act(o, g, **kw) for a, o, g in zip(solo, obs, dg)])
        tpa._same(got, want, f"{kind} {case} call {step}")
        step += 1
    assert pop.acting_counts()[0] > before[0]      # (the population's own entry was used)


@pytest.mark.parametrize("case", list(ae.BN_CASES))
@pytest.mark.parametrize("kind", ["SAC", "TQC"])
def test_batchnorm_acting_against_fp64(gcrl, kind, case):
    """Fused observe_act of the BatchNorm actors, eval and exploring (eps replayed from torch's host generator into
    GaussActor.sample's arithmetic, eval mode, the agent's running statistics)."""
    shape = ae.BN_CASES[case]
    D, G, A, H, L, n = shape
    ag, mod, host = build(gcrl, kind, shape)
    obs, dg = ae.raw_rows(5, n, D, G)
    x32 = ae.host_state(host[0], host[1], obs, dg)
    before = ag.acting_counts()
    run_paths(kind, case, ag, mod, shape, x32,
              [("observe_act", lambda ev: ag.observe_act(obs, dg, eval_action=ev, obs_normalize=True, g_normalize=True))])
    after = ag.acting_counts()
    assert after["calls"] - before["calls"] == 2 and after["launches"] - before["launches"] == 2      # one launch per call
