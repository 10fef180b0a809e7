"""GPU (-m gpu): merged acting of a SAC population (src/population.py SACPopulation.observe_act -> gcrl_pop_observe_act_bn ->
act_bn_pop_kernel / act_bn_pop_staged_kernel, csrc/act_bn.hip: ONE launch per vector step for all members) held to BITWISE equality
with standalone `SACAgent` twins of the same configs and seeds driven by their own `observe_act` in member order, torch's host
generator seeded identically before each side and compared after.  Every member has its own weights, BatchNorm running statistics
and normaliser statistics, and the rows differ on every call and for every member, so a launch that read another member's table
entry, another member's slice of the block or an earlier call's rows would be caught.

The class's `MERGE_ACTING_FROM` is a measured dispatch threshold; the tests that mean the merged launch set it to 2 on
the instance, and `acting_counts()` says which path ran."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_acting_bn as tab
import test_gpu_population_acting as tpa
import test_gpu_population_sac as tps
import test_gpu_population_td3 as tp3

pytestmark = pytest.mark.gpu

SMALL = dict(D=7, G=3, A=3, H=64, B=64)        # state 10: not a multiple of 4 — layer 0 takes the 4-byte weight loads, the others 16-byte
CFG5W = dict(D=19, G=3, A=3, H=256, B=64)      # the cfg 5 row width (H 256, L 3)


def _twins(gcrl, P, sh, seed0=700, merged=True, fill=False):
    S = sh["D"] + sh["G"]
    cfgs = tps._cfgs(P, sh["H"], sh["B"])
    seeds = list(range(seed0, seed0 + P))
    pop = gcrl.SACPopulation(S, sh["A"], cfgs, tpa.NENVS, 8, rng="engine", seeds=seeds)
    if merged:
        pop.MERGE_ACTING_FROM = 2
    solo = [gcrl.SACAgent(S, sh["A"], c, None, nenvs=tpa.NENVS, gradient_step=8, rng="engine", seed=s) for c, s in zip(cfgs, seeds)]
    for i in range(P):
        gen = np.random.default_rng(900 + i)
        obs_rows = (gen.standard_normal((40, sh["D"])) * (1 + i) + 0.3 * i).astype(np.float32)
        dg_rows = (gen.standard_normal((40, sh["G"])) * 0.2 * (1 + i)).astype(np.float32)
        for ag in (pop.members[i], solo[i]):
            tpa._normalizers(gcrl, ag, sh, i)                  # device normalisers, compute_reward, each member its own weights
            if fill:
                tps._fill(ag, S, sh["A"], i)                   # (the ring for update_many, created with that compute_reward)
            tab.scramble(ag, 40 + i)                           # ... BatchNorm affine parameters and running statistics
            ag.buffer.obs_normalizer.update(obs_rows)          # ... and normaliser statistics
            ag.buffer.dg_normalizer.update(dg_rows)
    return pop, solo


def _act(pop, solo, step, sh, n=tpa.NENVS, launches=1, staged=0, **kw):
    """one observe_act on both sides from identically seeded torch generators: bitwise per member, the generator consumed alike, and the
    launch counters advanced by exactly `launches` / `staged`"""
    rows = [tpa._rows(step, i, sh, n) for i in range(len(solo))]
    obs = [r[0]["observation"] for r in rows]
    dg = [r[0]["desired_goal"] for r in rows]
    before = pop.acting_counts()
    torch.manual_seed(7000 + step)
    got = pop.observe_act(obs, dg, **kw)
    st_pop = torch.get_rng_state()
    torch.manual_seed(7000 + step)
    want = [a.observe_act(o, g, **kw) for a, o, g in zip(solo, obs, dg)]
    assert torch.equal(st_pop, torch.get_rng_state()), "torch's host generator consumed differently"
    what = f"actions of step {step} (n={n}, {kw})"
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        # (a member on its own fallback — a host normaliser: select_action — returns float32, as the standalone agent does)
        assert g.dtype == w.dtype and g.shape == (n, sh["A"]) and (g.dtype == np.float64 or not launches), (what, i, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, i, np.abs(g - w).max())
    tpa._same(got, want, what)
    after = pop.acting_counts()
    assert after[1] - before[1] == launches and after[4] - before[4] == staged, (what, before, after)
    return rows, got


@pytest.mark.parametrize("P", [2, 3, 16])
def test_bitwise_against_the_members_own_entries(gcrl, P):
    """n = 1, 5 (a partial last workgroup), 8 and 32 (the block's limit) rows per member, sampled and deterministic actions, with and
    without the goal normaliser: one launch per call, none staged"""
    pop, solo = _twins(gcrl, P, SMALL)
    step = 0
    for g_norm in (False, True):
        for n in (1, 5, 8, 32):
            for ev in (False, True):
                _act(pop, solo, step, SMALL, n=n, eval_action=ev, g_normalize=g_norm)
                step += 1
    calls, launches, _, _, staged = pop.acting_counts()
    assert (calls, launches, staged) == (step, step, 0)


def test_cfg5_row_width(gcrl):
    pop, solo = _twins(gcrl, 4, CFG5W)
    _act(pop, solo, 0, CFG5W)
    _act(pop, solo, 1, CFG5W, eval_action=True, g_normalize=True)


def test_one_member_population_forwards_to_the_member(gcrl):
    pop, solo = _twins(gcrl, 1, SMALL)
    pop.MERGE_ACTING_FROM = 1
    _act(pop, solo, 0, SMALL, launches=0)
    _act(pop, solo, 1, SMALL, launches=0, eval_action=True)
    assert pop.acting_counts()[:2] == (2, 0)       # the native entry ran and handed the call to the member's own


def test_staged_form(gcrl):
    """33 rows per member are more than the pinned block holds (32): copies around the same one launch"""
    pop, solo = _twins(gcrl, 3, SMALL)
    _act(pop, solo, 0, SMALL, n=33, staged=1)
    _act(pop, solo, 1, SMALL, n=33, staged=1, eval_action=True, g_normalize=True)
    _act(pop, solo, 2, SMALL, n=8)                  # and back on the fast form
    assert pop.acting_counts()[:2] == (3, 3) and pop.acting_counts()[4] == 2


def test_fresh_parameters_and_statistics(gcrl):
    """The launch reads the live parameter vectors and running statistics: after update_many (which moves both) and after a write to
    one member's parameters and statistics the next call is bitwise the members' own — and differs from the call before"""
    P = 3
    pop, solo = _twins(gcrl, P, SMALL, fill=True)
    _, a0 = _act(pop, solo, 0, SMALL)
    got = pop.update_many(1, 4)
    want = [a.update_many(1, 4) for a in solo]
    for i in range(P):
        tps._same(got[i], want[i], ("update_many", i))
    _, a1 = _act(pop, solo, 0, SMALL)               # (the same rows and eps as before the update)
    for i in range(P):
        assert np.abs(a1[i] - a0[i]).max() > 1e-6, f"member {i}: the actions did not move with the update"
    for ag in (pop.members[1], solo[1]):
        ag.actor.set_flat((ag.actor.flat() * 0.7).astype(np.float32))
        ag.actor._set("bn_running_var", (ag.actor._get("bn_running_var") * 1.5).astype(np.float32))
    _, a2 = _act(pop, solo, 0, SMALL)
    assert np.abs(a2[1] - a1[1]).max() > 1e-6, "member 1: the actions did not move with its parameter write"
    for i in (0, 2):
        assert np.array_equal(a2[i], a1[i]), f"member {i} moved with member 1's parameter write"


def test_two_vector_steps_through_process_step(gcrl):
    P = 3
    pop, solo = _twins(gcrl, P, SMALL)
    for step in (1, 2):
        rows, acts = _act(pop, solo, step, SMALL)
        tpa._proc(pop, solo, step, rows, acts, tpa._dones(step))
    assert pop.acting_counts() == (2, 2, 2, 2, 0)
    tpa._compare_members(pop, solo)


def test_fallbacks_advance_no_launch_count(gcrl):
    from gcrl_amd.src.utils import RunningNormalizer
    P = 3
    pop, solo = _twins(gcrl, P, SMALL)
    # the measured threshold above P: the members' own entries
    pop.MERGE_ACTING_FROM = P + 1
    _act(pop, solo, 0, SMALL, launches=0)
    pop.MERGE_ACTING_FROM = 2
    # members with different row counts
    rows = [tpa._rows(1, i, SMALL, 8 if i == 0 else 5) for i in range(P)]
    obs, dg = [r[0]["observation"] for r in rows], [r[0]["desired_goal"] for r in rows]
    torch.manual_seed(11)
    got = pop.observe_act(obs, dg)
    torch.manual_seed(11)
    tpa._same(got, [a.observe_act(o, g) for a, o, g in zip(solo, obs, dg)], "different row counts")
    assert pop.acting_counts()[:2] == (0, 0)
    # a member with a host normaliser
    for ag in (pop.members[1], solo[1]):
        ag.buffer.obs_normalizer = RunningNormalizer(SMALL["D"])
    _act(pop, solo, 2, SMALL, launches=0)
    assert pop.acting_counts() == (0, 0, 0, 0, 0)


def test_refusals_on_the_device(gcrl):
    from gcrl_amd import _ffi
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    P, D, G, A, B = 3, SMALL["D"], SMALL["G"], SMALL["A"], SMALL["B"]
    pop, _ = _twins(gcrl, P, SMALL)
    obs = np.zeros((P, B + 1, D), np.float32)
    dg = np.zeros((P, B + 1, G), np.float32)
    out = np.full((P, B + 1, A), 7.0, np.float64)
    vp = lambda x: C.c_void_p(x.ctypes.data)

    def call(h, n=8, d=D, g=G, nzo=None):
        return _ffi.lib.gcrl_pop_observe_act_bn(h, nzo, None, vp(obs), d, vp(dg), g, n, None, vp(out), None)

    def refused(rc, *words):
        msg = _ffi.last_error()
        assert rc == _ffi.GCRL_ERR_ARG and all(w in msg for w in words), (rc, msg, words)
        assert np.all(out == 7.0), "a refused call wrote actions"

    td3 = gcrl.TD3Population(D + G, A, tp3._cfgs(2, SMALL["H"], B), tpa.NENVS, 8, rng="engine", seeds=[1, 2])
    refused(call(td3._pop.h), "kind", "gcrl_pop_observe_act")
    assert td3.acting_counts() == (0, 0, 0, 0, 0)
    refused(call(pop._pop.h, n=0), " n: ")
    refused(call(pop._pop.h, n=B + 1), " n: ")
    refused(call(pop._pop.h, d=D - 1), "obs_dim", "state_dim")
    refused(call(pop._pop.h, g=G + 1), "goal_dim", "state_dim")
    wrong = DeviceRunningNormalizer(D + 1)
    nzo = (C.c_void_p * P)(pop.members[0].buffer.obs_normalizer.handle, wrong.handle, pop.members[2].buffer.obs_normalizer.handle)
    refused(call(pop._pop.h, nzo=nzo), "nz_obs", "member 1")
    keep = pop.members[1].buffer.obs_normalizer
    pop.members[1].buffer.obs_normalizer = wrong
    rows = [tpa._rows(0, i, SMALL) for i in range(P)]
    with pytest.raises(ValueError, match="nz_obs"):
        pop.observe_act([r[0]["observation"] for r in rows], [r[0]["desired_goal"] for r in rows])
    pop.members[1].buffer.obs_normalizer = keep
    big = [tpa._rows(0, i, SMALL, n=B + 1) for i in range(P)]
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match=r"\bn\b"):
        pop.observe_act([r[0]["observation"] for r in big], [r[0]["desired_goal"] for r in big])
    assert torch.equal(state, torch.get_rng_state())        # refused before a generator is touched
    assert pop.acting_counts() == (0, 0, 0, 0, 0)           # ... and before any launch
