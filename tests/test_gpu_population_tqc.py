"""GPU (-m gpu): TQC populations (src/population.py TQCPopulation, csrc/agent_pop.inc gcrl_pop_create_layered) — P TQC agents on the
layer-per-launch schedule whose update steps share launches — held to BITWISE equality with standalone `TQCAgent`s given the same
config, seed, ring contents and calls: every metric tuple (9 entries on actor steps, 6 on critic-only steps) and the engine state of
every member (gcrl_agent_save_state: parameters, targets, Adam moments, log_alpha, BatchNorm running statistics, schedules, counters,
the device noise streams).

The guarantee is SAC's, "a standalone agent RUNNING THE SAME FORMS" (tests/test_gpu_population_sac.py): only form bit 1, the row-split
slab launches, exists on this schedule.  The population runs in the test's own process; its twins run there too when they pick the
same slab form, otherwise in a fresh child process with GCRL_NO_BN_RSPLIT=1.

Launch positions: every launch of the step has a population form except two per step — the TD / sort-truncate target and loss launch
(td_loss_kernel) and the step's single-workgroup metric launch (critic-only steps: mean_metric_kernel for q_value; actor steps:
actor_select_alpha_kernel, which carries that mean as a rider).  DESIGN.md 4f names them; `alone` must be exactly 2 per step."""
import ctypes as C
import os
import subprocess
import sys
import random

import numpy as np
import pytest

import test_gpu_population_sac as tps
from oracle.agent_oracle import make_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S, A, L, GSTEP = 10, 3, 3, 8
ALONE_PER_STEP = 2                           # td_loss + (mean_metric | actor_select_alpha): the launchers still on pop_defer
SHAPES = {"h64_b64": (2, 64, 64, 5, 2),      # P, H, B, critics, drop
          "h32_b96": (3, 32, 96, 3, 1)}      # B 96: no multiple of 64 — partial tiles and row groups
# two update_many calls and one update: actor steps are the even ones, log-alpha steps from the sixth step on (both do_alpha values)
CALLS = [(1, 8), (9, 8), (17, 1)]


def _cfgs(P, H, B, nc, drop):
    """members that differ in learning rates and their schedules, gamma, tau, alpha_lr, grad_clip (member 1: none) and top_drop"""
    out = []
    for i in range(P):
        out.append(make_config("TQC", hidden_dim=H, layer_count=L, batch_size=B, max_len=4000, ac_update_freq=2,
                               actor_lr=1e-3 * (1 + 0.25 * i), actor_lr_min=2e-4, ac_scheduler_steps=30 + i,
                               critic_lr=1e-3 * (1 + 0.5 * i), critic_lr_min=3e-4, cr_scheduler_steps=25 + 2 * i,
                               alpha_lr=3e-4 * (1 + i), alpha_min_steps=5,
                               gamma=0.98 - 0.01 * (i % 3), tau=0.05 + 0.01 * i, grad_clip=None if i == 1 else 1.0 + i,
                               num_critics=nc, top_quantiles_to_drop=max(0, drop - (i % 2))))
    return out


def _pop(gcrl, cfgs, seeds, rng="engine", nenvs=2):
    pop = gcrl.TQCPopulation(S, A, cfgs, nenvs, GSTEP, rng=rng, seeds=seeds)
    for i, m in enumerate(pop.members):
        assert isinstance(m, gcrl.TQCAgent) and m.num_critics == cfgs[i].num_critics and m.top_quantiles_to_drop == cfgs[i].top_quantiles_to_drop
        tps._fill(m, S, A, i)
    return pop


def _solo(gcrl, cfgs, seeds, rng="engine", nenvs=2):
    solo = [gcrl.TQCAgent(S, A, c, None, nenvs=nenvs, gradient_step=GSTEP, rng=rng, seed=s) for c, s in zip(cfgs, seeds)]
    for i, a in enumerate(solo):
        tps._fill(a, S, A, i)
    return solo


def _twins_run(gcrl, shape, seed0, calls):
    """standalone twins through the calls: per member the padded tuples of every call, their lengths, and the final state blob"""
    solo = _solo(gcrl, _cfgs(*shape), list(range(seed0, seed0 + shape[0])))
    out = {"forms": np.array(solo[0].meetings() & 1)}
    for c, (step0, n) in enumerate(calls):
        for i, a in enumerate(solo):
            t, lens = tps._tuples(a.update_many(step0, n) if n > 1 else [a.update(step0)])
            out[f"t_{c}_{i}"], out[f"l_{c}_{i}"] = t, np.array(lens)
    for i, a in enumerate(solo):
        out[f"s_{i}"] = tps._state(a)
        out[f"nb_{i}"] = np.array(int(a.actor.num_batches_tracked))
    return out


def _twins_to_file(gcrl, path, *args):
    np.savez(path, **_twins_run(gcrl, *args))


def _child(code, env_extra):
    env = dict(os.environ, **env_extra)
    env.pop("GCRL_POP_NO_WAITS", None)
    pre = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport gcrl_amd, test_gpu_population_tqc as t\n" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", pre + code + "\nprint('child ok')\n"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def _bitwise_case(gcrl, shape, seed0, calls=CALLS, tmp=None, row_split=False):
    P = shape[0]
    pop = _pop(gcrl, _cfgs(*shape), list(range(seed0, seed0 + P)))
    assert len(pop) == P
    member_forms = pop.members[0].meetings() & (1 | 2 | 8)
    forms = pop.forms()
    terms = pop.forms_terms()
    print("forms", forms, "members'", member_forms, "terms", terms)
    assert forms == tps._rule(pop), (forms, tps._rule(pop), terms)
    assert forms & 2 == 0 and terms[2][0] == 0            # form bit 2 has no meaning for TQC
    assert member_forms & ~1 == 0                          # no TQC agent runs the merged chain launch or the fused optimiser launch
    if tps._shared() or os.environ.get("GCRL_POP_NO_WAITS"):
        assert forms == 0, forms
    elif row_split:
        assert forms & 1, (forms, terms)
    want = None
    if (member_forms ^ forms) & 1:       # a standalone agent of this process runs the row-split slab launches, the population does not
        assert tmp is not None
        path = os.path.join(str(tmp), "twins.npz")
        _child("t._twins_to_file(gcrl_amd, %r, %r, %r, %r)" % (path, shape, seed0, calls), {"GCRL_NO_BN_RSPLIT": "1"})
        want = dict(np.load(path))
        assert int(want["forms"]) & 1 == forms & 1
    solo = None if want is not None else _solo(gcrl, _cfgs(*shape), list(range(seed0, seed0 + P)))
    steps = 0
    for c, (step0, n) in enumerate(calls):
        got = pop.update_many(step0, n) if n > 1 else [[t] for t in pop.update(step0)]
        steps += n
        for i in range(P):
            g, gl = tps._tuples(got[i])
            if solo is not None:
                w, wl = tps._tuples(solo[i].update_many(step0, n) if n > 1 else [solo[i].update(step0)])
            else:
                w, wl = want[f"t_{c}_{i}"], list(want[f"l_{c}_{i}"])
            assert gl == wl and set(gl) <= {6, 9}, (i, step0, gl, wl)
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (i, step0, g, w)
    for i, m in enumerate(pop.members):
        ws = tps._state(solo[i]) if solo is not None else want[f"s_{i}"]
        wn = int(solo[i].actor.num_batches_tracked) if solo is not None else int(want[f"nb_{i}"])
        assert np.array_equal(tps._state(m), ws), f"member {i}: engine state differs from the standalone agent"
        assert int(m.actor.num_batches_tracked) == wn, i
    merged, alone = pop.launch_counts()
    print("launch positions merged", merged, "alone", alone, "steps", steps)
    if P >= 2:
        assert merged > 0 and alone == ALONE_PER_STEP * steps, (merged, alone, steps)
    else:
        assert merged == 0 and alone > 0, (merged, alone)
    return want is not None


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bitwise_and_launch_counts(gcrl, name, tmp_path):
    _bitwise_case(gcrl, SHAPES[name], 21, tmp=tmp_path)


def test_one_member_population_is_bitwise_and_alone(gcrl, tmp_path):
    _bitwise_case(gcrl, (1, 64, 64, 5, 2), 31, tmp=tmp_path)


def test_row_split_shape_bitwise(gcrl, tmp_path):
    """B 256: the slab launches split their rows over row groups that exchange column partials, and the top layer's backward slab launch
    carries the sampling backward (the folded form, without SAC's selection rider): 2 members x 4 slabs x 4 row groups x 2 inputs = 64
    workgroups, resident at once on any device the suite runs on"""
    _bitwise_case(gcrl, (2, 64, 256, 5, 2), 41, calls=[(1, 8), (9, 1)], tmp=tmp_path, row_split=True)


def test_no_waits_population_against_twins_without_the_forms(gcrl, monkeypatch, tmp_path):
    """GCRL_POP_NO_WAITS=1 at creation: forms() is 0; where a standalone agent would run the row split (B 256) the twins run in a child
    process without it"""
    monkeypatch.setenv("GCRL_POP_NO_WAITS", "1")
    for shape in (SHAPES["h64_b64"], (2, 64, 256, 5, 2)):
        crossed = _bitwise_case(gcrl, shape, 51, calls=[(1, 8), (9, 1)], tmp=tmp_path)
        if shape[2] > 128:
            assert crossed or tps._shared()


def test_python_rng_matches_member_order(gcrl):
    shape = SHAPES["h64_b64"]
    cfgs = _cfgs(*shape)
    random.seed(1234)
    pop = _pop(gcrl, cfgs, [101, 102], rng="python")
    random.seed(1234)
    solo = _solo(gcrl, cfgs, [101, 102], rng="python")
    for step0, n in CALLS:
        random.seed(99 + step0)
        got = pop.update_many(step0, n)
        st_pop = random.getstate()
        random.seed(99 + step0)
        want = [a.update_many(step0, n) for a in solo]
        assert st_pop == random.getstate()
        for i in range(len(solo)):
            tps._same(got[i], want[i], (i, step0))
    for i in range(len(solo)):
        assert np.array_equal(tps._state(pop.members[i]), tps._state(solo[i])), i


def test_members_stay_ordinary_agents(gcrl):
    """a member's own update(step) between two population calls: the twin's bits"""
    shape = SHAPES["h32_b96"]
    cfgs = _cfgs(*shape)
    pop, solo = _pop(gcrl, cfgs, [61, 62, 63]), _solo(gcrl, cfgs, [61, 62, 63])
    for i, (g, a) in enumerate(zip(pop.update_many(1, 8), solo)):
        tps._same(g, a.update_many(1, 8), i)
    tps._same([pop.members[1].update(9)], [solo[1].update(9)], "member 1 alone")
    tps._same([pop.members[1].update(10)], [solo[1].update(10)], "member 1 alone")
    got = pop.update_many(11, 5)
    for i, a in enumerate(solo):
        tps._same(got[i], a.update_many(11, 5), i)
        assert np.array_equal(tps._state(pop.members[i]), tps._state(a)), i


def test_acting(gcrl):
    """pop.observe_act for 8 envs: with the threshold lowered ONE population launch per call, by default the members' own one-launch
    entries in member order — either way each member's own observe_act actions bit for bit"""
    import torch
    import test_gpu_acting_bn as tab
    import test_gpu_population_acting as tpa
    sh = tpa.CFG1
    P, H, B, nc, drop = SHAPES["h64_b64"]
    cfgs = _cfgs(P, H, B, nc, drop)
    pop = gcrl.TQCPopulation(S, A, cfgs, tpa.NENVS, GSTEP, rng="engine", seeds=[71, 72])
    solo = [gcrl.TQCAgent(S, A, c, None, nenvs=tpa.NENVS, gradient_step=GSTEP, rng="engine", seed=s) for c, s in zip(cfgs, [71, 72])]
    for i in range(P):
        for ag in (pop.members[i], solo[i]):
            tpa._normalizers(gcrl, ag, sh, i)
            tab.scramble(ag, 40 + i)

    def act(step, **kw):
        rows = [tpa._rows(step, i, sh) for i in range(P)]
        obs, dg = [r[0]["observation"] for r in rows], [r[0]["desired_goal"] for r in rows]
        torch.manual_seed(7000 + step)
        got = pop.observe_act(obs, dg, **kw)
        st_pop = torch.get_rng_state()
        torch.manual_seed(7000 + step)
        want = [a.observe_act(o, g, **kw) for a, o, g in zip(solo, obs, dg)]
        assert torch.equal(st_pop, torch.get_rng_state()), "torch's host generator consumed differently"
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype == np.float64 and g.shape == (tpa.NENVS, A), (i, g.dtype, g.shape)
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (step, i, np.abs(g - w).max())

    # default threshold: member by member — P launches of the members' own entry per call, none of the population's
    own = lambda: sum(m.acting_counts()["launches"] for m in pop.members)
    before = own()
    act(0)
    act(1, eval_action=True)
    assert own() - before == 2 * P and pop.acting_counts()[:2] == (0, 0), (own() - before, pop.acting_counts())
    # lowered: one population launch per call
    pop.MERGE_ACTING_FROM = 2
    before = own()
    act(2)
    act(3, eval_action=True)
    assert own() == before and pop.acting_counts()[:2] == (2, 2) and pop.acting_counts()[4] == 0, pop.acting_counts()


def test_engine_refuses_row_chain_acting_entry(gcrl):
    """gcrl_pop_observe_act builds its table from the row-chain actor, which a BatchNorm actor does not have: GCRL_ERR_ARG naming kind"""
    from gcrl_amd import _ffi
    pop = gcrl.TQCPopulation(S, A, _cfgs(*SHAPES["h64_b64"]), 2, GSTEP, rng="engine", seeds=[1, 2])
    obs = np.zeros((2, 1, 7), np.float32)
    dg = np.zeros((2, 1, 3), np.float32)
    modes = np.zeros(2, np.int32)
    out = np.full((2, 1, 3), 7.0, np.float64)
    rc = _ffi.lib.gcrl_pop_observe_act(pop._pop.h, None, None, C.c_void_p(obs.ctypes.data), 7, C.c_void_p(dg.ctypes.data), 3, 1, None,
                                       C.c_void_p(modes.ctypes.data), C.c_void_p(out.ctypes.data), None)
    assert rc == _ffi.GCRL_ERR_ARG and "kind" in _ffi.last_error(), (rc, _ffi.last_error())
    assert np.all(out == 7.0)
