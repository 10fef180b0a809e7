"""GPU (-m gpu): SAC populations (src/population.py SACPopulation, csrc/agent_pop.inc) — P SAC agents whose update steps share
launches — held to BITWISE equality with standalone `SACAgent`s given the same config, seed, ring contents and calls: the engine
state of every member (parameters, targets, Adam moments, log_alpha, BatchNorm running statistics, schedules, counters, the device
noise streams: gcrl_agent_save_state) and every metric tuple (9 entries on actor steps, 6 on critic-only steps).

The guarantee is "a standalone agent RUNNING THE SAME FORMS": the row-split BatchNorm slab launches sum a column's statistics in
another order than the one-workgroup launches, and a population admits a form with waits only when its WHOLE grid is resident at
once.  `pop.forms()` must equal the rule recomputed from `pop.forms_terms()`.  The population always runs in the test's own
process under its own admission; its twins run there too when they pick the same slab form, otherwise in a fresh child process
with the switches the population's forms imply (GCRL_NO_BN_RSPLIT / GCRL_NO_RC_MERGE / GCRL_NO_OPT_FUSE), tuples and state blobs
compared across the processes."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import her_oracle
from oracle.agent_oracle import make_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORM_KNOBS = {1: "GCRL_NO_BN_RSPLIT", 2: "GCRL_NO_RC_MERGE", 8: "GCRL_NO_OPT_FUSE"}


def _cfgs(P, H, B, L=3, freq=2):
    """the actor stepped every second step (critic-only steps run one actor forward, actor steps two co-scheduled ones), log-alpha
    steps from the sixth step on; members that differ in learning rates and their schedules, gamma, tau, alpha_lr and grad_clip
    (member 1: no clipping)"""
    out = []
    for i in range(P):
        out.append(make_config("SAC", hidden_dim=H, layer_count=L, batch_size=B, max_len=4000, ac_update_freq=freq,
                               actor_lr=1e-3 * (1 + 0.25 * i), actor_lr_min=2e-4, ac_scheduler_steps=30 + i,
                               critic_lr=1e-3 * (1 + 0.5 * i), critic_lr_min=3e-4, cr_scheduler_steps=25 + 2 * i,
                               alpha_lr=3e-4 * (1 + i), alpha_min_steps=5,
                               gamma=0.98 - 0.01 * (i % 3), tau=0.05 + 0.01 * i, grad_clip=None if i == 1 else 1.0 + i))
    return out


def _fill(ag, S, A, i):
    gen = np.random.default_rng(300 + i)          # each member its own episodes
    for ep in range(4 if ag.batch_size <= 64 else (8 if ag.batch_size <= 256 else 12)):
        for st in her_oracle.synthetic_episode(gen, 50, S, A):
            ag.push_her(ep % 2, *st)
    gen2 = np.random.default_rng(400 + i)
    for v in [ag.actor] + list(ag.critics):
        v.set_flat((v.flat() + 0.05 * gen2.standard_normal(v.numel())).astype(np.float32))
    ag.update_target_network()


def _state(ag):
    from gcrl_amd._ffi import check, lib
    n = int(lib.gcrl_agent_state_size(ag._h))
    blob = np.empty(n, np.uint8)
    check(lib.gcrl_agent_save_state(ag._h, blob.ctypes.data, n))
    return blob


def _tuples(ts):
    assert all(len(t) in (6, 9) for t in ts), [len(t) for t in ts]
    w = max(len(t) for t in ts)
    return np.array([[float(x) for x in t] + [0.0] * (w - len(t)) for t in ts], np.float64), [len(t) for t in ts]


def _pop(gcrl, S, A, cfgs, gstep, seeds, rng="engine"):
    pop = gcrl.SACPopulation(S, A, cfgs, 2, gstep, rng=rng, seeds=seeds)
    for i, m in enumerate(pop.members):
        assert isinstance(m, gcrl.SACAgent)
        _fill(m, S, A, i)
    return pop


def _solo(gcrl, S, A, cfgs, gstep, seeds, rng="engine"):
    solo = [gcrl.SACAgent(S, A, c, None, nenvs=2, gradient_step=gstep, rng=rng, seed=s) for c, s in zip(cfgs, seeds)]
    for i, a in enumerate(solo):
        _fill(a, S, A, i)
    return solo


def _same(got, want, what):
    (g, gl), (w, wl) = _tuples(got), _tuples(want)
    assert gl == wl, (what, gl, wl)
    assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, g, w)


def _shared():
    return os.environ.get("GCRL_SHARED_GPU", "0") not in ("", "0")


def _rule(pop):
    """the admission rule (include/gcrl.h gcrl_pop_forms_terms), recomputed here from its published terms: form f is on
    when every member has it on, the device is not shared, the population was not created with GCRL_POP_NO_WAITS, and — two or more
    members — 0 < want[f] <= capacity[f] (P x a member's workgroups of the form against what is resident at once)"""
    bits = 1 | 2 | 8
    for m in pop.members:
        bits &= m.meetings()
    if _shared() or os.environ.get("GCRL_POP_NO_WAITS"):
        return 0
    if len(pop) > 1:
        for bit, (want, cap) in pop.forms_terms().items():
            if not 0 < want <= cap:
                bits &= ~bit
    return bits


def _twins_run(gcrl, S, A, H, B, P, gstep, seed0, calls, meetings_off=False):
    """standalone twins through the calls: per member the padded tuples of every call, their lengths, and the final state blob"""
    cfgs = _cfgs(P, H, B)
    solo = _solo(gcrl, S, A, cfgs, gstep, list(range(seed0, seed0 + P)))
    if meetings_off:
        for a in solo:
            a.set_meetings(False)
    out = {"forms": np.array(solo[0].meetings() & (1 | 2 | 8))}
    for c, (step0, n) in enumerate(calls):
        for i, a in enumerate(solo):
            t, lens = _tuples(a.update_many(step0, n))
            out[f"t_{c}_{i}"], out[f"l_{c}_{i}"] = t, np.array(lens)
    for i, a in enumerate(solo):
        out[f"s_{i}"] = _state(a)
        out[f"nb_{i}"] = np.array(int(a.actor.num_batches_tracked))
    return out


def _twins_to_file(gcrl, path, *args, **kw):
    np.savez(path, **_twins_run(gcrl, *args, **kw))


def _child(code, env_extra):
    env = dict(os.environ, **env_extra)
    env.pop("GCRL_POP_NO_WAITS", None)
    pre = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport gcrl_amd, test_gpu_population_sac as t\n" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", pre + code + "\nprint('child ok')\n"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def _bitwise_case(gcrl, S, A, H, B, P, gstep, seed0, calls, meetings_off=False, row_split=False, tmp=None):
    """The population runs HERE, under its own admission.  Its twins run here too when a standalone agent of this process picks the
    slab form the population runs; otherwise they run in a fresh child process with the switches that pop.forms() implies
    (GCRL_NO_BN_RSPLIT=1, ...), and the tuples and state blobs are compared across the two processes."""
    args = (S, A, H, B, P, gstep, seed0, calls)
    pop = _pop(gcrl, S, A, _cfgs(P, H, B), gstep, list(range(seed0, seed0 + P)))
    assert len(pop) == P
    if meetings_off:
        for m in pop.members:
            m.set_meetings(False)
    member_forms = pop.members[0].meetings() & (1 | 2 | 8)
    forms = pop.forms()
    print("forms", forms, "members'", member_forms, "terms", pop.forms_terms())
    assert forms == _rule(pop), (forms, _rule(pop), pop.forms_terms())
    if meetings_off or _shared() or os.environ.get("GCRL_POP_NO_WAITS"):
        assert forms == 0, forms
    elif row_split:
        assert forms & 1, (forms, pop.forms_terms())      # the row groups exchange: the row-split population kernels are what runs
    if (member_forms ^ forms) & 1:
        # a standalone agent of this process runs the row-split slab launches, the population does not (the two slab forms differ in bits;
        # the merged chain launch and the fused optimiser compute the same bits as the launches that replace them)
        assert tmp is not None
        path = os.path.join(str(tmp), "twins.npz")
        knobs = {FORM_KNOBS[b]: "1" for b in FORM_KNOBS if (member_forms & b) and not (forms & b)}
        _child("t._twins_to_file(gcrl_amd, %r, *%r, meetings_off=%r)" % (path, args, meetings_off), knobs)
        want = dict(np.load(path))
        assert int(want["forms"]) & 1 == forms & 1
    else:
        want = None
    solo_here = None
    for c, (step0, n) in enumerate(calls):
        got = pop.update_many(step0, n)
        if want is None:
            if solo_here is None:
                solo_here = _solo(gcrl, S, A, _cfgs(P, H, B), gstep, list(range(seed0, seed0 + P)))
                if meetings_off:
                    for a in solo_here:
                        a.set_meetings(False)
            for i, a in enumerate(solo_here):
                _same(got[i], a.update_many(step0, n), (i, step0))
        else:
            for i in range(P):
                g, gl = _tuples(got[i])
                assert gl == list(want[f"l_{c}_{i}"]), (i, step0)
                assert np.array_equal(g.view(np.uint64), want[f"t_{c}_{i}"].view(np.uint64)), (i, step0, g, want[f"t_{c}_{i}"])
    for i, m in enumerate(pop.members):
        ws = _state(solo_here[i]) if want is None else want[f"s_{i}"]
        wn = int(solo_here[i].actor.num_batches_tracked) if want is None else int(want[f"nb_{i}"])
        assert np.array_equal(_state(m), ws), f"member {i}: engine state differs from the standalone agent"
        assert int(m.actor.num_batches_tracked) == wn, i
    merged, alone = pop.launch_counts()
    print("launch positions merged", merged, "alone", alone)
    if P >= 2:
        assert alone == 0 and merged > 0, (merged, alone)     # every recorded position went out as ONE population launch
    else:
        assert merged == 0 and alone > 0, (merged, alone)
    return want is not None


_case = _bitwise_case


# odd first steps and odd call lengths: actor and critic-only steps fall differently in every call
CALLS_SMALL = [(1, 7), (8, 5), (13, 8)]


@pytest.mark.parametrize("P", [1, 2, 3, 4, 8])
def test_h64_b64_bitwise_and_merged(gcrl, P):
    """one row group per slab: no launch with waits between row groups.  For P >= 2 EVERY recorded launch position must go out as
    one population launch (the new kernels are what ran)"""
    _case(gcrl, 10, 3, 64, 64, P, 8, 21, CALLS_SMALL)


@pytest.mark.parametrize("P", [2, 4])
def test_h64_b256_row_split_bitwise(gcrl, P, tmp_path):
    """B 256: the slab launches split their rows over four row groups that exchange column partials (at most 4 members x 4 slabs x 4
    row groups x 2 inputs = 128 workgroups: resident at once on any device of 128 CUs or more)"""
    _case(gcrl, 10, 3, 64, 256, P, 8, 31, CALLS_SMALL, row_split=True, tmp=tmp_path)


def test_h32_b200_ragged_bitwise(gcrl, tmp_path):
    """a ragged last row group (200 = 3 x 64 + 8) and a ragged last chain block; 3 x 2 x 4 x 2 = 48 workgroups"""
    _case(gcrl, 10, 3, 32, 200, 3, 8, 41, CALLS_SMALL, row_split=True, tmp=tmp_path)


def test_cfg5_shapes_bitwise(gcrl, tmp_path):
    """S 28 / A 4 / H 256 / B 512 (the cfg 5 shapes).  pop.forms() must be what the rule gives for P = 2, and the row split must be
    among them: 2 members x 16 slabs x 8 row groups x 2 inputs = 512 workgroups of 256 threads against 4 resident per CU (the forward
    kernel's 104 vector registers of 512 per SIMD lane; 5 KB of LDS) x 256 CUs = 1 024"""
    _case(gcrl, 28, 4, 256, 512, 2, 40, 51, [(1, 9), (10, 6)], row_split=True, tmp=tmp_path)


def test_not_admitted_forms_against_knobbed_twins(gcrl, monkeypatch, tmp_path):
    """The population does not admit what its members would run alone (GCRL_POP_NO_WAITS=1 at its creation stands in for a grid that
    is not resident at once): the members are built with the row split, the merged chain launch and the fused optimiser ON, the update
    call overrides them while recording and restores them — and every member must be bitwise a standalone agent built WITHOUT those
    forms, which runs in a child process with GCRL_NO_BN_RSPLIT / GCRL_NO_RC_MERGE / GCRL_NO_OPT_FUSE set"""
    monkeypatch.setenv("GCRL_POP_NO_WAITS", "1")
    crossed = _bitwise_case(gcrl, 10, 3, 64, 256, 3, 8, 121, CALLS_SMALL, tmp=tmp_path)
    monkeypatch.delenv("GCRL_POP_NO_WAITS")
    probe = gcrl.SACAgent(10, 3, _cfgs(1, 64, 256)[0], None, nenvs=2, gradient_step=8, rng="engine", seed=1)
    assert crossed == bool(probe.meetings() & 1)     # compared across processes wherever a standalone agent runs the row split
    assert crossed or _shared()


def test_single_step_update(gcrl):
    S, A = 10, 3
    cfgs = _cfgs(3, 64, 64)
    pop, solo = _pop(gcrl, S, A, cfgs, 8, [5, 6, 7]), _solo(gcrl, S, A, cfgs, 8, [5, 6, 7])
    for step in (1, 2, 3, 6, 7, 8):
        got = pop.update(step)
        want = [a.update_many(step, 1)[0] for a in solo]
        for i in range(3):
            _same([got[i]], [want[i]], (i, step))
    for i, (m, a) in enumerate(zip(pop.members, solo)):
        assert np.array_equal(_state(m), _state(a)), i


def test_meetings_off_bitwise(gcrl, tmp_path):
    _case(gcrl, 10, 3, 64, 256, 3, 8, 61, CALLS_SMALL, meetings_off=True, tmp=tmp_path)


def test_shared_gpu_child_bitwise():
    """GCRL_SHARED_GPU=1 (process-wide: no launch form with waits) in a fresh child process"""
    _child("assert t._bitwise_case(gcrl_amd, 10, 3, 64, 256, 3, 8, 71, t.CALLS_SMALL) is False", {"GCRL_SHARED_GPU": "1"})


def test_members_are_independent(gcrl):
    S, A = 10, 3
    base = _cfgs(3, 64, 64)
    other = _cfgs(3, 64, 64)
    other[1].actor_lr *= 3.0
    other[1].critic_lr *= 0.5
    other[1].alpha_lr *= 2.0
    pa = _pop(gcrl, S, A, base, 8, [81, 82, 83])
    pb = _pop(gcrl, S, A, other, 8, [81, 82, 83])
    for step0, n in CALLS_SMALL:
        pa.update_many(step0, n)
        pb.update_many(step0, n)
    for i in (0, 2):
        assert np.array_equal(_state(pa.members[i]), _state(pb.members[i])), i
    assert not np.array_equal(_state(pa.members[1]), _state(pb.members[1]))


def test_resume_member_into_standalone(gcrl, tmp_path):
    S, A = 10, 3
    cfgs = _cfgs(3, 64, 64)
    pop = _pop(gcrl, S, A, cfgs, 8, [91, 92, 93])
    pop.update_many(1, 7)
    pop.members[2].save_state(str(tmp_path / "m2"))
    resumed = gcrl.SACAgent(S, A, cfgs[2], None, nenvs=2, gradient_step=8, rng="engine", seed=93)
    resumed.load_state(str(tmp_path / "m2"))
    got = pop.update_many(8, 5)[2]
    want = resumed.update_many(8, 5)
    _same(got, want, "resumed")
    assert np.array_equal(_state(pop.members[2]), _state(resumed))


def test_python_rng_matches_member_order(gcrl):
    S, A = 10, 3
    cfgs = _cfgs(3, 64, 64)
    random.seed(1234)
    pop = _pop(gcrl, S, A, cfgs, 8, [101, 102, 103], rng="python")
    random.seed(1234)
    solo = _solo(gcrl, S, A, cfgs, 8, [101, 102, 103], rng="python")
    random.seed(99)
    got = pop.update_many(1, 7)
    st_pop = random.getstate()
    random.seed(99)
    want = [a.update_many(1, 7) for a in solo]
    st_solo = random.getstate()
    assert st_pop == st_solo
    for i in range(3):
        _same(got[i], want[i], i)
        assert np.array_equal(_state(pop.members[i]), _state(solo[i])), i


def test_acting_matches_members(gcrl):
    """pop.observe_act: the members' own one-launch entries in member order, torch's host generator consumed member after member;
    pop.process_step: the merged launch — for two vector steps"""
    import torch
    import test_gpu_population_acting as tpa
    sh = tpa.CFG1
    P, S = 3, sh["D"] + sh["G"]
    cfgs = _cfgs(P, sh["H"], sh["B"])
    seeds = [111, 112, 113]
    pop = gcrl.SACPopulation(S, sh["A"], cfgs, tpa.NENVS, 8, rng="engine", seeds=seeds)
    solo = [gcrl.SACAgent(S, sh["A"], c, None, nenvs=tpa.NENVS, gradient_step=8, rng="engine", seed=s) for c, s in zip(cfgs, seeds)]
    for i in range(P):
        tpa._normalizers(gcrl, pop.members[i], sh, i)
        tpa._normalizers(gcrl, solo[i], sh, i)
    for step in (1, 2):
        rows = [tpa._rows(step, i, sh) for i in range(P)]
        obs = [r[0]["observation"] for r in rows]
        dg = [r[0]["desired_goal"] for r in rows]
        torch.manual_seed(7000 + step)
        got = pop.observe_act(obs, dg)
        st_pop = torch.get_rng_state()
        torch.manual_seed(7000 + step)
        want = [a.observe_act(o, g) for a, o, g in zip(solo, obs, dg)]
        assert torch.equal(st_pop, torch.get_rng_state()), "torch's host generator consumed differently"
        tpa._same(got, want, f"actions of step {step}")
        tpa._proc(pop, solo, step, rows, got, tpa._dones(step))
    assert pop.acting_counts()[3] == 2          # process_step: one merged launch per call
    tpa._compare_members(pop, solo)


def test_engine_refuses_merged_acting(gcrl):
    """gcrl_pop_observe_act builds its table from the row-chain actor, which a BatchNorm actor does not have: GCRL_ERR_ARG"""
    import ctypes as C
    from gcrl_amd import _ffi
    pop = gcrl.SACPopulation(10, 3, _cfgs(2, 64, 64), 2, 8, rng="engine", seeds=[1, 2])
    obs = np.zeros((2, 1, 7), np.float32)
    dg = np.zeros((2, 1, 3), np.float32)
    modes = np.zeros(2, np.int32)
    out = np.full((2, 1, 3), 7.0, np.float64)
    rc = _ffi.lib.gcrl_pop_observe_act(pop._pop.h, None, None, C.c_void_p(obs.ctypes.data), 7, C.c_void_p(dg.ctypes.data), 3, 1, None,
                                       C.c_void_p(modes.ctypes.data), C.c_void_p(out.ctypes.data), None)
    assert rc == _ffi.GCRL_ERR_ARG and "kind" in _ffi.last_error(), (rc, _ffi.last_error())
    assert np.all(out == 7.0)
