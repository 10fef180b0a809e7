"""GPU (-m gpu): TD3 populations (src/population.py TD3Population, csrc/agent_pop.inc) — P TD3 agents whose update steps share
launches — held to BITWISE equality with standalone `TD3Agent`s given the same config, seed, ring contents and calls: the engine
state of every member (parameters, targets, Adam moments, schedules, counters, the device noise stream: gcrl_agent_save_state)
and every metric tuple (8 entries on actor steps, 6 on critic-only steps)."""
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


def _cfgs(P, H, B, L=3, freq=2):
    """target smoothing on, the actor stepped every second step; members that differ in learning rates and their schedules,
    gamma, tau and grad_clip (member 1: no clipping)"""
    out = []
    for i in range(P):
        out.append(make_config("TD3", hidden_dim=H, layer_count=L, batch_size=B, max_len=4000, ac_update_freq=freq,
                               policy_noise=0.2, noise_clamp=0.5,
                               actor_lr=1e-3 * (1 + 0.25 * i), actor_lr_min=2e-4, ac_scheduler_steps=30 + i,
                               critic_lr=1e-3 * (1 + 0.5 * i), critic_lr_min=3e-4, cr_scheduler_steps=25 + 2 * i,
                               gamma=0.98 - 0.01 * (i % 3), tau=0.05 + 0.01 * i, grad_clip=None if i == 1 else 1.0 + i))
    return out


def _fill(ag, S, A, i):
    gen = np.random.default_rng(300 + i)          # each member its own episodes
    for ep in range(4 if ag.batch_size <= 64 else 8):
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
    assert all(len(t) in (6, 8) for t in ts), [len(t) for t in ts]
    w = max(len(t) for t in ts)
    return np.array([[float(x) for x in t] + [0.0] * (w - len(t)) for t in ts], np.float64), [len(t) for t in ts]


def _pop(gcrl, S, A, cfgs, gstep, seeds, rng="engine"):
    pop = gcrl.TD3Population(S, A, cfgs, 2, gstep, rng=rng, seeds=seeds)
    for i, m in enumerate(pop.members):
        assert isinstance(m, gcrl.TD3Agent)
        _fill(m, S, A, i)
    return pop


def _solo(gcrl, S, A, cfgs, gstep, seeds, rng="engine"):
    solo = [gcrl.TD3Agent(S, A, c, None, nenvs=2, gradient_step=gstep, rng=rng, seed=s) for c, s in zip(cfgs, seeds)]
    for i, a in enumerate(solo):
        _fill(a, S, A, i)
    return solo


def _pair(gcrl, S, A, cfgs, gstep, seeds):
    return _pop(gcrl, S, A, cfgs, gstep, seeds), _solo(gcrl, S, A, cfgs, gstep, seeds)


def _same(got, want, what):
    (g, gl), (w, wl) = _tuples(got), _tuples(want)
    assert gl == wl, (what, gl, wl)
    assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, g, w)


def _run_and_compare(pop, solo, calls):
    for step0, n in calls:
        got = pop.update_many(step0, n)
        want = [a.update_many(step0, n) for a in solo]
        for i in range(len(solo)):
            _same(got[i], want[i], (i, step0))
    for i, (m, a) in enumerate(zip(pop.members, solo)):
        assert np.array_equal(_state(m), _state(a)), f"member {i}: engine state differs from the standalone agent"


# odd first steps and odd call lengths: actor and critic-only steps fall differently in every call
CALLS_SMALL = [(1, 7), (8, 5), (13, 8)]


@pytest.mark.parametrize("P", [1, 3, 4, 8])
def test_h64_bitwise(gcrl, P):
    S, A = 10, 3
    pop, solo = _pair(gcrl, S, A, _cfgs(P, 64, 64), 8, list(range(21, 21 + P)))
    assert len(pop) == P
    _run_and_compare(pop, solo, CALLS_SMALL)


@pytest.mark.parametrize("P", [1, 3, 4, 8])
def test_full_shape_bitwise(gcrl, P):
    """S 23 / A 4 / H 256 / B 256 (the headline shapes)"""
    S, A, gstep = 23, 4, 40
    pop, solo = _pair(gcrl, S, A, _cfgs(P, 256, 256), gstep, list(range(31, 31 + P)))
    _run_and_compare(pop, solo, [(1, 39), (40, 21)])


def test_single_step_update(gcrl):
    pop, solo = _pair(gcrl, 10, 3, _cfgs(3, 64, 64), 8, [5, 6, 7])
    for step in (1, 2, 3):
        got = pop.update(step)
        want = [a.update_many(step, 1)[0] for a in solo]
        for i in range(3):
            _same([got[i]], [want[i]], (i, step))
    for i, (m, a) in enumerate(zip(pop.members, solo)):
        assert np.array_equal(_state(m), _state(a)), i


def test_meetings_off_bitwise(gcrl):
    pop, solo = _pair(gcrl, 10, 3, _cfgs(3, 64, 64), 8, [41, 42, 43])
    for m in pop.members:
        m.set_meetings(False)
    assert all(m.meetings() & (2 | 8) == 0 for m in pop.members)
    _run_and_compare(pop, solo, CALLS_SMALL)


def test_shared_gpu_child_bitwise():
    """GCRL_SHARED_GPU=1 (process-wide: no launch form with waits) in a fresh child process"""
    env = dict(os.environ, GCRL_SHARED_GPU="1")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import gcrl_amd, test_gpu_population_td3 as t\n"
            "pop, solo = t._pair(gcrl_amd, 10, 3, t._cfgs(3, 64, 64), 8, [51, 52, 53])\n"
            "assert all(m.meetings() & (2 | 8) == 0 for m in pop.members)\n"
            "t._run_and_compare(pop, solo, t.CALLS_SMALL)\nprint('child ok')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_members_are_independent(gcrl):
    S, A = 10, 3
    base = _cfgs(3, 64, 64)
    other = _cfgs(3, 64, 64)
    other[1].actor_lr *= 3.0
    other[1].critic_lr *= 0.5
    pa = gcrl.TD3Population(S, A, base, 2, 8, rng="engine", seeds=[61, 62, 63])
    pb = gcrl.TD3Population(S, A, other, 2, 8, rng="engine", seeds=[61, 62, 63])
    for i in range(3):
        _fill(pa.members[i], S, A, i)
        _fill(pb.members[i], S, A, i)
    for step0, n in CALLS_SMALL:
        pa.update_many(step0, n)
        pb.update_many(step0, n)
    for i in (0, 2):
        assert np.array_equal(_state(pa.members[i]), _state(pb.members[i])), i
    assert not np.array_equal(_state(pa.members[1]), _state(pb.members[1]))


def test_resume_member_into_standalone(gcrl, tmp_path):
    S, A = 10, 3
    cfgs = _cfgs(3, 64, 64)
    pop, _ = _pair(gcrl, S, A, cfgs, 8, [71, 72, 73])
    pop.update_many(1, 7)
    pop.members[2].save_state(str(tmp_path / "m2"))
    resumed = gcrl.TD3Agent(S, A, cfgs[2], None, nenvs=2, gradient_step=8, rng="engine", seed=73)
    resumed.load_state(str(tmp_path / "m2"))
    got = pop.update_many(8, 5)[2]
    want = resumed.update_many(8, 5)
    _same(got, want, "resumed")
    assert np.array_equal(_state(pop.members[2]), _state(resumed))


def test_python_rng_matches_member_order(gcrl):
    S, A = 10, 3
    cfgs = _cfgs(3, 64, 64)
    random.seed(1234)
    pop = _pop(gcrl, S, A, cfgs, 8, [81, 82, 83], rng="python")
    random.seed(1234)
    solo = _solo(gcrl, S, A, cfgs, 8, [81, 82, 83], rng="python")
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
