"""GPU (-m gpu): DDPG populations (src/population.py, csrc/agent_pop.inc) — P agents whose update steps share launches — held to
BITWISE equality with standalone `DDPG` agents given the same config, seed, ring contents and calls: the engine state of every
member (parameters, targets, Adam moments, schedules, counters: gcrl_agent_save_state) and every metric tuple."""
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


def _cfgs(P, H, B, L=3):
    """members that differ in learning rates, gamma, tau and grad_clip (member 1: no clipping)"""
    out = []
    for i in range(P):
        out.append(make_config("DDPG", hidden_dim=H, layer_count=L, batch_size=B, max_len=4000,
                               actor_lr=1e-3 * (1 + 0.25 * i), actor_lr_min=2e-4, ac_scheduler_steps=30 + i,
                               critic_lr=1e-3 * (1 + 0.5 * i), critic_lr_min=3e-4, cr_scheduler_steps=25 + 2 * i,
                               gamma=0.98 - 0.01 * (i % 3), tau=0.05 + 0.01 * i, grad_clip=None if i == 1 else 1.0 + i))
    return out


def _fill(ag, S, A, i):
    gen = np.random.default_rng(100 + i)          # each member its own episodes
    for ep in range(4 if ag.batch_size <= 64 else 8):
        for st in her_oracle.synthetic_episode(gen, 50, S, A):
            ag.push_her(ep % 2, *st)
    gen2 = np.random.default_rng(200 + i)
    for v in (ag.actor, ag.critic):
        v.set_flat((v.flat() + 0.05 * gen2.standard_normal(v.numel())).astype(np.float32))
    ag.update_target_network()


def _state(ag):
    from gcrl_amd._ffi import check, lib
    n = int(lib.gcrl_agent_state_size(ag._h))
    blob = np.empty(n, np.uint8)
    check(lib.gcrl_agent_save_state(ag._h, blob.ctypes.data, n))
    return blob


def _tuples(ts):
    return np.array([[float(x) for x in t] for t in ts], np.float64)


def _pop(gcrl, S, A, cfgs, gstep, seeds, rng="engine"):
    pop = gcrl.DDPGPopulation(S, A, cfgs, 2, gstep, rng=rng, seeds=seeds)
    for i, m in enumerate(pop.members):
        _fill(m, S, A, i)
    return pop


def _solo(gcrl, S, A, cfgs, gstep, seeds, rng="engine"):
    solo = [gcrl.DDPG(S, A, c, None, nenvs=2, gradient_step=gstep, rng=rng, seed=s) for c, s in zip(cfgs, seeds)]
    for i, a in enumerate(solo):
        _fill(a, S, A, i)
    return solo


def _pair(gcrl, S, A, cfgs, gstep, seeds):
    return _pop(gcrl, S, A, cfgs, gstep, seeds), _solo(gcrl, S, A, cfgs, gstep, seeds)


def _run_and_compare(pop, solo, calls):
    for step0, n in calls:
        got = pop.update_many(step0, n)
        want = [a.update_many(step0, n) for a in solo]
        for i in range(len(solo)):
            g, w = _tuples(got[i]), _tuples(want[i])
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (i, step0, g, w)
    for i, (m, a) in enumerate(zip(pop.members, solo)):
        assert np.array_equal(_state(m), _state(a)), f"member {i}: engine state differs from the standalone agent"


def test_three_members_bitwise(gcrl):
    S, A = 10, 3
    pop, solo = _pair(gcrl, S, A, _cfgs(3, 64, 64), 8, [21, 22, 23])
    assert len(pop) == 3
    _run_and_compare(pop, solo, [(1, 8), (9, 8), (17, 8)])


@pytest.mark.parametrize("S,A,H,P", [(10, 3, 64, 8), (23, 4, 256, 4)])
def test_full_shapes_bitwise(gcrl, S, A, H, P):
    gstep = 40                     # a Polyak step (step % 40 == 0) at the end of each call
    pop, solo = _pair(gcrl, S, A, _cfgs(P, H, 256), gstep, list(range(31, 31 + P)))
    _run_and_compare(pop, solo, [(1, gstep), (gstep + 1, gstep)])


def test_calls_that_start_on_a_polyak_step_bitwise(gcrl):
    """A call whose FIRST step is a Polyak step (step % 40 == 0) takes the per-step path, which rebuilds the target actor's
    [in][out] copy in a launch of its own: that launch has to go through the population's recorder like the Polyak launch in
    front of it (it did not: gcrl_pop_update_n refused such a call, `pop.update(40)` included)."""
    pop, solo = _pair(gcrl, 10, 3, _cfgs(3, 64, 64), 8, [91, 92, 93])
    _run_and_compare(pop, solo, [(38, 2), (40, 1), (41, 3), (80, 4)])
    assert len(pop.update(120)) == 3


def test_single_member_is_standalone(gcrl):
    pop, solo = _pair(gcrl, 10, 3, _cfgs(1, 64, 64), 8, [5])
    _run_and_compare(pop, solo, [(1, 8), (9, 8)])
    assert len(pop.update(17)) == 1


def test_meetings_off_bitwise(gcrl):
    pop, solo = _pair(gcrl, 10, 3, _cfgs(3, 64, 64), 8, [41, 42, 43])
    for m in pop.members:
        m.set_meetings(False)
    assert all(m.meetings() & (2 | 8) == 0 for m in pop.members)
    _run_and_compare(pop, solo, [(1, 8), (9, 8)])


def test_shared_gpu_child_bitwise():
    """GCRL_SHARED_GPU=1 (process-wide: no launch form with waits) in a fresh child process"""
    env = dict(os.environ, GCRL_SHARED_GPU="1")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import gcrl_amd, test_gpu_population as t\n"
            "pop, solo = t._pair(gcrl_amd, 10, 3, t._cfgs(3, 64, 64), 8, [51, 52, 53])\n"
            "assert all(m.meetings() & (2 | 8) == 0 for m in pop.members)\n"
            "t._run_and_compare(pop, solo, [(1, 8), (9, 8)])\nprint('child ok')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_members_are_independent(gcrl):
    S, A = 10, 3
    base = _cfgs(3, 64, 64)
    other = _cfgs(3, 64, 64)
    other[1].actor_lr *= 3.0
    other[1].critic_lr *= 0.5
    pa = gcrl.DDPGPopulation(S, A, base, 2, 8, rng="engine", seeds=[61, 62, 63])
    pb = gcrl.DDPGPopulation(S, A, other, 2, 8, rng="engine", seeds=[61, 62, 63])
    for i in range(3):
        _fill(pa.members[i], S, A, i)
        _fill(pb.members[i], S, A, i)
    for step0 in (1, 9):
        pa.update_many(step0, 8)
        pb.update_many(step0, 8)
    for i in (0, 2):
        assert np.array_equal(_state(pa.members[i]), _state(pb.members[i])), i
    assert not np.array_equal(_state(pa.members[1]), _state(pb.members[1]))


def test_resume_member_into_standalone(gcrl, tmp_path):
    S, A = 10, 3
    cfgs = _cfgs(3, 64, 64)
    pop, solo = _pair(gcrl, S, A, cfgs, 8, [71, 72, 73])
    pop.update_many(1, 8)
    pop.members[2].save_state(str(tmp_path / "m2"))
    resumed = gcrl.DDPG(S, A, cfgs[2], None, nenvs=2, gradient_step=8, rng="engine", seed=73)
    resumed.load_state(str(tmp_path / "m2"))
    got = pop.update_many(9, 8)[2]
    want = resumed.update_many(9, 8)
    assert np.array_equal(_tuples(got).view(np.uint64), _tuples(want).view(np.uint64))
    assert np.array_equal(_state(pop.members[2]), _state(resumed))


def test_python_rng_matches_member_order(gcrl):
    S, A = 10, 3
    cfgs = _cfgs(3, 64, 64)
    random.seed(1234)
    pop = _pop(gcrl, S, A, cfgs, 8, [81, 82, 83], rng="python")
    random.seed(1234)
    solo = _solo(gcrl, S, A, cfgs, 8, [81, 82, 83], rng="python")
    random.seed(99)
    got = pop.update_many(1, 8)
    st_pop = random.getstate()
    random.seed(99)
    want = [a.update_many(1, 8) for a in solo]
    st_solo = random.getstate()
    assert st_pop == st_solo
    for i in range(3):
        assert np.array_equal(_tuples(got[i]).view(np.uint64), _tuples(want[i]).view(np.uint64)), i
        assert np.array_equal(_state(pop.members[i]), _state(solo[i])), i
