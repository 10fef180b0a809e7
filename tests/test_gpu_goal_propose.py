"""GPU (-m gpu): practice goals (csrc/goal_propose.hip, gcrl_amd.GoalProposer, agent.collect(practice=...)) held bit for bit to their
definition, tests/goal_propose_ref.py.  Every comparison is np.array_equal on bit views.

  (a) proposer.step against the definition after every one of 3 T + 2 steps under random clipped actions, at the four shapes of
      tests/goal_propose_cases.py (tests/test_goal_propose_ref.py asserts on the CPU that they reach ties, winners k > 0, declining
      envs, a wrapped archive);
  (b) archive lengths around the tile the kernel stages (read from the handle), pre-loaded through load_state on a grid on which
      squared distances equal radius^2 exactly, the live range wrapping around the end of the allocation;
  (c) desynchronised envs: a masked reset is not a roll-over;
  (d) collect(practice=p) == the host loop observe_act -> numpy env -> definition -> process_step; 0 copies, 0 syncs, and
      4 launches a step plus flushes plus one per roll-over step;
  (e) collect without the keyword: the same rows and 3 launches a step plus flushes;
  (f) a bitwise resume; (g) refusals name their field and consume nothing.

The collect tests run at the horizon 50, not 4: the collect entries refuse an env whose max_steps differs from the replay ring's
flush length, the literal 50 of the rings the agents build (as tests/test_gpu_collect_glide.py notes); they run 2 T + 3 steps, two
roll-overs, where the shapes of (a) cover the short horizons.  No case provokes a fault."""
import numpy as np
import pytest
import torch

import dev_env_ref as E
import goal_propose_cases as K
import goal_propose_ref as R
import test_gpu_collect as TC
import test_gpu_her_relabel as T0

pytestmark = pytest.mark.gpu

f32 = np.float32
bits = T0.bits
T, THR = TC.T, TC.THR
ENV_HEADER = 40                  # bytes ahead of the state words in DeviceGoalEnv.save_state()
PS = dict(capacity=128, candidates=8, radius=0.05, share=0.5, min_fill=30)      # the collect tests' proposer: 3 envs wrap it in 43 steps
OBS = {"reach": 7, "glide": 16}


def _state_words(env):
    n = env.num_envs
    blob = env.save_state()
    sw = (12, 12, 18, 15)[("reach", "push", "pick", "glide").index(env.kind)]
    return blob[ENV_HEADER:ENV_HEADER + n * sw * 4].view(f32).reshape(n, sw)


def _same(env, ref, p, rp, what):
    assert (p.head, p.len, p.counter) == (rp.head, rp.len, rp.q), (what, "head / len / q")
    assert np.array_equal(bits(p.archive()), bits(rp.logical())), (what, "archive")
    assert p.stats() == rp.stats(), what
    assert np.array_equal(bits(_state_words(env)), bits(R.state_words(ref))), (what, "env state")
    assert np.array_equal(bits(env.acting_rows()["rows"].cpu().numpy()), bits(ref.rows)), (what, "acting rows")


def _step_both(env, ref, p, rp, act):
    env.step(torch.from_numpy(act).cuda())
    p.step(env)
    rp.step_env(ref, act)


# ---------------------------------------------------------------- (a) proposer.step against the definition
@pytest.mark.parametrize("kind", ["reach", "push", "glide", "pick"])
def test_step_is_the_definition(gcrl, kind):
    case = K.CASES[kind]
    env = gcrl.DeviceGoalEnv(kind, case["N"], seed=K.ENV_SEED, max_steps=case["T"], threshold=K.THR)
    ref = K.ref_env(kind, case["N"], K.ENV_SEED, case["T"])
    p, rp = gcrl.GoalProposer(seed=K.PROP_SEED, **K.settings(case)), R.RefProposer(seed=K.PROP_SEED, **K.settings(case))
    for s, act in enumerate(K.actions(kind, case)):
        _step_both(env, ref, p, rp, act)
        _same(env, ref, p, rp, (kind, s))
    assert p.num_envs == case["N"] and rp.patched > 0 and rp.q == (3 * case["T"] + 2) // case["T"]
    assert env.stats() == ref.stats()


# ---------------------------------------------------------------- (b) archive lengths around the tile
def _preload(p, rp, arch, head, n):
    from gcrl_amd.src.goal_propose import STATE_HEADER
    blob = p.save_state()
    hdr = blob[:STATE_HEADER.itemsize].view(STATE_HEADER)
    assert int(hdr["capacity"][0]) == arch.shape[0] and blob.size == STATE_HEADER.itemsize + arch.size * 4
    hdr["head"], hdr["len"] = head, n
    blob[STATE_HEADER.itemsize:].view(f32)[:] = arch.reshape(-1)
    p.load_state(blob)
    rp.arch[:] = arch
    rp.head, rp.len = head, n


def test_archive_lengths_around_the_tile(gcrl):
    tile = gcrl.GoalProposer(64, min_fill=1).tile
    assert tile >= 64 and tile % 4 == 0
    cap = K.grid_capacity(tile)
    for L in K.grid_lengths(tile):
        arch, head, n = K.grid_archive(L, tile)
        st = dict(capacity=cap, candidates=K.GRID_C, radius=K.GRID_RADIUS, share=1.0, min_fill=1, seed=L)
        p, rp = gcrl.GoalProposer(**st), R.RefProposer(**st)
        _preload(p, rp, arch, head, n)
        assert (p.head, p.len) == (head, n) and np.array_equal(bits(p.archive()), bits(rp.logical()))
        env, ref = gcrl.DeviceGoalEnv("reach", 1, seed=L, max_steps=1, threshold=THR), E.RefEnv("reach", 1, seed=L, max_steps=1, threshold=THR)
        _step_both(env, ref, p, rp, np.zeros((1, 3), f32))          # T = 1: every step rolls over
        assert rp.len == L and len(rp.last) == 1 and rp.last[0]["took"]
        _same(env, ref, p, rp, ("L", L))
        assert np.array_equal(bits(ref.goal[0]), bits(rp.logical()[rp.last[0]["js"][rp.last[0]["best"]]]))


# ---------------------------------------------------------------- (c) desynchronised envs
def test_a_masked_reset_is_not_a_roll_over(gcrl):
    st = dict(capacity=64, candidates=4, radius=0.05, share=1.0, min_fill=1, seed=5)
    p, rp = gcrl.GoalProposer(**st), R.RefProposer(**st)
    env, ref, twin = gcrl.DeviceGoalEnv("reach", 5, seed=6, max_steps=4, threshold=THR), *(E.RefEnv("reach", 5, seed=6, max_steps=4, threshold=THR) for _ in range(2))
    gen = np.random.default_rng(1)
    mask = np.array([0, 1, 0, 1, 0], bool)
    for s in range(7):
        if s == 2:
            env.reset(mask); ref.reset(mask); twin.reset(mask)
        act = gen.uniform(-1, 1, (5, 3)).astype(f32)
        _step_both(env, ref, p, rp, act)
        twin.step(act)
        _same(env, ref, p, rp, ("desync", s))
        assert [r["env"] for r in rp.last] == {3: [0, 2, 4], 5: [1, 3]}.get(s, [])
        if s == 3:   # the envs whose t ran out are patched, the reset ones carry their task goals
            goals = env.acting_rows()["desired_goal"].cpu().numpy()
            assert np.array_equal(bits(goals[mask]), bits(twin.goal[mask])) and not np.array_equal(bits(goals[~mask]), bits(twin.goal[~mask]))
    assert p.counter == 2 and p.stats()["patched"] == 5


# ---------------------------------------------------------------- (d) collect(practice=p) against the host loop
class _Practised:
    """a numpy env whose step is followed by the definition's proposer step: what TC._host_loop drives"""

    def __init__(self, ref, rp):
        self.ref, self.rp = ref, rp

    def __getattr__(self, name):
        return getattr(self.ref, name)

    def step(self, act):
        return self.rp.step_env(self.ref, act)


def _flushes(gcrl, ag):
    return int(gcrl._ffi.lib.gcrl_her_flush_calls(ag.buffer.handle))


@pytest.mark.parametrize("kind", ["DDPG", "SAC"])
@pytest.mark.parametrize("env_kind", ["reach", "glide"])
@pytest.mark.parametrize("relabel,rng", [("push", "engine"), ("sample", "device")])
def test_collect_practice_is_the_host_loop(gcrl, kind, env_kind, relabel, rng):
    steps, n, first = 2 * T + 3, 3, 7
    seed = TC._pick_seed(steps)
    a, b = (TC._agent(gcrl, kind, seed=seed, nenvs=n, state_dim=OBS[env_kind] + 3, relabel=relabel, rng=rng) for _ in range(2))
    env, ref = gcrl.DeviceGoalEnv(env_kind, n, seed=9, max_steps=T, threshold=THR), K.ref_env(env_kind, n, 9, T)
    p, rp = gcrl.GoalProposer(seed=3, **PS), R.RefProposer(seed=3, **PS)
    rows_a = a.collect(env, first, practice=p)            # a first call: allocation, the first step's noise fill, the weight copies
    c0, f0, r0 = a.collect_counts(), _flushes(gcrl, a), p.stats()["roll_steps"]
    rows_a += a.collect(env, steps - first, practice=p)
    c1, f1, r1 = a.collect_counts(), _flushes(gcrl, a), p.stats()["roll_steps"]
    rows_b = TC._host_loop(gcrl, b, _Practised(ref, rp), steps, True, 0)
    assert rows_a == rows_b > 0
    TC._compare(a, b, env, ref, "practice")
    _same(env, ref, p, rp, "practice")
    assert rp.q == 2 and rp.patched > 0 and rp.head != 0
    K_ = steps - first
    assert r1 - r0 == 2 and f1 - f0 >= 1
    assert c1["steps"] - c0["steps"] == K_ and c1["launches"] - c0["launches"] == 4 * K_ + (f1 - f0) + (r1 - r0)
    assert c1["copies"] == 0 and c1["syncs"] == 0
    # evaluation never appends and never proposes
    before = p.save_state().tobytes()
    a.evaluate(env, n)
    assert p.save_state().tobytes() == before


# ---------------------------------------------------------------- (e) collect without the keyword
@pytest.mark.parametrize("kind", ["DDPG", "SAC"])
def test_collect_without_the_keyword_is_unchanged(gcrl, kind):
    a, b = (TC._agent(gcrl, kind, nenvs=5) for _ in range(2))
    env, tenv = (gcrl.DeviceGoalEnv("reach", 5, seed=1, max_steps=T, threshold=THR) for _ in range(2))
    assert a.collect(env, 7) == b.collect(tenv, 7, practice=None)
    K_ = T + 5
    for ag, e, kw in ((a, env, {}), (b, tenv, dict(practice=None))):
        c0, f0 = ag.collect_counts(), _flushes(gcrl, ag)
        ag.collect(e, K_, **kw)
        c1, f1 = ag.collect_counts(), _flushes(gcrl, ag)
        assert f1 - f0 >= 1 and c1["launches"] - c0["launches"] == 3 * K_ + (f1 - f0)
        assert c1["copies"] == 0 and c1["syncs"] == 0
    assert TC._snap(a, env) == TC._snap(b, tenv)


# ---------------------------------------------------------------- (f) resume
def test_resume_is_bitwise(gcrl, tmp_path):
    D, G, A = TC.D, TC.G, TC.A
    a = TC._agent(gcrl, "TD3", nenvs=3, relabel="sample", rng="device")
    a.set_collect_stream(seed=1234)
    env, p = gcrl.DeviceGoalEnv("reach", 3, seed=4, max_steps=T, threshold=THR), gcrl.GoalProposer(seed=3, **PS)
    a.collect(env, T + 1, practice=p)
    a.save_state(str(tmp_path / "st"))
    eblob, pblob = env.save_state(), p.save_state()
    assert p.stats()["roll_steps"] == 1 and p.stats()["patched"] >= 0
    b = TC._agent(gcrl, "TD3", nenvs=3, relabel="sample", rng="device")
    b.buffer._ensure(D + G, A, G)
    benv, bp = gcrl.DeviceGoalEnv("reach", 3, seed=123, max_steps=T, threshold=THR), gcrl.GoalProposer(seed=3, **PS)
    b.load_state(str(tmp_path / "st"))
    benv.load_state(eblob)
    bp.load_state(pblob)
    assert np.array_equal(bp.save_state(), pblob) and bp.num_envs == 3
    assert a.collect(env, T + 2, practice=p) == b.collect(benv, T + 2, practice=bp)
    assert p.stats()["roll_steps"] == 2
    assert np.array_equal(env.save_state(), benv.save_state()) and np.array_equal(p.save_state(), bp.save_state()) and TC._same_nz(a, b)
    for u, v in zip(a.buffer.rows() + a.buffer.tails(), b.buffer.rows() + b.buffer.tails()):
        assert np.array_equal(bits(u), bits(v))
    assert np.array_equal(T0._state(a), T0._state(b))


# ---------------------------------------------------------------- (g) refusals
def test_refusals_name_their_field_and_consume_nothing(gcrl):
    from gcrl_amd.src.goal_propose import STATE_HEADER
    err, lib = gcrl._ffi.GcrlError, gcrl._ffi.lib
    dev, twin = (TC._agent(gcrl, "DDPG", nenvs=3) for _ in range(2))
    mk = lambda n=3, seed=2: gcrl.DeviceGoalEnv("reach", n, seed=seed, max_steps=T, threshold=THR)
    env, tenv = mk(), mk()
    p, tp = (gcrl.GoalProposer(seed=3, **PS) for _ in range(2))
    assert dev.collect(env, 5, practice=p) == twin.collect(tenv, 5, practice=tp)
    snap = lambda: (TC._snap(dev, env), p.save_state().tobytes(), tuple(sorted(p.stats().items())))
    before = snap()
    zeros = lambda n: torch.zeros((n, 3), device="cuda")
    other, four = mk(seed=8), mk(n=4)
    other.step(zeros(3)); four.step(zeros(4))
    p2 = gcrl.GoalProposer(seed=3, **PS)
    p2.step(other)                                            # bound to another env
    small = gcrl.GoalProposer(2, 1, 0.05, 1.0, 1)
    group = gcrl.DeviceGoalEnvGroup("reach", 2, 3, [1, 2], max_steps=T, threshold=THR)
    for field, call in [(" env: ", lambda: p.step(other)), (" env: ", lambda: p.step(four)), (" capacity: ", lambda: small.step(env)),
                        ("members", lambda: p.step(group)), ("practice", lambda: dev.collect(env, 3, practice=object())),
                        (" env: ", lambda: dev.collect(env, 3, practice=p2)), (" capacity: ", lambda: dev.collect(env, 3, practice=small)),
                        ("steps", lambda: dev.collect(env, 0, practice=p))]:
        with pytest.raises(ValueError, match=field):
            call()
    assert lib.gcrl_goal_proposer_step(p.handle, group.handle, gcrl._ffi.stream_handle()) == -1 and b" members: " in lib.gcrl_last_error()
    with pytest.raises(err, match=" env: "):                  # the env's last step was taken in already
        p.step(env)
    # blobs of other settings, of another env count, of a head outside the archive
    for field, kw in [("capacity", dict(capacity=64)), ("candidates", dict(candidates=4)), ("radius", dict(radius=0.06)), ("share", dict(share=0.25)),
                      ("min_fill", dict(min_fill=5)), ("seed", dict(seed=4))]:
        with pytest.raises(ValueError, match=f" {field}: "):
            p.load_state(gcrl.GoalProposer(**dict(dict(PS, seed=3), **kw)).save_state())
    p4 = gcrl.GoalProposer(seed=3, **PS)
    p4.step(four)
    with pytest.raises(ValueError, match=" num_envs: "):
        p.load_state(p4.save_state())
    bad = p.save_state()
    bad[:STATE_HEADER.itemsize].view(STATE_HEADER)["head"] = PS["capacity"]
    with pytest.raises(ValueError, match=" head: "):
        p.load_state(bad)
    assert snap() == before, "a refusal consumed something"
    assert dev.collect(env, T, practice=p) == twin.collect(tenv, T, practice=tp)
    assert TC._snap(dev, env) == TC._snap(twin, tenv) and np.array_equal(p.save_state(), tp.save_state())
