"""GPU (-m gpu): the rest of the drop-in surface the trainer touches:
checkpoint interop with torch modules that have the reference's state_dict keys, select_action,
reset, the compute_reward classification, error behaviour, the device-RNG mode."""
import os
import random

import numpy as np
import pytest
import torch

from oracle import her_oracle
from oracle.agent_oracle import DetActor, GaussActor, OracleAgent, QNet, make_config

pytestmark = pytest.mark.gpu
S, A, H, L = 10, 3, 32, 2


def fill(agent, n_eps=2, seed=0):
    gen = np.random.default_rng(seed)
    for ep in range(n_eps):
        for st in her_oracle.synthetic_episode(gen, 50, S, A):
            agent.push_her(0, *st)


# "TQC-25x2": the distributional variant (n_quantiles = 25, 2 critics, top 2 dropped): Q-wide critic heads in every checkpoint
DISTRIBUTIONAL = dict(n_quantiles=25, num_critics=2, top_quantiles_to_drop=2)


def variant(kind):
    """(agent kind, extra constructor arguments) of a parametrised kind."""
    return ("TQC", DISTRIBUTIONAL) if kind == "TQC-25x2" else (kind, {})


@pytest.mark.parametrize("kind", ["DDPG", "TD3", "SAC", "TQC", "TQC-25x2"])
def test_checkpoints_round_trip_through_torch_modules(gcrl, tmp_path, kind):
    """save_weights() files load with strict=True into torch modules laid out like the reference's
    (src/model.py key names / shapes), and weights saved by those modules load back."""
    kind, kw = variant(kind)
    cfg = make_config(kind, hidden_dim=H, layer_count=L, batch_size=16)
    cls = dict(DDPG=gcrl.DDPG, TD3=gcrl.TD3Agent, SAC=gcrl.SACAgent, TQC=gcrl.TQCAgent)[kind]
    ag = cls(S, A, cfg, None, nenvs=1, gradient_step=2, rng="engine", seed=3, **kw)
    fill(ag)
    for step in (1, 2):
        ag.update(step)          # moves weights, BN statistics, log_alpha away from their init
    ag.save_weights(str(tmp_path))
    actor_mod = (GaussActor if kind in ("SAC", "TQC") else DetActor)(S, H, A, L)
    actor_mod.load_state_dict(torch.load(tmp_path / "actor.pth"), strict=True)
    names = {"DDPG": ["critic.pth"], "TD3": ["critic_1.pth", "critic_2.pth"], "SAC": ["critic_1.pth", "critic_2.pth"],
             "TQC": [f"critic_{i}.pth" for i in range(kw.get("num_critics", 5))]}[kind]
    assert len(names) == len(ag.critics)
    for i, fn in enumerate(names):
        if kw:      # the reference's Critic with a Q-wide head (oracle/quantile_tqc_oracle.py): same keys, the head [Q, H]
            from oracle.quantile_tqc_oracle import QuantileNet
            q = QuantileNet(S + A, H, L, kw["n_quantiles"])
        else:
            q = QNet(S + A, H, L)
        q.load_state_dict(torch.load(tmp_path / fn), strict=True)
        flat = np.concatenate([p.detach().numpy().reshape(-1) for p in q.parameters()])
        assert np.array_equal(flat, ag.critics[i].flat())
    flat = np.concatenate([p.detach().numpy().reshape(-1) for p in actor_mod.parameters()])
    assert np.array_equal(flat, ag.actor.flat())
    if kind in ("SAC", "TQC"):
        assert os.path.exists(tmp_path / "log_alpha.pth")
        bn = [m for m in actor_mod.base_net if isinstance(m, torch.nn.BatchNorm1d)]
        assert not torch.equal(bn[0].running_mean, torch.zeros(H))     # statistics travelled
    # and back: a fresh engine agent constructed with weights=dir reproduces the actor's outputs
    ag2 = cls(S, A, cfg, str(tmp_path), nenvs=1, gradient_step=2, rng="engine", seed=99, **kw)
    for c, c2 in zip(ag.critics, ag2.critics):
        assert np.array_equal(c.flat(), c2.flat())
    obs = np.random.default_rng(1).standard_normal((7, S)).astype(np.float32)
    assert np.array_equal(ag.select_action(obs, eval_action=True), ag2.select_action(obs, eval_action=True))
    with torch.no_grad():
        actor_mod.eval()
        x = torch.from_numpy(obs)
        if kind in ("SAC", "TQC"):
            want = actor_mod.sample(x, deterministic=True)[0].numpy()
        elif kind == "DDPG":
            want = np.clip(torch.tanh(actor_mod(x)).numpy(), -1, 1)    # double tanh, src/agent.py:1366
        else:
            want = actor_mod(x).numpy()                                 # src/agent.py:269
    assert np.allclose(ag.select_action(obs, eval_action=True), want, rtol=1e-5, atol=1e-6)


def test_select_action_exploration_branches(gcrl):
    cfg = make_config("DDPG", hidden_dim=H, layer_count=L, batch_size=16, noise_std=0.2)
    random.seed(7); np.random.seed(7)
    ag = gcrl.DDPG(S, A, cfg, None, nenvs=4, gradient_step=2, rng="python")
    obs = np.zeros((4, S), np.float32)
    # replay the reference's branch decisions with the same global streams (src/agent.py:1345-1360)
    st_py, st_np = random.getstate(), np.random.get_state()
    outs = [ag.select_action(obs) for _ in range(20)]
    random.setstate(st_py); np.random.set_state(st_np)
    eval_a = ag.select_action(obs, eval_action=True)
    n_random = 0
    for out in outs:
        if random.random() < 0.2:
            want = np.clip(np.random.randn(4, A), -1, 1)
            n_random += 1
        else:
            # the eval path is clip(tanh(actor(obs))) = tanh(actor(obs)): the same base action
            want = np.clip(eval_a + np.random.normal(0, 0.2, size=(4, A)), -1, 1)
        assert out.shape == (4, A) and np.all(np.abs(out) <= 1)
        assert np.allclose(out, want, atol=1e-5)
    assert 0 < n_random < 20


@pytest.mark.parametrize("path", ["select_action", "observe_act"])
@pytest.mark.parametrize("kind", ["DDPG", "TD3", "SAC", "TQC"])
def test_select_action_matches_reference_goldens(gcrl, golden, kind, path):
    """tests/golden/select_action.npz: 28 calls of the REFERENCE's select_action per agent (src/agent.py:1345-1366, :253-270,
    :641-647, :1044-1050) with all three host generators seeded — returned arrays (values and dtype) and the generators'
    states afterwards.  `select_action` (gcrl_agent_act_host / gcrl_agent_act) and the fused `observe_act`
    (gcrl_agent_observe_act) must return the same actions and leave `random`, `np.random` and torch's generator in the
    reference's state: same draws, same order, DDPG's epsilon branch included."""
    g = golden("select_action.npz")
    S_, A_, H_, L_ = (int(x) for x in g[f"{kind}_dims"])
    cfg = make_config(kind, hidden_dim=H_, layer_count=L_, batch_size=64, noise_std=float(g[f"{kind}_noise_std"][0]))
    cls = dict(DDPG=gcrl.DDPG, TD3=gcrl.TD3Agent, SAC=gcrl.SACAgent, TQC=gcrl.TQCAgent)[kind]
    ag = cls(S_, A_, cfg, None, nenvs=1, gradient_step=40, rng="python")
    ag.actor.set_flat(g[f"{kind}_actor"])
    if kind in ("SAC", "TQC"):
        ag.actor._set("bn_running_mean", g[f"{kind}_bn_mean"])
        ag.actor._set("bn_running_var", g[f"{kind}_bn_var"])
    seed = int(g["seed"][0])
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    worst = 0.0
    for i in range(int(g["n_calls"][0])):
        obs, ev, want = g[f"{kind}_obs{i}"], bool(g[f"{kind}_eval{i}"][0]), g[f"{kind}_act{i}"]
        if path == "select_action":
            got = ag.select_action(obs, eval_action=ev)
            assert str(got.dtype) == str(g[f"{kind}_dtype{i}"][0]), (i, got.dtype)
        else:   # the env's dict observation: [observation | desired_goal] (src/env.py:348-355), no normalisation
            got = ag.observe_act(obs[:, :S_ - 3], obs[:, S_ - 3:], eval_action=ev, obs_normalize=False, g_normalize=False)
        assert got.shape == want.shape
        worst = max(worst, float(np.max(np.abs(np.asarray(got, np.float64) - want))))
        assert np.allclose(got, want, rtol=1e-5, atol=2e-6), (kind, i, ev, got, want)
    assert np.array_equal(np.array(random.getstate()[1], np.uint32), g[f"{kind}_py_state"])
    name, keys, pos, has_gauss, cached = np.random.get_state()
    assert np.array_equal(np.asarray(keys, np.uint32), g[f"{kind}_np_keys"])
    assert [pos, has_gauss] == [int(x) for x in g[f"{kind}_np_pos"]] and cached == float(g[f"{kind}_np_cached"][0])
    assert np.array_equal(torch.get_rng_state().numpy(), g[f"{kind}_torch_state"])
    if kind == "DDPG":
        assert int(g["DDPG_eps_branches"][0]) > 0
    print(f"select_action[{kind}/{path}] worst |diff| {worst:.2e}")


def test_reset_and_alpha_view(gcrl):
    cfg = make_config("SAC", hidden_dim=H, layer_count=L, batch_size=16, alpha_min_steps=0.0, alpha_lr=1e-2)
    ag = gcrl.SACAgent(S, A, cfg, None, nenvs=1, gradient_step=2, rng="engine", seed=1)
    fill(ag)
    assert ag.alpha.item() == 1.0
    for step in (1, 2, 3):
        info = ag.update(step)
    assert len(info) == 9 and float(info[-1]) != 0.0            # alpha_loss is live past alpha_min_steps
    assert ag.alpha.item() != 1.0
    before = ag.actor.flat().copy()
    bn_before = ag.actor._get("bn_running_mean").copy()
    ag.reset()
    assert not np.array_equal(before, ag.actor.flat())
    assert ag.alpha.item() == 1.0                                # log_alpha re-created (src/agent.py:767-769)
    assert np.array_equal(bn_before, ag.actor._get("bn_running_mean"))   # BN statistics are NOT reset


def test_compute_reward_classification(gcrl):
    buf = gcrl.HERBuffer(1000, 50, 1, rng="engine", seed=1)
    buf.compute_reward = lambda ag, g, info: her_oracle.sparse_reward(ag, g, info, threshold=0.08)
    gen = np.random.default_rng(0)
    steps = her_oracle.synthetic_episode(gen, 50, S, A)
    for st in steps:
        buf.push(0, *st)
    orc = her_oracle.HERBufferOracle(1000, 50, 1, rng=random.Random(1))
    orc.compute_reward = buf.compute_reward
    for st in steps:
        orc.push(0, *st)
    assert np.array_equal(buf.rows()[3].view(np.uint32), orc.as_arrays()[3].view(np.uint32))   # thr 0.08 was detected
    dense = gcrl.HERBuffer(1000, 50, 1, rng="engine", seed=1)
    dense.compute_reward = her_oracle.dense_reward
    for st in steps:
        dense.push(0, *st)
    r = dense.rows()[3]
    assert np.all(r[1:5] <= 0) and len(np.unique(r)) > 10


@pytest.mark.parametrize("rng", ["engine", "device"])
def test_arbitrary_compute_reward_goes_through_the_host_callback(gcrl, rng):
    """The reference calls whatever callable was injected (src/env.py:105, src/buffer.py:166).  One that is not a goal-distance
    reward takes the host-callback path: same rows as the oracle (which calls it like the reference does), same number of calls
    in the same order; changing the callable later is honoured; an exception inside it surfaces from the push."""
    calls = []

    def shaped(ag, g, info):          # not a function of the distance alone: classifies as neither sparse nor dense
        assert info == {} and ag.dtype == np.float32 and ag.shape == g.shape == (3,)
        calls.append((ag.copy(), g.copy()))
        return np.float32(-np.abs(ag - g).sum() - 0.25 * float(ag[0] > g[1]))   # on axis probes this IS -distance: only the
                                                                                # general-position check tells it apart

    gen = np.random.default_rng(0)
    eps = [her_oracle.synthetic_episode(gen, T, S, A) for T in (50, 13, 50)]
    buf = gcrl.HERBuffer(2000, 50, 2, k_future=4, rng=rng, seed=1)
    buf.compute_reward = shaped
    orc = her_oracle.HERBufferOracle(2000, 50, 2, k_future=4, rng=her_oracle.HashRng(1) if rng == "device" else random.Random(1))
    orc.compute_reward = shaped
    for e, ep in enumerate(eps[:2]):
        for t, st in enumerate(ep):
            done = (e == 1 and t == len(ep) - 1)
            buf.push(e, st[0], st[1], st[2], st[3], done, st[5], st[6])
            if e == 0 and t == 0:
                assert len(calls) > 0       # the ring is created at the first push: the classification probes
                calls.clear()
    n_calls, calls_buf = len(calls), list(calls)
    calls.clear()
    for e, ep in enumerate(eps[:2]):
        for t, st in enumerate(ep):
            orc.push(e, st[0], st[1], st[2], st[3], (e == 1 and t == len(ep) - 1), st[5], st[6])
    assert n_calls == len(calls) == 4 * 49 + 4 * 12
    for (a0, g0), (a1, g1) in zip(calls_buf, calls):
        assert np.array_equal(a0, a1) and np.array_equal(g0, g1)
    for got, want in zip(buf.rows(), orc.as_arrays()):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a reassignment is honoured from the next flush on (the reference reads the attribute at every call)
    buf.compute_reward = lambda ag, g, info: np.float32(3.0) if ag[0] > g[0] else np.float32(-7.5)
    orc.compute_reward = buf.compute_reward
    for st in eps[2]:
        buf.push(0, *st)
        orc.push(0, *st)
    for got, want in zip(buf.rows(), orc.as_arrays()):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert set(np.unique(buf.rows()[3][-246:])) >= {3.0, -7.5}

    def broken(ag, g, info):
        raise KeyError("reward exploded")
    buf.compute_reward = broken
    with pytest.raises(KeyError):
        for st in eps[2]:
            buf.push(1, *st)
    # switching a built-in ring to another reward kind is still refused rather than ignored
    sparse = gcrl.HERBuffer(1000, 50, 1, rng="engine", seed=1)
    sparse.compute_reward = her_oracle.sparse_reward
    sparse.push(0, *eps[0][0])
    with pytest.raises(ValueError):
        sparse.compute_reward = shaped


def test_error_behaviour_matches_reference(gcrl):
    cfg = make_config("DDPG", hidden_dim=H, layer_count=L, batch_size=64)
    ag = gcrl.DDPG(S, A, cfg, None, nenvs=1, gradient_step=2, rng="engine", seed=1)
    assert not ag.is_buffer_filled()
    with pytest.raises(AssertionError):
        ag.update(1)                                             # nothing pushed yet
    bad = make_config("DDPG", hidden_dim=H, layer_count=L, buffer_type="NOPE")
    with pytest.raises(ValueError, match="Invalid Buffer type"):
        gcrl.DDPG(S, A, bad, None, nenvs=1, gradient_step=2)
    fill(ag, 1)
    assert ag.is_buffer_filled()
    with pytest.raises(TypeError):
        ag.push(np.zeros(S), np.zeros(A), 0.0, np.zeros(S), False)   # 5-arg push on a HER buffer, as in the reference


@pytest.mark.parametrize("k,nenvs", [(4, 8), (8, 11)])
def test_push_batch_equals_per_env_pushes_and_oracle(gcrl, k, nenvs):
    """Vector-env step API (§8f-1): nenvs transitions per call; envs reach the 50-step flush together
    (multi-episode flush launches with the in-kernel segment scan, chunked when the inline future
    indices would overflow), some terminate early.  Rows, order and RNG state must equal the
    reference's per-env loop (oracle) bit for bit."""
    Sx, Ax = 23, 4
    gen = np.random.default_rng(9)
    eps = [[her_oracle.synthetic_episode(gen, 50, Sx, Ax) for _ in range(3)] for _ in range(nenvs)]
    buf = gcrl.HERBuffer(20000, 50, nenvs, k_future=k, rng="engine", seed=5)
    orc = her_oracle.HERBufferOracle(20000, 50, nenvs, k_future=k, rng=random.Random(5))
    cursor = [(0, 0)] * nenvs            # (episode, step) per env
    early = {(1, 0): 17, (3, 1): 1, (6, 0): 30}   # (env, episode) -> terminate at this step
    for _ in range(120):
        rows = []
        for e in range(nenvs):
            ep, t = cursor[e]
            st = eps[e][ep % 3][t]
            done = early.get((e, ep)) == t + 1
            rows.append((st, done))
            cursor[e] = (ep + 1, 0) if (done or t + 1 >= 50) else (ep, t + 1)
        s = torch.from_numpy(np.stack([r[0][0] for r in rows])).cuda()
        ns = torch.from_numpy(np.stack([r[0][2] for r in rows])).cuda()
        buf.push_batch(s, np.stack([r[0][1] for r in rows]), ns, [r[0][3] for r in rows], [r[1] for r in rows],
                       np.stack([r[0][6] for r in rows]))
        for e, (st, done) in enumerate(rows):
            orc.push(e, st[0], st[1], st[2], st[3], done, st[5], st[6])
    assert len(buf) == len(orc) > 0
    for got, want in zip(buf.rows(), orc.as_arrays()):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got = buf.sample(64)
    want = orc.sample(64)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32))


# ------------------------------------------------------------------ full resume state (SURVEY.md §8f-2 extension)
def resume_agent(gcrl, kind, nenvs=2, state_dim=10, action_dim=3):
    from oracle.agent_oracle import make_config
    kind, kw = variant(kind)
    cfg = make_config(kind, hidden_dim=32, layer_count=2, batch_size=32, max_len=1000, ac_update_freq=2 if kind == "TD3" else 1,
                      policy_noise=0.2, actor_lr_min=1e-4, ac_scheduler_steps=25, critic_lr_min=2e-4, cr_scheduler_steps=30)
    cls = dict(DDPG=gcrl.DDPG, TD3=gcrl.TD3Agent, SAC=gcrl.SACAgent, TQC=gcrl.TQCAgent)[kind]
    return cls(state_dim, action_dim, cfg, None, nenvs=nenvs, gradient_step=10, rng="engine", seed=5, **kw)


@pytest.mark.parametrize("kind", ["DDPG", "TD3", "SAC", "TQC", "TQC-25x2"])
def test_full_state_resume_in_a_new_process(gcrl, tmp_path, kind):
    """save_state after 30 steps (ring wrapped, one episode half staged, cosine schedules mid-way, device-noise counter
    advanced), load into a fresh agent in a NEW process, continue 20 steps there and here: tuples, parameters, targets
    and ring contents bitwise equal."""
    import os
    import subprocess
    import sys
    from oracle import her_oracle
    ag = resume_agent(gcrl, kind)
    gen = np.random.default_rng(9)
    for ep in range(6):                      # 6 x 246 rows into a 1000-row ring: wraps
        for st in her_oracle.synthetic_episode(gen, 50, 10, 3):
            ag.push_her(ep % 2, *st)
    for st in her_oracle.synthetic_episode(gen, 50, 10, 3)[:17]:   # a partial episode stays staged
        ag.push_her(1, *st)
    ag.update_many(1, 10); ag.update_many(11, 10); ag.update_many(21, 10)
    state = str(tmp_path / "state")
    ag.save_state(state)
    want = [[float(x) for x in t] for t in ag.update_many(31, 10)] + [[float(x) for x in t] for t in ag.update_many(41, 10)]
    out = str(tmp_path / "child.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "resume_child.py"), kind, state, out, "31", "10", "41", "10"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(out)
    width = got["tuples"].shape[1]
    want = np.array([t + [0.0] * (width - len(t)) for t in want])
    assert np.array_equal(got["tuples"], want), np.abs(got["tuples"] - want).max()
    assert np.array_equal(got["actor"], ag.actor.flat()) and np.array_equal(got["critic"], ag.critics[-1].flat())
    assert np.array_equal(got["target"], ag.target_critics[0].flat())
    assert int(got["n"]) == len(ag.buffer) == 1000 and np.array_equal(got["rows"], ag.buffer.rows()[0])


def test_soft_target_update_matches_reference_formula(gcrl):
    """update_target_network(hard_update=False, tau) = tau*p + (1-tau)*p_target on every target (src/agent.py:1259-1271)."""
    ag = resume_agent(gcrl, "TD3")
    gen = np.random.default_rng(1)
    new = {}
    for v in [ag.actor] + ag.critics:
        new[v.name] = (0.3 * gen.standard_normal(v.numel())).astype(np.float32)
    old = {v.name: v.flat() for v in [ag.target_actor] + ag.target_critics}
    for v in [ag.actor] + ag.critics:
        v.set_flat(new[v.name])
    ag.update_target_network(hard_update=False, tau=0.25)
    torch.cuda.synchronize()
    for v in [ag.target_actor] + ag.target_critics:
        src = new[v.name.replace("target_", "")]
        want = (np.float32(0.25) * src + np.float32(0.75) * old[v.name]).astype(np.float32)
        assert np.array_equal(v.flat(), want), v.name
    # the row-chain kernels' [in][out] copies of the targets follow the soft update: the next step equals the step of
    # an agent whose targets were set to the same values through the parameter interface (which rebuilds the copies)
    from oracle import her_oracle
    twin = resume_agent(gcrl, "TD3")
    for v, w in zip([ag.actor, ag.target_actor] + ag.critics + ag.target_critics,
                    [twin.actor, twin.target_actor] + twin.critics + twin.target_critics):
        w.set_flat(v.flat())
    gen = np.random.default_rng(3)
    for st in her_oracle.synthetic_episode(gen, 50, 10, 3):
        ag.push_her(0, *st); twin.push_her(0, *st)
    a = [[float(x) for x in t] for t in ag.update_many(1, 2)]
    b = [[float(x) for x in t] for t in twin.update_many(1, 2)]
    assert a == b


def test_lazy_scalars_outlive_the_metrics_ring(gcrl):
    """A trainer keeps update() outputs in history containers (src/env.py:521-537): entries read long after 4096 later
    steps must still resolve, and np.mean over a deque of them equals the eager path."""
    from collections import deque
    from oracle import her_oracle
    ag = resume_agent(gcrl, "DDPG")
    gen = np.random.default_rng(2)
    for ep in range(3):
        for st in her_oracle.synthetic_episode(gen, 50, 10, 3):
            ag.push_her(0, *st)
    first = ag.update(1)
    hist = deque(maxlen=100)
    step = 2
    for _ in range(110):
        for t in ag.update_many(step, 40):
            hist.append(t[0])
        step += 40
    assert np.isfinite(float(first[0])) and np.isfinite(np.asarray(first[2]))      # 4400 steps later
    m = np.mean(hist)
    assert np.isfinite(m) and abs(m - np.mean([float(x) for x in hist])) < 1e-12 and np.asarray(first[2]).dtype == np.float32


# ------------------------------------------------------------------ acting side on the device
def test_device_normalizer_bit_exact_vs_reference(gcrl):
    """csrc/normalizer.hip against the golden captured from the reference's RunningNormalizer (src/utils.py:68-98):
    mean / var / count (float64) after every update and the normalised probe rows, bit for bit."""
    from conftest import load_golden
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    g = load_golden("normalizer.npz")
    nz = DeviceRunningNormalizer(int(g["D"][0]))
    for i in range(len(g["sizes"])):
        nz.update(g[f"x{i}"])
        assert np.array_equal(nz.mean, g[f"mean{i}"]) and np.array_equal(nz.var, g[f"var{i}"]) and nz.count == g[f"count{i}"][0], i
        z = nz.normalize(g["probe"])
        assert np.array_equal(z.astype(np.float32), g[f"norm32_{i}"]), i
    # save / load round trip through the reference's YAML layout
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        nz.save(d + "/n/obs.yaml")
        other = DeviceRunningNormalizer(int(g["D"][0]))
        other.load(d + "/n/obs.yaml")
        assert np.allclose(other.mean, nz.mean, rtol=1e-6) and other.count == nz.count


@pytest.mark.parametrize("g_norm", [False, True])
@pytest.mark.parametrize("kind", ["DDPG", "TD3", "SAC"])
def test_fused_acting_entries_equal_the_separate_calls(gcrl, kind, g_norm):
    _fused_vs_separate(gcrl, kind, g_norm, False)


@pytest.mark.parametrize("g_norm", [False, True])
def test_fused_acting_entries_with_loaded_normalizers(gcrl, g_norm, tmp_path):
    """The same with normalisers that were LOADED from the reference's yaml files (src/utils.py:108-117): float32 statistics
    and float32 arithmetic from then on (what a resumed or evaluating run does) — host numpy and the device agree bit for bit."""
    _fused_vs_separate(gcrl, "DDPG", g_norm, True, tmp_path)


def test_device_normalizer_after_load_bit_exact_vs_reference(gcrl, tmp_path):
    """csrc/normalizer.hip in the float32 regime against tests/golden/normalizer_loaded.npz, captured from the reference's
    RunningNormalizer after load(): statistics, normalised probes (float32 results), merges — bit for bit."""
    from conftest import load_golden
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    g = load_golden("normalizer_loaded.npz")
    path = tmp_path / "obs.yaml"
    path.write_text(str(g["yaml_text"]))
    nz = DeviceRunningNormalizer(int(g["D"][0]))
    assert not nz.float32
    nz.load(str(path))
    assert nz.float32 and nz.mean.dtype == np.float32
    assert np.array_equal(nz.mean, g["load_mean"]) and np.array_equal(nz.var, g["load_var"]) and nz.count == g["load_count"][0]
    z = nz.normalize(g["probe"])
    assert z.dtype == np.float32 and np.array_equal(z, g["load_norm"])
    for i in range(len(g["sizes"])):
        nz.update(g[f"x{i}"])
        assert np.array_equal(nz.mean, g[f"mean{i}"]) and np.array_equal(nz.var, g[f"var{i}"]) and nz.count == g[f"count{i}"][0], i
        assert np.array_equal(nz.normalize(g["probe"]), g[f"norm{i}"]), i


def test_device_normalizer_with_float64_rows_bit_exact_vs_reference(gcrl, tmp_path):
    """csrc/normalizer.hip fed the float64 rows the reference's trainer feeds its observation normaliser (src/utils.py:156: the
    vector env's observation batches are float64 arrays) against tests/golden/normalizer_f64.npz: created normaliser; loaded
    normaliser whose float32 statistics turn float64 with the first update (the float32 regime is not sticky
    there); float32 rows followed by float64 rows.  The rows cross the ABI as float32 (their values are float32-valued)."""
    from conftest import load_golden
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    g = load_golden("normalizer_f64.npz")
    D, probe = int(g["D"][0]), g["probe"]
    r32 = lambda z: np.asarray(z, np.float64).astype(np.float32)      # what the trainer keeps of a normalised row (src/env.py:189-190)
    nz = DeviceRunningNormalizer(D)
    for i in range(len(g["a_sizes"])):
        x = g[f"a_x{i}"]
        assert x.dtype == np.float64 and np.array_equal(x.astype(np.float32).astype(np.float64), x)
        nz.update(x)
        assert np.array_equal(nz.mean, g[f"a_mean{i}"]) and np.array_equal(nz.var, g[f"a_var{i}"]) and nz.count == g[f"a_count{i}"][0], i
        z = nz.normalize(probe)
        assert z.dtype == np.float64 and np.array_equal(r32(z), r32(g[f"a_norm{i}"])), i
    path = tmp_path / "obs.yaml"
    path.write_text(str(g["yaml_text"]))
    ld = DeviceRunningNormalizer(D)
    ld.load(str(path))
    assert ld.float32 and np.array_equal(ld.mean, g["load_mean"])
    z = ld.normalize(probe)
    assert z.dtype == np.float64 and np.array_equal(r32(z), r32(g["b_load_norm"]))
    for i in range(len(g["b_sizes"])):
        ld.update(g[f"b_x{i}"])
        assert not ld.float32 and ld.mean.dtype == np.float64, i
        assert np.array_equal(ld.mean, g[f"b_mean{i}"]) and np.array_equal(ld.var, g[f"b_var{i}"]) and ld.count == g[f"b_count{i}"][0], i
        assert np.array_equal(r32(ld.normalize(probe)), r32(g[f"b_norm{i}"])), i
    ld2 = DeviceRunningNormalizer(D)
    ld2.load(str(path))
    ld2.update(g["c_x32"])
    assert ld2.float32 and np.array_equal(ld2.mean, g["c_mean0"]) and np.array_equal(ld2.var, g["c_var0"])
    z32 = ld2.normalize(probe.astype(np.float32))
    assert z32.dtype == np.float32 and np.array_equal(z32, g["c_norm0_f32rows"])
    assert np.array_equal(r32(ld2.normalize(probe)), r32(g["c_norm0_f64rows"]))
    ld2.update(g["c_x64"])
    assert not ld2.float32 and np.array_equal(ld2.mean, g["c_mean1"]) and np.array_equal(ld2.var, g["c_var1"]) and ld2.count == g["c_count1"][0]
    assert np.array_equal(r32(ld2.normalize(probe)), r32(g["c_norm1"]))


@pytest.mark.parametrize("loaded", [False, True])
def test_fused_acting_entries_with_float64_observation_rows(gcrl, loaded, tmp_path):
    """The trainer's own dtypes: float64 observation batches (src/utils.py:156), float32 goal batches — fused device entries vs
    the separate calls with host numpy normalisers, bit for bit, with created and with loaded normalisers."""
    _fused_vs_separate(gcrl, "DDPG", True, loaded, tmp_path, obs64=True)


def _fused_vs_separate(gcrl, kind, g_norm, loaded, tmp_path=None, obs64=False, D=7, G=3, A=3, n=8, mt=False):
    """observe_act / process_step (one native call each per vector-env step, device normalisers) against the reference's
    call sequence made of the separate calls with host normalisers: same actions (same host RNG draws), same normaliser
    statistics, same ring rows bit for bit — including the episode flushes (HER relabel) inside the steps.  g_norm: goals
    normalised as well (g_normalize = True, src/env.py:167-175, :222-223: the goal normaliser sees [dg ; next_dg ; ag ; next_ag]).
    mt: the ring's Mersenne Twister ends in the same state as well."""
    import random
    from gcrl_amd.src.utils import DeviceRunningNormalizer, RunningNormalizer
    from oracle import her_oracle
    gen = np.random.default_rng(4)

    def build(device):
        ag = resume_agent(gcrl, kind, nenvs=n, state_dim=D + G, action_dim=A)
        Nz = DeviceRunningNormalizer if device else RunningNormalizer
        ag.buffer.obs_normalizer, ag.buffer.dg_normalizer = Nz(D), Nz(G)
        ag.buffer.compute_reward = her_oracle.sparse_reward
        return ag

    host, dev = build(False), build(True)
    for v, w in zip([host.actor] + host.critics, [dev.actor] + dev.critics):
        w.set_flat(v.flat())
    if loaded:
        for name, dim, sc in (("obs_normalizer", D, 3.0), ("dg_normalizer", G, 0.2)):
            warm = RunningNormalizer(dim)
            for _ in range(3):
                warm.update((gen.standard_normal((40, dim)) * sc + 0.5).astype(np.float32))
            warm.save(str(tmp_path / name / "n.yaml"))
            for ag in (host, dev):
                getattr(ag.buffer, name).load(str(tmp_path / name / "n.yaml"))
            assert getattr(host.buffer, name).mean.dtype == np.float32 and getattr(dev.buffer, name).float32

    def obs_dict():
        return dict(observation=(gen.standard_normal((n, D)).astype(np.float32) * 3 + 1).astype(np.float64 if obs64 else np.float32),
                    desired_goal=gen.uniform(-0.2, 0.2, (n, G)).astype(np.float32),
                    achieved_goal=gen.uniform(-0.2, 0.2, (n, G)).astype(np.float32))

    state = obs_dict()
    for step in range(60):                    # episodes flush at 50 staged transitions per env
        for ag, tag in ((host, "h"), (dev, "d")):
            random.seed(100 + step); np.random.seed(100 + step); torch.manual_seed(100 + step)
            if tag == "h":
                x = ag.normalize_state_batch(state["observation"], state["desired_goal"], True, g_norm)
                act_h = np.asarray(ag.select_action(x, eval_action=(step % 7 == 3)), np.float64)
            else:
                act_d = np.asarray(ag.observe_act(state["observation"], state["desired_goal"], eval_action=(step % 7 == 3), g_normalize=g_norm), np.float64)
        assert act_h.shape == act_d.shape == (n, A)
        assert np.allclose(act_h, act_d, rtol=0, atol=2e-6), (step, np.abs(act_h - act_d).max())
        nxt = obs_dict()
        rewards = -(gen.uniform(size=n) > 0.3).astype(np.float32)
        dones = np.zeros(n, bool)
        actions = act_h.astype(np.float32)
        # host: the reference's _process_step made of the separate calls
        host.update_normalizers([state["observation"], nxt["observation"]],
                                [state["desired_goal"], nxt["desired_goal"], state["achieved_goal"], nxt["achieved_goal"]], True, g_norm)
        s = torch.from_numpy(host.normalize_state_batch(state["observation"], state["desired_goal"], True, g_norm)).float().cuda()
        ns = torch.from_numpy(host.normalize_state_batch(nxt["observation"], nxt["desired_goal"], True, g_norm)).float().cuda()
        host.buffer.push_batch(s, actions, ns, rewards, dones, host.normalize_goal(nxt["achieved_goal"], g_norm))
        dev.process_step(state, actions, nxt, rewards, dones, g_normalize=g_norm)
        state = nxt
    hn, dn = host.buffer.obs_normalizer, dev.buffer.obs_normalizer
    assert np.array_equal(np.asarray(hn.mean), dn.mean) and np.array_equal(np.asarray(hn.var), dn.var) and hn.count == dn.count
    hg, dgn = host.buffer.dg_normalizer, dev.buffer.dg_normalizer
    assert np.array_equal(np.asarray(hg.mean), dgn.mean) and np.array_equal(np.asarray(hg.var), dgn.var) and hg.count == dgn.count
    assert (hg.count > (121 if loaded else 1)) == g_norm      # (loaded: warmed with 120 rows before)
    assert len(host.buffer) == len(dev.buffer) == min(1000, n * 246)      # 1000-row ring: wrapped
    for a, b in zip(host.buffer.rows(), dev.buffer.rows()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if mt:
        import ctypes
        from gcrl_amd._ffi import check, lib
        states = []
        for ag in (host, dev):
            buf = (ctypes.c_uint32 * 625)()
            check(lib.gcrl_mt_get_state(ag.buffer.rng.handle, buf))
            states.append(np.array(buf[:], np.uint32))
        assert np.array_equal(states[0], states[1]), "Mersenne Twister state differs"


@pytest.mark.parametrize("regime", ["created", "loaded", "obs64"])
@pytest.mark.parametrize("nenvs", [2, 5])
def test_fused_acting_entries_with_a_one_feature_goal(gcrl, nenvs, regime, tmp_path):
    """A 1-D goal under g_normalize: the goal normaliser is ONE feature wide and sees 4 * nenvs rows per step.  numpy reduces a
    contiguous (n, 1) array pairwise from 8 rows on (tests/numpy_pairwise_ref.py) - 2 envs are the first size at which that differs
    from the sequential sum a column of a wider normaliser gets; 5 envs give 20 rows, a ragged tail after two rounds of eight.  Fused
    process_step / observe_act against the separate host calls: statistics, ring rows and the ring's generator, bit for bit."""
    _fused_vs_separate(gcrl, "DDPG", True, regime == "loaded", tmp_path, obs64=regime == "obs64", D=9, G=1, A=3, n=nenvs, mt=True)


WIDTH_REGIMES = ["c32", "l32", "c64"]


@pytest.mark.parametrize("regime", WIDTH_REGIMES)
@pytest.mark.parametrize("D", [1, 2, 3])
def test_device_normalizer_at_one_two_and_three_features_bit_exact_vs_reference(gcrl, tmp_path, D, regime):
    """csrc/normalizer.hip against tests/golden/normalizer_widths.npz (make_golden_norm_widths.py): the reference's RunningNormalizer
    at 1, 2 and 3 features over batches of 1 .. 1000 rows - a one-feature batch is summed in numpy's pairwise order, a wider one
    row after row - created with float32 rows, loaded (float32 statistics), created with float64 rows.  Statistics after every
    update and the normalised probe (one row of it clipped), bit for bit."""
    from conftest import load_golden
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    g = load_golden("normalizer_widths.npz")
    sizes, k = [int(v) for v in g["sizes"]], f"d{D}_{regime}_"
    assert sizes == [1, 2, 7, 8, 9, 16, 33, 128, 129, 136, 1000]
    cast = np.float64 if regime == "c64" else np.float32
    r32 = lambda z: np.asarray(z, np.float64).astype(np.float32)      # what the trainer keeps of a normalised row (src/env.py:189-190)
    nz = DeviceRunningNormalizer(D)
    if regime == "l32":
        path = tmp_path / "n.yaml"
        path.write_text(str(g[f"d{D}_yaml_text"]))
        nz.load(str(path))
        assert nz.float32 and np.array_equal(nz.mean, g[f"d{D}_load_mean"]) and np.array_equal(nz.var, g[f"d{D}_load_var"])
    probe, x, at = g[f"d{D}_probe"].astype(cast), g[f"d{D}_x"], 0
    assert x.shape == (sum(sizes), D) and x.dtype == np.float32
    bad = []
    for i, n in enumerate(sizes):
        nz.update(np.ascontiguousarray(x[at:at + n].astype(cast)))
        at += n
        mean, var, z = nz.mean, nz.var, nz.normalize(probe)
        assert mean.dtype == g[k + "mean"].dtype and z.dtype == g[k + "norm"].dtype, (n, mean.dtype, z.dtype)
        ok = (np.array_equal(mean, g[k + "mean"][i]) and np.array_equal(var, g[k + "var"][i]) and nz.count == g[k + "count"][i]
              and np.array_equal(r32(z), r32(g[k + "norm"][i])))
        if not ok:
            bad.append(n)
    assert np.abs(r32(g[k + "norm"][-1])).max() == 5.0      # the clip engaged in the probe
    assert not bad, f"D = {D}, {regime}: differs from the reference from the batch of {bad[0]} rows on (batches {bad})"


def test_resume_with_device_normalizers(gcrl, tmp_path):
    """save_state / load_state with DeviceRunningNormalizer on the buffer (the configuration observe_act / process_step and
    examples/trainer_standin.py use): statistics restored on the device, the next fused step writes the same ring rows."""
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    from oracle import her_oracle
    D, G, n = 7, 3, 4
    gen = np.random.default_rng(12)

    def build():
        ag = resume_agent(gcrl, "DDPG", nenvs=n)
        ag.buffer.obs_normalizer, ag.buffer.dg_normalizer = DeviceRunningNormalizer(D), DeviceRunningNormalizer(G)
        ag.buffer.compute_reward = her_oracle.sparse_reward
        return ag

    def obs_dict():
        return dict(observation=gen.standard_normal((n, D)).astype(np.float32) * 2 - 1,
                    desired_goal=gen.uniform(-0.2, 0.2, (n, G)).astype(np.float32),
                    achieved_goal=gen.uniform(-0.2, 0.2, (n, G)).astype(np.float32))

    a = build()
    steps = [(obs_dict(), gen.uniform(-1, 1, (n, 3)).astype(np.float32), -(gen.uniform(size=n) > 0.3).astype(np.float32)) for _ in range(61)]
    for i in range(55):                        # one flush per env at 50, five transitions staged afterwards
        a.process_step(steps[i][0], steps[i][1], steps[i + 1][0], steps[i][2], np.zeros(n, bool))
    a.buffer.dg_normalizer.update(steps[0][0]["desired_goal"])
    a.save_state(str(tmp_path))
    b = build()
    b.load_state(str(tmp_path))
    for name in ("obs_normalizer", "dg_normalizer"):
        x, y = getattr(a.buffer, name), getattr(b.buffer, name)
        assert np.array_equal(x.mean, y.mean) and np.array_equal(x.var, y.var) and x.count == y.count and x.clip_range == y.clip_range
    assert a.buffer.obs_normalizer.count > 100
    for i in range(55, 60):
        for ag in (a, b):
            ag.process_step(steps[i][0], steps[i][1], steps[i + 1][0], steps[i][2], np.array([i == 57] * n))
    assert len(a.buffer) == len(b.buffer) > n * 246
    for x, y in zip(a.buffer.rows(), b.buffer.rows()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # a state of another agent kind is refused before anything is overwritten
    t = resume_agent(gcrl, "TD3", nenvs=n)
    before = t.actor.flat().copy()
    with pytest.raises(ValueError):
        t.load_state(str(tmp_path))
    assert np.array_equal(before, t.actor.flat())


def test_fused_entries_refuse_a_normalizer_of_another_size(gcrl):
    """A normaliser whose size is not the observation / goal width is an argument error (the reference raises numpy's
    broadcast error there), never an out-of-bounds device access."""
    from gcrl_amd.src.utils import DeviceRunningNormalizer
    from oracle import her_oracle
    GcrlError = ValueError        # GCRL_ERR_ARG surfaces as ValueError (_ffi.check)
    D, G, n = 7, 3, 4
    ag = resume_agent(gcrl, "DDPG", nenvs=n)
    ag.buffer.compute_reward = her_oracle.sparse_reward
    gen = np.random.default_rng(2)
    st = dict(observation=gen.standard_normal((n, D)).astype(np.float32), desired_goal=gen.standard_normal((n, G)).astype(np.float32),
              achieved_goal=gen.standard_normal((n, G)).astype(np.float32))
    act, rew = gen.uniform(-1, 1, (n, 3)).astype(np.float32), np.zeros(n, np.float32)
    ag.buffer.obs_normalizer, ag.buffer.dg_normalizer = DeviceRunningNormalizer(D + 2), DeviceRunningNormalizer(G)
    with pytest.raises(GcrlError):
        ag.process_step(st, act, st, rew, np.zeros(n, bool))
    with pytest.raises(GcrlError):
        ag.observe_act(st["observation"], st["desired_goal"], eval_action=True)
    ag.buffer.obs_normalizer, ag.buffer.dg_normalizer = DeviceRunningNormalizer(D), DeviceRunningNormalizer(G + 1)
    with pytest.raises(GcrlError):
        ag.observe_act(st["observation"], st["desired_goal"], eval_action=True, g_normalize=True)
    ag.buffer.dg_normalizer = DeviceRunningNormalizer(G)
    assert ag.observe_act(st["observation"], st["desired_goal"], eval_action=True, g_normalize=True).shape == (n, 3)
    assert len(ag.buffer) == 0


# ------------------------------------------------------------------ ReplayBuffer / PERBuffer
def test_replay_buffer_rows_and_sample_bit_exact(gcrl):
    """ReplayBuffer (src/buffer.py:8-35): one row per push, deque(maxlen) eviction, random.sample over the stored rows."""
    import random
    from oracle.replay_oracle import ReplayBufferOracle
    gen = np.random.default_rng(8)
    buf = gcrl.ReplayBuffer(300, rng="engine", seed=17)
    orc = ReplayBufferOracle(300, rng=random.Random(17))
    for i in range(420):      # evicts 120
        s, a, ns = gen.standard_normal(10).astype(np.float32), gen.uniform(-1, 1, 3).astype(np.float32), gen.standard_normal(10).astype(np.float32)
        r, d = float(-(i % 3 == 0)), bool(i % 11 == 0)
        buf.push(torch.from_numpy(s).cuda() if i % 2 else s, a, r, torch.from_numpy(ns).cuda() if i % 2 else torch.from_numpy(ns), d)
        orc.push(s, a, r, ns, d)
    assert len(buf) == len(orc) == 300
    with pytest.raises(AssertionError):
        buf.sample(301)
    for _ in range(3):
        got, want = buf.sample(64), orc.sample(64)
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("tag", ["ddpg", "td3", "sac", "tqc"])
def test_per_agent_matches_reference(gcrl, tag):
    """buffer_type="PER" end to end against the golden captured from the reference (tests/golden/make_golden.py gen_per):
    the prioritised draw (np.random.choice over float32 priorities: same indices), importance-sampling weights inside the
    critic losses, the per-sample td_error array in the returned tuple, priorities after every step."""
    from conftest import hparams_from_golden, load_golden
    g = load_golden(f"per_{tag}.npz")
    kind = str(g["kind"][0])
    S, A, B, N = (int(x) for x in g["dims"])
    cfg = hparams_from_golden(g)
    cls = dict(DDPG=gcrl.DDPG, TD3=gcrl.TD3Agent, SAC=gcrl.SACAgent, TQC=gcrl.TQCAgent)[kind]
    stoch = kind in ("SAC", "TQC")        # importance-weight branches src/agent.py:577-581, :993-997; goldens: 4 steps + eps
    ag = cls(S, A, cfg, None, nenvs=1, gradient_step=2 if stoch else 40, rng="engine", seed=0)
    assert isinstance(ag.buffer, gcrl.PERBuffer)
    views = {"actor": ag.actor, **{f"critic_{i}": c for i, c in enumerate(ag.critics)}}
    for n, v in views.items():
        v.set_flat(g[f"init_{n}"])
    ag.update_target_network()
    for i in range(N):
        ag.push(torch.from_numpy(g["rows_s"][i]).cuda(), g["rows_a"][i], float(g["rows_r"][i, 0]), torch.from_numpy(g["rows_ns"][i]).cuda(),
                bool(g["rows_d"][i, 0]))
    assert len(ag.buffer) == cfg.max_len
    np.random.seed(4242)
    for i, step in enumerate((1, 2, 3, 4) if stoch else (1, 2, 3)):
        kw = dict(noise=torch.zeros(B, A)) if kind == "TD3" else {}
        if stoch:
            kw = dict(eps_next=torch.from_numpy(g[f"step{i}_eps_next"]), eps_cur=torch.from_numpy(g[f"step{i}_eps_cur"]))
        info = ag.update(step, **kw)
        want = g[f"step{i}_tuple"]
        td_pos = {6: 2, 8: 3, 9: 3}[len(want)]
        if stoch:
            la = np.empty(1, np.float32)
            gcrl._ffi.check(gcrl._ffi.lib.gcrl_agent_get(ag._h, b"log_alpha", la.ctypes.data, 1))
            assert np.allclose(la, g[f"step{i}_log_alpha"], rtol=1e-5, atol=1e-7)
            assert np.allclose(ag.actor._get("bn_running_mean"), g[f"step{i}_bn_mean"], rtol=1e-5, atol=1e-6)
            assert np.allclose(ag.actor._get("bn_running_var"), g[f"step{i}_bn_var"], rtol=1e-5, atol=1e-6)
            # continue from the reference's state (parameters below; statistics and log_alpha here)
            ag.actor._set("bn_running_mean", g[f"step{i}_bn_mean"]); ag.actor._set("bn_running_var", g[f"step{i}_bn_var"])
            gcrl._ffi.check(gcrl._ffi.lib.gcrl_agent_set(ag._h, b"log_alpha", np.ascontiguousarray(g[f"step{i}_log_alpha"], np.float32).ctypes.data, 1))
        assert len(info) == len(want)
        td = np.asarray(info[td_pos])
        assert td.shape == g[f"step{i}_td"].shape and np.allclose(td, g[f"step{i}_td"], rtol=1e-5, atol=1e-6)
        got = np.array([float(np.mean(x)) if j == td_pos else float(x) for j, x in enumerate(info)])
        assert np.allclose(got, want, rtol=1e-5, atol=1e-6), (i, got, want)
        assert np.allclose(np.array(ag.buffer.priorities, np.float64), g[f"step{i}_priorities"], rtol=1e-5, atol=1e-7)
        assert abs(ag.beta - float(g[f"step{i}_beta"][0])) < 1e-12
        for n, v in views.items():
            k = f"step{i}_gradpre_{n}"
            if k in g.files:
                gg = v.grad_flat()
                assert float(np.max(np.abs(gg - g[k]))) <= 1e-6 + (3e-5 if stoch else 1e-5) * float(np.max(np.abs(g[k]))), (i, n)
            v.set_flat(g[f"step{i}_param_{n}"])     # continue from the reference's state
        # the reference's targets follow their own cadence; keep them in step with the golden run
        if kind == "DDPG":
            pass
    # Replay agents sample through random.sample like HER; smoke: a REPLAY-buffer agent updates
    cfg2 = hparams_from_golden(g); cfg2.buffer_type = "REPLAY"
    ag2 = cls(S, A, cfg2, None, nenvs=1, gradient_step=4, rng="engine", seed=1)
    for i in range(60):
        ag2.push(g["rows_s"][i], g["rows_a"][i], float(g["rows_r"][i, 0]), g["rows_ns"][i], bool(g["rows_d"][i, 0]))
    out = ag2.update_many(1, 4)
    assert all(np.isfinite([float(x) for x in t]).all() for t in out)
