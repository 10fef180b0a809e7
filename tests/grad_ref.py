"""The DEFINITION the gradient audit holds the engine to: one update step's losses of the four agent kinds, restated as plain
functions of flat parameter vectors (the engine's `flat()` order = `parameters()` order) and differentiated by torch autograd on
the CPU, in the dtype asked for (fp32 on one thread and fp64 on the same fp32 inputs).  No GPU.  Shared by tests/test_grad_ref.py
(which pins this file against the oracle's fp32 run and the real reference's recorded fp64 numbers) and
tests/test_gpu_gradient_audit.py (which holds every launch form's per-element gradients to it).

Written from the reference's lines, the same ones oracle/agent_oracle.py cites (under src/): the networks model.py:7-30 (Linear +
LeakyReLU stack, Tanh), :48-68 (critic), :86-141 (Linear + BatchNorm1d + ReLU trunk, mean / log_std heads clamped to [-20, 2],
tanh-squashed Gaussian with log(1 - a^2 + 1e-8)); the critic phase agent.py:1311-1343 (DDPG: clamped target, MSE), :173-230 (TD3:
clamped smoothing noise, min of the twins, smooth-L1, critic_0 never clipped :201), :557-618 (SAC: literal 0.2 entropy weight :569),
:960-1042 (TQC with scalar critics: sort, drop the top, mean; alpha-weighted entropy; forward inside the loop :990; Q metric from the
critics AFTER their steps :1013); importance weights (weights * loss).mean() :193-197, :577-581, :993-997, :1320-1325; the actor
phase :1288-1300 / :149-162 (-Q_0(s, pi(s)).mean()), :513-521 (SAC), :912-925 (TQC); the alpha loss :532-546 / :936-949.  It does
NOT import OracleAgent.

The optimiser step between the two phases (the actor phase differentiates through the critics AS STEPPED) is not restated: it is
tests/adam_ref.py's `reference_step` on fresh moments — or, on the GPU side, the engine's own stepped critics handed in as
`critics_after`, so that an optimiser ulp is not charged to the gradient.

Kinks: `Result.z[pass][layer]` holds the pre-activation of every hidden unit of every forward pass that has a backward pass
("critic_i": the critic phase on [s, a]; "actor": the actor phase on s; "critic_i@actor": the stepped critic on [s, pi(s)]).
`Step.flip_vectors(units)` re-runs the fp64 step once per listed (pass, layer, row, unit) with that unit's activation derivative
forced to its other side (value unchanged) and returns the change of every gradient; `FlipData` presents them in the fixture
layout tests/fullsize.explain_flips fits.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import adam_ref as ar

F32 = np.float32
LEAKY = 0.01                   # nn.LeakyReLU()'s default slope
KINDS = ("DDPG", "TD3", "SAC", "TQC")


def n_critics(kind, num_critics=5):
    return {"DDPG": 1, "TD3": 2, "SAC": 2, "TQC": num_critics}[kind]


def layout(net, in_dim, H, L, out_dim):
    """[(key, shape)] in parameters() order.  net: "mlp" (actor / critic) or "gauss" (the BatchNorm actor)."""
    out = []
    if net == "gauss":
        for l in range(L):
            k = in_dim if l == 0 else H
            out += [(f"{l}.weight", (H, k)), (f"{l}.bias", (H,)), (f"{l}.bn_weight", (H,)), (f"{l}.bn_bias", (H,))]
        return out + [("mean.weight", (out_dim, H)), ("mean.bias", (out_dim,)), ("log_std.weight", (out_dim, H)), ("log_std.bias", (out_dim,))]
    for l in range(L + 1):
        out += [(f"{l}.weight", (H if l < L else out_dim, in_dim if l == 0 else H)), (f"{l}.bias", (H if l < L else out_dim,))]
    return out


def numel(lay):
    return int(sum(int(np.prod(s)) for _, s in lay))


def unflat(vec, lay, dtype, grad):
    vec = np.asarray(vec)
    assert vec.size == numel(lay), (vec.size, numel(lay))
    out, off = {}, 0
    for key, shape in lay:
        n = int(np.prod(shape))
        t = torch.tensor(np.ascontiguousarray(vec[off:off + n]).reshape(shape), dtype=dtype)
        out[key] = t.requires_grad_(grad)
        off += n
    return out


def split(vec, lay):
    out, off = {}, 0
    for key, shape in lay:
        n = int(np.prod(shape))
        out[key] = np.asarray(vec)[off:off + n].reshape(shape)
        off += n
    return out


def _act(z, slope, flips):
    """LeakyReLU (slope 0.01) / ReLU (slope 0); flips: [(row, unit)] whose derivative is forced to the other side, value kept."""
    out = F.leaky_relu(z, slope) if slope else torch.relu(z)
    if flips:
        m = torch.zeros_like(z)
        for r, u in flips:
            m[r, u] = (slope - 1.0) if float(z.detach()[r, u]) > 0 else (1.0 - slope)
        out = out + m * (z - z.detach())
    return out


def _of_layer(flips, l):
    return [(r, u) for (ll, r, u) in (flips or ()) if ll == l]


def mlp_forward(p, x, L, tanh=False, flips=None):
    zs, h = [], x
    for l in range(L):
        z = F.linear(h, p[f"{l}.weight"], p[f"{l}.bias"])
        zs.append(z)
        h = _act(z, LEAKY, _of_layer(flips, l))
    out = F.linear(h, p[f"{L}.weight"], p[f"{L}.bias"])
    return (torch.tanh(out) if tanh else out), zs


def gauss_forward(p, x, L, eps, running, flips=None):
    """model.py:100-141 in train mode -> (action, logp [B, 1], z per layer (BatchNorm's output), batch (mean, biased var) per layer,
    the raw log_std head).  running: [(mean, var)] per layer, updated in place as BatchNorm1d does (momentum 0.1, unbiased var)."""
    zs, stats, h = [], [], x
    for l in range(L):
        lin = F.linear(h, p[f"{l}.weight"], p[f"{l}.bias"])
        stats.append((lin.detach().mean(0), lin.detach().var(0, unbiased=False)))
        z = F.batch_norm(lin, running[l][0], running[l][1], p[f"{l}.bn_weight"], p[f"{l}.bn_bias"], True, 0.1, 1e-5)
        zs.append(z)
        h = _act(z, 0.0, _of_layer(flips, l))
    mean = F.linear(h, p["mean.weight"], p["mean.bias"])
    ls_raw = F.linear(h, p["log_std.weight"], p["log_std.bias"])
    log_std = torch.clamp(ls_raw, -20.0, 2.0)
    std = log_std.exp()
    pre = mean + eps * std
    act = torch.tanh(pre)
    logp = torch.distributions.Normal(mean, std).log_prob(pre) - torch.log(1 - act.pow(2) + 1e-8)
    return act, logp.sum(dim=-1, keepdim=True), zs, stats, ls_raw


def _norm_like_reference(gs):
    """agent.py:1279-1286: python-float accumulation of per-tensor norms."""
    return sum(g.norm(2).item() ** 2 for g in gs) ** 0.5


def _post_clip_norm(gs, clip):
    if clip is None or clip < 0:
        return _norm_like_reference(gs)
    total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in gs]))
    coef = torch.clamp(clip / (total + 1e-6), max=1.0)
    return _norm_like_reference([g * coef for g in gs])


def _np(t):
    return t.detach().double().numpy().copy()


class Step:
    """One update step from explicit inputs.  nets: name -> flat fp32 vector ("actor", "target_actor", "critic_i",
    "target_critic_i").  hp: gamma, grad_clip, critic_lr, policy_noise, noise_clamp, top_drop, target_entropy, clamp_lo (default
    -1 / (1 - gamma)).  batch: (s, a, r [B, 1], ns, d [B, 1]).  weights: [B] importance weights or None."""

    def __init__(self, kind, S, A, H, L, hp, nets, batch, *, log_alpha=0.0, weights=None, noise=None, eps_next=None, eps_cur=None,
                 actor_step=True, alpha_step=False, num_critics=5, bn_running=None):
        assert kind in KINDS
        self.kind, self.S, self.A, self.H, self.L, self.hp = kind, S, A, H, L, dict(hp)
        self.C = n_critics(kind, num_critics)
        self.gauss = kind in ("SAC", "TQC")
        self.nets = {k: np.ascontiguousarray(v, dtype=F32).reshape(-1) for k, v in nets.items()}
        self.batch = [np.ascontiguousarray(x, dtype=F32) for x in batch]
        self.B = self.batch[0].shape[0]
        self.log_alpha, self.weights = float(F32(log_alpha)), None if weights is None else np.ascontiguousarray(weights, dtype=F32).reshape(-1, 1)
        self.noise, self.eps_next, self.eps_cur = noise, eps_next, eps_cur
        self.actor_step, self.alpha_step = actor_step, alpha_step and actor_step
        self.bn_running = bn_running
        self.lay_actor = layout("gauss" if self.gauss else "mlp", S, H, L, A)
        self.lay_critic = layout("mlp", S + A, H, L, 1)
        self.grad_nets = [f"critic_{i}" for i in range(self.C)] + (["actor"] if actor_step else [])

    def lay(self, net):
        return self.lay_actor if "actor" in net else self.lay_critic

    def clip_of(self, net):
        c = self.hp.get("grad_clip")
        return -1.0 if c is None or (self.kind == "TD3" and net == "critic_0") else float(c)    # agent.py:201

    def critics_after_reference(self, dtype, grads_flat):
        """The critics after their optimiser step (fresh moments, step 1): tests/adam_ref.py's reference_step."""
        out = []
        for i in range(self.C):
            n = f"critic_{i}"
            z = np.zeros_like(self.nets[n])
            r = ar.reference_step(dtype, self.kind, self.nets[n], z, z, grads_flat[n], 1, self.hp["critic_lr"], ar.weight_decay_of(self.kind),
                                  self.clip_of(n), 1.0)
            out.append(r.p)
        return out

    # ------------------------------------------------------------------------------------------------------------------ the step
    def run(self, dtype, critics_after=None, flips=None, order=None):
        """-> Result.  critics_after: the stepped critics' flat vectors (values representable in dtype) or None (adam_ref).
        flips: {pass: [(layer, row, unit)]}.  order: a row permutation the batch is presented in (per-row results come back in the
        given order)."""
        old = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return self._run(dtype, critics_after, flips or {}, order)
        finally:
            torch.set_num_threads(old)

    def _run(self, dtype, critics_after, flips, order):
        kind, hp, S, A, L, C, B = self.kind, self.hp, self.S, self.A, self.L, self.C, self.B
        assert not (flips and order is not None)
        perm = np.arange(B) if order is None else np.asarray(order)
        inv = np.argsort(perm)

        def T(x):
            return None if x is None else torch.tensor(np.ascontiguousarray(np.asarray(x, dtype=F32)[perm]), dtype=dtype)

        s, a, r, ns, d = (T(x) for x in self.batch)
        w, noise, eps_next, eps_cur = T(self.weights), T(self.noise), T(self.eps_next), T(self.eps_cur)
        gamma = hp["gamma"]
        R = SimpleNamespace(kind=kind, grads={}, z={}, cover={}, bn_batch={}, norms={}, post_norms={}, g_log_alpha=None, pi=None)
        actor = unflat(self.nets["actor"], self.lay_actor, dtype, True)
        tactor = None if self.gauss else unflat(self.nets["target_actor"], self.lay_actor, dtype, False)
        critics = [unflat(self.nets[f"critic_{i}"], self.lay_critic, dtype, True) for i in range(C)]
        tcritics = [unflat(self.nets[f"target_critic_{i}"], self.lay_critic, dtype, False) for i in range(C)]
        if self.gauss:
            running = self.bn_running or [(np.zeros(self.H, F32), np.ones(self.H, F32)) for _ in range(L)]
            running = [(torch.tensor(m, dtype=dtype), torch.tensor(v, dtype=dtype)) for m, v in running]
            alpha = torch.tensor([self.log_alpha], dtype=dtype).exp()
        cov = R.cover
        # ---- the target
        with torch.no_grad():
            if kind == "DDPG":
                na, _ = mlp_forward(tactor, ns, L, tanh=True)
                qt = [mlp_forward(tcritics[0], torch.cat([ns, na], dim=-1), L)[0]]
                y0 = r + gamma * (1.0 - d) * qt[0]
                lo = hp.get("clamp_lo")
                lo = -1.0 / (1.0 - gamma) if lo is None else lo
                y = torch.clamp(y0, min=lo, max=0.0)
                cov["clamp_lo"], cov["clamp_hi"] = int((y0 < lo).sum()), int((y0 > 0.0).sum())
                cov["unclamped"] = int(((y0 >= lo) & (y0 <= 0.0)).sum())
            elif kind == "TD3":
                nz0 = noise * hp["policy_noise"]
                nz = torch.clamp(nz0, -hp["noise_clamp"], hp["noise_clamp"])
                na0 = mlp_forward(tactor, ns, L, tanh=True)[0] + nz
                na = torch.clamp(na0, -1, 1)
                qt = [mlp_forward(t, torch.cat([ns, na], dim=-1), L)[0] for t in tcritics]
                y = r + gamma * (1 - d) * torch.min(qt[0], qt[1])
                cov["noise_lo"], cov["noise_hi"] = int((nz0 < -hp["noise_clamp"]).sum()), int((nz0 > hp["noise_clamp"]).sum())
                cov["action_clamped"] = int((na0.abs() > 1).sum())
            else:
                na, nlp, _, st_n, ls_n = gauss_forward(actor, ns, L, eps_next, running)
                R.bn_batch["next"] = [(_np(m), _np(v)) for m, v in st_n]
                qt = [mlp_forward(t, torch.cat([ns, na], dim=-1), L)[0] for t in tcritics]
                if kind == "SAC":
                    tq, ent = torch.min(qt[0], qt[1]), 0.2
                else:
                    srt, _ = torch.sort(torch.stack(qt), dim=0)
                    tq, ent = (srt[: -hp["top_drop"]].mean(dim=0) if hp["top_drop"] > 0 else torch.stack(qt).mean(dim=0)), alpha
                y = r + gamma * (1 - d) * (tq - ent * nlp)
                cov["log_std_lo"], cov["log_std_hi"] = int((ls_n < -20.0).sum()), int((ls_n > 2.0).sum())
            if kind in ("TD3", "SAC"):
                cov["min_is_0"], cov["min_is_1"] = int((qt[0] < qt[1]).sum()), int((qt[1] < qt[0]).sum())
        cov["terminal"], cov["non_terminal"] = int((d > 0).sum()), int((d == 0).sum())
        # ---- the critics
        x = torch.cat([s, a], dim=-1)
        loss_fn = F.smooth_l1_loss if kind == "TD3" else F.mse_loss
        losses, tds, qs = [], [], []
        for i, c in enumerate(critics):
            name = f"critic_{i}"
            q, zs = mlp_forward(c, x, L, flips=flips.get(name))
            loss = (w * loss_fn(q, y, reduction="none")).mean() if w is not None else loss_fn(q, y)
            gs = torch.autograd.grad(loss, [c[k] for k, _ in self.lay_critic])
            R.grads[name] = {k: _np(g) for (k, _), g in zip(self.lay_critic, gs)}
            R.norms[name], R.post_norms[name] = _norm_like_reference(gs), _post_clip_norm(gs, self.clip_of(name))
            R.z[name] = [_np(z)[inv] for z in zs]
            losses.append(loss.item())
            tds.append(torch.abs(q - y).detach())
            qs.append(q.detach())
        td_row = torch.stack(tds).max(dim=0)[0]
        R.y, R.td_abs = _np(y)[inv].reshape(-1), _np(td_row)[inv].reshape(-1)
        if kind == "TD3":
            cov["huber_saturated"] = int(sum((t >= 1.0).sum() for t in tds))
            cov["huber_quadratic"] = int(sum((t < 1.0).sum() for t in tds))
        if critics_after is None:
            critics_after = self.critics_after_reference(dtype, {n: self.flat(R, n) for n in R.grads})
        R.critics_after = [np.asarray(v, np.float64).reshape(-1) for v in critics_after]
        after = [unflat(v, self.lay_critic, dtype, False) for v in R.critics_after]
        td_mean = torch.mean(td_row).item()
        pn = [R.post_norms[f"critic_{i}"] for i in range(C)]
        if kind == "DDPG":
            cinfo = [losses[0], td_mean, qs[0].mean().item(), pn[0]]
        elif kind == "TQC":
            with torch.no_grad():
                qv = torch.stack([mlp_forward(c, x, L)[0] for c in after]).mean().item()
            cinfo = [float(np.mean(losses)), float(np.mean(losses)), td_mean, qv, float(np.mean(pn)), float(np.mean(pn))]
        else:
            cinfo = [losses[0], losses[1], td_mean, torch.cat(qs, dim=-1).mean().item(), pn[0], pn[1]]
        if not self.actor_step:
            R.tuple = cinfo
            self._unit_counts(R)
            if self.gauss:
                R.bn_running = [(_np(m), _np(v)) for m, v in running]
            return R
        # ---- the actor, through the critics as stepped
        logp = None
        if not self.gauss:
            pi, zs = mlp_forward(actor, s, L, tanh=True, flips=flips.get("actor"))
            q, zc = mlp_forward(after[0], torch.cat([s, pi], dim=-1), L, flips=flips.get("critic_0@actor"))
            R.z["critic_0@actor"] = [_np(z)[inv] for z in zc]
            aloss = -q.mean()
        else:
            pi, logp, zs, st_c, ls_c = gauss_forward(actor, s, L, eps_cur, running, flips=flips.get("actor"))
            R.bn_batch["cur"] = [(_np(m), _np(v)) for m, v in st_c]
            xa = torch.cat([s, pi], dim=-1)
            qa = []
            for i, c in enumerate(after):
                q, zc = mlp_forward(c, xa, L, flips=flips.get(f"critic_{i}@actor"))
                qa.append(q)
                R.z[f"critic_{i}@actor"] = [_np(z)[inv] for z in zc]
            if kind == "SAC":
                aloss = (0.2 * logp - torch.min(qa[0], qa[1])).mean()
                cov["actor_min_is_0"], cov["actor_min_is_1"] = int((qa[0] < qa[1]).sum()), int((qa[1] < qa[0]).sum())
            else:
                qv = torch.stack(qa)
                mq = torch.sort(qv, dim=0)[0][: -hp["top_drop"]].mean(dim=0) if hp["top_drop"] > 0 else qv.mean(dim=0)
                aloss = (alpha.detach() * logp - mq).mean()
            cov["log_std_lo"] += int((ls_c < -20.0).sum())
            cov["log_std_hi"] += int((ls_c > 2.0).sum())
            cov["log_std_inside"] = int(((ls_c >= -20.0) & (ls_c <= 2.0)).sum())
        gs = torch.autograd.grad(aloss, [actor[k] for k, _ in self.lay_actor])
        R.grads["actor"] = {k: _np(g) for (k, _), g in zip(self.lay_actor, gs)}
        R.norms["actor"], R.post_norms["actor"] = _norm_like_reference(gs), _post_clip_norm(gs, self.clip_of("actor"))
        R.z["actor"] = [_np(z)[inv] for z in zs]
        R.pi = _np(pi)[inv]
        self._unit_counts(R)
        if kind == "DDPG":
            R.tuple = [cinfo[0], aloss.item(), cinfo[1], cinfo[2], cinfo[3], R.post_norms["actor"]]
        else:
            R.tuple = cinfo[:2] + [aloss.item()] + cinfo[2:] + [R.post_norms["actor"]]
        if self.gauss:
            R.bn_running = [(_np(m), _np(v)) for m, v in running]
            al = 0.0
            if self.alpha_step:
                la = torch.tensor([self.log_alpha], dtype=dtype, requires_grad=True)
                loss = -(la * (logp + hp["target_entropy"]).detach()).mean()
                R.g_log_alpha = float(torch.autograd.grad(loss, la)[0].item())
                al = loss.item()
            R.tuple.append(al)
            R.logp = _np(logp)[inv].reshape(-1)
        return R

    # ------------------------------------------------------------------------------------------------------------------ helpers
    @staticmethod
    def _unit_counts(R):
        R.cover["units_pos"] = int(sum((z > 0).sum() for zz in R.z.values() for z in zz))
        R.cover["units_neg"] = int(sum((z < 0).sum() for zz in R.z.values() for z in zz))

    def flat(self, R, net):
        return np.concatenate([R.grads[net][k].reshape(-1) for k, _ in self.lay(net)])

    def flip_vectors(self, units, base, critics_after=None):
        """units: [(pass, layer, row, unit)].  base: the fp64 Result without flips.  -> one {net: flat change of its gradient} per
        unit (fp64; one extra step each)."""
        out = []
        for (ps, l, r, u) in units:
            Rf = self.run(torch.float64, critics_after=critics_after, flips={ps: [(int(l), int(r), int(u))]})
            out.append({n: self.flat(Rf, n) - self.flat(base, n) for n in base.grads})
        return out


def near_kink_units(R32, R64, factor=16.0):
    """[(pass, layer, row, unit)] whose fp64 pre-activation lies within factor x that layer's max |z32 - z64| of zero."""
    units = []
    for ps in sorted(R64.z):
        for l, (z32, z64) in enumerate(zip(R32.z[ps], R64.z[ps])):
            tau = factor * float(np.max(np.abs(z32 - z64)))
            rows, cols = np.nonzero(np.abs(z64) <= tau)
            units += [(ps, l, int(r), int(u)) for r, u in zip(rows, cols)]
    return units


class FlipData:
    """A step's fp64 gradients and flip vectors in the layout of the full-size fixtures (`g64_<net>`, `gnorm64_<net>`, `kink_units`,
    `kinku_<net>`, `kinkF_<net>`, `kinkdot_<net>`, `kinkgram_<net>`; every element sampled), so that tests/fullsize.explain_flips
    fits them unchanged.  Use: explain_flips(SimpleNamespace(g=FlipData(...)), {net: gradient})."""

    def __init__(self, g64: dict, vectors: list):
        self.d = {"kink_units": np.zeros((len(vectors), 6))}
        for n, g in g64.items():
            g = np.asarray(g, np.float64)
            rows = np.array([u for u, v in enumerate(vectors) if np.any(v[n] != 0)], dtype=np.int64)
            Fm = np.stack([vectors[u][n] for u in rows]) if rows.size else np.zeros((0, g.size))
            self.d.update({f"g64_{n}": g, f"gnorm64_{n}": np.array([np.sqrt(np.square(g).sum())]), f"kinku_{n}": rows, f"kinkF_{n}": Fm,
                           f"kinkdot_{n}": Fm @ g, f"kinkgram_{n}": Fm @ Fm.T})
        self.files = list(self.d)

    def __getitem__(self, k):
        return self.d[k]
