"""Q-filtered behaviour cloning on the prior-data rows of a batch (bc_weight= / q_filter=; csrc/her_bc.hip) restated in numpy, every
fp32 rounding included.  This file is the definition; the reference project has no counterpart (its actor loss is -mean Q alone).

An actor step of DDPG / TD3 on a batch of B rows whose last Bd rows are demonstrations (prior-data replay puts them there):

    L_actor = -mean_B Q0(s, pi(s)) + bc_weight * (1 / Bd) * sum_{b >= B - Bd} mask_b * sum_j (pi_bj - a_bj)^2

pi = actor(s) is the tanh output, a the batch's stored action, Q0 the first critic as this step's critic update left it (the weights
the -mean Q term uses; TD3: the reference's critic_1).  mask_b = 1 without the Q-filter; with it mask_b = (q_a[b] > q_pi[b]), strictly,
q_a = Q0(s, a), q_pi = Q0(s, pi) — a NaN on either side gives 0.  The mask is a constant of the step.  Rows b < B - Bd never take
part.  The denominator is always Bd, never the number of accepted rows (OpenAI Baselines' form), so no division depends on the data.

What the device adds to `dact` [B][Apad], the gradient w.r.t. the pre-tanh action that the critic's input-gradient chain leaves with
the tanh derivative applied — accepted rows, columns j < A only; every other word keeps its bits (a rejected row is not "added 0.0
to": that would turn a -0.0 into +0.0):

    dact[b][j] = fadd(dact[b][j], fmul(fmul(c, fsub(pi_bj, a_bj)), fsub(1, fmul(pi_bj, pi_bj))))      c = fp32((2 * bc_weight) / Bd)

with c evaluated in double and rounded once.  The two metric words of the step:

    row_b   = sum over j ascending of fmul(d, d), d = fsub(pi_bj, a_bj), from 0.0, one fadd per column
    acc_t   = thread t of 256 adds row_b of ITS accepted rows b = B - Bd + t, + 256, ... in that order, from 0.0
    wave_w  = xor-butterfly over the 64 lanes of wave w: for off in 32, 16, 8, 4, 2, 1: v_lane = fadd(v_lane, v_(lane ^ off))
              (fadd commutes, so every lane ends with the same bits; lane 0's are taken)
    total   = ((wave_0 + wave_1) + wave_2) + wave_3
    bc_loss = fmul(fp32(bc_weight / Bd), total)                bc_pass = fdiv(fp32(accepted rows), fp32(Bd))
"""
import numpy as np

F32 = np.float32
THREADS, WAVE = 256, 64


def weight_ok(w):
    """bc_weight: a finite number > 0 ("off" is None, never 0)"""
    return isinstance(w, (int, float, np.integer, np.floating)) and not isinstance(w, bool) and bool(np.isfinite(w)) and w > 0


def rows_ok(B, Bd):
    return isinstance(Bd, (int, np.integer)) and not isinstance(Bd, bool) and 1 <= int(Bd) <= int(B)


def scales(bc_weight, Bd):
    """(c, w_bd): fp32((2 * bc_weight) / Bd) and fp32(bc_weight / Bd), evaluated in double on the host"""
    return F32((2.0 * float(bc_weight)) / float(Bd)), F32(float(bc_weight) / float(Bd))


def mask_of(q_a, q_pi, B, Bd, q_filter=True):
    """[B] float32: 1.0 for an accepted row, 0.0 for a rejected one and for every row below B - Bd"""
    m = np.zeros(B, F32)
    if q_filter:
        with np.errstate(invalid="ignore"):
            m[B - Bd:] = (np.asarray(q_a, F32)[B - Bd:] > np.asarray(q_pi, F32)[B - Bd:]).astype(F32)
    else:
        m[B - Bd:] = 1.0
    return m


def butterfly(v):
    """the xor-butterfly sum over one wave's 64 lanes, lane 0's result"""
    v = np.array(v, F32, copy=True)
    assert v.shape == (WAVE,)
    lanes = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[lanes ^ off]).astype(F32)
    return v[0]


def step(pi, a, dact, mask, bc_weight, Bd):
    """pi, a [B][A] float32; dact [B][Apad] float32; mask [B] -> (dact after the launch (new array), bc_loss, bc_pass) as float32"""
    pi, a = np.asarray(pi, F32), np.asarray(a, F32)
    B, A = pi.shape
    assert rows_ok(B, Bd) and weight_ok(bc_weight) and a.shape == (B, A) and dact.shape[0] == B and dact.shape[1] >= A
    c, w_bd = scales(bc_weight, Bd)
    out = np.array(dact, F32, copy=True)
    acc = np.zeros(THREADS, F32)
    count = 0
    with np.errstate(all="ignore"):
        for i in range(Bd):                      # thread i % 256 meets its rows in ascending order
            b = B - Bd + i
            if not mask[b] > 0:
                continue
            s = F32(0.0)
            for j in range(A):
                d = F32(pi[b, j] - a[b, j])
                s = F32(s + F32(d * d))
                out[b, j] = F32(out[b, j] + F32(F32(c * d) * F32(F32(1.0) - F32(pi[b, j] * pi[b, j]))))
            acc[i % THREADS] = F32(acc[i % THREADS] + s)
            count += 1
        waves = [butterfly(acc[w * WAVE:(w + 1) * WAVE]) for w in range(THREADS // WAVE)]
        total = waves[0]
        for w in waves[1:]:
            total = F32(total + w)
        return out, F32(w_bd * total), F32(F32(count) / F32(Bd))


def loss_f64(pi, a, mask, bc_weight, Bd):
    """the term itself in float64 (what the fp32 bc_loss rounds)"""
    pi, a, m = np.asarray(pi, np.float64), np.asarray(a, np.float64), np.asarray(mask, np.float64)
    return float(bc_weight) / Bd * float((m[:, None] * (pi - a) ** 2).sum())
