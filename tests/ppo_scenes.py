"""The definitions of PPO sample collection (ca_policy_set_heads, ca_policy_evaluate, ca_rollout_policy_sample, ca_gae;
include/ca_env.h), restated in numpy for the tests.  No device and no library: tests/test_ppo_cpu.py checks the arithmetic against
exact rationals and float64 formulas, tests/test_gpu_ppo.py compares the kernels with it bit for bit.

Every fp32 operation is one rounding: numpy's float32 +, -, * are correctly rounded, the chains go through policy_scenes.fmaf32.
exp64 restates csrc/ca_math.h's exp64 in float64, operation by operation (no contraction: a product, then a sum)."""
import numpy as np

from tests import actseq_scenes as S
from tests import policy_scenes as PS

f32, f64 = np.float32, np.float64
LOGSTD_MIN, LOGSTD_MAX = f32(-20.0), f32(2.0)
HALF_LOG_2PI = f32(0.918938533)


def exp64(x):
    """e^x in float64 as the library computes it: k = round(x / ln 2), r = x - k ln2 in two parts, the degree-13 Taylor polynomial in
    Horner form, an exact scaling by 2^k.  Elementwise."""
    x = np.asarray(x, f64)
    kd = np.floor(x * 1.44269504088896338700e+00 + 0.5)
    r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10
    pl = np.full(x.shape, 1.0 / 6227020800.0, f64)
    for c in (1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0,
              1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0):
        pl = pl * r + c
    return np.ldexp(pl, kd.astype(np.int64))          # (2^k is exact and so is the product: no result here is subnormal)


def hidden_reference(x, Ws, bs):
    """The activations of the last hidden layer for rows x [M, 64]: mlp_reference's chain over the hidden layers Ws[:-1] of ONE set"""
    x = np.ascontiguousarray(x, f32)
    for W, b in zip(Ws[:-1], bs[:-1]):
        W, b = np.asarray(W, f32), np.asarray(b, f32)
        acc = np.broadcast_to(b[None, :], (x.shape[0], W.shape[0])).astype(f32)
        for k in range(W.shape[1]):
            acc = PS.fmaf32(x[:, k:k + 1], W[None, :, k], acc)
        x = np.where(acc > 0, acc, f32(0.0)).astype(f32)
    return x


def _row_chain(h, w, b):
    """the k-ordered fmaf chain from the bias b over h [M, K] with the row w [K]"""
    acc = np.full(h.shape[0], f32(b), f32)
    for k in range(h.shape[1]):
        acc = PS.fmaf32(h[:, k], f32(w[k]), acc)
    return acc


def heads_reference(obs, Ws, bs, sets=None, value=None, log_std=None):
    """(mean, ls_raw, value), each [A, N], for obs [A, N, 64]: Ws[l] [P, out, in], bs[l] [P, out] as actions_reference takes them;
    value = (w [P, K], b [P]) or None (+0), log_std = (w [P, K] or None: zeros, b [P]) or None (+0)."""
    obs = np.asarray(obs, f32)
    A, N = obs.shape[:2]
    mean, ls_raw, val = (np.zeros((A, N), f32) for _ in range(3))
    for a in range(A):
        p = 0 if sets is None else int(sets[a])
        h = hidden_reference(obs[a], [W[p] for W in Ws], [b[p] for b in bs])
        mean[a] = _row_chain(h, np.asarray(Ws[-1], f32)[p, 0], np.asarray(bs[-1], f32)[p, 0])
        if value is not None:
            val[a] = _row_chain(h, np.asarray(value[0], f32)[p], np.asarray(value[1], f32)[p])
        if log_std is not None:
            w = np.zeros(h.shape[1], f32) if log_std[0] is None else np.asarray(log_std[0], f32)[p]
            ls_raw[a] = _row_chain(h, w, np.asarray(log_std[1], f32)[p])
    return mean, ls_raw, val


def sample_reference(mean, ls_raw, eps=None, has_log_std=True, out="identity", limit=np.pi):
    """dict(actions=, logp=, log_std=) from the chains' results: the clamp, std = (float)exp64((double)ls), u = mean + std * eps in
    two operations, action = out(u), logp = ((-0.5 * (eps * eps)) - ls) - 0.918938533 left to right"""
    mean = np.asarray(mean, f32)
    if has_log_std:
        ls = np.fmin(np.fmax(np.asarray(ls_raw, f32), LOGSTD_MIN), LOGSTD_MAX).astype(f32)
        std = exp64(ls.astype(f64)).astype(f32)
    else:
        ls, std = np.zeros(mean.shape, f32), np.ones(mean.shape, f32)
    eps = np.zeros(mean.shape, f32) if eps is None else np.asarray(eps, f32).reshape(mean.shape)
    u = (mean + (std * eps).astype(f32)).astype(f32)
    logp = (((f32(-0.5) * (eps * eps).astype(f32)).astype(f32) - ls).astype(f32) - HALF_LOG_2PI).astype(f32)
    return dict(actions=PS.out_reference(u, out, limit), logp=logp, log_std=ls, u=u)


def evaluate_reference(obs, Ws, bs, sets=None, value=None, log_std=None, eps=None, out="identity", limit=np.pi):
    """What ca_policy_evaluate returns for obs [A, N, 64]: dict(actions=, logp=, value=, mean=, log_std=)"""
    mean, ls_raw, val = heads_reference(obs, Ws, bs, sets, value, log_std)
    s = sample_reference(mean, ls_raw, eps, log_std is not None, out, limit)
    return dict(actions=s["actions"], logp=s["logp"], value=val, mean=mean, log_std=s["log_std"])


def gae_reference(rewards, values, done, valid=None, gamma=0.95, lam=1.0):
    """(advantages, targets) [R, A, N] float32 of ca_gae's definition: rewards [R, A, N], values [R + 1, A, N], done [R, A],
    valid [R, A] or None"""
    rewards, values = np.asarray(rewards, f32), np.asarray(values, f32)
    R = rewards.shape[0]
    A, N = values.shape[1:]
    done = np.asarray(done).reshape(R, A)
    valid = np.ones((R, A), np.int32) if valid is None else np.asarray(valid).reshape(R, A)
    g = f32(gamma)
    gl = f32(g * f32(lam))
    adv = np.zeros((R, A, N), f32)
    tgt = np.zeros((R, A, N), f32)
    zero = np.zeros((A, N), f32)
    for r in range(R - 1, -1, -1):
        nd = (done[r] == 0)[:, None]
        next_v = np.where(nd, values[r + 1], zero)
        delta = (((rewards[r] + (g * next_v).astype(f32)).astype(f32)) - values[r]).astype(f32)
        next_a = np.where(nd, adv[r + 1], zero) if r < R - 1 else zero
        a = (delta + (gl * next_a).astype(f32)).astype(f32)
        a = np.where((valid[r] == 0)[:, None], zero, a)
        adv[r] = a
        tgt[r] = (a + values[r]).astype(f32)
    return adv, tgt


def row_records(entry_done, rewards, dones, hold, freeze):
    """(row_rewards [R, A, N] float32, row_dones [R, A] int32, row_valid [R, A] int32) of a sampling rollout from its own step
    records rewards [T, A, N] and dones [T, A]: from +0 one float32 add per step of the row that advanced the arena, in step order;
    the OR of the row's done entries; 1 iff the row's first step advanced the arena"""
    rewards = np.asarray(rewards, f32)
    T, A, N = rewards.shape
    dones = np.asarray(dones).reshape(T, A)
    adv = S.advanced_reference(entry_done, dones, freeze)
    R = (T + hold - 1) // hold
    rr, rd, rv = np.zeros((R, A, N), f32), np.zeros((R, A), np.int32), np.zeros((R, A), np.int32)
    for t in range(T):
        r = t // hold
        rr[r] = np.where(adv[t][:, None], (rr[r] + rewards[t]).astype(f32), rr[r])
        rd[r] |= (dones[t] != 0).astype(np.int32)
        if t % hold == 0:
            rv[r] = adv[t].astype(np.int32)
    return rr, rd, rv
