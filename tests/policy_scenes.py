"""The definition of a policy (ca_policy_configure, include/ca_env.h) and of a policy rollout's records (ca_rollout_policy), restated
in numpy for the tests.  No device and no library: tests/test_policy_cpu.py checks the arithmetic against exact rationals,
tests/test_gpu_policy.py compares the kernels with it bit for bit.

fmaf32 is an exact vectorised fp32 fused multiply-add: the product of two fp32 values is exact in float64 (48 significant bits, and
no fp32 product underflows there), the sum with c is rounded once to float64 and once more to fp32.  The second rounding can differ
from a single rounding only where the float64 sum lies exactly on the midpoint of two neighbouring fp32 values while the exact sum
does not; those elements -- a handful in a million -- are recomputed in exact rational arithmetic.  (math.fma would not help there:
with an exact product it returns the very float64 sum that sits on the midpoint.)

The rollout's return and first_done follow tests/actseq_scenes.py; the record rules are record_rows / rollout_records below."""
from fractions import Fraction

import numpy as np

from tests import actseq_scenes as S

f32, f64 = np.float32, np.float64


def fraction_to_f32(q):
    """The rational q rounded to fp32, to nearest, ties to even, subnormals and overflow included (a zero comes back as +0)."""
    q = Fraction(q)
    if q == 0:
        return f32(0.0)
    neg, q = q < 0, abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()        # 2^(e-1) < q < 2^(e+1)
    if Fraction(2) ** e > q:
        e -= 1                                                        # now 2^e <= q < 2^(e+1)
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    n = q / ulp
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    v = fl * ulp
    if v >= Fraction(2) ** 128:
        return f32(-np.inf) if neg else f32(np.inf)
    r = f32(float(v))                                                # (v has at most 25 significant bits: exact in float64 and fp32)
    return f32(-r) if neg else r


def fma_exact(a, b, c):
    """fmaf(a, b, c) of three finite fp32 scalars through exact rationals"""
    return fraction_to_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fmaf32(a, b, c, counter=None):
    """fmaf(a, b, c) elementwise on fp32 arrays (broadcast), exactly rounded for finite operands, the overflow threshold included; inf
    and NaN operands follow IEEE 754 through the float64 operations (inf * 0 and inf - inf are NaN, of no defined payload).  counter: a
    list that collects the number of elements that needed the exact path."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    with np.errstate(over="ignore", invalid="ignore"):
        s = a.astype(f64) * b.astype(f64) + c.astype(f64)
        r = s.astype(f32)
        toward = np.where(s > r.astype(f64), f32(np.inf), f32(-np.inf)).astype(f32)
        other = np.nextafter(r, toward)
        edge = np.where(np.isinf(r) & np.isfinite(s), np.copysign(2.0 ** 128, s), r.astype(f64))     # (the midpoint below an overflow is FLT_MAX's and 2^128's)
        mid = (edge + other.astype(f64)) * 0.5
        hazard = np.isfinite(s) & (r.astype(f64) != s) & (mid == s)
    if hazard.any():
        r = r.copy()
        for idx in zip(*np.nonzero(hazard)):
            r[idx] = fma_exact(a[idx], b[idx], c[idx])
    if counter is not None:
        counter.append(int(hazard.sum()))
    return r


def mlp_reference(x, Ws, bs):
    """The mean of the policy for rows x [M, 64]: Ws[l] [out, in], bs[l] [out] of ONE weight set.  Per layer the k-ordered fmaf chain
    from the bias; hidden layers acc > 0 ? acc : +0."""
    x = np.ascontiguousarray(x, f32)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        W, b = np.asarray(W, f32), np.asarray(b, f32)
        acc = np.broadcast_to(b[None, :], (x.shape[0], W.shape[0])).astype(f32)
        for k in range(W.shape[1]):
            acc = fmaf32(x[:, k:k + 1], W[None, :, k], acc)
        x = acc if l == len(Ws) - 1 else np.where(acc > 0, acc, f32(0.0)).astype(f32)
    return x[:, 0]


def out_reference(v, out="identity", limit=np.pi):
    v = np.asarray(v, f32)
    if out == "identity":
        return v
    lim = f32(limit)
    return np.fmin(np.fmax(v, -lim), lim).astype(f32)


def actions_reference(obs, Ws, bs, sets=None, noise=None, out="identity", limit=np.pi):
    """The actions [A, N] of ca_policy_actions for obs [A, N, 64]: Ws[l] [P, out, in], bs[l] [P, out]; arena a plays set sets[a] (None:
    set 0); action = out(mean + noise), the add only where noise is given."""
    obs = np.asarray(obs, f32)
    A, N = obs.shape[:2]
    mean = np.empty((A, N), f32)
    for a in range(A):
        p = 0 if sets is None else int(sets[a])
        mean[a] = mlp_reference(obs[a], [W[p] for W in Ws], [b[p] for b in bs])
    if noise is not None:
        mean = (mean + np.asarray(noise, f32).reshape(A, N)).astype(f32)
    return out_reference(mean, out, limit)


def record_rows(steps, hold):
    """(R, the steps at which a row starts): row r is observed and decided in front of step r * hold and drives steps
    r * hold .. min((r + 1) * hold, steps) - 1"""
    R = (steps + hold - 1) // hold
    return R, [r * hold for r in range(R)]


def rollout_records(observe, act, step, read, steps, hold, noise=None):
    """The loop of the definition on any environment given as four callables -- observe() -> obs [A, N, 64], act(obs_row, noise_row)
    -> actions [A, N], step(actions), read() -> (reward [A, N], arena_done [A]) --: returns dict(obs [R, A, N, 64], actions [R, A, N],
    rewards [steps, A, N], dones [steps, A]).  Every row, arena and step is recorded, whatever froze or was absent."""
    obs, actions, rewards, dones = [], [], [], []
    a = None
    for t in range(steps):
        if t % hold == 0:
            o = np.array(observe(), f32)
            a = np.array(act(o, None if noise is None else noise[t // hold]), f32)
            obs.append(o); actions.append(a)
        step(a)
        r, d = read()
        rewards.append(np.array(r, f32)); dones.append(np.array(d, np.int32))
    return dict(obs=np.asarray(obs, f32), actions=np.asarray(actions, f32), rewards=np.asarray(rewards, f32), dones=np.asarray(dones, np.int32))


def returns_and_first_done(entry_done, rewards, dones, weights, freeze, present=None):
    """returns [A, N] and first_done [A] of the call from its own reward and done records (the rule of tests/actseq_scenes.py)"""
    adv = S.advanced_reference(entry_done, dones, freeze)
    return S.returns_reference(rewards, adv, weights, present), S.first_done_reference(dones, adv)
