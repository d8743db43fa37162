"""Scenes that take the policy, its heads and their epilogue (ca_policy_configure, ca_policy_set_heads; include/ca_env.h) to the edges
of fp32: subnormal operands and results, sums that overflow in the middle of a chain, cancelling products, constructed rounding ties,
signed zeros, non-finite observations beside finite ones, and every corner of the heads' epilogue.  No device and no library: a builder
returns (Scene(layers, sets, obs, heads, eps), reach), where reach says -- from the restatement alone (tests/policy_scenes.py,
tests/ppo_scenes.py) -- that the scene got where it was sent.  tests/test_policy_edges_cpu.py asserts every reach,
tests/test_gpu_policy_edges.py compares the kernels with the restatement on the scenes, tools/policy_edges_report.py counts.

layers: [(W [P, out, in], b [P, out])]; sets [A] int32; obs [A, N, 64]; heads (value (w [P, K], b [P]), log_std (w [P, K] or None,
b [P])); eps [A, N].

The probe policy 64 -> 16 -> 1 reads hidden units out bit for bit: its output row is one-hot with weight 1.0 and bias +0, so the
mean is fmaf(h[j], 1, +0) == h[j] and every other term adds an exact zero; the value row is one-hot on another unit.  (Hidden
activations are >= +0, so those zeros are +0 and leave a positive sum alone.)"""
import collections
from fractions import Fraction

import numpy as np

from tests import policy_scenes as PS
from tests import ppo_scenes as PP

f32, f64 = np.float32, np.float64
TINY, FMAX = f32(np.finfo(f32).tiny), f32(np.finfo(f32).max)
HID = 16

Scene = collections.namedtuple("Scene", "layers sets obs heads eps")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def is_subnormal(a):
    a = np.abs(np.asarray(a, f32))
    return (a > 0) & (a < TINY)


def ulp_up(x):
    return np.nextafter(f32(x), f32(np.inf))


def ulp_down(x):
    return np.nextafter(f32(x), f32(-np.inf))


# ---- the tracing twin of mlp_reference ----------------------------------------------------------------------------------------------------
def mlp_trace(x, Ws, bs, fma=PS.fmaf32, counter=None):
    """mlp_reference's chains for rows x [M, 64] with every state kept: returns (out [M, width of the last layer] -- the last layer's
    accumulators, all its columns --, traces), traces[l] [K_l, M, out_l] the accumulators of layer l after every k.  fma: the fused
    multiply-add (the breakage checks pass a wrong one); counter: fmaf32's."""
    x = np.ascontiguousarray(x, f32)
    traces = []
    for l, (W, b) in enumerate(zip(Ws, bs)):
        W, b = np.asarray(W, f32), np.asarray(b, f32)
        acc = np.broadcast_to(b[None, :], (x.shape[0], W.shape[0])).astype(f32)
        tr = np.empty((W.shape[1],) + acc.shape, f32)
        for k in range(W.shape[1]):
            acc = fma(x[:, k:k + 1], W[None, :, k], acc) if counter is None else fma(x[:, k:k + 1], W[None, :, k], acc, counter)
            tr[k] = acc
        traces.append(tr)
        x = acc if l == len(Ws) - 1 else np.where(acc > 0, acc, f32(0.0)).astype(f32)
    return x, traces


def scene_sets(sc, a):
    """(Ws, bs) of the set arena a plays, with the heads as rows 1 (log-std; zeros where the head is state-free) and 2 (value) of
    the output layer -- the tile the kernel with heads computes"""
    p = 0 if sc.sets is None else int(sc.sets[a])
    Ws, bs = [np.asarray(W, f32)[p] for W, _ in sc.layers], [np.asarray(b, f32)[p] for _, b in sc.layers]
    K = Ws[-1].shape[1]
    value, log_std = sc.heads
    lw = np.zeros(K, f32) if log_std[0] is None else np.asarray(log_std[0], f32)[p]
    Ws[-1] = np.stack([Ws[-1][0], lw, np.asarray(value[0], f32)[p]])
    bs[-1] = np.asarray([bs[-1][0], np.asarray(log_std[1], f32)[p], np.asarray(value[1], f32)[p]], f32)
    return Ws, bs


def scene_trace(sc, fma=PS.fmaf32, counter=None, obs=None):
    """dict(mean=, ls_raw=, value= [A, N]; traces= per arena, as mlp_trace returns them) of a scene"""
    obs = np.asarray(sc.obs if obs is None else obs, f32)
    A, N = obs.shape[:2]
    out = dict(mean=np.empty((A, N), f32), ls_raw=np.empty((A, N), f32), value=np.empty((A, N), f32), traces=[])
    for a in range(A):
        o, tr = mlp_trace(obs[a], *scene_sets(sc, a), fma=fma, counter=counter)
        out["mean"][a], out["ls_raw"][a], out["value"][a] = o[:, 0], o[:, 1], o[:, 2]
        out["traces"].append(tr)
    return out


def read_outs(t):
    """the values a probe scene reads out: mean and value"""
    return np.stack([t["mean"], t["value"]])


def restated(sc):
    """(Ws, bs) as actions_reference and evaluate_reference take them"""
    return [W for W, _ in sc.layers], [b for _, b in sc.layers]


def probe_out(P, jm, jv, K=HID):
    """the output layer and the heads of the probe policy: the mean reads unit jm[p], the value unit jv[p]; the log-std is
    state-free, -0.5, and is no read-out"""
    W, vw = np.zeros((P, 1, K), f32), np.zeros((P, K), f32)
    for p in range(P):
        W[p, 0, jm[p]] = 1.0
        vw[p, jv[p]] = 1.0
    return (W, np.zeros((P, 1), f32)), ((vw, np.zeros(P, f32)), (None, np.full(P, -0.5, f32)))


# ---- subnormal ------------------------------------------------------------------------------------------------------------------------------
def subnormal_scene(seed=0, A=3, N=40):
    """Set 0: subnormal weights and biases under normal observations.  Set 1: ordinary weights and a subnormal bias under subnormal
    observations (arena 1) and under observations of 2^-124, whose products lie on both sides of the smallest normal (arena 2).  The
    mean is a one-hot read-out of a hidden unit; the value row of set 1 has ordinary weights and a subnormal bias over the subnormal
    activations, so their products are rounded among the subnormals."""
    rs = np.random.RandomState(seed)
    n = rs.standard_normal
    W0 = np.stack([n((HID, 64)) * 2.0 ** -133, n((HID, 64)) / 8]).astype(f32)
    b0 = np.stack([n(HID) * 2.0 ** -131, n(HID) * 2.0 ** -130]).astype(f32)
    (W1, b1), (value, log_std) = probe_out(2, jm=(3, 5), jv=(8, 0))
    value[0][1] = rs.choice([0.75, -1.5, 1.25, 0.375, -0.625], HID).astype(f32)
    value[1][1] = f32(3e-40)
    obs = n((A, N, 64)).astype(f32)
    obs[1] = (n((N, 64)) * 2.0 ** -131).astype(f32)
    obs[2] = (n((N, 64)) * 2.0 ** -124).astype(f32)
    sc = Scene([(W0, b0), (W1, b1)], np.asarray([0, 1, 1], np.int32)[:A], obs, (value, log_std), n((A, N)).astype(f32))
    t = scene_trace(sc)
    first = np.concatenate([tr[0].reshape(-1) for tr in t["traces"]])
    hidden = np.concatenate([np.where(tr[0][-1] > 0, tr[0][-1], f32(0)).reshape(-1) for tr in t["traces"]])
    through = sum(int((is_subnormal(tr[0]).any(axis=0) & ~is_subnormal(tr[0]).all(axis=0) & is_subnormal(tr[0][-1])).sum())
                  for tr in t["traces"])
    reach = dict(subnormal_obs=int(is_subnormal(obs).sum()), subnormal_weights=int(is_subnormal(W0).sum()),
                 subnormal_bias=int(is_subnormal(b0).sum()), first_layer_subnormal_states=int(is_subnormal(first).sum()),
                 chains_through_and_into_subnormal=through, subnormal_hidden=int(is_subnormal(hidden).sum()),
                 subnormal_means=int(is_subnormal(t["mean"]).sum()), subnormal_values=int(is_subnormal(t["value"]).sum()),
                 rounded_subnormal_values=int(is_subnormal(t["value"][1:]).sum()))
    return sc, reach


def ordinary_set_beside(sc, seed=5):
    """the scene's first weight set with an ordinary one beside it (weights ~ 1 / sqrt(fan-in)), for the rollout: (layers, heads)"""
    rs = np.random.RandomState(seed)
    layers = []
    for W, b in sc.layers:
        o, i = W.shape[1:]
        layers.append((np.stack([W[0], (rs.standard_normal((o, i)) / np.sqrt(i)).astype(f32)]),
                       np.stack([b[0], (0.3 * rs.standard_normal(o)).astype(f32)])))
    K = sc.layers[-1][0].shape[2]
    (vw, vb), (lw, lb) = sc.heads
    value = (np.stack([vw[0], (rs.standard_normal(K) / np.sqrt(K)).astype(f32)]), np.asarray([vb[0], 0.1], f32))
    lw0 = np.zeros(K, f32) if lw is None else lw[0]
    log_std = (np.stack([lw0, (0.5 * rs.standard_normal(K) / np.sqrt(K)).astype(f32)]), np.asarray([lb[0], -0.4], f32))
    return layers, (value, log_std)


# ---- mid-chain overflow ---------------------------------------------------------------------------------------------------------------------
# Unit j of the first layer owns four columns: an aligned group k = 4 s .. 4 s + 3 (one MFMA instruction) for even j, a group that
# starts at 4 s + 2 (two instructions) for odd j.  There its weights are +B, -B, +B, -B with B = FLT_MAX / 2, so an observation of 2
# brings the sum to FLT_MAX exactly and one of 4 past it.
OVERFLOW_START = {0: 0, 1: 6, 2: 12, 3: 18}
OVERFLOW_PATTERNS = [("inf, although the terms cancel", (4, 4, 0, 0)), ("-inf, ReLU: +0", (-4, -4, 0, 0)), ("inf, cancelled three terms later", (4, 0, 0, 4)),
                     ("FLT_MAX and stays", (2, 0, 0, 0)), ("FLT_MAX, then exactly 0", (2, 2, 0, 0)),
                     ("FLT_MAX, then inf by rounding", (2, 0, 2.0 ** -23, 0)), ("FLT_MAX, half an ulp short of inf", (2, 0, 2.0 ** -24, 0)),
                     ("inf four times over", (4, 4, 4, 4)), ("FLT_MAX, 0, FLT_MAX, 0", (2, 2, 2, 2)), ("-inf, cancelled by the next term", (0, 4, 4, 0))]


def overflow_scene(seed=1):
    """64 -> 16 -> 16 -> 1 with finite operands.  Layer 1 is the identity, so an inf of layer 0 meets fifteen zero weights there: NaN by
    the definition, +0 behind the ReLU; the unit's own row passes it on.  Set p reads units 2 p (aligned group) and 2 p + 1; a row
    drives the group of one of them through one pattern.  Where the mean reads an inf the value chain meets inf * 0 and is NaN."""
    rs = np.random.RandomState(seed)
    A, N = 2, 2 * len(OVERFLOW_PATTERNS)
    B = f32(FMAX / f32(2.0))
    W0 = (rs.standard_normal((HID, 64)) / 8).astype(f32)
    for j, s in OVERFLOW_START.items():
        W0[:, s:s + 4] = (rs.standard_normal((HID, 4)) / 64).astype(f32)
        W0[j, s:s + 4] = [B, -B, B, -B]
    W0 = np.stack([W0, W0])
    b0 = np.stack([(0.3 * rs.standard_normal(HID)).astype(f32)] * 2)
    b0[:, :4] = np.abs(b0[:, :4]) + f32(1.0)                   # (the read units start positive: FLT_MAX - FLT_MAX leaves them their tail)
    W1, b1 = np.stack([np.eye(HID, dtype=f32)] * 2), np.zeros((2, HID), f32)
    (W2, b2), heads = probe_out(2, jm=(0, 2), jv=(1, 3))
    obs = (0.5 * rs.standard_normal((A, N, 64))).astype(f32)
    target = np.zeros((A, N), np.int64)
    for a in range(A):
        for i in range(N):
            j = 2 * a + i % 2
            target[a, i] = j
            for jj, s in OVERFLOW_START.items():
                obs[a, i, s:s + 4] = 0.0
            obs[a, i, OVERFLOW_START[j]:OVERFLOW_START[j] + 4] = OVERFLOW_PATTERNS[i // 2][1]
    sc = Scene([(W0, b0), (W1, b1), (W2, b2)], np.asarray([0, 1], np.int32), obs, heads, rs.standard_normal((A, N)).astype(f32))
    t = scene_trace(sc)
    mid_inf, at_max, finite_sums = 0, 0, 0
    for a in range(A):
        tr0 = t["traces"][a][0]
        for i in range(N):
            chain = tr0[:, i, target[a, i]]
            at_max += int((np.abs(chain) == FMAX).any())
            if np.isinf(chain).any():
                mid_inf += 1
                p = int(sc.sets[a])
                exact = Fraction(float(b0[p, target[a, i]])) + sum(Fraction(float(x)) * Fraction(float(w)) for x, w in zip(obs[a, i], W0[p, target[a, i]]))
                finite_sums += int(abs(exact) < Fraction(2) ** 128 - Fraction(2) ** 103)
    l1 = np.concatenate([tr[1][-1].reshape(-1) for tr in t["traces"]])
    reach = dict(chains_with_mid_inf=mid_inf, of_them_with_a_finite_exact_sum=finite_sums, chains_at_flt_max=at_max,
                 nan_behind_inf_times_zero=int(np.isnan(l1).sum()), inf_means=int(np.isinf(t["mean"]).sum()), inf_values=int(np.isinf(t["value"]).sum()),
                 nan_read_outs=int(np.isnan(read_outs(t)).sum()), finite_read_outs=int(np.isfinite(read_outs(t)).sum()),
                 flt_max_read_outs=int((read_outs(t) == FMAX).sum()))
    return sc, reach


# ---- cancellation ---------------------------------------------------------------------------------------------------------------------------
CANCEL_INSIDE, CANCEL_ACROSS = 8, 22      # four-term groups p, q, -p, -q at k = 8 .. 11 (one instruction) and k = 22 .. 25 (two)


def cancellation_scene(seed=2, A=2, N=24):
    """x[2m+1] = x[2m] and W[j][2m+1] = -W[j][2m], bias +0: after a pair the accumulator holds what the first product's rounding left,
    and so on through 64 columns.  Two four-term groups p, q, -p, -q stand among the pairs.  Unit 2 i + 1 has the weights of unit 2 i
    negated: every rounding error comes out with the other sign, so one unit of each pair passes the ReLU.  Only a fused multiply-add
    that rounds after every k gives these sums."""
    rs = np.random.RandomState(seed)
    signed = lambda shape: (rs.uniform(1.0, 2.0, shape) * rs.choice([-1.0, 1.0], shape)).astype(f32)   # one binade: the products are of one size
    half = signed((HID // 2, 32))
    W = np.empty((HID // 2, 64), f32)
    W[:, 0::2], W[:, 1::2] = half, -half
    for s in (CANCEL_INSIDE, CANCEL_ACROSS):
        W[:, s + 2], W[:, s + 1], W[:, s + 3] = -W[:, s], half[:, s // 2 + 1], -half[:, s // 2 + 1]
    W0 = np.empty((1, HID, 64), f32)
    W0[0, 0::2], W0[0, 1::2] = W, -W
    b0 = np.zeros((1, HID), f32)
    (W1, b1), heads = probe_out(1, jm=(4,), jv=(5,))
    x = signed((A, N, 32))
    obs = np.repeat(x, 2, axis=2)
    for s in (CANCEL_INSIDE, CANCEL_ACROSS):
        obs[:, :, s:s + 4] = obs[:, :, s:s + 1]
    sc = Scene([(W0, b0), (W1, b1)], None, obs, heads, rs.standard_normal((A, N)).astype(f32))
    t = scene_trace(sc)
    small, total = 0, 0
    for a in range(A):
        tr = t["traces"][a][0]
        for m in range(32):
            if any(s <= 2 * m < s + 4 for s in (CANCEL_INSIDE, CANCEL_ACROSS)):
                continue
            after = np.abs(tr[2 * m + 1].astype(f64))
            prod = np.abs(obs[a][:, 2 * m:2 * m + 1].astype(f64) * W0[0][None, :, 2 * m].astype(f64))
            small += int(((after > 0) & (after < prod * 2.0 ** -20)).sum())
            total += after.size
    groups = []
    for s in (CANCEL_INSIDE, CANCEL_ACROSS):
        after = np.concatenate([np.abs(t["traces"][a][0][s + 3]).reshape(-1) for a in range(A)])
        groups.append(float(((after > 0) & (after < 2.0 ** -18)).mean()))
    ro = read_outs(t)
    reach = dict(pairs_small_and_nonzero=small / total, groups_small_and_nonzero=groups, positive_read_outs=int((ro > 0).sum()), read_outs=ro.size)
    return sc, reach


# ---- ties -----------------------------------------------------------------------------------------------------------------------------------
TIE_KINDS = ("normal tie", "normal, one float64 ulp off", "subnormal tie", "subnormal, one float64 ulp off")


def ties_scene(seed=3, A=3, N=32):
    """Layer 0 copies the first sixteen observation columns (identity rows, bias +0; they are positive), so the output chains run over
    values the row chooses: the mean is fmaf(x[k], c[k], x[0]) for the one k in 1 .. 4 where the row is not zero, the value
    fmaf(x[k], -c[k], x[0]).  Per row b = x[0] is a random fp32 and x[k] * c[k] is
      k = 1: (2 n + 1) half ulps of b exactly: the sum is a midpoint, from below for the mean and from above for the value;
      k = 2: (1 + 2^-23) (1 - 2^-23) half ulps: 2^-46 of a half ulp short of the midpoint -- the float64 sum cannot hold that
             and sits on the midpoint (the constructor of tests/test_policy_cpu.py::test_fmaf_agrees_with_exact_rationals);
      k = 3, 4: the same two among the subnormals, b = m 2^-149 and half an ulp = 2^-150.
    Three of four b of the rows that are one float64 ulp off are odd: rounding the float64 sum would go to the even neighbour, wrongly."""
    rs = np.random.RandomState(seed)
    W0, b0 = np.zeros((1, HID, 64), f32), np.zeros((1, HID), f32)
    W0[0, :, :HID] = np.eye(HID, dtype=f32)
    c = np.zeros(HID, f32)
    c[0], c[1], c[2], c[3], c[4] = 1.0, 2.0 ** -12, 2.0 ** -24 * (1 - 2.0 ** -23), 2.0 ** -75, 2.0 ** -75 * (1 - 2.0 ** -23)
    W1, b1 = c.reshape(1, 1, HID).copy(), np.zeros((1, 1), f32)
    vw = -c
    vw[0] = 1.0
    heads = ((vw.reshape(1, HID), np.zeros(1, f32)), (None, np.full(1, -0.5, f32)))
    obs = np.zeros((A, N, 64), f32)
    kind = np.arange(A * N).reshape(A, N) % 4
    for a in range(A):
        for i in range(N):
            kd = int(kind[a, i])
            base, odd = int(rs.randint(2 ** 22 + 256, 2 ** 23 - 256)), (1 if kd % 2 == 1 and (i // 4) % 4 != 3 else int(rs.randint(2)))
            m = base * 2 + odd                                                               # 24 bits, 50 ulps from either end of its binade
            n = int(rs.randint(0, 50))
            if kd < 2:
                q = int(rs.randint(-20, 21))
                obs[a, i, 0] = f32(m * 2.0 ** (q - 23))                                     # b in [2^q, 2^(q+1)): half an ulp is 2^(q-24)
                obs[a, i, 1 + kd] = f32((2 * n + 1) * 2.0 ** (q - 12)) if kd == 0 else f32((1 + 2.0 ** -23) * 2.0 ** q)
            else:
                obs[a, i, 0] = f32(((base >> 2) * 2 + odd) * 2.0 ** -149)                    # 2^21 <= m < 2^22
                obs[a, i, 1 + kd] = f32((2 * n + 1) * 2.0 ** -75) if kd == 2 else f32((1 + 2.0 ** -23) * 2.0 ** -75)
    assert (obs >= 0).all()
    sc = Scene([(W0, b0), (W1, b1)], None, obs, heads, rs.standard_normal((A, N)).astype(f32))
    count = []
    t = scene_trace(sc, counter=count)
    ro = read_outs(t)
    k = np.broadcast_to(kind, ro.shape)
    reach = dict(exact_path_elements=int(sum(count)), positive_read_outs=int((ro > 0).sum()), read_outs=ro.size,
                 normal_read_outs=int(((k < 2) & (ro >= TINY)).sum()), subnormal_read_outs=int(((k >= 2) & is_subnormal(ro)).sum()))
    return sc, reach


# ---- signed zeros ---------------------------------------------------------------------------------------------------------------------------
def zeros_scene(seed=4, A=2, N=16):
    """Set 0 is the probe policy.  Set 1 reads through -1.0 from a -0 bias with every other output weight -0: where the unit is +0
    every product is -0 and so is the mean; a ReLU that let -0 through would make it +0.  Rows: ordinary ones, all +0, all -0, -0
    scattered among ordinary values; first-layer biases are -0, +0 and ordinary; units 0 .. 3 have positive weights only, so a row of
    -0 keeps their chains at -0 from a -0 bias."""
    rs = np.random.RandomState(seed)
    W0 = (rs.standard_normal((HID, 64)) / 8).astype(f32)
    W0[:4] = np.abs(W0[:4])
    W0[4:, ::7] = 0.0
    W0[4:, 3::11] = -0.0
    b0 = (0.3 * rs.standard_normal(HID)).astype(f32)
    b0[[0, 1, 4]], b0[[2, 5]] = -0.0, 0.0
    W0, b0 = np.stack([W0, W0]), np.stack([b0, b0])
    (W1, b1), (value, log_std) = probe_out(2, jm=(0, 1), jv=(4, 6))
    W1[1], b1[1] = -0.0, -0.0
    W1[1, 0, 1] = -1.0
    value[0][1], value[1][1] = -0.0, -0.0
    value[0][1, 6] = -1.0
    obs = rs.standard_normal((A, N, 64)).astype(f32)
    obs[:, 0], obs[:, 1] = 0.0, -0.0
    obs[:, 2] = -np.abs(obs[:, 2])                          # units 0 .. 3 go negative: ReLU gives +0
    obs[:, 3, ::2] = -0.0
    obs[:, 4] = np.where(rs.uniform(size=(A, 64)) < 0.5, f32(-0.0), f32(0.0))
    obs[:, 5] = -0.0
    obs[:, 5, 9] = 2.0 ** -140
    eps = rs.standard_normal((A, N)).astype(f32)
    eps[:, 0::3], eps[:, 1::3] = -0.0, 0.0
    sc = Scene([(W0, b0), (W1, b1)], np.asarray([0, 1], np.int32), obs, (value, log_std), eps)
    t = scene_trace(sc)
    neg_zero = lambda v: int((bits(v) == 0x80000000).sum())
    states = np.concatenate([tr[0].reshape(-1) for tr in t["traces"]])
    relu_in = np.concatenate([tr[0][-1].reshape(-1) for tr in t["traces"]])
    zero_row = PS.mlp_reference(np.zeros((1, 64), f32), [W0[0], W1[0]], [b0[0], b1[0]])
    reach = dict(negative_zero_obs=neg_zero(obs), negative_zero_states=neg_zero(states), negative_zero_into_relu=neg_zero(relu_in),
                 negative_zero_means=neg_zero(t["mean"]), negative_zero_values=neg_zero(t["value"]), positive_zero_means=int((bits(t["mean"]) == 0).sum()),
                 zero_row_is_the_bias_chain=bool(same_bits(t["mean"][0, 0], zero_row[0])))
    return sc, reach


# ---- row isolation --------------------------------------------------------------------------------------------------------------------------
POISON = [(0, 0, 5, np.nan), (0, 15, 0, np.inf), (0, 16, 63, -np.inf), (0, 31, 17, np.nan), (1, 7, 33, np.inf)]   # (arena, row, column, value)


def isolation_scene(seed=6, A=3, N=32, hidden=(32,), clean=False):
    """Ordinary weights, two sets, sets [0, 1, 0]: a tile is one arena's 32 rows.  Arena 0 has a NaN, +inf, -inf and a NaN in one
    element each of rows 0, 15, 16 and 31, arena 1 -- the other set -- one +inf in row 7; every other row is standard normal.
    clean=True: the same scene with the poisoned rows zeroed."""
    rs = np.random.RandomState(seed)
    widths = (64,) + tuple(hidden) + (1,)
    layers = [((rs.standard_normal((2, o, i)) / np.sqrt(i)).astype(f32), (0.3 * rs.standard_normal((2, o))).astype(f32))
              for i, o in zip(widths[:-1], widths[1:])]
    K = hidden[-1]
    value = ((rs.standard_normal((2, K)) / np.sqrt(K)).astype(f32), (0.2 * rs.standard_normal(2)).astype(f32))
    log_std = ((0.5 * rs.standard_normal((2, K)) / np.sqrt(K)).astype(f32), (-0.5 + 0.2 * rs.standard_normal(2)).astype(f32))
    obs = rs.standard_normal((A, N, 64)).astype(f32)
    eps = rs.standard_normal((A, N)).astype(f32)
    poisoned = np.zeros((A, N), bool)
    for a, i, k, v in POISON:
        poisoned[a, i] = True
        if clean:
            obs[a, i] = 0.0
        else:
            obs[a, i, k] = v
    sc = Scene(layers, np.asarray([0, 1, 0], np.int32)[:A], obs, (value, log_std), eps)
    if clean:
        return sc, dict(poisoned=poisoned)
    t = scene_trace(sc)
    ref = scene_trace(isolation_scene(seed, A, N, hidden, clean=True)[0])
    res = np.stack([t["mean"], t["ls_raw"], t["value"]])
    res0 = np.stack([ref["mean"], ref["ls_raw"], ref["value"]])
    marked = []                 # a poisoned row's results are not finite, or they are what the ReLU's clamp of a NaN to +0 leaves:
    for a, i, k, v in POISON:   # the chain of the output biases, which is the zeroed row's only if every hidden bias is <= 0
        p = int(sc.sets[a])
        clamped = np.asarray([layers[-1][1][p, 0], log_std[1][p], value[1][p]], f32)
        marked.append(bool(not np.isfinite(res[:, a, i]).all() or (np.isnan(v) and same_bits(res[:, a, i], clamped))))
    reach = dict(poisoned=poisoned, poisoned_rows_marked=marked, poisoned_rows_differ=[bool(not same_bits(res[:, a, i], res0[:, a, i])) for a, i, _, _ in POISON],
                 others_finite=bool(np.isfinite(res[:, ~poisoned]).all()), others_equal_clean=bool(same_bits(res[:, ~poisoned], res0[:, ~poisoned])))
    return sc, reach


# ---- the heads' epilogue --------------------------------------------------------------------------------------------------------------------
LS_CASES = [("-20", -20.0), ("-20 - ulp", ulp_down(-20.0)), ("-20 + ulp", ulp_up(-20.0)), ("2", 2.0), ("2 - ulp", ulp_down(2.0)), ("2 + ulp", ulp_up(2.0)),
            ("+inf", np.inf), ("-inf", -np.inf), ("NaN", np.nan)]
EPS_CASES = [0.0, -0.0, 1e-42, 1e20, np.inf, -np.inf, 0.7]


def epilogue_scene(seed=7):
    """64 -> 16 -> 1, one set, ordinary weights on columns 3 .. 63.  Units 0, 1, 2 read 2 x[0], 2 x[1], 2 x[2] (x: the observation) and
    the log-std row is +1 on unit 0, -1 on unit 1, 0 on unit 2, bias +0: ls_raw = 2 x[0] or -2 x[1] exactly, +inf / -inf where that
    doubling overflows, NaN where unit 2 overflows and meets its zero weight.  The mean and the value give units 0 .. 2 a zero
    weight: they are ordinary while those are finite and NaN beside an inf.  Every ls case meets every eps case.  Two more rows have
    ls_raw = 0 (std = 1) over one observation, with eps = +0 and eps = -2 mean: u = mean and u = -mean exactly, and limit = |mean|."""
    rs = np.random.RandomState(seed)
    n_rows = len(LS_CASES) * len(EPS_CASES) + 2
    A, N = 2, (n_rows + 1) // 2
    W0 = (rs.standard_normal((1, HID, 64)) / 8).astype(f32)
    W0[0, :, :3] = 0.0
    W0[0, :3] = 0.0
    W0[0, 0, 0] = W0[0, 1, 1] = W0[0, 2, 2] = 2.0
    b0 = (0.3 * rs.standard_normal((1, HID))).astype(f32)
    b0[0, :3] = 0.0
    W1 = (rs.standard_normal((1, 1, HID)) / 4).astype(f32)
    vw = (rs.standard_normal((1, HID)) / 4).astype(f32)
    lw = np.zeros((1, HID), f32)
    W1[0, 0, :3], vw[0, :3] = 0.0, 0.0
    lw[0, 0], lw[0, 1] = 1.0, -1.0
    b1 = np.asarray([[0.2]], f32)
    heads = ((vw, np.asarray([-0.1], f32)), (lw, np.zeros(1, f32)))
    obs = rs.standard_normal((A * N, 64)).astype(f32)
    obs[:, :3] = 0.0
    eps = np.zeros(A * N, f32)
    want_ls = np.zeros(A * N, f32)
    r = 0
    for _, ls in LS_CASES:
        for e in EPS_CASES:
            if np.isnan(ls):
                obs[r, 2] = 3e38
            elif np.isinf(ls):
                obs[r, 0 if ls > 0 else 1] = 3e38
            else:
                obs[r, 0 if ls > 0 else 1] = f32(abs(f32(ls)) / f32(2.0))
            want_ls[r], eps[r] = ls, e
            r += 1
    obs[r + 1] = obs[r]
    sc = Scene([(W0, b0), (W1, b1)], None, obs.reshape(A, N, 64), heads, eps.reshape(A, N))
    mean = scene_trace(sc)["mean"].reshape(-1)
    eps[r], eps[r + 1] = 0.0, f32(-2.0) * mean[r]
    sc = sc._replace(eps=eps.reshape(A, N))
    t = scene_trace(sc)
    limit = float(abs(mean[r]))
    with np.errstate(all="ignore"):
        s = PP.sample_reference(t["mean"], t["ls_raw"], sc.eps, True, "clip", limit)
    u = s["u"].reshape(-1)
    got_ls = t["ls_raw"].reshape(-1)[:r]
    reach = dict(limit=limit, ls_raw_as_planned=bool(same_bits(np.where(np.isnan(got_ls), f32(0), got_ls), np.where(np.isnan(want_ls[:r]), f32(0), want_ls[:r]))
                                                     and np.array_equal(np.isnan(got_ls), np.isnan(want_ls[:r]))),
                 u_at_plus_limit=bool(max(u[r], u[r + 1]) == f32(limit)), u_at_minus_limit=bool(min(u[r], u[r + 1]) == -f32(limit)), nan_u=int(np.isnan(u).sum()),
                 nan_u_clips_to_minus_limit=bool((s["actions"].reshape(-1)[np.isnan(u)] == -f32(limit)).all()),
                 logp_minus_inf=int(np.isneginf(s["logp"]).sum()), clamped_low=int((t["ls_raw"] < -20).sum()), clamped_high=int((t["ls_raw"] > 2).sum()),
                 finite_means=int(np.isfinite(t["mean"]).sum()))
    return sc, reach


# name -> (builder, the comparison tolerates NaNs of any payload, out modes)
SCENES = collections.OrderedDict([
    ("subnormal", (subnormal_scene, False)), ("overflow", (overflow_scene, True)), ("cancellation", (cancellation_scene, False)),
    ("ties", (ties_scene, False)), ("zeros", (zeros_scene, False)), ("isolation", (isolation_scene, True)), ("epilogue", (epilogue_scene, True))])


# ---- wrong fused multiply-adds, for the checks that a scene can tell -------------------------------------------------------------------------
def fma_flushing(a, b, c, counter=None):
    """fmaf32 with subnormal operands flushed to zero (sign kept)"""
    flush = lambda v: np.where(is_subnormal(v), np.copysign(f32(0), v), v).astype(f32)
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    return PS.fmaf32(flush(a), flush(b), flush(c))


def fma_unfused(a, b, c, counter=None):
    """round(a * b) + c: two roundings"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return ((np.asarray(a, f32) * np.asarray(b, f32)).astype(f32) + np.asarray(c, f32)).astype(f32)


def fma_double_rounding(a, b, c, counter=None):
    """the float64 sum rounded again, the midpoint hazard ignored"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)
