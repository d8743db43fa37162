"""The reference of the reward terms (include/ca_env.h ca_reward_desc, csrc/ca_reward.h), built on tests/contact_scenes.py.

A numpy fp32 restatement, one numpy operation per kernel operation: the pair and wall distances are contact_scenes' (absSq,
distSqPointSegment), the comfort tests add `(r_i + r_j) + margin` and `r_i + margin` in that order, and the weighted sum is one
multiply, then one multiply and one add per term whose weight is not zero.  tests/test_reward_terms_cpu.py ties it to the unchanged
oracle and to exact rationals; tests/test_gpu_reward_terms.py compares the kernel with it bit for bit."""
from fractions import Fraction

import numpy as np

from tests import contact_scenes as CS

F = np.float32
TERMS = ("base", "collision", "wall", "near", "wall_near", "arrival", "step")
COUNTS = TERMS[1:]
N_TERMS = 7


def _f(x):
    return np.asarray(x, F)


def geometry_counts(px, py, radius, tables, margin, counts=None):
    """c1 .. c4 of positions px, py [A, N]: dict(collision, wall, near, wall_near) of int32 [A, N]; absent rows read 0."""
    px, py = _f(px), _f(py)
    A, N = px.shape
    rad = np.ascontiguousarray(np.broadcast_to(_f(radius), (A, N)))
    m = F(margin)
    counts = np.full(A, N, np.int64) if counts is None else np.asarray(counts, np.int64)
    rep = CS.reference(px, py, rad, tables, counts)
    out = dict(collision=rep["agents"].astype(np.int32), wall=rep["wall"].astype(np.int32), near=np.zeros((A, N), np.int32),
               wall_near=np.zeros((A, N), np.int32))
    for a in range(A):
        n = int(counts[a])
        x, y, r = px[a, :n], py[a, :n], rad[a, :n]
        d2 = CS.abs_sq(_f(x[:, None] - x[None, :]), _f(y[:, None] - y[None, :]))
        cr = _f(_f(r[:, None] + r[None, :]) + m)                                  # (r_i + r_j) + margin
        out["near"][a, :n] = ((d2 < _f(cr * cr)) & ~np.eye(n, dtype=bool)).sum(1)
        rm = _f(r + m)                                                            # r_i + margin
        out["wall_near"][a, :n] = rep["wall_d2"][a, :n] < _f(rm * rm)             # the smallest distance (inf without edges)
    return out


def weighted_sum(r_ref, c, weights):
    """r = w0 * r_ref; for k = 1 .. 6 ascending, where w_k != 0: r = r + w_k * (float)c_k.  r_ref [A, N] f32, c a list of six int
    [A, N], weights [A, 7] f32."""
    w = _f(weights)
    r = _f(w[:, 0:1] * _f(r_ref))
    for k in range(1, N_TERMS):
        wk = w[:, k:k + 1]
        with np.errstate(all="ignore"):
            nxt = _f(r + _f(wk * np.asarray(c[k - 1]).astype(F)))
        r = np.where(wk != 0, nxt, r).astype(F)
    return r


def full_weights(weights, A):
    w = _f(weights)
    return np.ascontiguousarray(np.broadcast_to(w, (A, N_TERMS)) if w.ndim == 1 else w).astype(F)


def shaped_reference(px, py, radius, tables, r_ref, weights, margin, arrival, step, counts=None, advanced=None, respawned=None):
    """What reward_terms_kernel leaves behind a step that left positions px, py [A, N] and the reference reward r_ref [A, N].
    weights [7] or [A, 7]; arrival, step: c5, c6 as the test derives them from the done flags (arrival_counts below); counts: agents
    per arena; advanced [A] bool: arenas the step advanced (None: all); respawned [A] bool: arenas the step respawned, whose c1 .. c4
    are 0 (None: none).  Returns dict(reward, ref, collision, ..., step, written): `written` [A, N] marks the rows the kernel writes
    -- the present rows of advanced arenas --, and elsewhere reward is r_ref and the counts are 0.  A count whose weight is 0 in every
    arena is 0."""
    px = _f(px)
    A, N = px.shape
    w = full_weights(weights, A)
    cnt = np.full(A, N, np.int64) if counts is None else np.asarray(counts, np.int64)
    adv = np.ones(A, bool) if advanced is None else np.asarray(advanced, bool)
    resp = np.zeros(A, bool) if respawned is None else np.asarray(respawned, bool)
    written = (np.arange(N)[None, :] < cnt[:, None]) & adv[:, None]
    g = geometry_counts(px, py, radius, tables, margin, cnt)
    c = [g["collision"], g["wall"], g["near"], g["wall_near"], np.asarray(arrival, np.int32), np.asarray(step, np.int32)]
    for k in range(4):
        c[k] = np.where(resp[:, None], 0, c[k])
    for k in range(6):
        c[k] = np.where(written & (w[:, k + 1] != 0).any(), c[k], 0).astype(np.int32)
    r_ref = _f(r_ref)
    out = dict(reward=np.where(written, weighted_sum(r_ref, c, w), r_ref).astype(F), ref=r_ref, written=written)
    out.update({name: c[k] for k, name in enumerate(COUNTS)})
    return out


def arrival_counts(done_mode_regoal, saved, after, counts=None, respawned=None, lastep_arrived=None):
    """(c5, c6) [A, N].  saved: agent_done (modes 0 / 1) or regoal_count (CA_DONE_REGOAL) in front of the step; after: the same field
    behind it.  respawned [A] bool and lastep_arrived [A] (the low half of the arena's last-episode word): in modes 0 / 1 an agent
    of a respawned arena with saved == 0 arrived iff every agent of the arena did."""
    saved, after = np.asarray(saved), np.asarray(after)
    A, N = saved.shape
    if done_mode_regoal:
        return (saved != after).astype(np.int32), np.ones((A, N), np.int32)
    arrived = (saved == 0) & (after != 0)
    if respawned is not None and np.asarray(respawned).any():
        cnt = np.full(A, N, np.int64) if counts is None else np.asarray(counts, np.int64)
        all_in = np.asarray(lastep_arrived, np.int64) == cnt
        arrived = np.where(np.asarray(respawned, bool)[:, None], (saved == 0) & all_in[:, None], arrived)
    return arrived.astype(np.int32), (saved == 0).astype(np.int32)


# ---- exact arithmetic -------------------------------------------------------------------------------------------------------------
def round_f32(q):
    """the float32 nearest to the rational q, ties to even: one IEEE rounding, from exact arithmetic"""
    q = Fraction(q)
    x = F(float(q))                                        # near q; the true rounding is x or a neighbour
    cands = [np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))]
    cands = [c for c in cands if np.isfinite(c)]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - q), int(c.view(np.uint32)) & 1))
    if best == 0 and q == 0:
        return F(0.0)
    return best


def exact_weighted_sum(r_ref, c, w):
    """the definition on scalars in exact rationals with one rounding per operation; the sign of a zero product follows IEEE"""
    def mul(a, b):
        a, b = F(a), F(b)
        if a == 0 or b == 0:
            return F(-0.0) if (np.signbit(a) != np.signbit(b)) else F(0.0)
        return round_f32(Fraction(float(a)) * Fraction(float(b)))

    def add(a, b):
        a, b = F(a), F(b)
        s = Fraction(float(a)) + Fraction(float(b))
        if s == 0:
            return F(-0.0) if (np.signbit(a) and np.signbit(b)) else F(0.0)
        return round_f32(s)
    r = mul(w[0], r_ref)
    for k in range(1, N_TERMS):
        if F(w[k]) != 0:
            r = add(r, mul(w[k], F(c[k - 1])))
    return r


# ---- hand-made states -------------------------------------------------------------------------------------------------------------
def boundary_pairs(R, margin):
    """contact_scenes.boundary_pairs about the comfort distance: pairs at exactly (R + R) + margin along x, one ulp inside and one ulp
    outside, and three coincident agents.  px, py [1, 9]."""
    cr = F(F(R) + F(R)) + F(margin)
    xs, ys = [], []
    for k, x1 in enumerate((cr, CS.ulp_in(cr, 0.0), CS.ulp_in(cr, 100.0))):
        xs += [F(0.0), x1]; ys += [F(10 * k), F(10 * k)]
    xs += [F(40.25)] * 3; ys += [F(-7.5)] * 3
    return _f(xs)[None, :], _f(ys)[None, :]


def wall_cases(R, margin):
    """contact_scenes.wall_cases about R + margin: at, one ulp inside and one ulp outside, on each of the three branches of
    distSqPointSegment (tables of CS.WALL).  px, py [1, 9]."""
    d0 = F(F(R) + F(margin))
    xs, ys = [], []
    for d in (d0, CS.ulp_in(d0, 0.0), CS.ulp_in(d0, 100.0)):
        xs += [F(1.5), F(-d), F(10.0)]
        ys += [d, F(0.0), F(-d)]
    return _f(xs)[None, :], _f(ys)[None, :]


def tile_scene(px, py, A, N, spread=100.0):
    """a hand-made one-arena scene [1, n] put into every arena of an A x N handle: the other rows far away and far from each other"""
    n = px.shape[1]
    assert n <= N
    X = np.empty((A, N), F); Y = np.empty((A, N), F)
    X[:, :n], Y[:, :n] = px[0], py[0]
    extra = np.arange(N - n, dtype=np.float64)
    X[:, n:] = (F(500.0) + extra * spread).astype(F)
    Y[:, n:] = F(900.0)
    return X, Y
