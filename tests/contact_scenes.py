"""Scenes and the reference of the per-agent contact report (include/ca_env.h ca_get_contacts, csrc/ca_contact.h).

The reference is a numpy fp32 restatement of the oracle's arena_collisions / distSqPointSegment (oracle/ca_oracle.cpp): float32
arrays, one numpy operation per oracle operation -- dx*dx + dy*dy, r_i + r_j, the three branches of distSqPointSegment with
a + r*(b - a) -- so its bits are the kernel's.  tests/test_contacts_cpu.py checks it against the unchanged oracle's per-arena
totals; tests/test_gpu_contacts.py compares the kernel with it bit for bit."""
import numpy as np

F = np.float32
INF = F(np.inf)
PLANES = ("agents", "wall", "nearest", "nearest_d2", "wall_d2")


def _f(x):
    return np.asarray(x, F)


def abs_sq(dx, dy):
    """ca_math.h absSq: x*x + y*y, each operation rounded to fp32"""
    return (_f(dx * dx) + _f(dy * dy)).astype(F)


def dist_sq_point_segment(edges, cx, cy):
    """ca_math.h / ca_oracle.cpp distSqPointSegment(a, b, c) for edges [E, 4] = (ax, ay, bx, by) and points cx, cy [P]: [P, E]"""
    e = _f(edges).reshape(-1, 4)
    ax, ay, bx, by = (e[None, :, k] for k in range(4))
    cx, cy = _f(cx)[:, None], _f(cy)[:, None]
    ux, uy = _f(bx - ax), _f(by - ay)            # b - a
    wx, wy = _f(cx - ax), _f(cy - ay)            # c - a
    with np.errstate(all="ignore"):
        r = _f(_f(_f(wx * ux) + _f(wy * uy)) / _f(_f(ux * ux) + _f(uy * uy)))   # dot(c - a, b - a) / absSq(b - a)
        da = abs_sq(wx, wy)                                                      # r < 0: absSq(c - a)
        db = abs_sq(_f(cx - bx), _f(cy - by))                                    # r > 1: absSq(c - b)
        qx, qy = _f(ax + _f(r * ux)), _f(ay + _f(r * uy))                        # a + r * (b - a)
        dm = abs_sq(_f(cx - qx), _f(cy - qy))
    return np.where(r < 0, da, np.where(r > 1, db, dm)).astype(F)


def table_edges(tab):
    """[E, 4] edges of a processed table: dict(verts [n, 2], next) of VecCollisionAvoidanceEnv.obstacle_table, or dict(px, py, next)
    of the oracle's"""
    if "verts" in tab:
        v = _f(tab["verts"]).reshape(-1, 2)
    else:
        v = np.stack([_f(tab["px"]), _f(tab["py"])], 1)
    nxt = np.asarray(tab["next"], np.int64)
    return np.concatenate([v, v[nxt]], 1).astype(F) if len(v) else np.zeros((0, 4), F)


def tables_of(env, A):
    """the edges of every arena of a GPU handle or an OracleEnv"""
    return [table_edges(env.obstacle_table(arena=a)) for a in range(A)]


def reference(px, py, radius, tables, counts=None):
    """The report of positions px, py [A, N], radii `radius` (a scalar or [A, N]), edge tables `tables` ([E, 4], or one per arena) and
    agents per arena `counts` ([A] or None): dict of the five [A, N] planes."""
    px, py = _f(px), _f(py)
    A, N = px.shape
    rad = np.ascontiguousarray(np.broadcast_to(_f(radius), (A, N)))
    counts = np.full(A, N, np.int64) if counts is None else np.asarray(counts, np.int64)
    out = dict(agents=np.zeros((A, N), np.int32), wall=np.zeros((A, N), np.int32), nearest=np.full((A, N), -1, np.int32),
               nearest_d2=np.full((A, N), INF, F), wall_d2=np.full((A, N), INF, F))
    for a in range(A):
        n = int(counts[a])
        x, y, r = px[a, :n], py[a, :n], rad[a, :n]
        d2 = abs_sq(_f(x[:, None] - x[None, :]), _f(y[:, None] - y[None, :]))     # absSq(p_i - p_j)
        cr = _f(r[:, None] + r[None, :])                                          # r_i + r_j
        other = ~np.eye(n, dtype=bool)                                            # j != i by index: coincident agents count
        out["agents"][a, :n] = ((d2 < _f(cr * cr)) & other).sum(1)
        if n > 1:
            key = np.where(other, d2, INF)
            j = np.argmin(key, 1)                                                 # the first minimum: ties go to the smaller index
            out["nearest"][a, :n] = j
            out["nearest_d2"][a, :n] = key[np.arange(n), j]
        e = tables[a] if isinstance(tables, (list, tuple)) else tables
        if len(e):
            dw = dist_sq_point_segment(e, x, y)
            out["wall"][a, :n] = (dw < _f(r * r)[:, None]).any(1)
            out["wall_d2"][a, :n] = dw.min(1)
    return out


def assert_report(got, want, what):
    """all five planes, bit for bit"""
    from tests import helpers as H
    for k in PLANES:
        g = got[k]
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        H._eq(g, want[k], "%s: %s" % (what, k))


# ---- hand-made states ------------------------------------------------------------------------------------------------------
def ulp_in(v, toward):
    return np.nextafter(F(v), F(toward))


def boundary_pairs(R=0.5):
    """One arena, radius R.  Pairs at distance exactly r_i + r_j along x (d2 == sqr(cr): not touching), one ulp inside and one ulp
    outside (np.nextafter on one coordinate), and three coincident agents (d2 == 0: each counts the two others).  Far apart from
    each other so that nothing else overlaps.  Returns px, py [1, N]."""
    cr = F(R) + F(R)
    xs, ys = [], []
    for k, x1 in enumerate((cr, ulp_in(cr, 0.0), ulp_in(cr, 10.0))):   # at, inside, outside
        xs += [F(0.0), x1]; ys += [F(10 * k), F(10 * k)]
    xs += [F(40.25)] * 3; ys += [F(-7.5)] * 3                          # coincident
    return _f(xs)[None, :], _f(ys)[None, :]


def nearest_cases():
    """One arena with radii of its own:
       - agents 0, 1, 2: 1 and 2 at the same squared distance from 0 (mirror images): 0's nearest is 1, the smaller index;
       - agents 3, 4, 5: 3 is small, 4 a small agent 1.5 away (no overlap: 0.2 + 0.2), 5 a large one 2.0 away that does overlap
         (0.2 + 1.9): the nearest neighbour of 3 is not the one it touches.
    Returns px, py, radius [1, 6]."""
    px = _f([[0.0, 1.25, -1.25, 20.0, 21.5, 18.0]])
    py = _f([[0.0, 0.5, -0.5, 5.0, 5.0, 5.0]])
    rad = _f([[0.3, 0.3, 0.3, 0.2, 0.2, 1.9]])
    return px, py, rad


WALL = [[(0.0, 0.0), (4.0, 0.0)], [(10.0, 0.0), (10.0, 4.0)]]   # two-vertex "polygons": each segment as an edge and its reverse


def wall_cases(R=0.5):
    """Agents around the segments (0,0)-(4,0) and (10,0)-(10,4), radius R, far enough from each other not to matter for the walls:
    at distance exactly R, one ulp inside and one ulp outside R (np.nextafter on one coordinate) from an interior point of the first
    (the projection branch), beyond its end point (0,0) on its line, and beyond the end point (10,0) of the second on its line (the
    r < 0 branch of an edge and the r > 1 branch of its reverse).  The end points have a zero in the coordinate that carries the
    distance, so that the ulp survives the subtraction.  Returns px, py [1, 9]."""
    R = F(R)
    xs, ys = [], []
    for d in (R, ulp_in(R, 0.0), ulp_in(R, 10.0)):
        xs += [F(1.5), F(-d), F(10.0)]            # above the first edge | left of (0,0) | below (10,0)
        ys += [d, F(0.0), F(-d)]
    return _f(xs)[None, :], _f(ys)[None, :]


DOORWAY_CENTRE = (2.25, 5.0)   # the gap of the reference env's doorway world: its two pillars and, 5 away, the outer walls


def random_state(A, N, seed, centre=DOORWAY_CENTRE):
    """A crowded box around `centre` -- side 1.2 sqrt(N) up to 12, so that agents of radius 0.5 overlap a few others each and some
    lie on the walls of the doorway world --, with agent N - 1 on top of agent 0 (d2 == 0).  px, py [A, N] float32."""
    rng = np.random.RandomState(seed)
    half = F(min(6.0, max(1.0, 0.6 * np.sqrt(N))))
    px = (F(centre[0]) + rng.uniform(-half, half, (A, N)).astype(F)).astype(F)
    py = (F(centre[1]) + rng.uniform(-half, half, (A, N)).astype(F)).astype(F)
    if N >= 4:
        px[:, N - 1], py[:, N - 1] = px[:, 0], py[:, 0]
    return px, py


def doorway_actions(A, N, seed, steps):
    """the actions of the doorway runs: `steps` draws of uniform(-1, 1) [A, N] from RandomState(seed)"""
    rng = np.random.RandomState(seed)
    for s in range(steps):
        yield s, rng.uniform(-1, 1, (A, N)).astype(F)
