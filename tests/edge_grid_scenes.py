"""Scenes of the static edge grid (ca_tiled_edge_grid; csrc/ca_edge_grid_host.h builds it, csrc/ca_tiled.h walks it) and a numpy
fp32 restatement of what include/ca_env.h and csrc/ca_math.h write down: the cell expression, the walk with its corner rule, and
distSqPointSegment.  tests/test_edge_grid_cpu.py checks the builder with them by brute force, without a device;
tests/test_gpu_edge_grid.py runs the hall worlds on a grid handle against the CPU oracle."""
import numpy as np

from collision_avoidance_amd import scenarios

F = np.float32


# ---- the worlds ---------------------------------------------------------------------------------------------------------------
def hall(N, shift=(0.0, 0.0)):
    """The crowd's enclosing box (clockwise, as tests/tiled_scenes.two_boxes) with counter-clockwise 0.5 x 0.5 pillars at 1.25 + 3 k on
    both axes: N = 300 -> 122 polygons, 488 edges; N = 1100 -> 1940 edges."""
    e = scenarios.crowd_envsize(N)
    sx, sy = shift
    polys = [[(sx, sy), (sx, sy + e), (sx + e, sy + e), (sx + e, sy)]]
    at = [1.25 + 3.0 * k for k in range(int(e)) if 1.25 + 3.0 * k + 0.5 < e]
    for y in at:
        for x in at:
            polys.append([(sx + x, sy + y), (sx + x + 0.5, sy + y), (sx + x + 0.5, sy + y + 0.5), (sx + x, sy + y + 0.5)])
    return polys


def lone_box(N):
    e = scenarios.crowd_envsize(N)
    return [[(0.25 * e, 0.0), (0.25 * e, 0.9 * e), (0.8 * e, 0.9 * e), (0.8 * e, 0.0)]]


def edges_of(polys):
    """[n, 4] float32 (px, py, qx, qy): the edges of closed polygons, in the order the library numbers them (no edge cuts here)"""
    out = []
    for q in polys:
        q = np.asarray(q, F)
        for i in range(len(q)):
            out.append((q[i][0], q[i][1], q[(i + 1) % len(q)][0], q[(i + 1) % len(q)][1]))
    return np.asarray(out, F).reshape(-1, 4)


def subdivided(polys, pieces):
    """every edge cut into `pieces` collinear edges (more edges, the same walls)"""
    out = []
    for q in polys:
        q = np.asarray(q, np.float64)
        r = []
        for i in range(len(q)):
            a, b = q[i], q[(i + 1) % len(q)]
            r += [tuple(a + (b - a) * (k / pieces)) for k in range(pieces)]
        out.append(r)
    return out


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def cell(v, x0, ics, g):
    """include/ca_env.h: (int)fminf(fmaxf(floorf((v - x0) * ics), 0), g - 1), every operation in fp32"""
    t = np.floor(((np.asarray(v, F) - F(x0)).astype(F) * F(ics)).astype(F))
    return np.fmin(np.fmax(t, F(0.0)), F(g - 1)).astype(np.int64)


def dist_sq_point_segment(e, px, py):
    """csrc/ca_math.h distSqPointSegment for edges e [E, 4] and points px, py [P]: [P, E] float32, every operation rounded once
    (numpy's float32 division is the correctly rounded one)"""
    ax, ay, bx, by = (e[None, :, k].astype(F) for k in range(4))
    cx, cy = np.asarray(px, F)[:, None], np.asarray(py, F)[:, None]
    ux, uy = (bx - ax).astype(F), (by - ay).astype(F)
    wx, wy = (cx - ax).astype(F), (cy - ay).astype(F)
    with np.errstate(all="ignore"):
        r = ((wx * ux).astype(F) + (wy * uy).astype(F)).astype(F) / ((ux * ux).astype(F) + (uy * uy).astype(F)).astype(F)
        da = ((wx * wx).astype(F) + (wy * wy).astype(F)).astype(F)
        vx, vy = (cx - bx).astype(F), (cy - by).astype(F)
        db = ((vx * vx).astype(F) + (vy * vy).astype(F)).astype(F)
        qx, qy = (ax + (r * ux).astype(F)).astype(F), (ay + (r * uy).astype(F)).astype(F)
        mx, my = (cx - qx).astype(F), (cy - qy).astype(F)
        dm = ((mx * mx).astype(F) + (my * my).astype(F)).astype(F)
    return np.where(r < 0, da, np.where(r > 1, db, dm)).astype(F)


def walk(d, cell_start, entries, x, y, reach, dedupe=True):
    """the edge ids the kernel takes for an agent at (x, y) with `reach` (the obstacle range, or the radius for the wall test): the cells
    of cell(fl(x - reach)) .. cell(fl(x + reach)) and the rows likewise, an entry only in the low corner of the two rectangles'
    intersection"""
    x, y, reach = F(x), F(y), F(reach)
    cxlo, cxhi = int(cell(F(x - reach), d.x0, d.ics_x, d.gx)), int(cell(F(x + reach), d.x0, d.ics_x, d.gx))
    cylo, cyhi = int(cell(F(y - reach), d.y0, d.ics_y, d.gy)), int(cell(F(y + reach), d.y0, d.ics_y, d.gy))
    out = []
    for r in range(cylo, cyhi + 1):
        for c in range(cxlo, cxhi + 1):
            w = entries[cell_start[r * d.gx + c]:min(cell_start[r * d.gx + c + 1], d.n_entries)].astype(np.int64)
            if dedupe:
                w = w[(np.maximum((w >> 16) & 0xFF, cxlo) == c) & (np.maximum(w >> 24, cylo) == r)]
            out.append(w & 0xFFFF)
    return (np.concatenate(out) if out else np.zeros(0, np.int64)), (cxhi - cxlo + 1) * (cyhi - cylo + 1)


def ulps(v, k):
    v = np.asarray(v, F)
    i = v.view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7FFFFFFF), i) + k
    return np.where(i < 0, (-i) | 0x80000000, i).astype(np.uint32).view(F)


# ---- the seeded sets of tests/test_edge_grid_cpu.py (tests/abi/edge_grid_main.cpp builds sets of the same kinds) -----------------
def _diagonals(rng, n, side, origin=(0.0, 0.0)):
    a = rng.uniform(0, side, (n, 2)) + origin
    b = rng.uniform(0, side, (n, 2)) + origin
    return np.concatenate([a, b], axis=1).astype(F)


def edge_sets():
    """name -> (edges [n, 4] float32, range)"""
    rng = np.random.RandomState(17)
    box = lambda x0, y0, x1, y1: [[(x0, y0), (x0, y1), (x1, y1), (x1, y0)]]   # noqa: E731
    far = box(5e4, -5e4, 5e4 + 500.0, -5e4 + 500.0) + \
        [[(5e4 + x, -5e4 + y), (5e4 + x + 0.5, -5e4 + y), (5e4 + x + 0.5, -5e4 + y + 0.5), (5e4 + x, -5e4 + y + 0.5)]
         for x, y in rng.uniform(5, 490, (40, 2))]
    line = np.asarray([(x, 3.0, x + w, 3.0) for x, w in zip(np.arange(0.0, 60.0, 2.5), rng.uniform(0.5, 2.4, 24))], F)
    return {
        "pillars": (edges_of(hall(300)[1:]), 2.0),
        "hall": (edges_of(hall(300)), 2.0),                                   # the box's edges span the whole table
        "box_and_pillars": (edges_of(box(-7.0, -3.0, 40.0, 21.0) + hall(300)[1:30]), 1.7),
        "diagonals": (_diagonals(rng, 12, 90.0, (-20.0, 10.0)), 2.0),
        "translated": (edges_of(far), 2.0),
        "single": (np.asarray([(1.0, 2.0, 4.5, 3.25)], F), 2.0),
        "one_line": (line, 1.3),
    }


def points_for(edges, d, rng_range, n=2000, seed=0):
    """at least n seeded points of the four kinds: inside the box, outside it on every side, on cell boundaries, at `range` +- 1 ulp
    from an edge (beside it and beyond its ends)"""
    rng = np.random.RandomState(seed)
    R = float(rng_range)
    lo = np.minimum(edges[:, :2].min(0), edges[:, 2:].min(0)).astype(np.float64)
    hi = np.maximum(edges[:, :2].max(0), edges[:, 2:].max(0)).astype(np.float64)
    span = np.maximum(hi - lo, 1.0)
    q = n // 4
    pts = [rng.uniform(lo, hi, (q, 2))]
    for k in range(q):                                                                   # outside, on every side, near and far
        side, dist = k % 4, (rng.uniform(0, 1.2 * R) if k % 3 else rng.uniform(3 * R, 60.0))
        p = rng.uniform(lo - 2 * R, hi + 2 * R)
        p[side // 2] = (lo[side // 2] - dist) if side % 2 == 0 else (hi[side // 2] + dist)
        pts.append(p[None, :])
    csx, csy = F(1.0) / F(d.ics_x), F(1.0) / F(d.ics_y)
    for k in range(q):                                                                   # on cell boundaries: x0 + k * cell_size exactly
        bx = F(F(d.x0) + F(rng.randint(0, d.gx + 1)) * csx)
        by = F(F(d.y0) + F(rng.randint(0, d.gy + 1)) * csy)
        mode = k % 3
        p = (bx, by) if mode == 0 else ((bx, rng.uniform(lo[1], hi[1])) if mode == 1 else (rng.uniform(lo[0], hi[0]), by))
        pts.append(np.asarray(p, np.float64)[None, :])
    out = [np.concatenate(pts).astype(F)]
    e64 = edges.astype(np.float64)
    for k in range(q):                                                                   # at distance range +- 1 ulp from an edge
        ed = e64[rng.randint(len(e64))]
        a, b = ed[:2], ed[2:]
        u = (b - a) / np.linalg.norm(b - a)
        nrm = np.asarray([-u[1], u[0]]) * (1 if k % 2 else -1)
        base = (a + rng.uniform(0, 1) * (b - a) + nrm * R) if k % 4 < 2 else ((a - u * R) if k % 4 == 2 else (b + u * R))
        base = base.astype(F)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                out.append(np.asarray([[ulps(base[0], dx), ulps(base[1], dy)]], F))
    p = np.concatenate(out).astype(F)
    return p[:, 0].copy(), p[:, 1].copy()
