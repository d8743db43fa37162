"""Scenes of the tiled path's uniform-grid neighbour search (ca_create_ex with CA_CREATE_TILED | CA_CREATE_TILED_GRID; csrc/ca_tiled.h),
and a numpy fp32 model of its cell rule.  tests/test_tiled_grid_cpu.py asserts on the CPU oracle and the model alone that every
scene exercises what it claims; tests/test_gpu_tiled_grid.py runs the same scenes on a grid handle and compares bit for bit.

The model takes the table (cells_x, cells_y, cell_size) as arguments -- the GPU tests hand it ca_tiled_grid_info()'s values --:
  c(v)    = (int)floor(fl(v * ics)),  ics = fl(1 / cell_size)
  bucket  = (c(y) & (cells_y - 1)) * cells_x + (c(x) & (cells_x - 1))
  scanned = columns c(fl(x - B)) .. c(fl(x + B)), at most cells_x of them, wrapped; rows likewise; B = fl(fl(nd * 1.0001) + 1e-4)
Nothing but the scenes' own claims is ever checked against the model: the reference of every list is App. A.2 (nbr_scenes.ref_lists,
and the oracle)."""
import numpy as np

from tests import helpers as H
from tests import nbr_scenes as NS

F = np.float32


class Model(object):
    def __init__(self, cells_x, cells_y, cell_size, nd):
        assert cells_x & (cells_x - 1) == 0 and cells_y & (cells_y - 1) == 0 and cell_size > 0
        self.gx, self.gy, self.cs, self.nd = int(cells_x), int(cells_y), F(cell_size), F(nd)
        self.ics = F(F(1.0) / self.cs)
        self.B = F(F(self.nd * F(1.0001)) + F(1e-4))

    def cell(self, v):
        """the unwrapped cell coordinate (v: scalar or array)"""
        return np.floor((np.asarray(v, F) * self.ics).astype(F)).astype(np.int64)

    def bucket(self, x, y):
        return (self.cell(y) & (self.gy - 1)) * self.gx + (self.cell(x) & (self.gx - 1))

    def span(self, v):
        """(lo, hi): the unwrapped cells of fl(v - B) and fl(v + B)"""
        v = np.asarray(v, F)
        return self.cell((v - self.B).astype(F)), self.cell((v + self.B).astype(F))

    def scanned(self, x, y):
        """the buckets agent (x, y) scans, in the kernel's order; no bucket twice"""
        (xl, xh), (yl, yh) = self.span(x), self.span(y)
        cols = [int((xl + k) & (self.gx - 1)) for k in range(min(int(xh - xl), self.gx - 1) + 1)]
        rows = [int((yl + k) & (self.gy - 1)) for k in range(min(int(yh - yl), self.gy - 1) + 1)]
        out = [r * self.gx + c for r in rows for c in cols]
        assert len(set(out)) == len(out)
        return out

    def candidates(self, px, py, i):
        """the agents (i among them) in the buckets agent i scans: px, py [N]"""
        b = self.bucket(px, py)
        return np.flatnonzero(np.isin(b, self.scanned(px[i], py[i])))

    def lists(self, px, py, K):
        """App. A.2 over the scanned buckets only: counts [N], indices [N, K] (-1 beyond the count) of one arena"""
        N = len(px)
        r2 = F(self.nd * self.nd)
        cnt, idx = np.zeros(N, np.int64), np.full((N, K), -1, np.int64)
        for i in range(N):
            js = self.candidates(px, py, i)
            js = js[js != i]
            dx, dy = (px[i] - px[js]).astype(F), (py[i] - py[js]).astype(F)
            dsq = (dx * dx + dy * dy).astype(F)
            js, dsq = js[dsq < r2], dsq[dsq < r2]
            order = np.lexsort((js, dsq))[:K]
            cnt[i] = order.size
            idx[i, :order.size] = js[order]
        return cnt, idx


def model_of(info, nd):
    """the model of a handle's table: info = VecCollisionAvoidanceEnv.tiled_grid_info()"""
    assert info["grid"] and info["cell_size"] > 0, info
    return Model(info["cells_x"], info["cells_y"], info["cell_size"], nd)


def params(N, **over):
    return H.scenario_params("crowd", N, **over)   # K = 10, range 5


def place(env, fld, px, py):
    """px, py [N] into a one-arena env (oracle or GPU handle; fld: its field constants)"""
    env.set(fld.FLD_POS_X, np.ascontiguousarray(px[None, :], F))
    env.set(fld.FLD_POS_Y, np.ascontiguousarray(py[None, :], F))


# ---- the aliasing scene: clumps a whole table apart share their buckets ------------------------------------------------------
def aliasing_scene(N, m, seed=31):
    """Four clumps of N / 4 agents, each uniform in a square of three neighbour ranges: one across the origin (negative coordinates, the
    cell border at 0 inside it), the others cells_x * cs, cells_y * cs and both away from it -- so every bucket of the first clump
    holds agents of the others, strangers that only the distance test keeps out.  Returns px, py [N] in a seeded random order."""
    rng = np.random.RandomState(seed)
    side = 3.0 * float(m.nd)
    W, Hh = m.gx * float(m.cs), m.gy * float(m.cs)
    centres = [(0.0, 0.0), (W, 0.0), (0.0, -Hh), (-W, Hh)]
    px, py = np.empty(N, F), np.empty(N, F)
    for k in range(N):
        cx, cy = centres[k % 4]
        px[k], py[k] = F(cx + rng.uniform(-0.5, 0.5) * side), F(cy + rng.uniform(-0.5, 0.5) * side)
    perm = rng.permutation(N)
    return px[perm], py[perm]


def aliasing_claims(px, py, m):
    """(pairs in one bucket more than nd apart, strangers -- beyond nd -- inside agent 0 .. 15's scanned blocks)"""
    b = m.bucket(px, py)
    far = 0
    for k in np.unique(b):
        js = np.flatnonzero(b == k)
        d2 = (px[js].astype(np.float64)[:, None] - px[js][None, :]) ** 2 + (py[js].astype(np.float64)[:, None] - py[js][None, :]) ** 2
        far += int((d2 > float(m.nd) ** 2).sum()) // 2
    strangers = 0
    for i in range(16):
        js = m.candidates(px, py, i)
        d2 = (px[js].astype(np.float64) - float(px[i])) ** 2 + (py[js].astype(np.float64) - float(py[i])) ** 2
        strangers += int((d2 > 4.0 * float(m.nd) ** 2).sum())   # (twice the range away: from another clump)
    return far, strangers


# ---- the boundary scene: pairs at the edge of the range whose candidate stands in the outermost scanned column or row -----------
BOUNDARY_PAIRS = [(axis, sign, off, c) for axis in (0, 1) for sign in (1, -1) for off, c in ((-1, 0), (0, 0), (-1, -3), (0, 5))]


def _first_of_cell(m, c):
    """the first float of unwrapped cell c"""
    lo, hi = F((c - 1) * float(m.cs)), F((c + 1) * float(m.cs))
    b = NS._first_at_least(lambda v: int(m.cell(v)), lo, hi, c)
    assert b is not None and int(m.cell(b)) == c and int(m.cell(NS.ulps(b, -1))) == c - 1
    return b


def _plant(rng, m, sign, off, c, other):
    """agent i and candidate j along one axis: j's coordinate t is the first float of cell c (sign > 0: j beyond i) or the last float
    of cell c - 1 (sign < 0), the other coordinates differ by about 0.1, and dsq(i, j) lies `off` ulps from fl(nd^2).
    Returns (ti, oi, tj, oj): the axis coordinate and the other coordinate of each."""
    r2 = F(m.nd * m.nd)
    b = _first_of_cell(m, c)
    tj = b if sign > 0 else NS.ulps(b, -1)
    for _ in range(200):
        oi = F(other + rng.uniform(-0.3, 0.3))
        delta = rng.uniform(0.05, 0.3)
        ti0 = F(float(tj) - sign * np.sqrt(float(m.nd) ** 2 - delta ** 2))
        tis, ojs = NS.ulps(ti0, np.arange(-300, 301)), NS.ulps(F(oi + delta), np.arange(-60, 61))
        dt, do = (tis - tj).astype(F), (oi - ojs).astype(F)
        dsq = (dt[:, None] * dt[:, None]) + (do[None, :] * do[None, :])
        offs = dsq.view(np.int32).astype(np.int64) - NS._ord(r2)
        hit = np.argwhere(offs == off)
        if hit.size:
            a, k = hit[rng.randint(len(hit))]
            return tis[a], oi, tj, ojs[k]
    raise AssertionError("no pair %d ulps from the range at cell %d" % (off, c))


def boundary_scene(N, m, seed=41):
    """px, py [N] in a seeded random order and the planted pairs [dict(i, j, axis, sign, off, c)].  Pairs along x stand in rows four
    ranges apart around x = 0, pairs along y in columns four ranges apart from x = 20 nd on; a jittered lattice of the other agents
    (spacing 1.2: full lists) fills x in [-15 nd - .., -6 nd], across y = 0 -- more than two ranges from every planted agent."""
    rng = np.random.RandomState(seed)
    nd = float(m.nd)
    pts, pairs = [], []
    for k, (axis, sign, off, c) in enumerate(BOUNDARY_PAIRS):
        slot = 4.0 * nd * (k % 8)
        ti, oi, tj, oj = _plant(rng, m, sign, off, c, slot if axis == 0 else 20.0 * nd + slot)
        a, b = ((ti, oi), (tj, oj)) if axis == 0 else ((oi, ti), (oj, tj))
        pairs.append(dict(i=len(pts), j=len(pts) + 1, axis=axis, sign=sign, off=off, c=c))
        pts += [a, b]
    need = N - len(pts)
    side = int(np.ceil(np.sqrt(need)))
    x1 = -6.0 * nd
    for k in range(need):
        pts.append((F(x1 - 1.2 * (k % side) + rng.uniform(-0.1, 0.1)), F(-8.0 + 1.2 * (k // side) + rng.uniform(-0.1, 0.1))))
    perm = rng.permutation(N)
    px, py = np.empty(N, F), np.empty(N, F)
    px[perm], py[perm] = [p[0] for p in pts], [p[1] for p in pts]
    for p in pairs:
        p["i"], p["j"] = int(perm[p["i"]]), int(perm[p["j"]])
    return px, py, pairs


def boundary_claims(px, py, pairs, m, cnt, idx):
    """asserts what the boundary scene claims, on the lists cnt [N], idx [N, K] of a reference; returns the number of pairs whose
    candidate stands in the outermost scanned column or row"""
    r2 = F(m.nd * m.nd)
    outer = 0
    for p in pairs:
        i, j = p["i"], p["j"]
        dsq = NS.pair_dsq(px[i], py[i], px[j], py[j])
        assert int(dsq.view(np.int32)) - NS._ord(r2) == p["off"], p
        listed = j in idx[i, :cnt[i]].tolist()
        assert listed == (p["off"] < 0) and (i in idx[j, :cnt[j]].tolist()) == listed, p
        ti, tj = (px[i], px[j]) if p["axis"] == 0 else (py[i], py[j])
        lo, hi = m.span(ti)
        cj = int(m.cell(tj))
        assert cj == (int(hi) if p["sign"] > 0 else int(lo)), (p, cj, lo, hi)     # the outermost column / row of i's block
        assert abs(cj - int(m.cell(ti))) >= 2, p
        assert cj == (p["c"] if p["sign"] > 0 else p["c"] - 1), p
        outer += 1
    return outer


# ---- degenerate fills ------------------------------------------------------------------------------------------------------------
def one_cell_positions(N, m, seed=51):
    """every agent inside cell (0, 0)"""
    rng = np.random.RandomState(seed)
    cs = float(m.cs)
    px, py = rng.uniform(0.05, 0.95, N) * cs, rng.uniform(0.05, 0.95, N) * cs
    return px.astype(F), py.astype(F)
