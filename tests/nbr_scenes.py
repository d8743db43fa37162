"""Seeded fp32 scenes that put agent pairs at the edge of the neighbour range (App. A.2), next to the cell boundaries of the
uniform grid that the one-lane scan of large arenas builds (csrc/ca_nbr.h), for tests/test_nbr_boundary_cpu.py and
tests/test_gpu_nbr_boundary.py.

Two restatements live here and must not be confused:
  * ref_lists -- THE REFERENCE: App. A.2 in plain numpy fp32, dx = fl(xi - xj), dsq = fl(fl(dx^2) + fl(dy^2)) < fl(nd^2),
    the K smallest by (dsq, index).  Both the oracle and the kernels are compared with it.
  * Grid -- THE AIMING MODEL: the kernel's cell rule (bounding box, cell size, cell index) as it stood when the fixed
    cx +- RC block was scanned.  It only decides where the generator plants pairs; nothing is ever checked against it
    except that the planted pairs really straddle RC + 1 cells.

make_scenes(N, nd, K, regime) returns pos_x, pos_y [A, N] and, per arena, the planted features:
  * "aim_x", "aim_y", "aim_diag": pairs (i, j) that are neighbours by App. A.2 but RC + 1 cells apart under the aiming
    model (along x, along y, and along x while straddling a row boundary), found by searching the float grid;
  * "dsq": pairs whose fp32 dsq lies a chosen number of ulps from fl(nd^2) (-64 .. -1: neighbours; 0 and above: not);
  * "tie": an agent with K - 1 nearer neighbours and four more at a bit-identical dsq, one per side (different cells):
    the K-th slot goes to the lowest index of the four;
  * "coincident": three agents at one point (dsq = 0: the composite-key scan's fallback for arenas of <= 64 agents).
Every feature sits in a hole of a background lattice (no background agent within 1.05 nd of it), so the planted
neighbours are within the K nearest.  An agent at a negative, non-round corner and one at the opposite corner fix the
bounding box; the arena's extent selects the regime:
  "half": GMAX 32, cs = nd / 2 (RC 2);  "wide": GMAX 32, cs = extent / 31.5, a few ulps >= nd (RC 1);
  "g16": GMAX 16, cs = nd (RC 1).
Arena a is translated by TRANSLATIONS[a % 4] (up to 9e4: inside CA_MAX_COORD)."""
import numpy as np

F = np.float32
TRANSLATIONS = (0.0, 1013.37, 10007.3, 90011.7)
DSQ_OFFSETS = (0, -1, 1, -64, -2, 2, -32, -3, -16, -4, -8)   # (in the order they are planted while agents last)
REGIMES = ("half", "wide", "g16")


# ---- float grid helpers ----------------------------------------------------------------------------------------------
def _ord(x):
    """float32 -> an integer that is monotone in the value (consecutive floats differ by 1)."""
    i = int(np.array(x, F).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def _unord(n):
    n = int(n)
    b = n if n >= 0 else ((-n) | 0x80000000)
    return np.array(b & 0xFFFFFFFF, np.uint32).view(F)[()]


def ulps(x, k):
    """x stepped by k float32 ulps (k may be an array)."""
    k = np.asarray(k, np.int64)
    n = _ord(x) + k
    b = np.where(n >= 0, n, (-n) | 0x80000000).astype(np.uint32)
    return b.view(F) if b.ndim else b.view(F)[()]


def _first_at_least(f, lo, hi, target):
    """The smallest float x in [lo, hi] with f(x) >= target (f monotone non-decreasing), or None."""
    a, b = _ord(lo), _ord(hi)
    if f(_unord(b)) < target:
        return None
    while a < b:
        m = (a + b) // 2
        if f(_unord(m)) >= target:
            b = m
        else:
            a = m + 1
    return _unord(a)


# ---- the reference (App. A.2) ------------------------------------------------------------------------------------------
def pair_dsq(xi, yi, xj, yj):
    """fp32 dsq of App. A.2 as agent i computes it for candidate j (no fused multiply-add)."""
    dx = F(F(xi) - F(xj))
    dy = F(F(yi) - F(yj))
    return F(F(dx * dx) + F(dy * dy))


def ref_lists(px, py, nd, K):
    """App. A.2 in numpy fp32: for every arena and agent, the agents j != i with dsq < fl(nd^2), the K smallest by
    (dsq, index).  Returns counts [A, N] and indices [A, N, K] (-1 beyond the count)."""
    px, py = np.asarray(px, F), np.asarray(py, F)
    A, N = px.shape
    r2 = F(F(nd) * F(nd))
    counts = np.zeros((A, N), np.int64)
    idx = np.full((A, N, K), -1, np.int64)
    cols = np.arange(N)
    for a in range(A):
        dx = px[a][:, None] - px[a][None, :]
        dy = py[a][:, None] - py[a][None, :]
        dsq = dx * dx + dy * dy             # (float32 elementwise: fl(fl(dx^2) + fl(dy^2)))
        assert dsq.dtype == F
        ok = (dsq < r2) & (cols[None, :] != cols[:, None])
        for i in range(N):
            js = cols[ok[i]]
            if K == 0 or js.size == 0:
                continue
            order = np.lexsort((js, dsq[i, js]))[:K]
            counts[a, i] = order.size
            idx[a, i, :order.size] = js[order]
    return counts, idx


# ---- the aiming model (the kernel's cell rule, NOT the reference) ------------------------------------------------------
class Grid(object):
    """The uniform grid of ca_nbr.h's one-lane scan, restated in fp32 for aiming: bounding box (x0, y0, x1, y1), cell size
    cs = max(half * nd, max(ex, ey) * fl(1 / (GMAX - 0.5))), RC = 1 if cs >= nd else 2, cell = (int)(fl(x - x0) * fl(1 / cs))
    clamped to [0, G - 1]."""

    def __init__(self, x0, y0, x1, y1, nd, gmax):
        self.x0, self.y0, self.nd, self.gmax = F(x0), F(y0), F(nd), gmax
        ex, ey = F(F(x1) - self.x0), F(F(y1) - self.y0)
        half = F(0.5) if gmax >= 32 else F(1.0)
        self.cs = max(F(half * self.nd), F(max(ex, ey) * F(F(1.0) / F(gmax - 0.5))))
        self.RC = 1 if self.cs >= self.nd else 2
        self.ics = F(F(1.0) / self.cs)
        self.Gx = min(gmax, int(F(ex * self.ics)) + 1)
        self.Gy = min(gmax, int(F(ey * self.ics)) + 1)

    def cell_x(self, x):
        return min(self.Gx - 1, max(0, int(F(F(F(x) - self.x0) * self.ics))))

    def cell_y(self, y):
        return min(self.Gy - 1, max(0, int(F(F(F(y) - self.y0) * self.ics))))

    def cell(self, x, y):
        return self.cell_x(x), self.cell_y(y)


def grid_for(px, py, nd, regime):
    """The aiming model of one arena's positions."""
    return Grid(px.min(), py.min(), px.max(), py.max(), nd, 16 if regime == "g16" else 32)


# ---- the generator -----------------------------------------------------------------------------------------------------
def _extent(regime, x0, nd):
    """The far corner coordinate x1 (> x0) that puts the arena in the regime."""
    nd = F(nd)
    if regime == "half":
        return F(x0 + F(15.5) * nd)
    if regime == "g16":
        return F(x0 + F(15.4) * nd)
    # "wide": the smallest extent whose cell size reaches nd (cs = fl(ex * fl(1 / 31.5)) a few ulps >= nd)
    c = F(F(1.0) / F(31.5))
    x1 = _first_at_least(lambda x: F(F(x - x0) * c), F(x0 + F(31.0) * nd), F(x0 + F(32.0) * nd), nd)
    assert x1 is not None
    return x1


class _Arena(object):
    def __init__(self, rng, N, nd, K, regime, shift):
        self.rng, self.N, self.nd, self.K, self.regime = rng, N, F(nd), K, regime
        # the corner: negative and non-round, 0.3 / 0.7 of the extent below the arena's origin, jittered until the aiming
        # model has a pair to aim along each axis.  (A pair is aimable where pos - x0 rounds more coarsely at the far
        # agent than at the near one -- the distance crosses a power of two -- while pos itself is fine-grained: near
        # the origin.  In the translated arenas the subtraction is exact and only the product with 1 / cs can round,
        # which rarely yields a pair: those arenas carry the other features.)
        E = float(nd) * {"half": 15.5, "g16": 15.4, "wide": 31.5}[regime]
        best = None
        for t in range(20):
            cx0 = F(shift - 0.3 * E - rng.uniform(0.1, 0.9))
            cy0 = F(shift - 0.7 * E - rng.uniform(0.1, 0.9))
            cx1 = _extent(regime, cx0, nd)
            cy1 = F(cy0 + F(cx1 - cx0) * F(0.97))               # ey < ex: the x extent sets the cell size
            self.box = (cx0, cy0, cx1, cy1)
            self.g = Grid(cx0, cy0, cx1, cy1, nd, 16 if regime == "g16" else 32)
            cand = (self._aim_axis(0), self._aim_axis(1))
            score = min(len(cand[0]), 1) + min(len(cand[1]), 1)
            if best is None or score > best[0]:
                best = (score, self.box, self.g, cand)
            if score == 2 or (shift != 0.0 and t >= 3):
                break
        _, self.box, self.g, self.cand = best
        self.feats = []       # (kind, [(x, y), ...], info)
        self.used = 2         # the two corner agents

    # a feature's agents must keep 1.1 nd from every other feature's agents and from the corners
    def _free(self, pts):
        m = F(1.1) * self.nd
        x0, y0, x1, y1 = self.box
        for (x, y) in pts:
            if not (x0 + m < x < x1 - m and y0 + m < y < y1 - m):
                return False
            for _, q, _ in self.feats:
                for (u, v) in q:
                    if (float(x) - float(u)) ** 2 + (float(y) - float(v)) ** 2 < (2.3 * float(self.nd)) ** 2:
                        return False
        return True

    def _add(self, kind, pts, info=None):
        if self.used + len(pts) > self.N or not self._free(pts):
            return False
        self.feats.append((kind, [(F(x), F(y)) for x, y in pts], info or {}))
        self.used += len(pts)
        return True

    def _rand_point(self):
        x0, y0, x1, y1 = self.box
        m = 1.2 * float(self.nd)
        return F(self.rng.uniform(float(x0) + m, float(x1) - m)), F(self.rng.uniform(float(y0) + m, float(y1) - m))

    # -- aimed pairs: neighbours by App. A.2, RC + 1 cells apart under the aiming model
    def _aim_axis(self, axis):
        """[(lo, hi)] along the axis: lo the largest coordinate of some cell c, hi the smallest of cell c + RC + 1, their
        fp32 distance below nd (so fl(d^2) < fl(nd^2) may hold)."""
        g = self.g
        cellf = g.cell_x if axis == 0 else g.cell_y
        c0, c1 = (self.box[0], self.box[2]) if axis == 0 else (self.box[1], self.box[3])
        G = g.Gx if axis == 0 else g.Gy
        out = []
        for c in range(1, G - g.RC - 2):
            b1 = _first_at_least(cellf, c0, c1, c + 1)            # first coordinate of cell c + 1
            b2 = _first_at_least(cellf, c0, c1, c + g.RC + 1)
            if b1 is None or b2 is None:
                continue
            lo = ulps(b1, -1)
            if cellf(lo) != c or cellf(b2) != c + g.RC + 1:
                continue
            d = F(lo - b2)
            if F(d * d) < F(self.nd * self.nd):
                out.append((lo, b2))
        return out

    def add_aimed(self, kind):
        axis = 1 if kind == "aim_y" else 0
        cands = list(self.cand[axis])
        self.rng.shuffle(cands)
        r2 = F(self.nd * self.nd)
        for lo, hi in cands[:40]:
            for _ in range(6):
                ox, oy = self._rand_point()
                o2 = oy if axis == 0 else ox        # the other coordinate
                if kind == "aim_diag":              # straddle a boundary of the other axis: i at the top of a row, j at the start of the next
                    cellf = self.g.cell_y
                    b = _first_at_least(cellf, self.box[1], self.box[3], cellf(o2) + 1)
                    if b is None:
                        continue
                    oi, oj = ulps(b, -1), b
                    if pair_dsq(lo, oi, hi, oj) >= r2:
                        continue
                    pts = [(lo, oi), (hi, oj)]
                elif axis == 0:
                    pts = [(lo, o2), (hi, o2)]
                else:
                    pts = [(o2, lo), (o2, hi)]
                if self.rng.rand() < 0.5:
                    pts = pts[::-1]                 # the aimed agent i may sit on either side
                if self._add(kind, pts):
                    return True
        return False

    # -- a pair whose dsq lies `off` ulps from fl(nd^2)
    def add_dsq(self, off):
        r2 = F(self.nd * self.nd)
        for _ in range(20):
            xi, yi = self._rand_point()
            th = self.rng.uniform(0, 2 * np.pi)
            bx, by = F(xi + self.nd * F(np.cos(th))), F(yi + self.nd * F(np.sin(th)))
            kx = np.arange(-300, 301)
            ky = np.arange(-6, 7)
            xs, ys = ulps(bx, kx), ulps(by, ky)
            dx = (xi - xs).astype(F)
            dy = (yi - ys).astype(F)
            dsq = (dx[:, None] * dx[:, None]) + (dy[None, :] * dy[None, :])
            offs = dsq.view(np.int32).astype(np.int64) - _ord(r2)
            hit = np.argwhere(offs == off)
            if hit.size == 0:
                continue
            a, b = hit[self.rng.randint(len(hit))]
            assert pair_dsq(xi, yi, xs[a], ys[b]) == dsq[a, b]
            if self._add("dsq", [(xi, yi), (xs[a], ys[b])], dict(off=off)):
                return True
        return False

    # -- K-th slot tie: K - 1 nearer agents and four at a bit-identical dsq, one on each side
    def add_tie(self):
        if self.K < 1:
            return False
        q = F(2.0 ** -8)
        for _ in range(20):
            xc, yc = self._rand_point()
            xc, yc = F(np.round(xc / q) * q), F(np.round(yc / q) * q)   # few significant bits: xc +- r exact
            r = F(np.round(F(0.62) * self.nd / q) * q)
            ring = []
            th0 = self.rng.uniform(0, 2 * np.pi)
            for k in range(self.K - 1):
                th = th0 + 2 * np.pi * k / max(1, self.K - 1)
                rr = F(0.3) * self.nd * F(1.0 + 0.1 * self.rng.rand())
                ring.append((F(xc + rr * F(np.cos(th))), F(yc + rr * F(np.sin(th)))))
            tied = [(F(xc + r), yc), (F(xc - r), yc), (xc, F(yc + r)), (xc, F(yc - r))]
            d = [pair_dsq(xc, yc, x, y) for x, y in tied]
            if len(set(np.array(d, F).view(np.uint32).tolist())) != 1 or any(pair_dsq(xc, yc, x, y) >= d[0] for x, y in ring):
                continue
            if len(set(self.g.cell(x, y) for x, y in tied)) != 4:     # one candidate per cell
                continue
            if self._add("tie", [(xc, yc)] + tied + ring):
                return True
        return False

    def add_coincident(self):
        for _ in range(20):
            x, y = self._rand_point()
            if self._add("coincident", [(x, y)] * 3):
                return True
        return False

    def finish(self):
        """Corners + features + the background lattice (sparsest that supplies the rest), in a seeded random order."""
        x0, y0, x1, y1 = self.box
        pts = [(x0, y0), (x1, y1)]
        for _, q, _ in self.feats:
            pts += q
        need = self.N - len(pts)
        fx = np.array([p[0] for p in pts[2:]], np.float64)
        fy = np.array([p[1] for p in pts[2:]], np.float64)
        clear = 1.05 * float(self.nd)
        bg = None
        for m in range(2, 200):
            s = (float(x1) - float(x0)) / m
            gx, gy = np.meshgrid(np.arange(m) + 0.5, np.arange(m) + 0.5)
            cx = float(x0) + s * (gx.ravel() + self.rng.uniform(-0.05, 0.05, gx.size))
            cy = float(y0) + s * 0.97 * (gy.ravel() + self.rng.uniform(-0.05, 0.05, gy.size))
            cx, cy = cx.astype(F), cy.astype(F)
            keep = (cx > x0) & (cx < x1) & (cy > y0) & (cy < y1)
            if fx.size:
                d2 = (cx.astype(np.float64)[:, None] - fx[None, :]) ** 2 + (cy.astype(np.float64)[:, None] - fy[None, :]) ** 2
                keep &= (d2 >= clear * clear).all(axis=1)
            if keep.sum() >= need:
                sel = np.flatnonzero(keep)
                sel = np.sort(self.rng.choice(sel, need, replace=False))
                bg = list(zip(cx[sel], cy[sel]))
                break
        assert bg is not None, "no lattice supplies %d background agents" % need
        pts += bg
        perm = self.rng.permutation(self.N)          # agent index = perm position: ties meet every index order
        px = np.empty(self.N, F)
        py = np.empty(self.N, F)
        px[perm] = [p[0] for p in pts]
        py[perm] = [p[1] for p in pts]
        feats, k = [], 2
        for kind, q, info in self.feats:
            feats.append(dict(kind=kind, idx=[int(perm[k + t]) for t in range(len(q))], **info))
            k += len(q)
        return px, py, feats


def make_scenes(N, nd, K, regime, A=4, seed=0):
    """pos_x, pos_y [A, N] (float32) and, per arena, the list of planted features:
    dict(kind=..., idx=[agent indices], off=...) -- for the pairs idx = [i, j] (i the aimed agent)."""
    assert regime in REGIMES, regime
    rng = np.random.RandomState(seed)
    PX, PY, FE = np.empty((A, N), F), np.empty((A, N), F), []
    for a in range(A):
        ar = _Arena(rng, N, nd, K, regime, TRANSLATIONS[a % len(TRANSLATIONS)])
        for kind in ("aim_x", "aim_y", "aim_diag"):
            ar.add_aimed(kind)
        opt = ["tie", "coincident"] + list(DSQ_OFFSETS)
        if N < 64:                                   # small arenas: a different choice in every arena
            rng.shuffle(opt)
        for f in opt:
            if f == "tie":
                ar.add_tie()
            elif f == "coincident":
                ar.add_coincident()
            else:
                ar.add_dsq(f)
        PX[a], PY[a], fe = ar.finish()
        FE.append(fe)
    return PX, PY, FE


# ---- the scene sets of the tests: name -> (N, neighbor_dist, max_neighbors, regime); tests/test_gpu_nbr_boundary.py
# names the scan path each one runs on
CASES = {
    "quad16": (16, 5.0, 5, "half"), "quad64": (64, 5.0, 10, "half"), "quad128": (128, 5.0, 10, "half"),
    "ck16": (16, 5.0, 5, "half"), "ck64": (64, 5.0, 10, "half"),
    "scan65": (65, 5.0, 10, "half"), "scan100": (100, 5.0, 10, "half"),
    "grid32_250_k16": (250, 5.0, 16, "half"), "grid32_300_world": (300, 5.0, 10, "half"),
    "grid32_300_help": (300, 5.0, 10, "wide"),   # (the one-lane CA_PAIR=0 path; the scenes are seeded from the name, so it stays)
    "grid16_600": (600, 3.0, 10, "g16"), "grid16_1024": (1024, 3.0, 10, "g16"),
    "pair192": (192, 5.0, 10, "half"), "pair300": (300, 5.0, 10, "half"), "pair512": (512, 5.0, 10, "wide"),
}
WORLD_CASES = ("grid32_300_world",)     # a small world (16 edges) with more than four edges in some agent's range


def case_scenes(name):
    N, nd, K, regime = CASES[name]
    seed = sum(ord(c) * (t + 1) for t, c in enumerate(name)) % 100003
    return make_scenes(N, nd, K, regime, A=4, seed=seed)


def two_octagons(px, py, feats, nd):
    """Per arena: two counter-clockwise octagons (radius 0.5, 16 edges) 1.3 to either side of a background agent that is
    at least 2.5 nd from every planted feature -- that agent has edges of both in range (more than four)."""
    worlds = []
    for a in range(px.shape[0]):
        taken = set(k for f in feats[a] for k in f["idx"])
        fx = px[a][sorted(taken)].astype(np.float64)
        fy = py[a][sorted(taken)].astype(np.float64)
        c = None
        for k in range(px.shape[1]):
            x, y = float(px[a, k]), float(py[a, k])
            if k in taken or x in (float(px[a].min()), float(px[a].max())) or y in (float(py[a].min()), float(py[a].max())):
                continue
            if fx.size == 0 or ((fx - x) ** 2 + (fy - y) ** 2).min() > (2.5 * nd) ** 2:
                c = (x, y)
                break
        assert c is not None
        polys = []
        for sx in (-1.3, 1.3):
            th = np.arange(8) * (2 * np.pi / 8) + np.pi / 8
            polys.append([(c[0] + sx + 0.5 * np.cos(t), c[1] + 0.5 * np.sin(t)) for t in th])
        worlds.append(polys)
    return worlds
