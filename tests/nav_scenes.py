"""The definition of the navigation fields (ca_nav_configure / ca_nav_pref, include/ca_env.h), restated in numpy for the tests, and the
test worlds.  No device and no library: tests/test_nav_cpu.py checks the host builder and the definition's uniqueness against it,
tests/test_gpu_nav.py compares the kernels with it bit for bit.

fp32 throughout.  A sum d + w of two fp32 values is formed in float64 and rounded to fp32: float64 carries 53 >= 2 * 24 + 2 bits, so
the two roundings give the correctly rounded fp32 sum.  Rounding is monotone, so the minimum of rounded sums is the rounded minimum.
The field is computed by a label-setting pass (Dijkstra's order); jacobi() and raster() relax the same equations in other orders."""
import heapq

import numpy as np

from tests import edge_grid_scenes as E

F = np.float32
OFFSETS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
STAY, NONE = 8, 9
SQRT2 = F(1.41421354)
INF = F(np.inf)


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
class Grid:
    def __init__(self, x0, y0, cell, gx, gy):
        self.x0, self.y0, self.cell, self.gx, self.gy = F(x0), F(y0), F(cell), int(gx), int(gy)
        self.ics = F(F(1.0) / self.cell)
        self.w = (self.cell,) * 4 + (F(self.cell * SQRT2),) * 4

    def centres(self):
        """(cx [gx], cy [gy]) float32: x0 + ((float)c + 0.5f) * cell"""
        cx = (self.x0 + ((np.arange(self.gx).astype(F) + F(0.5)).astype(F) * self.cell).astype(F)).astype(F)
        cy = (self.y0 + ((np.arange(self.gy).astype(F) + F(0.5)).astype(F) * self.cell).astype(F)).astype(F)
        return cx, cy

    def cell_of(self, x, y):
        return E.cell(x, self.x0, self.ics, self.gx), E.cell(y, self.y0, self.ics, self.gy)


def edges_of_table(tab):
    """[n, 4] (px, py, qx, qy) of a processed obstacle table: dict(verts [n, 2], next [n]) or the oracle's dict(px, py, next)"""
    if "verts" in tab:
        v = np.asarray(tab["verts"], F)
    else:
        v = np.stack([tab["px"], tab["py"]], axis=1).astype(F)
    return np.concatenate([v, v[np.asarray(tab["next"], np.int64)]], axis=1).astype(F).reshape(-1, 4)


def blocked_mask(edges, g, clearance):
    """uint8 [gy, gx]: 1 iff some edge has distSqPointSegment(p, q, centre) < clearance * clearance"""
    cx, cy = g.centres()
    px, py = np.tile(cx, g.gy), np.repeat(cy, g.gx)
    edges = np.asarray(edges, F).reshape(-1, 4)
    if len(edges) == 0:
        return np.zeros((g.gy, g.gx), np.uint8)
    c2 = F(F(clearance) * F(clearance))
    out = np.zeros(len(px), bool)
    for k in range(0, len(edges), 256):
        out |= (E.dist_sq_point_segment(edges[k:k + 256], px, py) < c2).any(axis=1)
    return out.reshape(g.gy, g.gx).astype(np.uint8)


def _neighbours(blocked):
    """per cell the allowed moves [(k, neighbour index)] of an unblocked cell (in grid, unblocked, no corner cutting), and for every
    cell all in-grid neighbours [(k, index)]"""
    gy, gx = blocked.shape
    free = lambda x, y: 0 <= x < gx and 0 <= y < gy and not blocked[y, x]   # noqa: E731
    allowed, every = [], []
    for y in range(gy):
        for x in range(gx):
            al, ev = [], []
            for k, (dx, dy) in enumerate(OFFSETS):
                ux, uy = x + dx, y + dy
                if not (0 <= ux < gx and 0 <= uy < gy):
                    continue
                ev.append((k, uy * gx + ux))
                if blocked[uy, ux] or (k >= 4 and not (free(x + dx, y) and free(x, y + dy))):
                    continue
                al.append((k, uy * gx + ux))
            allowed.append(al)
            every.append(ev)
    return allowed, every


def _round(v):
    return float(F(v))


def field(blocked, g, source):
    """(dist float32 [gy, gx], next uint8 [gy, gx]) for the source cell (cx, cy): the label-setting pass, then the pointers"""
    gy, gx = blocked.shape
    allowed, every = _neighbours(blocked)
    w = [float(v) for v in g.w]
    src = source[1] * gx + source[0]
    assert not blocked[source[1], source[0]]
    d = [float("inf")] * (gx * gy)
    d[src] = 0.0
    heap, done = [(0.0, src)], [False] * (gx * gy)
    while heap:
        dc, c = heapq.heappop(heap)
        if done[c]:
            continue
        done[c] = True
        for k, u in allowed[c]:             # (the moves are symmetric: u reaches c by the opposite move, of the same weight)
            nd = _round(dc + w[k])
            if nd < d[u]:
                d[u] = nd
                heapq.heappush(heap, (nd, u))
    return np.asarray(d, F).reshape(gy, gx), pointers(blocked, g, np.asarray(d, F).reshape(gy, gx), source)


def pointers(blocked, g, dist, source):
    gy, gx = blocked.shape
    allowed, every = _neighbours(blocked)
    w = [float(v) for v in g.w]
    d = [float(v) for v in dist.reshape(-1)]
    nxt = np.full(gx * gy, NONE, np.uint8)
    for c in range(gx * gy):
        if c == source[1] * gx + source[0]:
            nxt[c] = STAY
        elif not blocked.reshape(-1)[c]:
            if d[c] < float("inf"):
                nxt[c] = min(k for k, u in allowed[c] if _round(d[u] + w[k]) == d[c])
        else:
            cand = [(d[u], k) for k, u in every[c] if d[u] < float("inf")]
            if cand:
                nxt[c] = min(cand)[1]
    return nxt.reshape(gy, gx)


def jacobi(blocked, g, source, max_sweeps=None):
    """the same equations relaxed from +inf, every cell from the previous sweep's image; returns (dist, sweeps to the fixed point)"""
    gy, gx = blocked.shape
    free = blocked == 0
    d = np.full((gy, gx), np.inf, np.float64)
    d[source[1], source[0]] = 0.0
    pad = lambda a, v: np.pad(a, 1, constant_values=v)   # noqa: E731
    fp = pad(free, False)
    sweeps = 0
    while True:
        dp = pad(d, np.inf)
        best = np.full((gy, gx), np.inf, np.float64)
        for k, (dx, dy) in enumerate(OFFSETS):
            nb = dp[1 + dy:1 + dy + gy, 1 + dx:1 + dx + gx]
            ok = fp[1 + dy:1 + dy + gy, 1 + dx:1 + dx + gx]
            if k >= 4:
                ok = ok & fp[1:1 + gy, 1 + dx:1 + dx + gx] & fp[1 + dy:1 + dy + gy, 1:1 + gx]
            cand = np.where(ok, (nb + float(g.w[k])).astype(F).astype(np.float64), np.inf)
            best = np.minimum(best, cand)
        new = np.where(free, np.minimum(d, best), np.inf)
        new[source[1], source[0]] = 0.0
        sweeps += 1
        if np.array_equal(new, d):
            return d.astype(F), sweeps
        d = new
        assert max_sweeps is None or sweeps <= max_sweeps, sweeps


def raster(blocked, g, source, reverse=False):
    """... relaxed in place in raster order (reverse: from the last cell to the first) until a sweep changes nothing"""
    gy, gx = blocked.shape
    allowed, _ = _neighbours(blocked)
    w = [float(v) for v in g.w]
    src = source[1] * gx + source[0]
    d = [float("inf")] * (gx * gy)
    d[src] = 0.0
    order = [c for c in range(gx * gy) if c != src and not blocked.reshape(-1)[c]]
    if reverse:
        order.reverse()
    sweeps = 0
    while True:
        changed = False
        for c in order:
            if allowed[c]:
                m = _round(min(d[u] + w[k] for k, u in allowed[c]))
                if m < d[c]:
                    d[c] = m
                    changed = True
        sweeps += 1
        if not changed:
            return np.asarray(d, F).reshape(gy, gx), sweeps


# ---- per step ----------------------------------------------------------------------------------------------------------------------
def nav_pref(g, fields, cls, lookahead, pos_x, pos_y, goal_x, goal_y, pref_dir, navigated, set_of_arena=None):
    """The preferred velocities and distances of one call: fields[s][k] = (dist, next, blocked) of set s, target k; cls / pos / goal
    [A, N]; navigated bool [A, N] (present, not done, not frozen -- the caller's; class >= 0 is tested here); pref_dir(px, py, gx, gy)
    the direction function (oracle.pref_dir64).  Returns (px [A, N] float32, py, dist [A, N] float32, mask [A, N] of written rows)."""
    A, N = cls.shape
    out_x, out_y, out_d = np.zeros((A, N), F), np.zeros((A, N), F), np.zeros((A, N), F)
    mask = np.zeros((A, N), bool)
    cxs, cys = g.centres()
    for a in range(A):
        s = 0 if set_of_arena is None else set_of_arena[a]
        for i in range(N):
            k = int(cls[a, i])
            if not navigated[a, i] or k < 0:
                continue
            dist, nxt, _ = fields[s][k]
            px, py = F(pos_x[a, i]), F(pos_y[a, i])
            cx, cy = g.cell_of(px, py)
            wx, wy, moved, p = int(cx), int(cy), False, NONE
            for _ in range(lookahead):
                p = int(nxt[wy, wx])
                if p >= 8:
                    break
                wx, wy, moved = wx + OFFSETS[p][0], wy + OFFSETS[p][1], True
            if not moved or p == STAY:
                dx, dy = pref_dir(px, py, float(goal_x[a, i]), float(goal_y[a, i]))
            else:
                dx, dy = pref_dir(px, py, float(cxs[wx]), float(cys[wy]))
            out_x[a, i], out_y[a, i], out_d[a, i], mask[a, i] = F(dx), F(dy), dist[int(cy), int(cx)], True
    return out_x, out_y, out_d, mask


def all_fields(edge_sets, g, clearance, targets):
    """fields[s][k] for targets [S, G, 2] (or [G, 2] with one edge set)"""
    targets = np.asarray(targets, F)
    if targets.ndim == 2:
        targets = targets[None]
    out = []
    for s, edges in enumerate(edge_sets):
        blk = blocked_mask(edges, g, clearance)
        row = []
        for t in targets[s]:
            cx, cy = g.cell_of(t[0], t[1])
            d, n = field(blk, g, (int(cx), int(cy)))
            row.append((d, n, blk))
        out.append(row)
    return out


# ---- the worlds -------------------------------------------------------------------------------------------------------------------
def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def doorway_world(pen=False):
    """the reference's doorway world (scenarios.obstacles('doorway')); pen: plus a box whose edges run through the centres of the
    ring of cells round cell (9, 7) of DOORWAY_GRID -- an enclosure nothing leads out of"""
    polys = [[(-15.0, 0.0), (-15.0, 10.0), (10.0, 10.0), (10.0, 0.0)],
             [(2.0, 0.0), (2.5, 0.0), (2.5, 4.4), (2.0, 4.4)],
             [(2.0, 5.6), (2.5, 5.6), (2.5, 10.0), (2.0, 10.0)]]
    if pen:
        polys.append(rect(6.5, 6.5, 8.5, 8.5))
    return polys


DOORWAY_GRID = dict(x0=-2.0, y0=0.0, cell=1.0, gx=12, gy=10)      # the wall's cells are column 4; the door is rows 4 and 5
DOORWAY_CLEARANCE = 0.05                                           # (the door is 1.2 wide: a clearance of 0.5 would close it at cell = 1)
DOORWAY_TARGETS = ((-1.0, 5.0), (8.5, 2.5))


def block_world(k=0):
    """four square blocks on an 8 x 8 grid of unit cells, moved with k (a world per arena)"""
    at = [(1.5 + (k % 2), 1.5), (5.0, 1.5 + k % 3), (1.5, 5.0 - (k % 2)), (4.5 + (k % 2), 4.5)]
    return [rect(x, y, x + 1.0, y + 1.0) for x, y in at]


BLOCK_GRID = dict(x0=0.0, y0=0.0, cell=1.0, gx=8, gy=8)
BLOCK_CLEARANCE = 0.3
BLOCK_TARGETS = ((0.5, 0.5), (7.5, 7.5), (7.5, 0.5))               # arena k takes BLOCK_TARGETS[k]


def serpentine_world(n=64):
    """thin walls through the centres of every odd row of an n x n grid of unit cells, each leaving one cell open at alternating ends:
    the shortest path from one corner to the other runs through every corridor"""
    polys = []
    for r in range(1, n - 1, 2):
        if r % 4 == 1:
            polys.append(rect(0.0, r + 0.45, n - 1.1, r + 0.55))
        else:
            polys.append(rect(1.1, r + 0.45, float(n), r + 0.55))
    return polys


SERPENTINE_CLEARANCE = 0.3


def hall_world(w=64.0, h=32.0):
    return [[(0.0, 0.0), (0.0, h), (w, h), (w, 0.0)]]


HALL_GRID = dict(x0=0.0, y0=0.0, cell=0.25, gx=256, gy=128)
HALL_CLEARANCE = 0.3


def trap_world():
    """a hall with a cup open to the left: agents that start left of it and want to the right of it walk into the cup"""
    return [[(-2.0, -2.0), (-2.0, 12.0), (12.0, 12.0), (12.0, -2.0)],
            rect(6.0, 2.0, 6.2, 8.0), rect(3.0, 1.8, 6.2, 2.0), rect(3.0, 8.0, 6.2, 8.2)]


TRAP_GRID = dict(x0=-2.0, y0=-2.0, cell=0.5, gx=28, gy=28)
TRAP_CLEARANCE = 0.75
TRAP_TARGET = (9.0, 5.0)
TRAP_STEPS = 1200
TRAP_LOOKAHEAD = 6     # 3 units: every goal lies within that many pointer steps of the shared target, so an agent near it heads for its own goal


def trap_agents(n=8):
    """positions and goals of n agents in two columns left of the cup, every goal of its own behind the cup's back wall"""
    i = np.arange(n)
    px, py = (0.0 - 1.2 * (i // 4)).astype(F), (3.2 + 1.2 * (i % 4)).astype(F)
    gx, gy = 8.0 + 2.0 * (i // 4), 2.6 + 1.6 * (i % 4)
    return px, py, gx.astype(np.float64), gy.astype(np.float64)


def trap_params():
    """ca_config fields of the trap runs: the reference env's constants, done when within 2 R of the goal, no step cap"""
    return dict(time_step=1 / 60., neighbor_dist=1.5, max_neighbors=5, time_horizon=1.5, time_horizon_obst=1.5, radius=0.5, max_speed=1.0,
                max_step=0, done_mode=1, done_x_thresh=2.0, reward_scale=0.3, spawn_x0=-1.5, spawn_x1=1.0, spawn_y0=3.0, spawn_y1=7.0,
                goal_x0=8.0, goal_x1=10.0, goal_y0=3.0, goal_y1=7.0, max_obst_neighbors=16)


def trap_setup(env, fld, A, n=8):
    """the trap's start state on an oracle or a device environment (fld: the module that names its fields), after init_scenario:
    arena a is arena 0 moved up by 0.05 a"""
    px, py, gx, gy = trap_agents(n)
    rep = lambda v, dt, da=0.0: np.stack([(v + da * a) for a in range(A)]).astype(dt)   # noqa: E731
    env.set(fld.FLD_POS_X, rep(px, F)); env.set(fld.FLD_POS_Y, rep(py, F, 0.05))
    env.set(fld.FLD_VEL_X, np.zeros((A, n), F)); env.set(fld.FLD_VEL_Y, np.zeros((A, n), F))
    env.set(fld.FLD_PREF_X, np.ones((A, n), F)); env.set(fld.FLD_PREF_Y, np.zeros((A, n), F))
    for f, v in ((fld.FLD_GOAL_X, gx), (fld.FLD_GOAL_Y, gy), (fld.FLD_GOAL2_X, gx), (fld.FLD_GOAL2_Y, gy)):
        env.set(f, rep(v, np.float64))
    env.set(fld.FLD_AGENT_DONE, np.zeros((A, n), np.int32)); env.set(fld.FLD_ARENA_DONE, np.zeros(A, np.int32))
    env.set(fld.FLD_STEP_COUNT, np.zeros(A, np.int32))


def trap_cpu_run(A, steps, navigate, every=None, lookahead=TRAP_LOOKAHEAD, n=8):
    """the behaviour loop on the CPU oracle: restatement's nav_pref -> set(PREF_X / PREF_Y) -> orca_step, `steps` times (navigate=False:
    orca_step alone).  Returns dict(done [A, n], obst_collisions, records [(pos_x, pos_y, vel_x, vel_y)] after every `every`-th step)."""
    from oracle import oracle as o
    e = o.OracleEnv(o.make_config(n_arenas=A, n_agents=n, seed=0, **trap_params()))
    e.set_obstacles(trap_world())
    e.init_scenario(o.SCN_DOORWAY)
    trap_setup(e, o, A, n)
    g = Grid(**TRAP_GRID)
    fields = all_fields([edges_of_table(e.obstacle_table(cap=256))], g, TRAP_CLEARANCE, [TRAP_TARGET])
    cls, records = np.zeros((A, n), np.int32), []
    for s in range(steps):
        if navigate:
            px, py, _, m = nav_pref(g, fields, cls, lookahead, e.get(o.FLD_POS_X), e.get(o.FLD_POS_Y), e.get(o.FLD_GOAL_X), e.get(o.FLD_GOAL_Y),
                                    o.pref_dir64, e.get(o.FLD_AGENT_DONE) == 0)
            cx, cy = e.get(o.FLD_PREF_X), e.get(o.FLD_PREF_Y)
            cx[m], cy[m] = px[m], py[m]
            e.set(o.FLD_PREF_X, cx); e.set(o.FLD_PREF_Y, cy)
        e.orca_step(flags=o.F_STATS)
        if every and (s + 1) % every == 0:
            records.append(tuple(e.get(f) for f in (o.FLD_POS_X, o.FLD_POS_Y, o.FLD_VEL_X, o.FLD_VEL_Y)))
    return dict(done=e.get(o.FLD_AGENT_DONE), obst_collisions=e.stats()["obst_collisions"], records=records, fields=fields)
