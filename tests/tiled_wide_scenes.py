"""Scenes of the wide tiled handle (ca_create_ex with CA_CREATE_TILED_WIDE; csrc/ca_tiled.h tiled_solve_kernel<..., WideObstLists>):
pillar halls that bring more than 16 obstacle edges in range of an agent, for crowds larger than the ordinary wide handle's 128.
tests/test_tiled_wide_cpu.py runs every sequence below on the oracle alone (the input guard: lists above 16, none that overflows
unless the scene says so); tests/test_gpu_tiled_wide.py runs the same sequences on the HIP handle beside the oracle.  A sequence
takes the HIP handles as a list -- empty in the guard -- so both files execute the same steps with the same seeds."""
import numpy as np

from collision_avoidance_amd import _lib, alan, scenarios
from oracle import oracle as o
from tests import helpers as H
from tests import wide_worlds as W

PLAIN, GRID = 33, 37          # CA_CREATE_TILED | CA_CREATE_TILED_WIDE, ... | CA_CREATE_TILED_GRID
TILE = 64                     # the tile of a handle with lists above 16
FULL = o.F_OBS | o.F_STATS
LDS_PER_CU = 160 * 1024

# name -> (N, arguments of scenarios.pillar_hall, steps the GPU test runs, edges of the hall)
HALLS = {
    "130": (130, (130, 60, 0.8), 100, 3140),
    "300": (300, (300, 40, 1.0), 120, 4628),
    "1100": (1100, (1100, 60, 1.0), 10, 14404),
}
DENSE = dict(N=130, args=(130, 40, 0.65), kw=dict(size=0.2, x0=0.3, y0=0.3), steps=40, edges=4904)   # overflows lists of 64


def hall(name):
    return scenarios.pillar_hall(*HALLS[name][1])


def dense_hall():
    return scenarios.pillar_hall(*DENSE["args"], **DENSE["kw"])


def n_edges(polys):
    return sum(len(q) for q in polys)


def hall_worlds(name, A=2):
    """arena 0 the hall, every other arena the border only"""
    N = HALLS[name][0]
    return [hall(name)] + [[W.border(scenarios.envsize("crowd", N))] for _ in range(A - 1)]


def tiled_kw(flags, edge_grid=False):
    return dict(tiled="grid" if flags == GRID else True, tiled_wide=True, edge_grid=edge_grid)


def make_gpu(A, N, worlds, S, flags, edge_grid=False, seed=8, allow=False, **over):
    p = H.scenario_params("crowd", N, **over)
    return H.make_gpu(A, N, "crowd", p, seed=seed, polys=dict(per_arena=worlds), max_obst_neighbors=S, allow_obst_overflow=allow,
                      **tiled_kw(flags, edge_grid))


def make_oracle(A, N, worlds, S, seed=8, **over):
    return W.make_pair(A, N, worlds, S, seed=seed, gpu=False, **over)[1]


def gpu_step(g):
    def f(act):
        if act is None:
            g.orca_step(with_obs=True, stats=True)
        else:
            g.step(act, stats=True)
    return f


def stepper(gs, e):
    """one step of every HIP handle in gs and of the oracle"""
    fs = [gpu_step(g) for g in gs] + [W.oracle_step(e)]

    def f(act):
        for s in fs:
            s(act)
    return f


class Top(object):
    """the largest obstacle list the oracle has shown"""

    def __init__(self, e):
        self.e, self.top = e, 0

    def look(self):
        self.top = max(self.top, int(self.e.get(o.FLD_OBST_COUNT).max()))
        return self.top


def run_alternate(gs, e, A, N, steps, every=50, same=None):
    """W.alternate (seed 2) on every handle; same(s) where the GPU test compares; returns the largest list of the oracle"""
    top = Top(e)
    step = stepper(gs, e)

    def both(act):
        step(act)
        top.look()

    W.alternate(both, A, N, steps, every=every, check=same)
    return top.top


# ---- the ring (tests/test_gpu_wide_obstacle_lists.py _ring_pair: 3 arenas of 2 agents near the centre of a ring of short edges) ----
def ring_gpu(n_edges_, S, flags, allow=False, A=3, N=2):
    p = H.scenario_params("doorway", N)
    g = H.make_gpu(A, N, "doorway", p, seed=3, arena_offset=40, max_obst_neighbors=S, polys=W.ring_world(n_edges_),
                   allow_obst_overflow=allow, **tiled_kw(flags))
    px, py = W.ring_positions(A, N)
    g.set(_lib.FLD_POS_X, px); g.set(_lib.FLD_POS_Y, py)
    return g


def ring_oracle(n_edges_, S, A=3, N=2):
    c = H.make_oracle(A, N, "doorway", H.scenario_params("doorway", N), seed=3, arena_offset=40, max_obst_neighbors=S,
                      polys=W.ring_world(n_edges_))
    px, py = W.ring_positions(A, N)
    c.set(o.FLD_POS_X, px); c.set(o.FLD_POS_Y, py)
    return c


def run_ring(gs, c, steps=40, A=3, N=2):
    rng = np.random.RandomState(9)
    top = Top(c)
    for s in range(steps):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        for g in gs:
            g.step(act, stats=True)
        c.step(act, flags=FULL)
        top.look()
    return top.top


# ---- the rest of a tiled handle, on the N = 130 hall --------------------------------------------------------------------------------
def run_alan(gs, e, steps=10):
    for env in gs + [e]:
        env.alan_configure(alan.DEFAULT_ACTIONS)
    top = Top(e)
    for s in range(steps):
        for g in gs:
            g.alan_step(stats=True, with_obs=(s == steps - 1))
        e.alan_step(flags=o.F_STATS | (o.F_OBS if s == steps - 1 else 0))
        top.look()
    return top.top


def run_resets(gs, e, A, N, same=None):
    """20 alternating steps, reset_masked of arena 0, 60 steps with auto-reset (the handles are made with max_step=40: every arena
    ends an episode and starts another); returns the largest list before and after the reset"""
    tops = [run_alternate(gs, e, A, N, 20, every=20, same=(lambda s: same("before the reset")) if same else None)]
    mask = np.array([1] + [0] * (A - 1), np.int32)
    for g in gs:
        g.reset_masked(mask)
    e.reset_masked(mask, flags=o.F_OBS)
    if same:
        same("reset_masked")
    rng = np.random.RandomState(6)
    top = Top(e)
    for s in range(60):
        if s % 2:
            act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
            for g in gs:
                g.step(act, stats=True, autoreset=True)
            e.step(act, flags=FULL | o.F_AUTORESET)
        else:
            for g in gs:
                g.orca_step(with_obs=True, stats=True, autoreset=True)
            e.orca_step(flags=FULL | o.F_AUTORESET)
        top.look()
        if same and s % 20 == 19:
            same("auto-reset step %d" % s)
    return tops + [top.top]


def run_worlds_come_and_go(gs, e, A, N, worlds, same=None):
    """the hall, the border for every arena, the hall again: 10 alternating steps each; the largest list of each stage"""
    tops = []
    for stage, install in enumerate((None, "border", "hall")):
        for env in gs + [e]:
            if install == "border":
                env.set_obstacles([W.border(scenarios.envsize("crowd", N))])
            elif install == "hall":
                env.set_obstacles_per_arena(worlds)
        tops.append(run_alternate(gs, e, A, N, 10, every=10, same=(lambda s, st=stage: same("stage %d" % st)) if same else None))
    return tops


# ---- the largest size: 16384 agents, the crowd's border and one ring of 24 edges ------------------------------------------------------
LARGEST = dict(N=16384, S=24, agents=(0, 8191, 16383), spots=((4.6, 5.0), (5.4, 4.9), (5.0, 5.6)))


def largest_world():
    return [W.border(scenarios.envsize("crowd", LARGEST["N"]))] + W.ring_world(24)


def largest_place(env, fld):
    """three agents -- of the first tile, of a middle one and of the last -- into the ring"""
    px, py = env.get(fld.FLD_POS_X).copy(), env.get(fld.FLD_POS_Y).copy()
    for i, (x, y) in zip(LARGEST["agents"], LARGEST["spots"]):
        px[0, i], py[0, i] = x, y
    env.set(fld.FLD_POS_X, np.ascontiguousarray(px, np.float32))
    env.set(fld.FLD_POS_Y, np.ascontiguousarray(py, np.float32))
