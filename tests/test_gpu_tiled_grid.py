"""The tiled path's uniform-grid neighbour search on the GPU (ca_create_ex with CA_CREATE_TILED | CA_CREATE_TILED_GRID;
csrc/ca_tiled.h): the arena's agents counting-sorted by cell across workgroups, an agent testing the cells its range touches.
Everything is compared bit for bit with the CPU oracle through tests/helpers.py, on the scenes of tests/tiled_scenes.py and
tests/tiled_grid_scenes.py (which tests/test_tiled_cpu.py and tests/test_tiled_grid_cpu.py check on the oracle alone)."""
import ctypes as C
import os

import numpy as np
import pytest

from collision_avoidance_amd import _lib, alan
from oracle import oracle as o
from tests import helpers as H
from tests import tiled_grid_scenes as G
from tests import tiled_scenes as S

pytestmark = pytest.mark.gpu

NO_GRID = dict(grid=False, cells_x=0, cells_y=0, cell_size=0.0, sort_launches=0)


def _is_grid(g):
    gi, ti, li = g.tiled_grid_info(), g.tiled_info(), g.launch_info()
    assert g.tiled and ti["tiled"] and ti["tile_agents"] == S.TILE and ti["tiles_per_arena"] == (g.N + S.TILE - 1) // S.TILE, ti
    assert gi["grid"] and gi["cell_size"] > 0 and gi["sort_launches"] >= 1, gi
    for side in (gi["cells_x"], gi["cells_y"]):
        assert side >= 8 and side & (side - 1) == 0, gi
    assert ti["launches_per_step"] == gi["sort_launches"] + 3, (ti, gi)
    assert li["lanes_per_agent"] == 1 and li["rollout_one_launch"] == 0, li
    return gi


def _grid(A, N, scenario, p, **kw):
    g = H.make_gpu(A, N, scenario, p, tiled="grid", **kw)
    _is_grid(g)
    return g


def _lists_equal(g, other, what):
    for lists in ("neighbor_lists", "obstacle_neighbor_lists"):   # (an empty slot reads -1 at the handle's own id width: masked)
        (gc, gi), (pc, pi) = getattr(g, lists)(), getattr(other, lists)()
        H._eq(gc, pc, "%s, counts of %s" % (what, lists))
        mask = np.arange(gi.shape[2])[None, None, :] < gc[:, :, None]
        H._eq(np.where(mask, gi, -1), np.where(mask, pi, -1), "%s, %s" % (what, lists))


# ---- 1. box scenes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.BOXES))
def test_box_scenes(name):
    scenario, A, N, seed, p = S.box_scene(name)
    g = _grid(A, N, scenario, p, seed=seed)
    orc = H.make_oracle(A, N, scenario, p, seed=seed)
    for s, act in enumerate(S.box_actions(name)):
        g.step(act, stats=True)
        orc.step(act, flags=S.FULL)
        H.assert_state_equal(g, orc, "%s step %d" % (name, s), obs=True, reward=True)
    H.assert_stats_equal(g, orc, name)
    g.close()


# ---- 2. ordinary sizes: against the oracle, a plain tiled handle and an ordinary handle ------------------------------------------
@pytest.mark.parametrize("A,N", [(3, 100), (3, 129), (2, 300), (1, 1024)])
def test_ordinary_sizes(A, N):
    p = H.scenario_params("crowd", N)
    g = _grid(A, N, "crowd", p, seed=21)
    tiled = H.make_gpu(A, N, "crowd", p, seed=21, tiled=True)
    plain = H.make_gpu(A, N, "crowd", p, seed=21)
    orc = H.make_oracle(A, N, "crowd", p, seed=21)
    assert tiled.tiled_info()["launches_per_step"] == 3 and tiled.tiled_grid_info() == NO_GRID and plain.tiled_grid_info() == NO_GRID
    rng = np.random.RandomState(21)
    for s in range(20):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        for e in (g, tiled, plain):
            e.step(act, stats=True)
        orc.step(act, flags=S.FULL)
        H.assert_state_equal(g, orc, "grid %dx%d step %d" % (A, N, s), obs=True, reward=True)
    for other, what in ((tiled, "grid against plain tiled handle"), (plain, "grid against ordinary handle")):
        for name in ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "REWARD", "OBS"):
            f = getattr(_lib, "FLD_" + name)
            H._eq(g.get(f), other.get(f), "%s, %s" % (what, name))
        _lists_equal(g, other, what)
    H.assert_stats_equal(g, orc, "grid")
    for e in (g, tiled, plain):
        e.close()


# ---- 3. the lattice: ties at the K-th distance, candidates out of index order ----------------------------------------------------
def test_lattice_ties():
    p = S.lattice_params()
    g = _grid(1, S.LATTICE_N, "crowd", p, seed=3, polys=[])
    orc = H.make_oracle(1, S.LATTICE_N, "crowd", p, seed=3, polys=[])
    S.lattice_place(g, _lib)
    S.lattice_place(orc, o)
    g.orca_step()
    orc.orca_step(flags=0)
    H.assert_state_equal(g, orc, "lattice")
    g.close()


# ---- 4. the boundary scene and the aliasing scene ------------------------------------------------------------------------------
class _forced_cells(object):
    """CA_TILED_CELLS around a create (the library latches it there)"""

    def __init__(self, side):
        self.side = side

    def __enter__(self):
        self.old = os.environ.get("CA_TILED_CELLS")
        if self.side is not None:
            os.environ["CA_TILED_CELLS"] = str(self.side)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("CA_TILED_CELLS", None)
        else:
            os.environ["CA_TILED_CELLS"] = self.old


def _placed_scene(N, side, build, what, steps=3):
    p = G.params(N)
    with _forced_cells(side):
        g = _grid(1, N, "crowd", p, seed=1, polys=[])
    gi = g.tiled_grid_info()
    if side is not None:
        assert gi["cells_x"] == gi["cells_y"] == side, gi
    m = G.model_of(gi, p["neighbor_dist"])
    px, py = build(m)
    orc = H.make_oracle(1, N, "crowd", p, seed=1, polys=[])
    G.place(g, _lib, px, py)
    G.place(orc, o, px, py)
    for s in range(steps):   # (the first step meets the scene as planted; the later ones re-sort the agents that moved)
        g.orca_step(stats=True)
        orc.orca_step(flags=o.F_STATS)
        H.assert_state_equal(g, orc, "%s step %d" % (what, s))
    H.assert_stats_equal(g, orc, what)
    g.close()
    return m


@pytest.mark.parametrize("N", [300, 1100])
def test_boundary_scene(N):
    def build(m):
        px, py, pairs = G.boundary_scene(N, m)
        cnt, idx = m.lists(px, py, 10)
        assert G.boundary_claims(px, py, pairs, m, cnt, idx) == len(G.BOUNDARY_PAIRS)   # (on this handle's own table)
        return px, py
    _placed_scene(N, None, build, "boundary %d" % N, steps=1)


@pytest.mark.parametrize("N", [300, 1100])
@pytest.mark.parametrize("side", [None, 8])
def test_aliasing_scene(N, side):
    def build(m):
        px, py = G.aliasing_scene(N, m)
        far, strangers = G.aliasing_claims(px, py, m)
        assert far > N and strangers > 0, (far, strangers)
        return px, py
    _placed_scene(N, side, build, "aliasing %d cells %s" % (N, side))


# ---- 5. degenerate fills ------------------------------------------------------------------------------------------------------------
def test_all_agents_in_one_cell():
    _placed_scene(300, None, lambda m: G.one_cell_positions(300, m), "one cell", steps=2)


def test_no_agent_neighbours():
    N = 300
    p = H.scenario_params("crowd", N, max_neighbors=0)
    g = _grid(1, N, "crowd", p, seed=2)
    orc = H.make_oracle(1, N, "crowd", p, seed=2)
    rng = np.random.RandomState(2)
    for s in range(3):
        act = rng.uniform(-1, 1, (1, N)).astype(np.float32)
        g.step(act, stats=True)
        orc.step(act, flags=S.FULL)
        H.assert_state_equal(g, orc, "K = 0 step %d" % s, obs=True, reward=True)
    g.close()


@pytest.mark.parametrize("N", [1, 127, 128, 129])
def test_tile_edges(N):
    p = H.scenario_params("crowd", N)
    g = _grid(2, N, "crowd", p, seed=7)
    orc = H.make_oracle(2, N, "crowd", p, seed=7)
    rng = np.random.RandomState(7)
    for s in range(5):
        act = rng.uniform(-1, 1, (2, N)).astype(np.float32)
        g.step(act, stats=True)
        orc.step(act, flags=S.FULL)
        H.assert_state_equal(g, orc, "N = %d step %d" % (N, s), obs=True, reward=True)
    H.assert_stats_equal(g, orc, "N = %d" % N)
    g.close()


# ---- 6. episode machinery across tiles ------------------------------------------------------------------------------------------------
def test_each_arena_ends_at_its_own_step():
    p = H.scenario_params("crowd", S.ENDS_N)
    g = _grid(2, S.ENDS_N, "crowd", p, seed=9)
    orc = H.make_oracle(2, S.ENDS_N, "crowd", p, seed=9)
    S.ends_setup(g, _lib)
    S.ends_setup(orc, o)
    g.rollout(S.ENDS_STEPS, stats=True, freeze=True)
    orc.rollout(S.ENDS_STEPS, flags=o.F_STATS | o.F_FREEZE)
    H.assert_state_equal(g, orc, "ends")
    H._eq(g.get(_lib.FLD_ARRIVE_STEP), orc.get(o.FLD_ARRIVE_STEP), "ends arrive_step")
    gs, os_ = g.get(_lib.FLD_ARENA_STATS), orc.get(o.FLD_ARENA_STATS)
    for col in (0, 1, 2, 3, 4, 6, 7):   # (5: the sum of rewards, no rewards in an ORCA-only rollout)
        H._eq(gs[:, col], os_[:, col], "ends arena_stats column %d" % col)
    assert g.get(_lib.FLD_ARENA_DONE).all() and (gs[:, 6] > 0).all()
    H.assert_stats_equal(g, orc, "ends")
    g.close()


def test_autoreset_across_tiles():
    scenario, A, N, seed, p = S.box_scene("doorway_1x1300", max_step=8)
    g = _grid(A, N, scenario, p, seed=seed)
    orc = H.make_oracle(A, N, scenario, p, seed=seed)
    for s, act in enumerate(S.box_actions("doorway_1x1300")[:20]):
        g.step(act, stats=True, autoreset=True)
        orc.step(act, flags=S.FULL | o.F_AUTORESET)
        H.assert_state_equal(g, orc, "autoreset step %d" % s, obs=True, reward=True)
        H._eq(g.get(_lib.FLD_ARENA_STATS)[:, :5], orc.get(o.FLD_ARENA_STATS)[:, :5], "autoreset step %d arena counters" % s)
    H.assert_stats_equal(g, orc, "autoreset")
    assert g.stats()["episodes"] == 2 and g.get(_lib.FLD_EPISODE)[0] == orc.get(o.FLD_EPISODE)[0]
    g.close()


def test_per_arena_worlds():
    A, N = 2, 1100
    p = H.scenario_params("crowd", N)
    worlds = S.two_boxes(N)
    g = _grid(A, N, "crowd", p, seed=6, polys=worlds)
    orc = H.make_oracle(A, N, "crowd", p, seed=6, polys=worlds)
    rng = np.random.RandomState(6)
    for s in range(5):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        g.step(act, stats=True)
        orc.step(act, flags=S.FULL)
        H.assert_state_equal(g, orc, "two boxes step %d" % s, obs=True, reward=True)
    H.assert_stats_equal(g, orc, "two boxes")
    assert g.stats()["obst_collisions"] > 0
    g.close()


def test_alan_step_and_rollout():
    A, N = 1, 1100
    p = H.scenario_params("crowd", N)
    g = _grid(A, N, "crowd", p, seed=8)
    orc = H.make_oracle(A, N, "crowd", p, seed=8)
    g.alan_configure(alan.DEFAULT_ACTIONS)
    orc.alan_configure(alan.DEFAULT_ACTIONS)
    u = np.random.RandomState(8).uniform(0, 1, (A, N))
    g.alan_step(u, stats=True)
    orc.alan_step(u, flags=o.F_STATS)
    H.assert_state_equal(g, orc, "alan step", reward=True)
    g.alan_rollout(6, stats=True, freeze=True)
    for _ in range(6):
        orc.alan_step(flags=o.F_STATS | o.F_FREEZE)
    H.assert_state_equal(g, orc, "alan rollout", reward=True)
    H._eq(g.get(_lib.FLD_ALAN_ACTION), orc.get(o.FLD_ALAN_ACTION), "alan action")
    for f in ("FLD_ALAN_WEIGHTS", "FLD_ALAN_TIMES"):
        H._eq(g.get(getattr(_lib, f)), orc.get(getattr(o, f)), "alan " + f)
    H.assert_stats_equal(g, orc, "alan")
    g.close()


def test_resets_then_a_step():
    A, N = 2, 1100
    p = H.scenario_params("crowd", N)
    g = _grid(A, N, "crowd", p, seed=4)
    orc = H.make_oracle(A, N, "crowd", p, seed=4)
    rng = np.random.RandomState(4)
    for s in range(2):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        g.step(act, stats=True)
        orc.step(act, flags=S.FULL)
    e = p["spawn_x1"]
    px, py = rng.uniform(0, e, (A, N)).astype(np.float32), rng.uniform(0, e, (A, N)).astype(np.float32)
    g.reset(px, py, with_obs=True)
    orc.reset(px, py, flags=o.F_OBS)
    H.assert_state_equal(g, orc, "reset with positions", obs=True)
    g.orca_step(with_obs=True, stats=True)
    orc.orca_step(flags=S.FULL)
    H.assert_state_equal(g, orc, "step after reset", obs=True)
    g.reset_masked([0, 1], with_obs=True)
    orc.reset_masked([0, 1], flags=o.F_OBS)
    H.assert_state_equal(g, orc, "reset_masked", obs=True)
    act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
    g.step(act, stats=True)
    orc.step(act, flags=S.FULL)
    H.assert_state_equal(g, orc, "step after the resets", obs=True, reward=True)
    H.assert_stats_equal(g, orc, "resets")
    g.close()


# ---- 7. the call itself ----------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_create_ex_flags_and_refusals():
    L = _lib.load()
    p = H.scenario_params("crowd", 1100)
    h = C.c_void_p()

    def cfg(n, s=4):
        return _lib.Config(n_arenas=1, n_agents=n, arena_offset=0, seed=0, max_obst_neighbors=s, **p)
    for flags in (4, 8, 13):
        assert L.ca_create_ex(C.byref(cfg(1100)), flags, 0, None, C.byref(h)) == -1 and not h.value, flags
    assert L.ca_create_ex(C.byref(cfg(1100, 17)), 5, 0, None, C.byref(h)) == -5 and b"no tiled form" in L.ca_last_error(None)
    assert L.ca_create_ex(C.byref(cfg(1100)), 5, 0, None, C.byref(h)) == 0 and h.value
    assert L.ca_destroy(h) == 0

    plain = H.make_gpu(1, 300, "crowd", H.scenario_params("crowd", 300), seed=1)
    tiled = H.make_gpu(1, 300, "crowd", H.scenario_params("crowd", 300), seed=1, tiled=True)
    assert plain.tiled_grid_info() == NO_GRID and tiled.tiled_grid_info() == NO_GRID
    assert tiled.tiled_info()["launches_per_step"] == 3
    plain.close()
    tiled.close()

    g = _grid(1, 1100, "crowd", p, seed=1)
    orc = H.make_oracle(1, 1100, "crowd", p, seed=1)
    ti, li = g.tiled_info(), g.launch_info()
    assert li["block"] == S.TILE and li["grid"] == ti["tiles_per_arena"] and li["lds_bytes"] == 0, li   # the bin launch
    for call, args in (("ca_set_agent_params", lambda a: (_ptr(a), None, None, None, a.nbytes, 0)),
                       ("ca_set_agent_counts", lambda a: (_ptr(np.asarray([7], np.int32)), 4, 0))):
        a = np.full((1, 1100), 0.4, np.float32)
        assert getattr(L, call)(g.h, *args(a)) == -1, call
        assert b"tiled" in L.ca_last_error(g.h), L.ca_last_error(g.h)
    g.orca_step(stats=True)                        # the handle keeps working
    orc.orca_step(flags=o.F_STATS)
    H.assert_state_equal(g, orc, "after the refusals")
    g.close()


def test_profile_counts_every_launch():
    N = 300
    g = _grid(1, N, "crowd", H.scenario_params("crowd", N), seed=1)
    g.profile(1)
    for _ in range(4):
        g.orca_step()
    prof = g.profile_read()
    assert prof["step_kernel"][0] == 4 * g.tiled_info()["launches_per_step"], prof
    g.close()


def test_overflow_names_the_agent():
    p = H.scenario_params("crowd", S.OVF_N)
    g = _grid(1, S.OVF_N, "crowd", p, seed=2, max_obst_neighbors=1, arena_offset=5)
    S.overflow_place(g, _lib)
    g.orca_step()
    with pytest.raises(RuntimeError) as ei:
        g.sync()
    msg = str(ei.value)
    assert "(-5)" in msg and "arena 5, agent %d had 2 obstacle edges" % S.OVF_AGENT in msg, msg
    assert g.stats()["obst_overflow"] == 1
    g.reset_stats()
    g.sync()
    g.close()


# ---- 8. run-to-run identity -----------------------------------------------------------------------------------------------------------
def test_two_runs_are_identical():
    """the order inside a cell comes from atomics and differs from run to run; nothing the handle leaves may depend on it"""
    scenario, A, N, seed, p = S.box_scene("crowd_2x1500")
    acts = S.box_actions("crowd_2x1500")[:10]
    runs = []
    for _ in range(2):
        g = _grid(A, N, scenario, p, seed=seed)
        for act in acts:
            g.step(act, stats=True)
        fields = ["POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "REWARD", "OBS", "AGENT_DONE", "STEP_COUNT",
                  "ARENA_DONE", "EPISODE", "NB_COUNT", "NB_IDX", "OBST_COUNT", "OBST_IDX", "ARENA_STATS"]
        runs.append([g.get(getattr(_lib, "FLD_" + f)) for f in fields])
        g.close()
    for f, x, y in zip(fields, runs[0], runs[1]):
        if f == "ARENA_STATS":   # (column 5: the sum of rewards, added in the order the waves arrive)
            x, y = np.delete(x, 5, axis=1), np.delete(y, 5, axis=1)
        H._eq(x, y, "two runs, " + f)


# ---- 9. the largest size ---------------------------------------------------------------------------------------------------------------
def test_largest_arena():
    N = _lib.MAX_AGENTS_LARGE
    p = H.scenario_params("crowd", N)
    g = _grid(1, N, "crowd", p, seed=5)
    orc = H.make_oracle(1, N, "crowd", p, seed=5)
    assert g.tiled_info()["tiles_per_arena"] == N // S.TILE
    rng = np.random.RandomState(5)
    for s in range(3):
        act = rng.uniform(-1, 1, (1, N)).astype(np.float32)
        g.step(act, stats=True)
        orc.step(act, flags=S.FULL)
    H.assert_state_equal(g, orc, "16384 agents", obs=True, reward=True)
    H.assert_stats_equal(g, orc, "16384 agents")
    g.close()
