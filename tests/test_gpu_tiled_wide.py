"""Obstacle lists of 17 .. 64 edges on a tiled handle (ca_create_ex with CA_CREATE_TILED_WIDE, flags 33 and 37; csrc/ca_tiled.h
tiled_solve_kernel<KMAX, TILE, SEARCH, WideObstLists> and csrc/ca_obs.h obs_kernel<256, true, false, WideObstLists>): crowds of more
than 128 agents in pillar halls without truncated lists.  Everything is compared bit for bit with the unchanged CPU oracle at the
same capacity through tests/helpers.py; the sequences are those of tests/tiled_wide_scenes.py, which tests/test_tiled_wide_cpu.py
runs on the oracle alone (lists above 16, none that overflows unless the scene is there to overflow)."""
import ctypes as C
import os

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from oracle import oracle as o
from tests import helpers as H
from tests import tiled_wide_scenes as T
from tests import wide_worlds as W

pytestmark = pytest.mark.gpu

FORMS = [(T.PLAIN, False), (T.GRID, False), (T.GRID, True)]           # flags 33, flags 37, flags 37 with the static edge grid


def _is_wide_tiled(g, flags):
    """a tile of 64 whose line table fits a CU, the launches of the flags without bit 32"""
    ti, li = g.tiled_info(), g.launch_info()
    assert ti["tiled"] and ti["tile_agents"] == T.TILE and ti["tiles_per_arena"] == (g.N + T.TILE - 1) // T.TILE, ti
    assert ti["launches_per_step"] == (6 if flags == T.GRID else 3), ti
    table = ti["tile_agents"] * ((g.K + g.S) * 16 + 8)
    assert table <= T.LDS_PER_CU, (ti, g.K, g.S)
    assert li["lanes_per_agent"] == 1 and li["rollout_one_launch"] == 0 and li["block"] == T.TILE, li
    if flags == T.PLAIN:                                               # (a grid handle reports its bin launch: no dynamic LDS)
        assert li["lds_bytes"] == table, (li, table)
    return ti


def _no_overflow(g, top):
    """what every test that expects no overflow asserts"""
    g.sync()                                                           # (raises if a list overflowed)
    assert g.stats()["obst_overflow"] == 0 and top > 16, top


def _same(gs, e, what):
    for k, g in enumerate(gs):
        H.assert_state_equal(g, e, "%s, handle %d" % (what, k), obs=True, reward=True)


def _same_stats(gs, e, what):
    for k, g in enumerate(gs):
        H.assert_stats_equal(g, e, "%s, handle %d" % (what, k))


def _close(gs):
    for g in gs:
        g.close()


# ---- 1. smallest shapes: the ring ------------------------------------------------------------------------------------------------------
def test_ring_of_64_with_a_list_that_holds_every_edge():
    gs = [T.ring_gpu(64, 64, flags) for flags in (T.PLAIN, T.GRID)]
    for g, flags in zip(gs, (T.PLAIN, T.GRID)):
        _is_wide_tiled(g, flags)
    c = T.ring_oracle(64, 64)
    top = T.run_ring(gs, c)
    _same(gs, c, "ring 64"); _same_stats(gs, c, "ring 64")
    assert top == 64
    for g in gs:
        _no_overflow(g, int(g.get(_lib.FLD_OBST_COUNT).max()))
    _close(gs)


@pytest.mark.parametrize("flags", [T.PLAIN, T.GRID])
def test_ring_of_24_with_a_list_of_20(flags):
    g = T.ring_gpu(24, 20, flags)
    _is_wide_tiled(g, flags)
    g.orca_step(stats=True)
    with pytest.raises(RuntimeError) as ei:
        g.sync()
    msg = str(ei.value)
    assert "(-5)" in msg and "overflowed" in msg and "max_obst_neighbors=20" in msg and "24 obstacle edges" in msg, msg
    assert g.get(_lib.FLD_OBST_COUNT).max() == 20
    g.close()
    g, c = T.ring_gpu(24, 20, flags, allow=True), T.ring_oracle(24, 20)   # accepted: the oracle's truncation, the nearest 20
    T.run_ring([g], c)
    g.sync()
    _same([g], c, "ring 24 / 20"); _same_stats([g], c, "ring 24 / 20")
    assert g.stats()["obst_overflow"] > 0
    g.close()


# ---- 2. two tiles and a partial one, at every K class; five tiles ----------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 10, 16])
def test_hall_130_on_every_search(K):
    """tiles of 64, 64 and 2 agents; arena 1 holds the border only.  One oracle run serves the three searches."""
    N, _, steps, _ = T.HALLS["130"]
    worlds = T.hall_worlds("130")
    gs = [T.make_gpu(2, N, worlds, 64, flags, eg, max_neighbors=K) for flags, eg in FORMS]
    for g, (flags, eg) in zip(gs, FORMS):
        assert _is_wide_tiled(g, flags)["tiles_per_arena"] == 3 and g.edge_grid_info()["on"] == (1 if eg else 0)
    e = T.make_oracle(2, N, worlds, 64, max_neighbors=K)
    top = T.run_alternate(gs, e, 2, N, steps, same=lambda s: _same(gs, e, "hall 130, K = %d, step %d" % (K, s)))
    _same_stats(gs, e, "hall 130")
    for g in gs:
        _no_overflow(g, int(g.get(_lib.FLD_OBST_COUNT)[0].max()))
    assert top > 16
    _close(gs)


def test_hall_300_five_tiles():
    N, _, steps, _ = T.HALLS["300"]
    worlds = T.hall_worlds("300")
    g = T.make_gpu(2, N, worlds, 64, T.GRID, True)
    assert _is_wide_tiled(g, T.GRID)["tiles_per_arena"] == 5
    e = T.make_oracle(2, N, worlds, 64)
    top = T.run_alternate([g], e, 2, N, steps, every=60, same=lambda s: _same([g], e, "hall 300 step %d" % s))
    _same_stats([g], e, "hall 300")
    _no_overflow(g, top)
    g.close()


# ---- 3. equal to the ordinary wide handle -----------------------------------------------------------------------------------------------
def test_equal_to_the_ordinary_wide_handle():
    N, worlds = 100, W.hall_b_worlds(2)
    g = T.make_gpu(2, N, worlds, 64, T.PLAIN)
    plain, e = W.make_pair(2, N, worlds, 64)
    _is_wide_tiled(g, T.PLAIN)
    assert not plain.tiled and plain.launch_info()["lds_bytes"] == plain.launch_info()["block"] * ((plain.K + plain.S) * 16 + 32)
    top = T.run_alternate([g, plain], e, 2, N, 60, every=60, same=lambda s: _same([g, plain], e, "hall B step %d" % s))
    for name in ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "REWARD", "OBS"):
        f = getattr(_lib, "FLD_" + name)
        H._eq(g.get(f), plain.get(f), "tiled against the ordinary wide handle, " + name)
    (gc, gi), (pc, pi) = g.obstacle_neighbor_lists(), plain.obstacle_neighbor_lists()
    H._eq(gc, pc, "obstacle counts")
    mask = np.arange(gi.shape[2])[None, None, :] < gc[:, :, None]
    H._eq(np.where(mask, gi, -1), np.where(mask, pi, -1), "obstacle lists")
    _same_stats([g, plain], e, "hall B")
    _no_overflow(g, top); _no_overflow(plain, top)
    _close([g, plain])


# ---- 4. ids above 1023, many tiles ------------------------------------------------------------------------------------------------------
def test_hall_1100():
    N, _, steps, _ = T.HALLS["1100"]
    worlds = T.hall_worlds("1100", 1)
    g = T.make_gpu(1, N, worlds, 64, T.GRID, True)
    assert _is_wide_tiled(g, T.GRID)["tiles_per_arena"] == 18
    e = T.make_oracle(1, N, worlds, 64)
    top = T.run_alternate([g], e, 1, N, steps, every=5, same=lambda s: _same([g], e, "hall 1100 step %d" % s))
    _same_stats([g], e, "hall 1100")
    _no_overflow(g, top)
    assert (g.get(_lib.FLD_OBST_COUNT)[0, 1024:] > 16).any() and g.neighbor_lists()[1].max() > 1023
    g.close()


# ---- 5. truncation at a full list of 64 -----------------------------------------------------------------------------------------------
def test_dense_hall_truncates_like_the_oracle():
    """4904 edges, more than 64 of them in range of some agents: the largest key falls off a full list, under the arrival order of
    the scan (edge ids ascending) and of the edge-grid walk (cell by cell)"""
    N, steps = T.DENSE["N"], T.DENSE["steps"]
    worlds = [T.dense_hall()]
    gs = [T.make_gpu(1, N, worlds, 64, T.GRID, eg, allow=True) for eg in (True, False)] + [T.make_gpu(1, N, worlds, 64, T.PLAIN, allow=True)]
    e = T.make_oracle(1, N, worlds, 64)
    top = T.run_alternate(gs, e, 1, N, steps, every=20, same=lambda s: _same(gs, e, "dense hall step %d" % s))
    for g in gs:
        g.sync()
    _same_stats(gs, e, "dense hall")                                    # (obst_overflow among them)
    assert top == 64 and e.stats()["obst_overflow"] > 0
    _close(gs)


# ---- 6. the rest of a tiled handle on the wide kernels ----------------------------------------------------------------------------------
def test_rollout_and_trace():
    N, worlds = 130, T.hall_worlds("130")
    g, e = T.make_gpu(2, N, worlds, 64, T.GRID, True), T.make_oracle(2, N, worlds, 64)
    g.rollout(30, stats=True)
    for s in range(30):
        e.orca_step(flags=o.F_STATS)
    H.assert_state_equal(g, e, "rollout(30)")
    tr = g.rollout(5, stats=True, trace=dict(every=1, channels=("pos", "vel"), arenas=False))
    rec = tr["agents"].cpu().numpy()
    top = 0
    for r in range(5):
        e.orca_step(flags=o.F_STATS)
        top = max(top, int(e.get(o.FLD_OBST_COUNT).max()))
        for c, f in enumerate((o.FLD_POS_X, o.FLD_POS_Y, o.FLD_VEL_X, o.FLD_VEL_Y)):
            H._eq(rec[r, c], e.get(f), "trace record %d, channel %d" % (r, c))
    g.rollout(1, with_obs=True, stats=True); e.orca_step(flags=T.FULL)
    H.assert_state_equal(g, e, "after the traced rollout", obs=True)
    H.assert_stats_equal(g, e, "rollout")
    assert g.stats()["agent_steps"] == 36 * 2 * N
    _is_wide_tiled(g, T.GRID)
    _no_overflow(g, top)
    g.close()


@pytest.mark.parametrize("flags,eg", [(T.PLAIN, False), (T.GRID, True)])
def test_alan_steps(flags, eg):
    N, worlds = 130, T.hall_worlds("130")
    g, e = T.make_gpu(2, N, worlds, 64, flags, eg), T.make_oracle(2, N, worlds, 64)
    top = T.run_alan([g], e)
    H.assert_state_equal(g, e, "alan steps", obs=True, reward=True)
    H._eq(g.get(_lib.FLD_ALAN_ACTION), e.get(o.FLD_ALAN_ACTION), "alan action")
    for gf, of in ((_lib.FLD_ALAN_WEIGHTS, o.FLD_ALAN_WEIGHTS), (_lib.FLD_ALAN_TIMES, o.FLD_ALAN_TIMES)):
        assert np.array_equal(g.get(gf).view(np.uint64), e.get(of).view(np.uint64))
    H.assert_stats_equal(g, e, "alan steps")
    _no_overflow(g, top)
    g.close()


def test_reset_masked_and_auto_reset():
    N, worlds = 130, T.hall_worlds("130")
    g, e = T.make_gpu(2, N, worlds, 64, T.GRID, True, max_step=40), T.make_oracle(2, N, worlds, 64, max_step=40)
    tops = T.run_resets([g], e, 2, N, same=lambda what: H.assert_state_equal(g, e, what, obs=True))
    H.assert_stats_equal(g, e, "resets")
    assert g.stats()["episodes"] >= 2
    _no_overflow(g, min(tops))
    g.close()


def test_installing_worlds_leaves_the_kernels():
    N, worlds = 130, T.hall_worlds("130")
    g, e = T.make_gpu(2, N, worlds, 64, T.PLAIN), T.make_oracle(2, N, worlds, 64)
    ti, li = g.tiled_info(), g.launch_info()

    def same(what):
        H.assert_state_equal(g, e, what, obs=True, reward=True)
        assert g.tiled_info() == ti and g.launch_info() == li, what       # a small world does not change the kernel of a wide handle
    tops = T.run_worlds_come_and_go([g], e, 2, N, worlds, same=same)
    H.assert_stats_equal(g, e, "worlds come and go")
    assert tops[1] <= 4
    _is_wide_tiled(g, T.PLAIN)
    _no_overflow(g, min(tops[0], tops[2]))
    g.close()


# ---- 7. refusals on a live wide handle, and lists of up to 16 ---------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_refusals_on_a_live_wide_handle():
    N, worlds = 130, T.hall_worlds("130")
    g, e = T.make_gpu(2, N, worlds, 64, T.GRID, True), T.make_oracle(2, N, worlds, 64)
    L = _lib.load()
    for call, args in (("ca_set_agent_params", lambda a: (_ptr(a), None, None, None, a.nbytes, 0)),
                       ("ca_set_agent_counts", lambda a: (_ptr(np.asarray([7, 7], np.int32)), 8, 0))):
        a = np.full((2, N), 0.4, np.float32)
        assert getattr(L, call)(g.h, *args(a)) == -1, call
        assert b"tiled" in L.ca_last_error(g.h), L.ca_last_error(g.h)
    top = T.run_alternate([g], e, 2, N, 4, every=4, same=lambda s: _same([g], e, "after the refusals"))   # the handle keeps working
    _no_overflow(g, top)
    g.close()


@pytest.mark.parametrize("flags", [T.PLAIN, T.GRID])
def test_lists_of_16_are_the_handle_without_the_flag(flags):
    N = 300
    p = H.scenario_params("crowd", N)
    polys = scenarios.pillar_hall(N, 6, 3.0)
    kw = T.tiled_kw(flags)
    g = H.make_gpu(1, N, "crowd", p, seed=8, polys=polys, max_obst_neighbors=16, **kw)
    ref = H.make_gpu(1, N, "crowd", p, seed=8, polys=polys, max_obst_neighbors=16, tiled=kw["tiled"])
    assert g.tiled_info() == ref.tiled_info() and g.tiled_info()["tile_agents"] == 128 and g.launch_info() == ref.launch_info()
    rng = np.random.RandomState(2)
    for s in range(20):
        act = rng.uniform(-1, 1, (1, N)).astype(np.float32)
        for env in (g, ref):
            env.step(act, stats=True)
    for name in ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "REWARD", "OBS", "OBST_COUNT", "OBST_IDX", "NB_COUNT", "NB_IDX"):
        f = getattr(_lib, "FLD_" + name)
        H._eq(g.get(f), ref.get(f), "flags %d against flags %d, %s" % (flags, flags - 32, name))
    g.sync(); ref.sync()
    gs, rs = g.stats(), ref.stats()
    assert {k: v for k, v in gs.items() if k != "sum_reward"} == {k: v for k, v in rs.items() if k != "sum_reward"}, (gs, rs)
    assert abs(gs["sum_reward"] - rs["sum_reward"]) <= 1e-9 * max(1.0, abs(rs["sum_reward"]))   # (added in another order)
    _close([g, ref])


# ---- 8. the largest size, and the tiles the environment may ask for ---------------------------------------------------------------------
def test_largest_size():
    L = T.LARGEST
    N, S = L["N"], L["S"]
    p = H.scenario_params("crowd", N)
    g = H.make_gpu(1, N, "crowd", p, seed=8, polys=T.largest_world(), max_obst_neighbors=S, **T.tiled_kw(T.GRID))
    e = H.make_oracle(1, N, "crowd", p, seed=8, polys=T.largest_world(), max_obst_neighbors=S)
    ti = _is_wide_tiled(g, T.GRID)
    assert ti["tiles_per_arena"] == N // ti["tile_agents"] == 256
    T.largest_place(g, _lib); T.largest_place(e, o)
    for s in range(2):
        g.orca_step(with_obs=(s == 1), stats=True)
        e.orca_step(flags=o.F_STATS | (o.F_OBS if s == 1 else 0))
        H.assert_state_equal(g, e, "16384 agents, step %d" % s, obs=(s == 1))
        c = g.get(_lib.FLD_OBST_COUNT)
        assert [int(c[0, i]) for i in L["agents"]] == [24, 24, 24], c[0, list(L["agents"])]
    H.assert_stats_equal(g, e, "16384 agents")
    _no_overflow(g, int(g.get(_lib.FLD_OBST_COUNT).max()))
    g.close()


class _env(object):
    """Environment switches for the duration of a ca_create (the handle latches them)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_tile_of_the_environment_is_honoured_where_the_table_fits():
    """CA_TILE=128: K = 10 with S = 64 fits a CU (152576 B) and computes the same bits; K = 16 with S = 64 (164864 B) is refused, and
    so is CA_TILE=256 with S = 64 -- nothing is launched above the limit.  CA_TILE=256 serves S = 20 with K = 5."""
    N, worlds = 130, T.hall_worlds("130")
    with _env(CA_TILE="128"):
        g = T.make_gpu(2, N, worlds, 64, T.PLAIN)
    ti, li = g.tiled_info(), g.launch_info()
    assert ti["tile_agents"] == 128 and ti["tiles_per_arena"] == 2 and li["block"] == 128 and li["lds_bytes"] == 152576, (ti, li)
    e = T.make_oracle(2, N, worlds, 64)
    top = T.run_alternate([g], e, 2, N, 10, every=10, same=lambda s: _same([g], e, "CA_TILE=128"))
    _no_overflow(g, top)
    g.close()
    Lb = _lib.load()
    h = C.c_void_p()
    for tile, K, S in (("128", 16, 64), ("256", 10, 64), ("256", 16, 40)):
        cfg = _lib.Config(n_arenas=1, n_agents=N, max_obst_neighbors=S, **H.scenario_params("crowd", N, max_neighbors=K))
        with _env(CA_TILE=tile):
            rc = Lb.ca_create_ex(C.byref(cfg), T.PLAIN, 0, None, C.byref(h))
        msg = Lb.ca_last_error(None).decode()
        assert rc == -5 and not h.value, (tile, K, S, rc)
        assert "does not fit the 160 KiB of LDS of a CU" in msg and "max_obst_neighbors=%d" % S in msg, msg
    with _env(CA_TILE="256"):
        g = T.ring_gpu(24, 24, T.GRID)
    assert g.tiled_info()["tile_agents"] == 256
    c = T.ring_oracle(24, 24)
    assert T.run_ring([g], c, steps=6) == 24
    _same([g], c, "CA_TILE=256")
    _no_overflow(g, 24)
    g.close()
