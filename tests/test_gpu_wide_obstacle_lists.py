"""Obstacle-neighbour lists of 17 .. 64 edges on the GPU: RVO2 keeps every edge in range of an agent
(collision_avoidence_env.py:249, 301-318), and with max_obst_neighbors up to 64 so do the wide LDS-table solve kernel and the
wide observation.  Everything is bit for bit the CPU oracle's at the same capacity (the oracle takes any capacity); the worlds
are those of tests/wide_worlds.py, whose lists tests/test_wide_obstacle_lists_cpu.py checks on the oracle (above 16, never
above 64).  The error paths tested here are return codes."""
import ctypes as C
import os

import numpy as np
import pytest

from collision_avoidance_amd import _lib, alan
from oracle import oracle as o
from tests import helpers as H
from tests import wide_worlds as W

pytestmark = pytest.mark.gpu

FLAGS = o.F_OBS | o.F_STATS


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


def _is_wide_table(g):
    """launch_info() of a handle on the wide LDS-table kernel: one lane per agent, no one-launch rollout, a table of K + S lines
    per lane.  (With S > 16 that LDS size belongs to the wide instantiation alone: the 16-entry table kernel cannot be launched
    with it, and a run on it would not match the oracle at this capacity.)"""
    li = g.launch_info()
    assert li["lanes_per_agent"] == 1 and li["rollout_one_launch"] == 0, li
    assert li["lds_bytes"] == li["block"] * ((g.K + g.S) * 16 + 32), (li, g.K, g.S)


def _ring_pair(n_edges, S, allow=False, switches=None, A=3, N=2):
    p = H.scenario_params("doorway", N)
    with _env(**(switches or {})):
        g = H.make_gpu(A, N, "doorway", p, seed=3, arena_offset=40, max_obst_neighbors=S, polys=W.ring_world(n_edges),
                       allow_obst_overflow=allow)
    c = H.make_oracle(A, N, "doorway", p, seed=3, arena_offset=40, max_obst_neighbors=S, polys=W.ring_world(n_edges))
    px, py = W.ring_positions(A, N)
    for e, fx, fy in ((g, _lib.FLD_POS_X, _lib.FLD_POS_Y), (c, o.FLD_POS_X, o.FLD_POS_Y)):
        e.set(fx, px); e.set(fy, py)
    return g, c


@pytest.mark.parametrize("n_edges", [24, 64])
@pytest.mark.parametrize("switches", [None, {"CA_QUAD": "1"}, {"CA_REG_LINES": "1"}], ids=["default", "CA_QUAD=1", "CA_REG_LINES=1"])
def test_ring_with_a_list_that_holds_every_edge(n_edges, switches):
    g, c = _ring_pair(n_edges, n_edges, switches=switches)
    _is_wide_table(g)                                        # the switches do not apply to a handle with lists above 16
    rng = np.random.RandomState(9)
    top = 0
    for s in range(40):
        act = rng.uniform(-1, 1, (3, 2)).astype(np.float32)
        g.step(act, stats=True); c.step(act, flags=FLAGS)
        top = max(top, int(g.get(_lib.FLD_OBST_COUNT).max()))
    g.sync()                                                 # (raises if a list overflowed)
    H.assert_state_equal(g, c, "ring %d" % n_edges, obs=True, reward=True)
    H.assert_stats_equal(g, c, "ring %d" % n_edges)
    assert g.stats()["obst_overflow"] == 0 and top == n_edges
    g.close()


def test_ring_of_24_with_a_list_of_20():
    g, _ = _ring_pair(24, 20)
    _is_wide_table(g)
    g.orca_step(stats=True)
    with pytest.raises(RuntimeError) as ei:
        g.sync()
    msg = str(ei.value)
    assert "(-5)" in msg and "overflowed" in msg and "max_obst_neighbors=20" in msg and "24 obstacle edges" in msg and "at most 64" in msg, msg
    assert g.get(_lib.FLD_OBST_COUNT).max() == 20
    g.close()
    g, c = _ring_pair(24, 20, allow=True)                    # accepted: the oracle's truncation, the nearest 20
    rng = np.random.RandomState(9)
    for s in range(40):
        act = rng.uniform(-1, 1, (3, 2)).astype(np.float32)
        g.step(act, stats=True); c.step(act, flags=FLAGS)
    g.sync()
    H.assert_state_equal(g, c, "ring 24 / 20", obs=True, reward=True)
    H.assert_stats_equal(g, c, "ring 24 / 20")
    assert g.stats()["obst_overflow"] > 0
    g.close()


def test_ragged_squares_world_without_the_overflow_opt_in():
    """The world tests/test_worlds.py has to run with allow_obst_overflow=True at capacity 16: per-arena tables, sixteen
    agent groups of several arenas per observation workgroup (DENSE), six arenas per solve wave."""
    g, e = W.make_pair(4, 10, W.ragged_squares_worlds(10), 64)
    _is_wide_table(g)
    top = 0
    for s in range(250):
        g.orca_step(with_obs=True, stats=True); e.orca_step(flags=FLAGS)
        if s % 10 == 0:
            top = max(top, int(g.get(_lib.FLD_OBST_COUNT).max()))
        if s % 50 == 49:
            H.assert_state_equal(g, e, "squares step %d" % s, obs=True)
    g.sync()
    H.assert_stats_equal(g, e, "squares")
    assert g.stats()["obst_overflow"] == 0 and top > 32, top
    g.close()


def _gpu_step(g):
    def f(act):
        if act is None:
            g.orca_step(with_obs=True, stats=True)
        else:
            g.step(act, stats=True)
    return f


@pytest.mark.parametrize("name,N,worlds,steps,over", [
    ("A", 64, W.hall_a_worlds, 300, {}),                         # one arena per 64-lane workgroup
    ("B", 100, W.hall_b_worlds, 200, {}),                        # 128 lanes: 156.7 KB of LDS
    ("A/K16", 64, W.hall_a_worlds, 100, {"max_neighbors": 16}),  # the K-class 16 table: 84 KB
])
def test_pillar_halls(name, N, worlds, steps, over):
    g, e = W.make_pair(2, N, worlds(2), 64, **over)
    _is_wide_table(g)
    gs, es = _gpu_step(g), W.oracle_step(e)

    def both(act):
        gs(act); es(act)
    W.alternate(both, 2, N, steps, check=lambda s: H.assert_state_equal(g, e, "hall %s step %d" % (name, s), obs=True, reward=True))
    g.sync()
    H.assert_stats_equal(g, e, "hall " + name)
    assert g.stats()["obst_overflow"] == 0 and g.get(_lib.FLD_OBST_COUNT)[0].max() > 16
    g.close()


def test_rollout_on_a_wide_handle_is_t_steps():
    """ca_rollout on a wide handle: T launches of the wide kernel (no one-launch form), equal to T oracle steps."""
    g, e = W.make_pair(2, 64, W.hall_a_worlds(2), 64)
    _is_wide_table(g)
    g.rollout(60, stats=True)
    for s in range(60):
        e.orca_step(flags=o.F_STATS)
    g.rollout(1, with_obs=True, stats=True); e.orca_step(flags=FLAGS)
    g.sync()
    H.assert_state_equal(g, e, "rollout", obs=True)
    H.assert_stats_equal(g, e, "rollout")
    assert g.stats()["agent_steps"] == 61 * 2 * 64 and g.get(_lib.FLD_OBST_COUNT)[0].max() > 16
    g.close()


def test_pillar_hall_a_in_rounds():
    """More arenas than the chip holds at once with a 78 KB table each (two workgroups per CU): the launch runs in rounds --
    there is no register-line fallback for lists above 16.  One table for every arena, every arena started like arena 0."""
    N, hall = 64, W.pillar_hall(64, 14, 1.0)
    p = H.scenario_params("crowd", N)
    A = 640                                                   # 256 CUs x 2 resident workgroups = 512
    g = H.make_gpu(A, N, "crowd", p, seed=8, polys=hall, max_obst_neighbors=64)
    e = H.make_oracle(1, N, "crowd", p, seed=8, polys=hall, max_obst_neighbors=64)
    _is_wide_table(g)
    assert g.launch_info()["grid"] == A
    for f in (_lib.FLD_POS_X, _lib.FLD_POS_Y, _lib.FLD_VEL_X, _lib.FLD_VEL_Y, _lib.FLD_PREF_X, _lib.FLD_PREF_Y,
              _lib.FLD_GOAL_X, _lib.FLD_GOAL_Y, _lib.FLD_GOAL2_X, _lib.FLD_GOAL2_Y):
        v = g.get(f)
        g.set(f, np.broadcast_to(v[:1], v.shape).copy())
    rng = np.random.RandomState(4)
    for s in range(100):
        if s % 2:
            act = rng.uniform(-1, 1, (1, N)).astype(np.float32)
            g.step(np.broadcast_to(act, (A, N)).copy(), stats=True); e.step(act, flags=FLAGS)
        else:
            g.orca_step(with_obs=True, stats=True); e.orca_step(flags=FLAGS)
        if s % 50 == 49:
            for f, of in ((_lib.FLD_POS_X, o.FLD_POS_X), (_lib.FLD_POS_Y, o.FLD_POS_Y), (_lib.FLD_VEL_X, o.FLD_VEL_X),
                          (_lib.FLD_OBS, o.FLD_OBS), (_lib.FLD_OBST_COUNT, o.FLD_OBST_COUNT), (_lib.FLD_REWARD, o.FLD_REWARD)):
                v = g.get(f)
                H._eq(v[:1], e.get(of), "rounds: arena 0 against the oracle, field %d step %d" % (f, s))
                H._eq(v, np.broadcast_to(v[:1], v.shape), "rounds: every arena against arena 0, field %d step %d" % (f, s))
    g.sync()
    assert g.stats()["obst_overflow"] == 0 and g.get(_lib.FLD_OBST_COUNT).max() > 16
    g.close()


def test_worlds_come_and_go_on_one_wide_handle():
    """A many-edge world, the plain border for every arena, the many-edge world again; then reset_masked and auto-reset
    (tests/wide_worlds.py come_and_go; its lists are checked on the oracle by tests/test_wide_obstacle_lists_cpu.py)."""
    N, A = 10, 4
    worlds = W.come_and_go_worlds(N)
    g, e = W.make_pair(A, N, worlds, 64, max_step=90)

    def same(what):
        H.assert_state_equal(g, e, what, obs=True)
        _is_wide_table(g)                                       # installing a small world does not change the kernel of a wide handle
    tops = W.come_and_go(g, e, A, N, worlds, same=same)
    g.sync()
    assert tops[0] > 16 and tops[1] <= 4 and tops[2] > 16 and tops[3] > 16, tops
    assert g.stats()["episodes"] >= A
    H.assert_stats_equal(g, e, "one wide handle")
    assert g.stats()["obst_overflow"] == 0
    g.close()


def test_alan_online_rollout_on_a_wide_handle():
    """ALAN's bandit around the wide solve: select -> solve -> update (the fused forms have no wide instantiation)."""
    N, A = 10, 4
    g, e = W.make_pair(A, N, W.ragged_squares_worlds(N), 64)
    g.alan_configure(alan.DEFAULT_ACTIONS); e.alan_configure(alan.DEFAULT_ACTIONS)
    _is_wide_table(g)

    def same(what):
        H.assert_state_equal(g, e, what, reward=True)
        H._eq(g.get(_lib.FLD_ALAN_ACTION), e.get(o.FLD_ALAN_ACTION), what + " action")
        for gf, of in ((_lib.FLD_ALAN_WEIGHTS, o.FLD_ALAN_WEIGHTS), (_lib.FLD_ALAN_TIMES, o.FLD_ALAN_TIMES)):
            assert np.array_equal(g.get(gf).view(np.uint64), e.get(of).view(np.uint64)), what
    for s in range(10):
        g.alan_step(stats=True, with_obs=(s == 9)); e.alan_step(flags=o.F_STATS | (o.F_OBS if s == 9 else 0))
    same("alan steps")
    H._eq(g.get(_lib.FLD_OBS), e.get(o.FLD_OBS), "alan obs")
    g.alan_rollout(120, stats=True, freeze=True)
    for s in range(120):
        e.alan_step(flags=o.F_STATS | o.F_FREEZE)
    g.sync()
    same("alan rollout")
    H.assert_stats_equal(g, e, "alan rollout")
    assert g.get(_lib.FLD_OBST_COUNT).max() > 16 and len(np.unique(g.get(_lib.FLD_ALAN_ACTION))) > 1
    g.close()


@pytest.mark.parametrize("N,K", [(200, 10), (128, 16)])
def test_shapes_that_do_not_fit_are_refused(N, K):
    L = _lib.load()
    h = C.c_void_p()
    cfg = _lib.Config(n_arenas=2, n_agents=N, max_obst_neighbors=64, **H.scenario_params("crowd", N, max_neighbors=K))
    rc = L.ca_create(C.byref(cfg), 0, None, C.byref(h))
    assert rc == -5 and not h.value, rc
    msg = L.ca_last_error(None).decode()
    assert "does not fit the 160 KiB of LDS of a CU" in msg and "max_obst_neighbors=64" in msg, msg
    # arenas above 128 agents have no wide kernel, even where a table would fit the LDS (S = 17, K = 5 at 256 lanes: 98 KB)
    cfg = _lib.Config(n_arenas=2, n_agents=200, max_obst_neighbors=17, **H.scenario_params("crowd", 200, max_neighbors=5))
    assert L.ca_create(C.byref(cfg), 0, None, C.byref(h)) == -5 and not h.value
    msg = L.ca_last_error(None).decode()
    assert "max_obst_neighbors=17" in msg and "at most 128 agents" in msg and "n_agents=200" in msg, msg
    # ... while the shapes next to them are served
    for n, k in ((128, 10), (64, 16)):
        cfg = _lib.Config(n_arenas=2, n_agents=n, max_obst_neighbors=64, **H.scenario_params("crowd", n, max_neighbors=k))
        assert L.ca_create(C.byref(cfg), 0, None, C.byref(h)) == 0 and h.value, L.ca_last_error(None)
        L.ca_destroy(h)
