"""neighbor_dist and max_neighbors per agent on the GPU (ca_set_agent_sensing), the two remaining arguments the reference hands to
every addAgent call (collision_avoidence_env.py:126-133).  The CPU oracle carries both per agent at its core, so everything is held
bit for bit: mixed agents against the oracle's PyRVOSimulator and the numpy rule (tests/agent_sensing_scenes.py, whose inputs
tests/test_agent_sensing_cpu.py checks on the CPU alone), arenas with constants of their own against an oracle environment configured
with them.  Every test asserts launch_info() / tiled_info(), so that it cannot pass on another kernel."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib, alan, scenarios
from oracle import oracle as o
from tests import agent_count_scenes as AC
from tests import agent_param_scenes as S
from tests import agent_sensing_scenes as Z
from tests import helpers as H
from tests import tiled_param_scenes as T

pytestmark = pytest.mark.gpu

_KIND = {17: True, 21: "grid", 1: True, 5: "grid", 33: True, 0: False}
_FIELDS = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "AGENT_DONE", "STEP_COUNT", "ARENA_DONE", "EPISODE",
           "REGOAL_COUNT", "REWARD", "OBS", "NB_COUNT", "OBST_COUNT", "NB_IDX", "OBST_IDX", "ARENA_STATS")


def _is_sensing(g, params=None, counts=False):
    """launch_info() of an ordinary handle with per-agent sensing: the one-lane LDS-line-table kernel family of ca_set_agent_params (a
    table of K + S lines, the staged arena, the misc ints and the staged radii per lane), T launches per rollout"""
    li = g.launch_info()
    assert li["agent_sensing"] is True and li["lanes_per_agent"] == 1 and li["rollout_one_launch"] == 0, li
    assert li["lds_bytes"] == li["block"] * ((g.K + g.S) * 16 + 36), (li, g.K, g.S)
    assert li["agent_counts"] is counts and (params is None or li["agent_params"] is params), li
    assert not g.tiled_info()["tiled"]
    return li


def _is_tiled_sensing(g, flags):
    """a tiled handle of `flags` with per-agent sensing: the launches of its uniform twin, one lane per agent"""
    li, ti = g.launch_info(), g.tiled_info()
    assert li["agent_sensing"] is True and li["lanes_per_agent"] == 1 and li["rollout_one_launch"] == 0, li
    assert ti["tiled"] and ti["launches_per_step"] == (6 if flags & 4 else 3), ti
    assert li["lds_bytes"] == (0 if flags & 4 else ti["tile_agents"] * ((g.K + g.S) * 16 + 8)), (li, ti)
    if flags & 4:
        assert g.tiled_grid_info()["sort_launches"] == 3 and g.tiled_grid_info()["cell_size"] == 0.5 * Z.NEIGHBOR_DIST   # the uniform handle's sort
    return li


def _set_state(g, pos, vel, goal):
    pref = np.stack([S.pref_of(pos[a], goal[a]) for a in range(pos.shape[0])])
    for name, v in (("POS_X", pos[..., 0]), ("POS_Y", pos[..., 1]), ("VEL_X", vel[..., 0]), ("VEL_Y", vel[..., 1]),
                    ("PREF_X", pref[..., 0]), ("PREF_Y", pref[..., 1]), ("GOAL_X", goal[..., 0]), ("GOAL_Y", goal[..., 1]),
                    ("GOAL2_X", goal[..., 0]), ("GOAL2_Y", goal[..., 1])):
        g.set(getattr(_lib, "FLD_" + name), np.ascontiguousarray(v))


def _handle(scenes, flags=0, params=False, sensing=True, **kw):
    """the scenes as arenas of one handle made with create flags `flags` (0: an ordinary handle), a world each; the handle's own
    values are the recipe's capacities (range 5, 10 neighbours)"""
    A, N = len(scenes), len(scenes[0]["pos"])
    worlds = [sc.get("world", S.WORLD) for sc in scenes]
    g = H.make_gpu(A, N, None, T.params(), polys=dict(per_arena=worlds), max_obst_neighbors=S.MAX_OBST_NEIGHBORS, tiled=_KIND[flags],
                   tiled_params=flags in (17, 21), tiled_wide=flags == 33, **kw)
    _set_state(g, np.stack([sc["pos"] for sc in scenes]), np.stack([sc["vel"] for sc in scenes]), np.stack([sc["goal"] for sc in scenes]))
    if params:
        g.set_agent_params(**{k: np.stack([sc[k] for sc in scenes]) for k in S.PARAM_NAMES})
    if sensing:
        g.set_agent_sensing(neighbor_dist=np.stack([sc["neighbor_dist"] for sc in scenes]), max_neighbors=np.stack([sc["max_neighbors"] for sc in scenes]))
    return g


def _lists(g, a=0):
    """(count [N], idx [N, K]) of arena a with -1 beyond the count -- where the device holds its narrow -1 (an 8-bit id up to 256
    agents, 16 bits above and on tiled handles), which is asserted: a slot at or beyond K_i never keeps a stale id"""
    nc, ni = g.neighbor_lists()
    beyond = np.arange(g.K)[None, :] >= nc[a][:, None]
    empty = 0xFFFF if (g.tiled_info()["tiled"] or g.N > 256) else 0xFF
    assert (ni[a][beyond] == empty).all(), (a, np.unique(ni[a][beyond]))
    return nc[a], np.where(beyond, -1, ni[a])


def _against_sims(g, sims, steps, what, uniform, contacts=False):
    """orca_step(stats, no_done) x steps: after every step positions, velocities and both neighbour lists equal the simulators' bit for
    bit -- slots at or beyond the count hold -1 --, and the per-arena collision counter grew by the number of overlapping pairs of the
    positions read back (and, `contacts`, by half the sum of the contact report's `agents` plane)"""
    coll = g.arena_stats()["collisions"].astype(np.int64)
    for s in range(steps):
        g.orca_step(stats=True, no_done=True)
        for sim in sims:
            sim.step()
        px, py, vx, vy = (g.get(f) for f in (_lib.FLD_POS_X, _lib.FLD_POS_Y, _lib.FLD_VEL_X, _lib.FLD_VEL_Y))
        oc, oi = g.obstacle_neighbor_lists()
        now = g.arena_stats()["collisions"].astype(np.int64)
        touching = g.contacts()["agents"] if contacts else None
        for a, sim in enumerate(sims):
            w = "%s arena %d step %d" % (what, a, s)
            sp, sv = sim.positions(), sim.velocities()
            H._eq(np.stack([px[a], py[a]], 1), sp, w + " position")
            H._eq(np.stack([vx[a], vy[a]], 1), sv, w + " velocity")
            (snc, sni), (soc, soi) = sim.agent_neighbors(), sim.obstacle_neighbors(cap=g.S)
            nc, ni = _lists(g, a)
            H._eq(nc, snc, w + " agent-neighbour count")
            H._eq(ni, sni, w + " agent neighbours")                    # (the whole [N, K] table: -1 from the count on)
            H._eq(oc[a], soc, w + " obstacle-neighbour count")
            H._eq(np.where(np.arange(g.S)[None, :] < soc[:, None], oi[a], -1), soi, w + " obstacle neighbours")
            pairs = T.pair_count(sp, sim.radii(uniform))
            assert now[a] - coll[a] == pairs, (w, now[a] - coll[a], pairs)
            if contacts:
                assert int(touching[a].sum()) == 2 * pairs, (w, int(touching[a].sum()), pairs)
        coll = now
    return coll


def _observation_check(g, sims, uniform, what):
    """the observation of the state the handle holds, against observation_segments / laser with the 5.0 ray table on the simulators'
    own lists: OBS_TOL; only excusable_rays are left out, at most OBS_MAX_LEFT_OUT of all rays"""
    obs = np.array(g.observe()).reshape(len(sims), -1, 16, 4)
    rays = left_out = 0
    for a, sim in enumerate(sims):
        pos, vel, goal, rad = sim.positions(), sim.velocities(), sim.sc["goal"], sim.radii(uniform)
        (nc, ni), (oc, oi), edges = sim.agent_neighbors(), sim.obstacle_neighbors(), sim.obstacle_edges()
        for i in range(sim.n):
            seg = S.observation_segments(pos, vel, rad, i, ni[i, :nc[i]], oi[i, :oc[i]], edges, np.float32)
            f32 = S.laser(pos, goal, seg, i, np.float32)
            f64 = S.laser(pos, goal, seg.astype(np.float64), i, np.float64)
            skip = S.excusable_rays(f32, f64)
            err = np.abs(obs[a, i].astype(np.float64) - f32.astype(np.float64)).max(axis=1)
            rays += 16
            left_out += int(skip.sum())
            assert (err[~skip] <= S.OBS_TOL).all(), ("%s arena %d agent %d" % (what, a, i), err, skip)
    print(what, "rays", rays, "left out", left_out)
    assert left_out <= S.OBS_MAX_LEFT_OUT * rays, (left_out, rays)


# ---- 1. mixed agents: the recipe, 16 x 12, the composite-key path ---------------------------------------------------------------
@pytest.mark.parametrize("params", [False, True], ids=["sensing alone", "with set_agent_params on top"])
def test_mixed_agents_equal_the_simulator(params):
    scenes = [Z.draw(seed) for seed in Z.SEEDS]
    g = _handle(scenes, params=params)
    li = _is_sensing(g, params=params)
    assert li["block"] == 64 and g.N <= 64
    sims = [Z.Sim(sc, uniform=not params) for sc in scenes]
    coll = _against_sims(g, sims, Z.STEPS, "mixed", uniform=not params)
    assert coll.sum() > 100 and g.stats()["obst_overflow"] == 0
    _observation_check(g, sims, not params, "mixed")
    _is_sensing(g, params=params)
    got = g.agent_sensing()
    H._eq(got["neighbor_dist"], np.stack([sc["neighbor_dist"] for sc in scenes]), "agent_sensing() neighbor_dist")
    H._eq(got["max_neighbors"], np.stack([sc["max_neighbors"] for sc in scenes]), "agent_sensing() max_neighbors")
    g.close()


# ---- 2. the three search shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,n,side,block", [(1, 100, 14.0, 128), (1, 200, 20.0, 256), (3, 70, 12.0, 128)],
                         ids=["100 agents: exact scan", "200 agents: LDS grid", "70 agents x 3 arenas"])
def test_search_shapes_equal_the_simulator(A, n, side, block):
    scenes = [Z.crowd(7 + a, n, side) for a in range(A)]
    g = _handle(scenes, params=True)
    assert _is_sensing(g, params=True)["block"] == block and n > 64
    _against_sims(g, [Z.Sim(sc) for sc in scenes], 10, "%d agents" % n, uniform=False)
    g.close()


# ---- 3. the range and tie boundary, on every search path --------------------------------------------------------------------------
@pytest.mark.parametrize("n,flags,block", [(24, 0, 64), (100, 0, 128), (200, 0, 256), (150, 17, None), (150, 21, None)],
                         ids=["composite keys", "exact scan", "LDS grid", "tiled 17", "tiled 21"])
def test_range_and_tie_boundary_against_the_numpy_rule(n, flags, block, monkeypatch):
    """pairs whose dsq lies -2, -1, 0, +1 ulps from fl(nd_i^2) of an nd_i that is not the handle's, and an agent with K_i - 1 nearer
    neighbours and four more at a bit-identical dsq (tests/agent_sensing_scenes.boundary_scene), after one orca_step"""
    if flags:
        monkeypatch.setenv("CA_TILE", "64")
    sc = Z.boundary_scene(n)
    g = _handle([sc], flags)
    if flags:
        _is_tiled_sensing(g, flags)
        assert g.tiled_info()["tile_agents"] == 64 and g.tiled_info()["tiles_per_arena"] == 3
    else:
        assert _is_sensing(g, params=False)["block"] == block
    cnt, idx, _ = Z.ref_lists(sc["pos"], sc["neighbor_dist"], sc["max_neighbors"])
    assert sorted(idx[0, :cnt[0]]) == [1, 2] and list(idx[5, :cnt[5]]) == [6, 7, 8]
    g.orca_step(no_done=True)
    nc, ni = _lists(g)
    H._eq(nc, cnt, "count")
    H._eq(ni, idx, "list")
    g.close()


# ---- 4. constants per arena: an oracle environment per arena, configured with that arena's values --------------------------------
@pytest.mark.parametrize("counts", [None, (12, 5, 1, 9, 12, 7)], ids=["every arena full", "with set_agent_counts"])
def test_constants_per_arena_doorway_with_autoreset(counts):
    """[A] arrays, 6 x 12 in the reference env's own world, CA_DONE_XLESS, max_step 50, CA_F_AUTORESET, 120 steps: state, lists, reward
    and all statistics against one OracleEnv per arena whose ca_config carries that arena's neighbor_dist and max_neighbors.  The
    observation is NOT compared here: the oracle environment sizes its ray table from the arena's neighbor_dist, the handle from its
    own (the laser range stays the handle's: collision_avoidence_env.py:321-332 takes it from the environment, not from the agent)."""
    A, N = 6, 12
    p = dict(scenarios.env_params(), max_step=50, neighbor_dist=Z.NEIGHBOR_DIST, max_neighbors=Z.MAX_NEIGHBORS)
    polys = scenarios.obstacles("doorway", N)
    sc = AC.draw(A, N, (5.0, 0.5), (9.5, 9.5), 31, goal2=((1.0, 5.0), (-10.0, 5.0)))
    nd, K = Z.arena_constants(A, 77)
    g = H.make_gpu(A, N, None, p, seed=31, polys=polys, max_obst_neighbors=16)
    n_of = (N,) * A if counts is None else counts
    if counts is not None:
        sc = AC.with_decoys(sc, counts)
        g.set_agent_counts(np.asarray(counts, np.int32))
    g.set_agent_sensing(neighbor_dist=nd, max_neighbors=K)           # [A] arrays: one value per arena
    AC.set_state(g, _lib, sc)
    rag = Z.ArenaOracles(N, n_of, p, polys, 31, nd, K, g.S)
    for a, (n, e) in enumerate(zip(rag.counts, rag.orc)):
        AC.set_state(e, o, sc, rows=(a, int(n)))
    _is_sensing(g, params=False, counts=counts is not None)
    rng = np.random.RandomState(5)
    for s in range(120):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        g.step(act, with_obs=False, stats=True, autoreset=True)
        for a, (n, e) in enumerate(zip(rag.counts, rag.orc)):
            e.step(act[a:a + 1, :n], flags=o.F_STATS | o.F_AUTORESET)
        if s % 20 == 19 or s in (49, 50):
            AC.same(g, rag, "doorway step %d" % s, obs=False)
    _is_sensing(g, params=False, counts=counts is not None)                 # configuration: it survived the resets
    assert g.stats()["episodes"] >= 2 * A and g.stats()["obst_overflow"] == 0
    H._eq(g.agent_sensing()["max_neighbors"], np.repeat(K[:, None], N, 1), "after the resets")
    g.close()


# ---- 5. identity --------------------------------------------------------------------------------------------------------------------
def _crowd(A=8, N=12, seed=11, **kw):
    return H.make_gpu(A, N, "crowd", scenarios.bench_params(N, 5.0, 10), seed=seed, **kw)


def _same_handles(g1, g2, what):
    for n in _FIELDS:
        a, b = g1.get(getattr(_lib, "FLD_" + n)), g2.get(getattr(_lib, "FLD_" + n))
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, n)


def _steps(g, n, seed=3):
    rng = np.random.RandomState(seed)
    for s in range(n):
        g.step(rng.uniform(-1, 1, (g.A, g.N)).astype(np.float32), stats=True)


def test_arrays_equal_to_the_handles_values_give_the_bits_of_the_per_agent_handle():
    A, N = 8, 12
    g, ref = _crowd(A, N), _crowd(A, N)
    cfgv = {k: np.full((A, N), getattr(g.cfg, k), np.float32) for k in S.PARAM_NAMES}
    ref.set_agent_params(**cfgv)
    g.set_agent_params(**cfgv)
    before = g.launch_info()
    assert before == ref.launch_info() and before["agent_params"] and not before["agent_sensing"]
    g.set_agent_sensing(neighbor_dist=np.full((A, N), g.cfg.neighbor_dist, np.float32), max_neighbors=np.full((A, N), g.cfg.max_neighbors, np.int32))
    _is_sensing(g, params=True)
    _steps(g, 20); _steps(ref, 20)
    _same_handles(g, ref, "config values, 20 steps")
    g.clear_agent_sensing()
    assert g.launch_info() == before                                           # clearing one keeps the other
    _steps(g, 5, seed=4); _steps(ref, 5, seed=4)
    _same_handles(g, ref, "after clear_agent_sensing")
    g.set_agent_sensing(max_neighbors=3)                                       # a scalar; neighbor_dist returns to the handle's
    _is_sensing(g, params=True)
    g.clear_agent_params()
    _is_sensing(g, params=False)                                               # ... and the other way round
    H._eq(g.agent_sensing()["max_neighbors"], np.full((A, N), 3, np.int32), "scalar")
    H._eq(g.agent_sensing()["neighbor_dist"], np.full((A, N), g.cfg.neighbor_dist, np.float32), "None = the handle's value")
    g.orca_step()
    assert g.neighbor_lists()[0].max() == 3
    g.clear_agent_sensing()
    plain = _crowd(A, N)
    assert g.launch_info() == plain.launch_info() and not g.launch_info()["agent_sensing"]
    g.close(); ref.close(); plain.close()


# ---- 6. tiled handles ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,edge_grid", [(17, False), (21, False), (21, True)], ids=["flags 17", "flags 21", "flags 21, edge grid"])
def test_tiled_handles_equal_the_simulator(flags, edge_grid, monkeypatch):
    """150 agents at tile 64 (three tiles, the last one partial), 10 steps against the simulator, statistics checked: the scene holds
    the three cases the close launch's list shortcut must refuse (tests/agent_sensing_scenes.tiled_scene)"""
    monkeypatch.setenv("CA_TILE", "64")
    sc = Z.tiled_scene()
    g = _handle([sc], flags, params=True, edge_grid=edge_grid)
    _is_tiled_sensing(g, flags)
    assert g.tiled_info()["tile_agents"] == 64 and g.tiled_info()["tiles_per_arena"] == 3
    assert bool(g.edge_grid_info()["on"]) is edge_grid
    coll = _against_sims(g, [Z.Sim(sc)], 10, "tiled %d" % flags, uniform=False, contacts=True)
    assert coll[0] > 100                                                       # (the clump alone overlaps in dozens of pairs per step)
    _is_tiled_sensing(g, flags)
    g.close()


# ---- 7. ALAN --------------------------------------------------------------------------------------------------------------------------
def test_alan_step_with_constants_per_arena_and_rollout():
    """ca_alan_step with given uniforms, 4 x 12, 30 steps (select -> solve, the sensing kernel -> update) against one OracleEnv per
    arena; then rollout(20) against 20 orca_steps of a twin"""
    A, N = 4, 12
    p = dict(scenarios.alan_params(N, "crowd"), neighbor_dist=Z.NEIGHBOR_DIST, max_neighbors=Z.MAX_NEIGHBORS)
    polys = Z.box(scenarios.crowd_envsize(N))
    e = scenarios.crowd_envsize(N)
    sc = AC.draw(A, N, 0.5, e - 0.5, 33)
    nd, K = Z.arena_constants(A, 78)
    g, twin = (H.make_gpu(A, N, None, p, seed=33, polys=polys) for _ in range(2))
    rag = Z.ArenaOracles(N, (N,) * A, p, polys, 33, nd, K, g.S)
    for h in (g, twin):
        h.set_agent_sensing(neighbor_dist=nd, max_neighbors=K)
        AC.set_state(h, _lib, sc)
        h.alan_configure(alan.DEFAULT_ACTIONS)
    for a, en in enumerate(rag.orc):
        AC.set_state(en, o, sc, rows=(a, N))
        en.alan_configure(alan.DEFAULT_ACTIONS)
    _is_sensing(g, params=False)
    rng = np.random.RandomState(7)
    for s in range(30):
        u = rng.uniform(0, 1, (A, N))
        for h in (g, twin):
            h.alan_step(u, with_obs=False, stats=True)
        for a, en in enumerate(rag.orc):
            en.alan_step(u[a:a + 1], flags=o.F_STATS)
        if s % 10 == 9:
            AC.same(g, rag, "alan step %d" % s, obs=False)
            act, w, tm = g.get(_lib.FLD_ALAN_ACTION), g.get(_lib.FLD_ALAN_WEIGHTS), g.get(_lib.FLD_ALAN_TIMES)
            for a, en in enumerate(rag.orc):
                H._eq(act[a:a + 1], en.get(o.FLD_ALAN_ACTION), "alan action")
                H._eq(w[a:a + 1], en.get(o.FLD_ALAN_WEIGHTS), "alan weights")
                H._eq(tm[a:a + 1], en.get(o.FLD_ALAN_TIMES), "alan times")
    g.rollout(20, stats=True)
    for s in range(20):
        twin.orca_step(stats=True)
    g.observe(); twin.observe()
    _same_handles(g, twin, "rollout(20) against 20 orca_steps")
    _is_sensing(g, params=False)
    g.close(); twin.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def _raw_set(g, nd, k, nbytes=None):
    L = _lib.load()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = L.ca_set_agent_sensing(g.h, ptr(nd), ptr(k), g.A * g.N * 4 if nbytes is None else nbytes, 0)
    return rc, (L.ca_last_error(g.h) or b"").decode()


@pytest.mark.parametrize("configured", [False, True], ids=["untouched handle", "handle with sensing"])
def test_refused_values_and_sizes_leave_the_handle_as_it_was(configured):
    g, ref = _crowd(3), _crowd(3)
    first = dict(neighbor_dist=np.random.RandomState(2).uniform(1, 5, (g.A, g.N)).astype(np.float32),
                 max_neighbors=np.random.RandomState(3).randint(0, 11, (g.A, g.N)).astype(np.int32))
    if configured:
        g.set_agent_sensing(**first); ref.set_agent_sensing(**first)
    before = g.launch_info()
    good_nd, good_k = np.full((g.A, g.N), 2.0, np.float32), np.full((g.A, g.N), 4, np.int32)
    for bad in (np.float32(g.cfg.neighbor_dist) + np.float32(1e-3), 5e-4, 0.0, -1.0, np.nan, np.inf):   # above the capacity, below CA_MIN_LENGTH, ...
        nd = good_nd.copy(); nd[1, 7] = bad
        rc, msg = _raw_set(g, nd, good_k)
        assert rc == -5 and "neighbor_dist=" in msg and "arena 1, agent 7" in msg, (bad, rc, msg)
    for bad in (-1, g.cfg.max_neighbors + 1, 1 << 20):
        k = good_k.copy(); k[2, 5] = bad
        rc, msg = _raw_set(g, good_nd, k)
        assert rc == -5 and "max_neighbors=" in msg and "arena 2, agent 5" in msg, (bad, rc, msg)
    for nbytes in (g.A * g.N * 4 - 4, g.A * g.N * 8, 0):
        rc, msg = _raw_set(g, good_nd, good_k, nbytes)
        assert rc == -4, (nbytes, rc, msg)
    assert g.launch_info() == before
    got = g.agent_sensing()
    H._eq(got["neighbor_dist"], first["neighbor_dist"] if configured else np.full((g.A, g.N), g.cfg.neighbor_dist, np.float32), "agent_sensing()")
    H._eq(got["max_neighbors"], first["max_neighbors"] if configured else np.full((g.A, g.N), g.cfg.max_neighbors, np.int32), "agent_sensing()")
    _steps(g, 5); _steps(ref, 5)
    _same_handles(g, ref, "after refused calls")
    g.close(); ref.close()


def test_refused_handles_step_on_as_their_untouched_twins():
    """a handle with obstacle lists of 32, and the tiled handles of flags 1, 5 and 33: CA_EINVAL, and the handle keeps working"""
    made = [lambda: _crowd(3, max_obst_neighbors=32)]
    sc = Z.crowd(9, 150, 15.0)
    made += [lambda f=f: _handle([sc], f, sensing=False) for f in (1, 5, 33)]
    for k, make in enumerate(made):
        g, ref = make(), make()
        before = g.launch_info()
        rc, msg = _raw_set(g, np.full((g.A, g.N), 2.0, np.float32), np.full((g.A, g.N), 4, np.int32))
        assert rc == -1 and ("wide obstacle lists" in msg if k == 0 else "CA_CREATE_TILED_PARAMS" in msg), (k, rc, msg)
        assert g.launch_info() == before and not before["agent_sensing"]
        for h in (g, ref):
            for s in range(3):
                h.orca_step(with_obs=True, stats=True)
        _same_handles(g, ref, "refused handle %d" % k)
        g.close(); ref.close()


def test_a_line_table_that_does_not_fit_is_refused():
    g = _crowd(2, 512, max_obst_neighbors=16)
    before = g.launch_info()
    rc, msg = _raw_set(g, np.full((g.A, g.N), 2.0, np.float32), None)
    assert rc == -5 and "does not fit" in msg, (rc, msg)
    assert g.launch_info() == before and not before["agent_sensing"]
    g.orca_step()
    g.close()


def test_constructor_keyword_and_configuration_survives_scenario_and_reset():
    A, N = 3, 12
    sens = dict(neighbor_dist=np.random.RandomState(9).uniform(1, 5, (A, N)).astype(np.float32), max_neighbors=np.asarray([2, 0, 7], np.int32))
    g = _crowd(A, N, agent_sensing=sens)
    _is_sensing(g, params=False)
    g.init_scenario("crowd"); g.reset(); g.reset_masked(np.asarray([1, 0, 1], np.int32))
    _is_sensing(g, params=False)
    H._eq(g.agent_sensing()["neighbor_dist"], sens["neighbor_dist"], "after reset")
    H._eq(g.agent_sensing()["max_neighbors"], np.repeat(sens["max_neighbors"][:, None], N, 1), "after reset")
    assert not any("SENS" in k.upper() or "NEIGHBOR_DIST" in k.upper() for k in g.get_state())            # configuration, not state
    g.orca_step()
    nc = g.neighbor_lists()[0]
    assert nc[0].max() <= 2 and nc[1].max() == 0 and nc[2].max() <= 7
    g.close()
