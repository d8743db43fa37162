"""ORCA parameters per agent on the tiled handles (ca_create_ex with CA_CREATE_TILED_PARAMS: flags 17 and 21; csrc/ca_tiled.h's
AgentParams instantiations of the tiled kernels).  Held bit for bit against what the suite already holds to the oracle: the ordinary per-agent handle up to
its 1024 agents (tests/test_gpu_agent_params.py), the oracle's PyRVOSimulator above them (tests/tiled_param_scenes.py), and the
uniform tiled handles where the arrays equal the configuration.  Every test asserts launch_info() / tiled_info(), so that it cannot
pass on another kernel family."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib, alan, scenarios
from tests import agent_param_scenes as S
from tests import edge_grid_scenes as E
from tests import helpers as H
from tests import tiled_param_scenes as T

pytestmark = pytest.mark.gpu

_STATE = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "AGENT_DONE", "STEP_COUNT", "ARENA_DONE", "EPISODE",
          "REGOAL_COUNT", "REWARD", "OBS")
_COUNTERS = ("episodes", "collisions", "obst_collisions", "goals_reached", "obst_overflow", "frozen_steps", "last_episode_steps",
             "last_episode_arrived")
_KIND = {17: True, 21: "grid", 1: True, 5: "grid", 0: False}


def _set_state(g, pos, vel, goal):
    """positions, velocities, targets and the preferred velocity towards the target, [A,N,2] each"""
    pref = np.stack([S.pref_of(pos[a], goal[a]) for a in range(pos.shape[0])])
    for name, v in (("POS_X", pos[..., 0]), ("POS_Y", pos[..., 1]), ("VEL_X", vel[..., 0]), ("VEL_Y", vel[..., 1]),
                    ("PREF_X", pref[..., 0]), ("PREF_Y", pref[..., 1]), ("GOAL_X", goal[..., 0]), ("GOAL_Y", goal[..., 1]),
                    ("GOAL2_X", goal[..., 0]), ("GOAL2_Y", goal[..., 1])):
        g.set(getattr(_lib, "FLD_" + name), np.ascontiguousarray(v))


def _handle(scenes, flags, p=None, set_params=True, worlds=None, **kw):
    """the scenes as arenas of one handle made with create flags `flags` (0: the ordinary handle), their parameters set"""
    A, N = len(scenes), len(scenes[0]["pos"])
    worlds = [sc["world"] for sc in scenes] if worlds is None else worlds
    g = H.make_gpu(A, N, None, p or T.params(), polys=dict(per_arena=worlds), max_obst_neighbors=S.MAX_OBST_NEIGHBORS,
                   tiled=_KIND[flags], tiled_params=flags in (17, 21), **kw)
    _set_state(g, np.stack([sc["pos"] for sc in scenes]), np.stack([sc["vel"] for sc in scenes]), np.stack([sc["goal"] for sc in scenes]))
    if set_params:
        g.set_agent_params(**{k: np.stack([sc[k] for sc in scenes]) for k in S.PARAM_NAMES})
    return g


def _is_tiled_params(g, flags, on=True):
    """a tiled handle of `flags` whose parameters are set (or not): the launches of its uniform twin, one lane per agent"""
    li, ti = g.launch_info(), g.tiled_info()
    assert li["agent_params"] is on and li["lanes_per_agent"] == 1 and li["rollout_one_launch"] == 0, li
    assert ti["tiled"] and ti["launches_per_step"] == (6 if flags & 4 else 3), ti
    assert li["lds_bytes"] == (0 if flags & 4 else ti["tile_agents"] * ((g.K + g.S) * 16 + 8)), (li, ti)
    return li


def _snapshot(g):
    out = {n: g.get(getattr(_lib, "FLD_" + n)) for n in _STATE}
    (nc, ni), (oc, oi) = g.neighbor_lists(), g.obstacle_neighbor_lists()
    out["nb_count"], out["obst_count"] = nc, oc
    out["nb"] = np.where(np.arange(ni.shape[2])[None, None, :] < nc[:, :, None], ni, -1)
    out["obst"] = np.where(np.arange(oi.shape[2])[None, None, :] < oc[:, :, None], oi, -1)
    out["arena_stats"], out["stats"] = g.arena_stats(), g.stats()
    return out


def _same_snapshot(got, want, what):
    for n in _STATE + ("nb_count", "obst_count", "nb", "obst"):
        H._eq(got[n], want[n], "%s %s" % (what, n))
    for k in _COUNTERS:
        assert np.array_equal(got["arena_stats"][k], want["arena_stats"][k]), (what, k, got["arena_stats"][k], want["arena_stats"][k])
    for a, b in zip(got["arena_stats"]["sum_reward"], want["arena_stats"]["sum_reward"]):
        assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (what, a, b)
    for k in ("agent_steps", "episodes", "collisions", "obst_collisions", "goals_reached", "obst_overflow"):
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"][k], want["stats"][k])
    a, b = got["stats"]["sum_reward"], want["stats"]["sum_reward"]
    assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (what, a, b)


# ---- 1. against the ordinary per-agent handle ---------------------------------------------------------------------------------------
_SIDE1, _CAP1 = 20.0, 22


def _p1():
    return T.params(done_mode=_lib.DONE_REGOAL, max_step=_CAP1, reward_scale=0.3, spawn_x0=0.5, spawn_x1=_SIDE1 - 0.5, spawn_y0=0.5,
                    spawn_y1=_SIDE1 - 0.5, goal_x0=0.5, goal_x1=_SIDE1 - 0.5, goal_y0=0.5, goal_y1=_SIDE1 - 0.5)


def _run1(g):
    """20 full steps, then 5 with CA_F_AUTORESET across the step cap: a snapshot after every step"""
    rng = np.random.RandomState(4)
    snaps = []
    for s in range(25):
        act = rng.uniform(-1, 1, (g.A, g.N)).astype(np.float32)
        g.step(act, with_obs=True, stats=True, autoreset=s >= 20)
        snaps.append(_snapshot(g))
    return snaps


@pytest.fixture(scope="module")
def ordinary():
    scenes = [T.scene(21, 200, _SIDE1), T.scene(22, 200, _SIDE1)]
    g = _handle(scenes, 0, _p1())
    li = g.launch_info()
    assert li["agent_params"] and g.tiled_info()["tiled"] is False, li
    snaps = _run1(g)
    assert snaps[-1]["stats"]["episodes"] == 2 and snaps[-1]["stats"]["collisions"] > 0 and snaps[-1]["stats"]["obst_overflow"] == 0
    assert (snaps[19]["EPISODE"] == 0).all() and (snaps[-1]["EPISODE"] == 1).all()
    g.close()
    return dict(scenes=scenes, snaps=snaps)


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("flags", [17, 21])
def test_equals_the_ordinary_per_agent_handle(ordinary, flags, tile, monkeypatch):
    monkeypatch.setenv("CA_TILE", str(tile))
    g = _handle(ordinary["scenes"], flags, _p1())
    _is_tiled_params(g, flags)
    assert g.tiled_info()["tile_agents"] == tile and g.tiled_info()["tiles_per_arena"] == (4 if tile == 64 else 2)
    for s, (got, want) in enumerate(zip(_run1(g), ordinary["snaps"])):
        _same_snapshot(got, want, "flags %d tile %d step %d" % (flags, tile, s))
    _is_tiled_params(g, flags)
    g.close()


# ---- 2 - 4. above 1024 agents and the sparse crowd, against the simulator -----------------------------------------------------------------
def _sim_steps(sc, steps):
    """the scene on the simulator: after every step positions, velocities, both lists and the overlapping pairs"""
    sim = S.Sim(sc)
    out = []
    for s in range(steps):
        sim.step()
        pos = sim.positions()
        out.append(dict(pos=pos, vel=sim.velocities(), nb=sim.agent_neighbors(), obst=sim.obstacle_neighbors(cap=S.MAX_OBST_NEIGHBORS),
                        pairs=T.pair_count(pos, sc["radius"])))
    return sim, out


def _against(g, ref, what):
    """orca_step(stats, no_done) per recorded step: positions, velocities and both lists equal the simulator's bit for bit, and the
    collision counter grew by the number of overlapping pairs"""
    coll = int(g.arena_stats()["collisions"][0])
    for s, want in enumerate(ref):
        g.orca_step(stats=True, no_done=True)
        w = "%s step %d" % (what, s)
        px, py, vx, vy = (g.get(f)[0] for f in (_lib.FLD_POS_X, _lib.FLD_POS_Y, _lib.FLD_VEL_X, _lib.FLD_VEL_Y))
        H._eq(np.stack([px, py], 1), want["pos"], w + " position")
        H._eq(np.stack([vx, vy], 1), want["vel"], w + " velocity")
        (nc, ni), (oc, oi) = g.neighbor_lists(), g.obstacle_neighbor_lists()
        (snc, sni), (soc, soi) = want["nb"], want["obst"]
        H._eq(nc[0], snc, w + " agent-neighbour count")
        H._eq(np.where(np.arange(g.K)[None, :] < snc[:, None], ni[0], -1), sni, w + " agent neighbours")
        H._eq(oc[0], soc, w + " obstacle-neighbour count")
        H._eq(np.where(np.arange(g.S)[None, :] < soc[:, None], oi[0], -1), soi, w + " obstacle neighbours")
        now = int(g.arena_stats()["collisions"][0])
        assert now - coll == want["pairs"], (w, now - coll, want["pairs"])
        coll = now


@pytest.fixture(scope="module")
def large():
    """1100 agents on a grid handle next to the simulator for 5 steps (checked step by step), then observed once"""
    sc = T.scene(21, 1100, 47.0)
    sim, ref = _sim_steps(sc, 5)
    g = _handle([sc], 21)
    _is_tiled_params(g, 21)
    assert g.tiled_info()["tiles_per_arena"] == 9
    _against(g, ref, "1100 agents, grid")
    ids = g.neighbor_lists()[1]
    obs = np.array(g.observe()).reshape(1100, 16, 4)
    _is_tiled_params(g, 21)
    out = dict(sc=sc, sim=sim, ref=ref, obs=obs, max_id=int(ids.max()), overflow=g.stats()["obst_overflow"])
    g.close()
    return out


def test_above_1024_agents_equals_the_simulator(large):
    assert large["max_id"] > 1023 and large["overflow"] == 0 and large["ref"][-1]["pairs"] > 100   # (compared step by step in the fixture)
    g = _handle([large["sc"]], 17)                                            # the scan of the whole arena: steps 1 and 2
    _is_tiled_params(g, 17)
    _against(g, large["ref"][:2], "1100 agents, plain")
    g.close()


def test_observation_above_1024_agents(large):
    """As test_mixed_agents_observation of tests/test_gpu_agent_params.py: every neighbour as the octagon of ITS radius, through the
    oracle's fp32 comp_laser; the project's 3e-5 absolute; a ray is left out only where fp32 and fp64 comp_laser on the same segments
    differ by more than that, at most 1 % of the rays."""
    sim = large["sim"]
    pos, vel, goal, rad = sim.positions(), sim.velocities(), sim.sc["goal"], sim.sc["radius"]
    (nc, ni), (oc, oi), edges = sim.agent_neighbors(), sim.obstacle_neighbors(), sim.obstacle_edges()
    rays = left_out = on_agent = unequal = 0
    worst = 0.0
    for i in range(sim.n):
        seg = S.observation_segments(pos, vel, rad, i, ni[i, :nc[i]], oi[i, :oc[i]], edges, np.float32)
        f32 = S.laser(pos, goal, seg, i, np.float32)
        f64 = S.laser(pos, goal, seg.astype(np.float64), i, np.float64)
        skip = S.excusable_rays(f32, f64)
        got = large["obs"][i]
        err = np.abs(got.astype(np.float64) - f32.astype(np.float64)).max(axis=1)
        rays += 16
        left_out += int(skip.sum())
        unequal += int((got.view(np.uint32) != f32.view(np.uint32)).any(axis=1).sum())
        on_agent += int(S.rays_on_agents(pos, goal, seg, 8 * nc[i], i).sum())
        worst = max(worst, float(err[~skip].max()) if (~skip).any() else 0.0)
        assert (err[~skip] <= S.OBS_TOL).all(), ("agent %d" % i, err, skip)
    print("rays", rays, "left out", left_out, "not bit-equal", unequal, "largest error", worst, "on an agent's octagon", on_agent)
    assert left_out <= S.OBS_MAX_LEFT_OUT * rays, (left_out, rays)
    assert on_agent >= 1000, on_agent


def test_sparse_crowd_counts_pairs_through_the_lists():
    """300 agents in a 60 x 60 box: lists that are not full, the list branch of the pair count"""
    sc = T.scene(24, 300, 60.0)
    _, ref = _sim_steps(sc, 10)
    assert min(r["nb"][0].min() for r in ref) < S.MAX_NEIGHBORS
    g = _handle([sc], 21)
    _is_tiled_params(g, 21)
    _against(g, ref, "sparse")
    g.close()


# ---- 5. the edge grid with unequal ranges ----------------------------------------------------------------------------------------------------
def test_edge_grid_is_built_for_the_largest_range():
    N = 200
    e = scenarios.crowd_envsize(N)
    sc = S.draw(23, N, 0.5, e - 0.5)
    sc["time_horizon_obst"] = np.random.RandomState(5).uniform(0.5, 1.0, N).astype(np.float32)
    sc["world"] = E.hall(N)
    largest = float(T.obstacle_range(sc).max())
    assert 2.25 < largest < 2.26
    p = T.params(done_mode=_lib.DONE_REGOAL, max_step=0, goal_x0=0.5, goal_x1=e - 0.5, goal_y0=0.5, goal_y1=e - 0.5)
    before = _handle([sc], 21, p, set_params=False, edge_grid=True)      # the edge grid first, then the parameters
    cfg_info = before.edge_grid_info()
    assert cfg_info["on"] == 1 and 2.0 <= cfg_info["cell_size_x"] < largest and 2.0 <= cfg_info["cell_size_y"] < largest, cfg_info
    prm = {k: sc[k][None, :] for k in S.PARAM_NAMES}
    before.set_agent_params(**prm)
    after = _handle([sc], 21, p)                                          # the parameters first, then the edge grid
    after.set_edge_grid(True)
    scan = _handle([sc], 21, p)                                           # the scan of the arena's table
    for g in (before, after):
        info = g.edge_grid_info()
        assert info["on"] == 1 and info["cell_size_x"] >= largest and info["cell_size_y"] >= largest and info["entries"] > 0, info
    assert before.edge_grid_info() == after.edge_grid_info() and scan.edge_grid_info()["on"] == 0
    for g in (before, after, scan):
        _is_tiled_params(g, 21)
    rng = np.random.RandomState(6)
    for s in range(10):
        act = rng.uniform(-1, 1, (1, N)).astype(np.float32)
        snaps = []
        for g in (before, after, scan):
            g.step(act, with_obs=True, stats=True)
            snaps.append(_snapshot(g))
        _same_snapshot(snaps[0], snaps[2], "grid before the parameters, step %d" % s)
        _same_snapshot(snaps[1], snaps[2], "grid after the parameters, step %d" % s)
    st = scan.stats()
    assert st["obst_overflow"] == 0 and st["obst_collisions"] > 0 and scan.obstacle_neighbor_lists()[0].max() > 0, st
    before.clear_agent_params()
    assert before.edge_grid_info() == cfg_info
    _is_tiled_params(before, 21, on=False)
    for g in (before, after, scan):
        g.close()


# ---- 6. the radius in the wall and goal tests -------------------------------------------------------------------------------------------------
def _two_arenas(radius, pos, goal):
    """two arenas of one agent each in an empty box, the agent at rest, on a flags-17 handle"""
    box = [[(0.0, 0.0), (0.0, 10.0), (10.0, 10.0), (10.0, 0.0)]]
    p = T.params(done_mode=_lib.DONE_GOAL, max_step=0)
    g = H.make_gpu(2, 1, None, p, polys=box, tiled=True, tiled_params=True)
    z = np.zeros((2, 1, 2), np.float32)
    _set_state(g, np.asarray(pos, np.float32).reshape(2, 1, 2), z, np.asarray(goal, np.float64).reshape(2, 1, 2))
    g.set_agent_params(radius=np.asarray(radius, np.float32))
    _is_tiled_params(g, 17)
    return g


def test_wall_hits_and_arrival_take_the_agents_radius():
    # 0.45 from the wall x = 0, heading along it: counts with r = 0.5 (0.2025 < 0.25), not with r = 0.4 (0.16)
    g = _two_arenas([0.5, 0.4], [(0.45, 5.0), (0.45, 5.0)], [(0.45, 9.0), (0.45, 9.0)])
    g.orca_step(stats=True, no_done=True)
    x = g.get(_lib.FLD_POS_X)[:, 0]
    assert (x < 0.5).all() and (x > 0.4).all(), x
    assert list(g.arena_stats()["obst_collisions"]) == [1, 0], g.arena_stats()
    g.close()
    # CA_DONE_GOAL, 0.9 from the goal: r = 0.5 arrives (0.9 < 1.0; the step brings it at most 1 / 60 closer), r = 0.3 does not (0.6)
    g = _two_arenas([0.5, 0.3], [(5.0, 5.0), (5.0, 5.0)], [(5.9, 5.0), (5.9, 5.0)])
    g.orca_step(stats=True)
    assert list(g.get(_lib.FLD_AGENT_DONE)[:, 0]) == [1, 0] and list(g.arena_stats()["goals_reached"]) == [1, 0]
    g.close()


# ---- 7. the calls -------------------------------------------------------------------------------------------------------------------------------
_RAW = _STATE + ("NB_COUNT", "OBST_COUNT", "NB_IDX", "OBST_IDX", "ARENA_STATS")


def _same_handles(g1, g2, what):
    for n in _RAW:
        a, b = g1.get(getattr(_lib, "FLD_" + n)), g2.get(getattr(_lib, "FLD_" + n))
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, n)


def _steps(g, n, seed):
    rng = np.random.RandomState(seed)
    for s in range(n):
        g.step(rng.uniform(-1, 1, (g.A, g.N)).astype(np.float32), stats=True)


def _crowd(N, flags, A=1, seed=11):
    return H.make_gpu(A, N, "crowd", H.scenario_params("crowd", N), seed=seed, tiled=_KIND[flags], tiled_params=flags in (17, 21))


def test_config_values_and_clear_give_the_uniform_bits():
    N = 1100
    g, ref = _crowd(N, 21), _crowd(N, 5)
    _is_tiled_params(g, 21, on=False)                                        # no parameters yet: the uniform kernels
    assert g.launch_info() == ref.launch_info()
    g.set_agent_params(**{k: np.full((1, N), getattr(g.cfg, k), np.float32) for k in S.PARAM_NAMES})
    _is_tiled_params(g, 21)
    assert not ref.launch_info()["agent_params"]
    _steps(g, 10, 1); _steps(ref, 10, 1)
    _same_handles(g, ref, "config values")
    g.clear_agent_params()
    _is_tiled_params(g, 21, on=False)
    assert g.launch_info() == ref.launch_info()
    _steps(g, 3, 2); _steps(ref, 3, 2)
    _same_handles(g, ref, "after clear_agent_params")
    g.close(); ref.close()


def _raw_set(g, arrays, nbytes=None):
    L = _lib.load()
    ptrs = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in arrays]
    rc = L.ca_set_agent_params(g.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], g.A * g.N * 4 if nbytes is None else nbytes, 0)
    return rc, (L.ca_last_error(g.h) or b"").decode()


@pytest.mark.parametrize("configured", [False, True], ids=["no parameters yet", "parameters set"])
def test_refused_calls_leave_the_handle_as_it_was(configured):
    A, N = 2, 150
    g, ref = _crowd(N, 21, A), _crowd(N, 21, A)
    rng = np.random.RandomState(2)
    first = {k: rng.uniform(*S.RANGES[k], size=(A, N)).astype(np.float32) for k in S.PARAM_NAMES}
    if configured:
        g.set_agent_params(**first); ref.set_agent_params(**first)
    before = g.launch_info()
    good = np.full((A, N), 0.4, np.float32)
    for k, name in enumerate(S.PARAM_NAMES):
        for bad_value in (np.nan, 0.0, 2e3):
            arrays = [good.copy() for _ in range(4)]
            arrays[k][1, 7] = bad_value
            rc, msg = _raw_set(g, arrays)
            assert rc == -5 and name + "=" in msg and "arena 1, agent 7" in msg, (name, bad_value, rc, msg)
    for nbytes in (A * N * 4 - 4, A * N * 8, 0):
        rc, msg = _raw_set(g, [good] * 4, nbytes)
        assert rc == -4, (nbytes, rc, msg)
    L = _lib.load()
    counts = np.full(A, N - 1, np.int32)
    assert L.ca_set_agent_counts(g.h, counts.ctypes.data_as(C.c_void_p), A * 4, 0) == -1 and b"tiled" in L.ca_last_error(g.h)
    assert g.launch_info() == before and before["agent_params"] is configured
    got = g.agent_params()
    for k in S.PARAM_NAMES:
        H._eq(got[k], first[k] if configured else np.full((A, N), getattr(g.cfg, k), np.float32), "agent_params() " + k)
    _steps(g, 5, 3); _steps(ref, 5, 3)
    _same_handles(g, ref, "after refused calls")
    g.close(); ref.close()


def test_a_handle_made_without_the_flag_keeps_refusing():
    g, ref = _crowd(150, 5), _crowd(150, 5)
    rc, msg = _raw_set(g, [np.full((1, 150), 0.4, np.float32)] * 4)
    assert rc == -1 and "tiled" in msg, (rc, msg)
    assert not g.launch_info()["agent_params"]
    _steps(g, 3, 4); _steps(ref, 3, 4)
    _same_handles(g, ref, "flags 5")
    g.close(); ref.close()


@pytest.mark.parametrize("flags", [17, 21])
def test_alan_step_equals_the_ordinary_per_agent_handle(ordinary, flags):
    u = np.random.RandomState(8).uniform(0, 1, (2, 200))
    snaps = []
    for f in (0, flags):
        g = _handle(ordinary["scenes"], f, _p1())
        g.alan_configure(alan.DEFAULT_ACTIONS)
        if f:
            _is_tiled_params(g, f)
        g.alan_step(u, with_obs=True, stats=True)
        snap = _snapshot(g)
        snap["alan"] = [g.get(getattr(_lib, "FLD_ALAN_" + n)) for n in ("ACTION", "WEIGHTS", "TIMES")]
        snaps.append(snap)
        g.close()
    _same_snapshot(snaps[1], snaps[0], "alan step, flags %d" % flags)
    for a, b, n in zip(snaps[1]["alan"], snaps[0]["alan"], ("action", "weights", "times")):
        H._eq(a, b, "alan " + n)


def test_rollout_trace_equals_single_steps():
    sc = T.scene(24, 300, 60.0)
    g, ref = _handle([sc], 21), _handle([sc], 21)
    tr = g.rollout(4, stats=True, trace=dict(every=1, channels=("pos", "vel"), arenas=False))
    rec = tr["agents"].cpu().numpy()
    _is_tiled_params(g, 21)
    for r in range(4):
        ref.orca_step(stats=True)
        for c, f in enumerate((_lib.FLD_POS_X, _lib.FLD_POS_Y, _lib.FLD_VEL_X, _lib.FLD_VEL_Y)):
            H._eq(rec[r, c], ref.get(f), "trace record %d, channel %d" % (r, c))
    _same_handles(g, ref, "traced rollout")
    g.close(); ref.close()
