"""The differential scenes of tests/orca_scenes.py on the HIP kernels: every scene is one arena of ONE batched environment
(its own obstacle table, its agents padded to eight with far-away bystanders), advanced by one ORCA step and compared with
the oracle bit for bit -- new velocities, positions, agent- and obstacle-neighbour lists.  tests/test_oracle_orca_definition.py
compares the oracle on the SAME scenes with an independent fp64 restatement, branch by branch (every branch of SURVEY
App. A.3 / A.4 / A.5 taken 100+ times); this file closes the chain for each solve kernel, and every row asserts through the
handle's own reports that it ran the kernel it names:
  lane / table / quad   the register-line lane kernel with its solved-apart path (more than four edges in range), the
                        LDS-line-table kernel, the four-lanes kernel
  wide, params, counts  the wide-list, the per-agent-parameter (arrays equal to the configuration) and the per-arena-count
                        (every arena holds its scene's agents alone: the bystander rows are absent) instantiations of the table kernel
  tiled, tiled_grid, tiled_edges                 the tiled solve (flags 1), with the uniform-grid search (flags 5), with the static edge grid
  tiled_params, tiled_grid_params                flags 17 and 21 (the second with the edge grid), arrays equal to the configuration
  tiled_wide, tiled_grid_wide                    flags 33 and 37 with lists of 20
  pair                  (its own test: it needs arenas of 129 .. 512 agents and lists of at most four edges) the two-lanes kernel
  K classes             table and tiled with max_neighbors 5 (lists cut by K) and, padded to 17 agents, max_neighbors 16
  lists of 64           the `slats` and `crossing` families (17 .. 56 edges in range) on the wide kernel, flags 33, flags 37 and
                        flags 37 with the edge grid
  parameters per agent  with_agent_params(all_scenes) against one simulator of the oracle per arena: the per-agent handle, the same
                        with per-arena counts, flags 17, flags 21, flags 21 with the edge grid"""
import functools
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import orca_scenes as S
from oracle import oracle as o

pytestmark = pytest.mark.gpu
N_PAD = 8


@functools.lru_cache(None)
def _scenes(which):
    """the seeded scene lists, generated once for every test of this file (nobody changes them)"""
    return {"all": S.all_scenes, "dense": S.dense_scenes, "slats": S.slats_scenes, "crossing": S.crossing_scenes}[which](1.0)


def _batch(scenes, n_pad):
    A = len(scenes)
    pos = np.zeros((A, n_pad, 2), np.float32)
    vel = np.zeros((A, n_pad, 2), np.float32)
    pref = np.zeros((A, n_pad, 2), np.float32)
    for a, sc in enumerate(scenes):
        n = len(sc["pos"])
        assert n <= n_pad
        pos[a, :n], vel[a, :n], pref[a, :n] = sc["pos"], sc["vel"], sc["pref"]
        for k in range(n, n_pad):          # bystanders: beyond every range, 100 apart
            pos[a, k] = (1000.0 + 100.0 * k, 2000.0)
    worlds = [[np.asarray(q, np.float32) for q in sc["polys"]] for sc in scenes]
    return pos, vel, pref, worlds


def _params(n_pad, max_neighbors=None):
    return dict(time_step=S.DT, neighbor_dist=S.NEIGHBOR_DIST, max_neighbors=n_pad - 1 if max_neighbors is None else max_neighbors, time_horizon=S.TAU,
                time_horizon_obst=S.TAU_OBST, radius=S.R, max_speed=S.VMAX, max_step=0, done_mode=1, done_x_thresh=0.0,
                reward_scale=0.3, spawn_x0=0.0, spawn_x1=1.0, spawn_y0=0.0, spawn_y1=1.0, goal_x0=0.0, goal_x1=1.0,
                goal_y0=0.0, goal_y1=1.0)


KERNELS = ["lane", "table", "quad", "tiled", "wide", "params", "counts", "tiled_grid", "tiled_edges", "tiled_params", "tiled_grid_params",
           "tiled_wide", "tiled_grid_wide"]
# how each kernel is selected: environment switches at ca_create, constructor arguments, the obstacle-list capacity of both sides
_Q0 = {"CA_QUAD": "0"}
SELECT = {"lane": (_Q0, {}, 16), "table": ({"CA_QUAD": "0", "CA_REG_LINES": "0"}, {}, 16), "quad": ({"CA_QUAD": "1"}, {}, 16),
          "tiled": (_Q0, {"tiled": True}, 16), "wide": (_Q0, {}, 20), "params": (_Q0, {}, 16), "pair": (_Q0, {}, 4),
          "counts": (_Q0, {}, 16), "tiled_grid": (_Q0, {"tiled": "grid"}, 16), "tiled_edges": (_Q0, {"tiled": "grid", "edge_grid": True}, 16),
          "tiled_params": (_Q0, {"tiled": True, "tiled_params": True}, 16),
          "tiled_grid_params": (_Q0, {"tiled": "grid", "tiled_params": True, "edge_grid": True}, 16),
          "tiled_wide": (_Q0, {"tiled": True, "tiled_wide": True}, 20), "tiled_grid_wide": (_Q0, {"tiled": "grid", "tiled_wide": True}, 20),
          # lists of 64 (the slats and crossing families)
          "wide64": (_Q0, {}, S.WIDE_CAP), "tiled_wide64": (_Q0, {"tiled": True, "tiled_wide": True}, S.WIDE_CAP),
          "tiled_grid_wide64": (_Q0, {"tiled": "grid", "tiled_wide": True}, S.WIDE_CAP),
          "tiled_edges_wide64": (_Q0, {"tiled": "grid", "tiled_wide": True, "edge_grid": True}, S.WIDE_CAP)}
PARAM_ROWS = ("params", "tiled_params", "tiled_grid_params")     # arrays that hold the configuration's values
# parameters per agent (orca_scenes.with_agent_params) against the oracle's simulators
SELECT.update({"hetero": (_Q0, {}, 16), "hetero_counts": (_Q0, {}, 16), "hetero_tiled": (_Q0, {"tiled": True, "tiled_params": True}, 16),
               "hetero_tiled_grid": (_Q0, {"tiled": "grid", "tiled_params": True}, 16),
               "hetero_tiled_edges": (_Q0, {"tiled": "grid", "tiled_params": True, "edge_grid": True}, 16)})


@pytest.mark.parametrize("kernel", KERNELS)
def test_differential_scenes_gpu_equals_oracle(kernel):
    _scenes_gpu_equals_oracle(kernel, "all", _scenes("all"), N_PAD).close()


def test_pair_kernel_room_and_notch_scenes_gpu_equal_oracle():
    """The two-lanes kernel (arenas of 129 .. 512 agents, register lines, lists of at most four edges) on the families that hold the
    covered edges and the non-convex vertices: the same scenes padded to 130 agents with the file's bystanders, lists of four.
    Left out are only the scenes in which some agent has more than four edges in range (on the oracle, with lists of 16): 491 of
    the 3000 `room` scenes and no `notch` scene."""
    every = _scenes("all")
    in_range = _oracle_step("all", every, N_PAD, 16, _params(N_PAD)).get(o.FLD_OBST_COUNT).max(axis=1)   # (the oracle run of the tests above)
    scenes = [(sc, n) for sc, n in zip(every, in_range) if sc["family"] in ("room", "notch")]
    assert sum(sc["family"] == "room" for sc, _ in scenes) == 3000 and sum(sc["family"] == "notch" for sc, _ in scenes) == 900
    keep = [sc for sc, n in scenes if n <= 4]
    dropped = [sc["family"] for sc, n in scenes if n > 4]
    print("dropped %d room, %d notch scenes" % (dropped.count("room"), dropped.count("notch")))
    assert dropped.count("notch") == 0 and len(dropped) <= 491, (len(dropped), dropped.count("notch"))
    _scenes_gpu_equals_oracle("pair", "room+notch<=4", keep, 130, max_neighbors=10).close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_dense_overlap_scenes_gpu_equals_oracle(kernel):
    """The dense-overlap family (tests/orca_scenes.py: ten neighbours = a full list at the bench's maxNeighbors 10, three to
    seven of them overlapping the focus agent, in every other scene two of those on opposite sides of it, a wall in range):
    LP3 on nearly anti-parallel far-away lines, where LP1's discriminant is fp32 noise (tests/orca_lp.py) and any other order
    of the same arithmetic gives another answer.  Every agent of every scene, bit for bit; and the scenes do reach the
    regime: some focus agents leave the speed disc by more than 1 %, one of them by more than maxSpeed itself."""
    from collision_avoidance_amd import _lib
    g = _scenes_gpu_equals_oracle(kernel, "dense", _scenes("dense"), 11)
    speed = np.hypot(g.get(_lib.FLD_VEL_X), g.get(_lib.FLD_VEL_Y))
    assert np.isfinite(speed).all()
    assert (speed[:, 0] > 1.01 * S.VMAX).sum() >= 4 and speed[:, 0].max() > 2.0 * S.VMAX, np.sort(speed[:, 0])[-8:]
    g.close()


@pytest.mark.parametrize("n_pad,K", [(N_PAD, 5), (17, 16)], ids=["lists cut by K", "class 16"])
@pytest.mark.parametrize("kernel", ["table", "tiled"])
def test_differential_scenes_other_neighbour_list_classes(kernel, n_pad, K):
    """The kernels are instantiated per class of max_neighbors: the scenes once with max_neighbors 5, which cuts the lists of the
    crowds of seven and eight, and once padded to 17 agents with max_neighbors 16."""
    every = _scenes("all")
    g = _scenes_gpu_equals_oracle(kernel, "all", every, n_pad, max_neighbors=K)
    assert g.K == K
    if K == 5:
        uncut = _oracle_step("all", every, N_PAD, 16, _params(N_PAD)).get(o.FLD_NB_COUNT)      # (the oracle run of the rows above: K = 7)
        assert ((uncut > K) & (g.neighbor_lists()[0] == K)).sum() >= 1000
    g.close()


@pytest.mark.parametrize("kernel", ["wide64", "tiled_wide64", "tiled_grid_wide64", "tiled_edges_wide64"])
@pytest.mark.parametrize("family", ["slats", "crossing"])
def test_lists_of_more_than_16_edges_gpu_equal_oracle(family, kernel):
    """The `slats` and `crossing` families (17 .. 56 short walls' edges in range of the focus agent, walls cut by processObstacles,
    up to 30 uncovered lines in one programme) with lists of 64: the wide insertion, the already-covered scan over more than 16
    lines and LP3 with more than 16 hard lines, on the ordinary wide kernel and the tiled ones."""
    g = _scenes_gpu_equals_oracle(kernel, family, _scenes(family), N_PAD)
    count = g.obstacle_neighbor_lists()[0]
    assert g.S == S.WIDE_CAP and (count[:, 0] > 16).all() and count.max() <= S.WIDE_CAP, (count[:, 0].min(), count.max())
    assert g.stats()["obst_overflow"] == 0
    g.close()


HETERO_ROWS = ["hetero", "hetero_counts", "hetero_tiled", "hetero_tiled_grid", "hetero_tiled_edges"]


@functools.lru_cache(None)
def _hetero():
    """with_agent_params(all_scenes) and one simulator of the oracle per scene after its doStep: positions, velocities and both
    neighbour lists of every agent, and the overlapping pairs of the new positions (computed once, nobody changes them)"""
    from tests.test_gpu_agent_params import _pair_count
    scenes = S.with_agent_params(_scenes("all"))
    A, K = len(scenes), N_PAD - 1
    ref = dict(pos=np.zeros((A, N_PAD, 2), np.float32), vel=np.zeros((A, N_PAD, 2), np.float32), nb_count=np.zeros((A, N_PAD), np.int32),
               nb=np.full((A, N_PAD, K), -1, np.int32), ob_count=np.zeros((A, N_PAD), np.int32), ob=np.full((A, N_PAD, 16), -1, np.int32),
               pairs=np.zeros(A, np.int64))
    for a, sc in enumerate(scenes):
        sim = S.run_oracle_sim(sc, capture=False)[2]
        for i in range(len(sc["pos"])):
            ref["pos"][a, i], ref["vel"][a, i] = sim.getAgentPosition(i), sim.getAgentVelocity(i)
            ref["nb_count"][a, i], ref["ob_count"][a, i] = sim.getAgentNumAgentNeighbors(i), sim.getAgentNumObstacleNeighbors(i)
            ref["nb"][a, i, :ref["nb_count"][a, i]] = [sim.getAgentAgentNeighbor(i, k) for k in range(ref["nb_count"][a, i])]
            ref["ob"][a, i, :ref["ob_count"][a, i]] = [sim.getAgentObstacleNeighbor(i, k) for k in range(ref["ob_count"][a, i])]
        ref["pairs"][a] = _pair_count(ref["pos"][a, :len(sc["pos"])], sc["radius"])
    assert ref["ob_count"].max() == 16          # (ranges of up to 3 x 1.4 + 0.7: the subdivided rooms fill the lists to the brim)
    return scenes, ref


@pytest.mark.parametrize("kernel", HETERO_ROWS)
def test_scenes_with_parameters_per_agent_gpu_equal_the_simulators(kernel):
    """Radius, max_speed and both horizons of its own for every agent of every scene (the scenes and draws that
    tests/test_oracle_orca_definition.py::test_every_branch_by_value_per_agent_parameters holds to the restatement, role by role):
    one ORCA step against one simulator of the oracle per arena, each agent added with its own values -- positions, velocities,
    both neighbour lists, bit for bit, and the collision counter against the overlapping pairs of the new positions.  The
    bystanders carry the configuration's values; with per-arena counts they are absent."""
    from collision_avoidance_amd import _lib
    scenes, ref = _hetero()
    pos, vel, pref, worlds = _batch(scenes, N_PAD)
    A = len(scenes)
    g = _handle(kernel, A, N_PAD, _params(N_PAD), worlds)
    counts = np.array([len(sc["pos"]) for sc in scenes], np.int32)
    if kernel == "hetero_counts":
        g.set_agent_counts(counts)
    prm = {k: np.full((A, N_PAD), S.PARAM_DEFAULTS[k], np.float32) for k in S.PARAM_NAMES}
    for a, sc in enumerate(scenes):
        for k in S.PARAM_NAMES:
            prm[k][a, :counts[a]] = sc[k]
    g.set_agent_params(**prm)
    _is_the_kernel(g, kernel, SELECT[kernel][1])
    _set_scene_state(g, _lib, pos, vel, pref)
    coll = g.arena_stats()["collisions"].astype(np.int64)
    g.orca_step(stats=True, no_done=True)
    g.sync()
    _is_the_kernel(g, kernel, SELECT[kernel][1])
    here = np.arange(N_PAD)[None, :] < counts[:, None]
    what = "scenes/" + kernel
    H._eq(np.stack([g.get(_lib.FLD_POS_X), g.get(_lib.FLD_POS_Y)], -1)[here], ref["pos"][here], what + " position")
    H._eq(np.stack([g.get(_lib.FLD_VEL_X), g.get(_lib.FLD_VEL_Y)], -1)[here], ref["vel"][here], what + " velocity")
    for (gc, gi), cnt, idx, name in ((g.neighbor_lists(), ref["nb_count"], ref["nb"], "agent"), (g.obstacle_neighbor_lists(), ref["ob_count"], ref["ob"], "obstacle")):
        H._eq(gc[here], cnt[here], "%s %s-neighbour count" % (what, name))
        assert not gc[~here].any(), what + ": a bystander with a neighbour"
        H._eq(np.where(np.arange(idx.shape[2])[None, None, :] < cnt[:, :, None], gi[:, :, :idx.shape[2]], -1), idx, "%s %s neighbours" % (what, name))
    assert np.array_equal(g.arena_stats()["collisions"].astype(np.int64) - coll, ref["pairs"]), what
    assert g.stats()["obst_overflow"] == 0 and ref["pairs"].sum() >= 1000
    nv = np.stack([g.get(_lib.FLD_VEL_X)[:, 0], g.get(_lib.FLD_VEL_Y)[:, 0]], 1)
    assert np.mean(np.linalg.norm(nv - pref[:, 0], axis=1) > 1e-3) > 0.3
    g.close()


def _set_scene_state(env, F, pos, vel, pref):
    goal = (pos + pref).astype(np.float64)
    env.set(F.FLD_POS_X, pos[..., 0]); env.set(F.FLD_POS_Y, pos[..., 1])
    env.set(F.FLD_VEL_X, vel[..., 0]); env.set(F.FLD_VEL_Y, vel[..., 1])
    env.set(F.FLD_PREF_X, pref[..., 0]); env.set(F.FLD_PREF_Y, pref[..., 1])
    env.set(F.FLD_GOAL_X, goal[..., 0]); env.set(F.FLD_GOAL_Y, goal[..., 1])
    env.set(F.FLD_GOAL2_X, goal[..., 0]); env.set(F.FLD_GOAL2_Y, goal[..., 1])


_ORACLE = {}


def _oracle_step(tag, scenes, n_pad, max_obst, p):
    """-> the oracle after one ORCA step on the scenes: computed once per (scene list, padding, list capacities) and shared by the
    kernels compared with it; nobody changes it afterwards"""
    key = (tag, n_pad, max_obst, p["max_neighbors"])
    if key not in _ORACLE:
        pos, vel, pref, worlds = _batch(scenes, n_pad)
        c = o.OracleEnv(o.make_config(n_arenas=len(scenes), n_agents=n_pad, seed=0, max_obst_neighbors=max_obst, **p))
        c.set_obstacles_per_arena(worlds)
        _set_scene_state(c, o, pos, vel, pref)
        c.orca_step(flags=o.F_STATS | o.F_NODONE)
        _ORACLE[key] = c
    return _ORACLE[key]


def _is_the_kernel(g, kernel, ctor):
    """The handle's own reports name the family the row claims, so a row that quietly ran another kernel fails here (the LDS sizes:
    tests/test_gpu_wide_obstacle_lists.py, test_gpu_agent_params.py, test_gpu_agent_counts.py, test_gpu_tiled_params.py,
    test_gpu_tiled_wide.py -- each is its instantiation's alone)."""
    info, ti, gi = g.launch_info(), g.tiled_info(), g.tiled_grid_info()
    tiled, grid = bool(ctor.get("tiled")), ctor.get("tiled") == "grid"
    per_agent = kernel in PARAM_ROWS or kernel.startswith("hetero")
    counts = kernel in ("counts", "hetero_counts")
    assert info["lanes_per_agent"] == {"quad": 4, "pair": 2}.get(kernel, 1), info
    assert info["agent_params"] is per_agent and info["agent_counts"] is counts, info
    assert ti["tiled"] is tiled and gi["grid"] is grid, (ti, gi)
    table = (g.K + g.S) * 16
    if tiled:
        assert ti["launches_per_step"] == (6 if grid else 3) and ti["tiles_per_arena"] == 1, ti
        assert ti["tile_agents"] == (64 if g.S > 16 else 128), (ti, g.S)
        if not grid and (per_agent or g.S > 16):
            assert info["lds_bytes"] == ti["tile_agents"] * (table + 8), (info, ti)
        on = [g.edge_grid_info(a)["on"] for a in (0, g.A // 2, g.A - 1)]
        assert on == [1 if ctor.get("edge_grid") else 0] * 3, on
    elif per_agent or counts:
        assert info["rollout_one_launch"] == 0 and info["lds_bytes"] == info["block"] * (table + 36), (info, g.K, g.S)
    elif g.S > 16:
        assert info["rollout_one_launch"] == 0 and info["lds_bytes"] == info["block"] * (table + 32), (info, g.K, g.S)


_ROW_FIELDS = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "AGENT_DONE")


def _present_rows_equal_oracle(g, c, counts, pos, vel, what):
    """A handle with per-arena counts against the PADDED oracle: the bystanders of the oracle stand beyond every range and at rest,
    so the rows that are present must come out bit for bit as there, lists and statistics included; the absent rows keep the
    position and velocity they were given and have empty lists."""
    from collision_avoidance_amd import _lib
    present = np.arange(g.N)[None, :] < counts[:, None]
    assert np.array_equal(g.agent_mask(), present)
    for n in _ROW_FIELDS:
        H._eq(g.get(getattr(_lib, "FLD_" + n))[present], c.get(getattr(o, "FLD_" + n))[present], "%s %s" % (what, n))
    for (gc, gi), fc, fi, name in ((g.neighbor_lists(), o.FLD_NB_COUNT, o.FLD_NB_IDX, "agent"), (g.obstacle_neighbor_lists(), o.FLD_OBST_COUNT, o.FLD_OBST_IDX, "obstacle")):
        oc, oi = c.get(fc), c.get(fi)
        assert not oc[~present].any() and not gc[~present].any(), what + ": a bystander with a neighbour"
        H._eq(gc, oc, "%s %s-neighbour count" % (what, name))
        mask = np.arange(oi.shape[2])[None, None, :] < oc[:, :, None]
        H._eq(np.where(mask, gi, -1), np.where(mask, oi, -1), "%s %s neighbours" % (what, name))
    for n, v in (("POS_X", pos[..., 0]), ("POS_Y", pos[..., 1]), ("VEL_X", vel[..., 0]), ("VEL_Y", vel[..., 1])):
        H._eq(g.get(getattr(_lib, "FLD_" + n))[~present], v[~present], "%s absent rows %s" % (what, n))
    gs, cs = g.stats(), c.stats()
    for k in ("episodes", "collisions", "obst_collisions", "goals_reached", "obst_overflow"):
        assert gs[k] == cs[k], "%s stats.%s gpu=%d oracle=%d" % (what, k, gs[k], cs[k])
    assert gs["agent_steps"] == int(counts.sum()) and cs["agent_steps"] == g.A * g.N, (gs, cs)


def _handle(kernel, A, n_pad, p, worlds):
    """the GPU handle of a row of SELECT with a world per arena"""
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    over, ctor, max_obst = SELECT[kernel]
    old = {k: os.environ.get(k) for k in over}
    os.environ.update(over)
    try:
        return VecCollisionAvoidanceEnv(A, n_pad, scenario=None, params=p, seed=0, max_obst_neighbors=max_obst, use_torch=False,
                                        obstacles=dict(per_arena=worlds), **ctor)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _scenes_gpu_equals_oracle(kernel, tag, scenes, n_pad, max_neighbors=None):
    """-> the open GPU handle, after one ORCA step that equalled the oracle's"""
    from collision_avoidance_amd import _lib
    pos, vel, pref, worlds = _batch(scenes, n_pad)
    A = len(scenes)
    p = _params(n_pad, max_neighbors)
    over, ctor, max_obst = SELECT[kernel]
    g = _handle(kernel, A, n_pad, p, worlds)
    if kernel in PARAM_ROWS:   # per-agent arrays that hold the configuration's values: the AgentParams instantiations, the uniform run's bits
        full = lambda v: np.full((A, n_pad), v, np.float32)
        g.set_agent_params(radius=full(p["radius"]), max_speed=full(p["max_speed"]), time_horizon=full(p["time_horizon"]),
                           time_horizon_obst=full(p["time_horizon_obst"]))
    counts = np.array([len(sc["pos"]) for sc in scenes], np.int32)
    if kernel == "counts":     # every arena holds its scene's agents alone: the bystander rows are absent
        g.set_agent_counts(counts)
    _is_the_kernel(g, kernel, ctor)
    c = _oracle_step(tag, scenes, n_pad, max_obst, p)
    _set_scene_state(g, _lib, pos, vel, pref)
    g.orca_step(stats=True, no_done=True)
    g.sync()                                     # (no world here has more edges in range than the lists hold: the overflow status stays clear)
    _is_the_kernel(g, kernel, ctor)
    if kernel == "counts":
        _present_rows_equal_oracle(g, c, counts, pos, vel, "scenes/" + kernel)
    else:
        H.assert_state_equal(g, c, "scenes/" + kernel)
        H.assert_stats_equal(g, c, "scenes/" + kernel)
    # the step did something in every family: the focus agent's velocity changed from its preferred one somewhere
    nv = np.stack([g.get(_lib.FLD_VEL_X)[:, 0], g.get(_lib.FLD_VEL_Y)[:, 0]], 1)
    fam = np.array([sc["family"] for sc in scenes])
    for f in sorted(set(fam)):
        m = fam == f
        assert np.mean(np.linalg.norm(nv[m] - pref[m, 0], axis=1) > 1e-3) > 0.3, f
    return g
