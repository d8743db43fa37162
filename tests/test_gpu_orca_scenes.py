"""The differential scenes of tests/orca_scenes.py on the HIP kernels: every scene is one arena of ONE batched environment
(its own obstacle table, its agents padded to eight with far-away bystanders), advanced by one ORCA step and compared with
the oracle bit for bit -- new velocities, positions, agent- and obstacle-neighbour lists.  tests/test_oracle_orca_definition.py
compares the oracle on the SAME scenes with an independent fp64 restatement, branch by branch (every branch of SURVEY
App. A.3 / A.4 / A.5 taken 100+ times); this file closes the chain for each solve kernel: the register-line lane kernel with
its solved-apart path (more than four edges in range), the LDS-line-table kernel, the four-lanes kernel, the tiled solve, the
wide-list and the per-agent-parameter instantiations of the table kernel and (its own test: it needs arenas of 129 .. 512 agents
and lists of at most four edges) the two-lanes kernel."""
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
    return S.all_scenes(1.0) if which == "all" else S.dense_scenes(1.0)


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


KERNELS = ["lane", "table", "quad", "tiled", "wide", "params"]
# how each kernel is selected: environment switches at ca_create, constructor arguments, the obstacle-list capacity of both sides
SELECT = {"lane": ({"CA_QUAD": "0"}, {}, 16), "table": ({"CA_QUAD": "0", "CA_REG_LINES": "0"}, {}, 16), "quad": ({"CA_QUAD": "1"}, {}, 16),
          "tiled": ({"CA_QUAD": "0"}, {"tiled": True}, 16), "wide": ({"CA_QUAD": "0"}, {}, 20), "params": ({"CA_QUAD": "0"}, {}, 16),
          "pair": ({"CA_QUAD": "0"}, {}, 4)}


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


def _scenes_gpu_equals_oracle(kernel, tag, scenes, n_pad, max_neighbors=None):
    """-> the open GPU handle, after one ORCA step that equalled the oracle's"""
    from collision_avoidance_amd import _lib
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    pos, vel, pref, worlds = _batch(scenes, n_pad)
    A = len(scenes)
    p = _params(n_pad, max_neighbors)
    over, ctor, max_obst = SELECT[kernel]
    old = {k: os.environ.get(k) for k in over}
    os.environ.update(over)
    try:
        g = VecCollisionAvoidanceEnv(A, n_pad, scenario=None, params=p, seed=0, max_obst_neighbors=max_obst, use_torch=False,
                                     obstacles=dict(per_arena=worlds), **ctor)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    if kernel == "params":   # per-agent arrays that hold the configuration's values: the AgentParams instantiation, the uniform run's bits
        full = lambda v: np.full((A, n_pad), v, np.float32)
        g.set_agent_params(radius=full(p["radius"]), max_speed=full(p["max_speed"]), time_horizon=full(p["time_horizon"]),
                           time_horizon_obst=full(p["time_horizon_obst"]))
    info = g.launch_info()
    assert info["lanes_per_agent"] == {"quad": 4, "pair": 2}.get(kernel, 1), info
    assert info["agent_params"] == (kernel == "params"), info
    assert g.tiled_info()["tiled"] == (kernel == "tiled"), g.tiled_info()
    if kernel == "wide":   # (tests/test_gpu_wide_obstacle_lists.py _is_wide_table: with S > 16 this LDS size is the wide instantiation's alone)
        assert info["rollout_one_launch"] == 0 and info["lds_bytes"] == info["block"] * ((g.K + g.S) * 16 + 32), (info, g.K, g.S)
    c = _oracle_step(tag, scenes, n_pad, max_obst, p)
    _set_scene_state(g, _lib, pos, vel, pref)
    g.orca_step(stats=True, no_done=True)
    g.sync()                                     # (no world here has more edges in range than the lists hold: the overflow status stays clear)
    H.assert_state_equal(g, c, "scenes/" + kernel)
    H.assert_stats_equal(g, c, "scenes/" + kernel)
    # the step did something in every family: the focus agent's velocity changed from its preferred one somewhere
    nv = np.stack([g.get(_lib.FLD_VEL_X)[:, 0], g.get(_lib.FLD_VEL_Y)[:, 0]], 1)
    fam = np.array([sc["family"] for sc in scenes])
    for f in sorted(set(fam)):
        m = fam == f
        assert np.mean(np.linalg.norm(nv[m] - pref[m, 0], axis=1) > 1e-3) > 0.3, f
    return g
