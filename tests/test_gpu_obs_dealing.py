"""The observation kernel deals two pieces of work over the workgroup instead of per agent (ca_obs.h): the neighbour windows of
the pre-pass go to its first 16 K lanes (lane L: agent L / K, slot L % K), and the obstacle neighbours become one list of
(agent, edge slot) items per workgroup that phase A tests lane per (item, ray).  Any dealing of the same (segment, ray) tests
gives the same keys, so every case here is the CPU oracle's observation bit for bit, compared after EVERY step through
helpers.assert_state_equal(..., obs=True): the headline shape, more wall items than a wave-trip holds, the wide lists, lists
that are not full and partial workgroups, gathered neighbours, per-agent radii and absent rows."""
import os

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from oracle import oracle as o
from tests import agent_count_scenes as CS
from tests import helpers as H
from tests import wide_worlds as W

pytestmark = pytest.mark.gpu

FLAGS = o.F_OBS | o.F_STATS


def _make(env, fn):
    """fn() with the environment switches `env` set (ca_create latches them)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _crowd_pair(A, N, K, seed=5, **kw):
    """The bench's world at another shape: the crowd inside its boundary walls, bench_params(N, 5, K)"""
    p = scenarios.bench_params(N, 5.0, K)
    return H.make_gpu(A, N, "crowd", p, seed=seed, **kw), H.make_oracle(A, N, "crowd", p, seed=seed)


def _full_steps(g, e, A, N, steps, what, seed=3, lo=-0.5, hi=0.5):
    """`steps` full steps (actions in, observation out), the two compared after each"""
    rng = np.random.RandomState(seed)
    for s in range(steps):
        act = rng.uniform(lo, hi, (A, N)).astype(np.float32)
        g.step(act, stats=True); e.step(act, flags=FLAGS)
        H.assert_state_equal(g, e, "%s step %d" % (what, s), obs=True)


@pytest.mark.parametrize("A", [8, 3], ids=["8 arenas, XCD remap", "3 arenas"])
def test_headline_kernels_on_an_overlapping_crowd(A):
    """64 agents, K = 10, range 5, walls: 300 ORCA-only steps bring the uniform starts together, then 20 full steps."""
    N = 64
    g, e = _make({"CA_QUAD": "0"}, lambda: _crowd_pair(A, N, 10, seed=0))
    li = g.launch_info()
    assert li["lanes_per_agent"] == 1, li                                               # the one-lane solve
    assert li["obs_grid"] == A * (N // 16), li                                          # 16 agents = 256 lanes per workgroup
    g.rollout(300, stats=True); e.rollout(300, flags=o.F_STATS)
    _full_steps(g, e, A, N, 20, "headline %d" % A)
    nc, oc = e.get(o.FLD_NB_COUNT), e.get(o.FLD_OBST_COUNT)
    assert nc.mean() > 9.0 and 0 < (oc > 0).mean() < 0.6, (nc.mean(), (oc > 0).mean())   # full lists, walls for some agents
    g.close()


def _corner_scene(A, N):
    """Every agent within 1.45 of the corner (0, 0) of the box, at rest.  Arena 1: on an arc around the corner, every agent heading
    straight away from it, so that its ray 8 (straight back) runs through the common end point of the two walls."""
    rng = np.random.RandomState(12)
    pos = rng.uniform(0.2, 1.45, (A, N, 2)).astype(np.float32)
    goal = rng.uniform(2.0, 6.0, (A, N, 2))
    th = np.linspace(0.15, np.pi / 2 - 0.15, N)
    pos[1] = np.stack([1.4 * np.cos(th), 1.4 * np.sin(th)], 1).astype(np.float32)
    goal[1] = pos[1].astype(np.float64) * 3.0
    return dict(pos=pos, vel=np.zeros((A, N, 2), np.float32), goal=goal, goal2=goal.copy())


def test_more_wall_items_than_a_wave_trip_and_rays_through_an_end_point():
    """2 x 16 agents in one corner of an 8 x 8 box, placed by ca_reset: two wall neighbours each, 32 items = 512 (item, ray) lanes
    per workgroup of 256.  Agents of radius 0.05 (obstacle range 1.5 + 0.05), so that no neighbour's octagon stands between an
    agent of arena 1 and the corner: what its ray 8 returns is decided by the two walls' tests at their common end point."""
    A, N = 2, 16
    p = dict(scenarios.bench_params(N, 5.0, 10), radius=0.05)
    g = H.make_gpu(A, N, "crowd", p, seed=5, polys=CS.box_world(N))
    e = H.make_oracle(A, N, "crowd", p, seed=5, polys=CS.box_world(N))
    assert g.launch_info()["obs_grid"] == A
    sc = _corner_scene(A, N)
    g.reset(sc["pos"][..., 0], sc["pos"][..., 1], with_obs=False); e.reset(sc["pos"][..., 0], sc["pos"][..., 1], flags=0)
    CS.set_state(g, _lib, sc); CS.set_state(e, o, sc)
    for s in range(5):
        g.orca_step(with_obs=True, stats=True); e.orca_step(flags=FLAGS)
        H.assert_state_equal(g, e, "corner step %d" % s, obs=True)
        assert (e.get(o.FLD_OBST_COUNT) == 2).all(), e.get(o.FLD_OBST_COUNT)
        if s == 0:   # (a step moves an agent by at most 1 / 60)
            back = e.get(o.FLD_OBS).reshape(A, N, 16, 4)[1, :, 8, :2]
            d = np.hypot(back[:, 0], back[:, 1])                 # the corner 1.4 away, or nothing: the ray slips between the walls
            assert ((np.abs(d - 1.4) < 0.05) | (d == 0)).all() and 0 < (d == 0).sum() < N, d
    g.close()


def test_wide_lists_hundreds_of_items_per_workgroup():
    """Pillar hall A at capacity 64: up to 34 edges per agent, so several hundred items in a workgroup's list."""
    A, N = 2, 64
    g, e = W.make_pair(A, N, W.hall_a_worlds(A), 64)
    es = W.oracle_step(e)

    def both(act):
        if act is None:
            g.orca_step(with_obs=True, stats=True)
        else:
            g.step(act, stats=True)
        es(act)
    W.alternate(both, A, N, 6, every=1, check=lambda s: H.assert_state_equal(g, e, "hall A step %d" % s, obs=True))
    oc = e.get(o.FLD_OBST_COUNT)[0]
    assert oc.max() > 16 and oc.reshape(4, 16).sum(axis=1).max() > 200, (oc.max(), oc.reshape(4, 16).sum(axis=1))
    g.close()


@pytest.mark.parametrize("A,N,K", [(7, 5, 10), (3, 17, 10), (2, 50, 10), (2, 40, 16), (2, 64, 5)],
                         ids=["5 agents: nn < K, 16 agents of several arenas per workgroup", "17 agents: a workgroup of one agent",
                              "50 agents: a workgroup of two", "K = 16: windows on all 256 lanes", "K = 5"])
def test_lists_that_are_not_full_and_partial_workgroups(A, N, K):
    g, e = _crowd_pair(A, N, K)
    assert g.launch_info()["obs_grid"] == (-(-A * N // 16) if N < 16 else A * -(-N // 16))
    _full_steps(g, e, A, N, 8, "%d agents, K = %d" % (N, K), lo=-1.0, hi=1.0)
    nc = e.get(o.FLD_NB_COUNT)
    assert nc.max() == min(K, N - 1) and (N > K or nc.max() < K), nc.max()
    g.close()


def test_one_arena_of_300_agents_gathers_its_neighbours():
    """16-bit neighbour ids; the window lanes read another agent's position from global memory"""
    A, N = 1, 300
    g, e = _crowd_pair(A, N, 10)
    assert g.launch_info()["obs_grid"] == 19
    _full_steps(g, e, A, N, 5, "300 agents")
    g.close()


class _Arena(object):
    """Rows [:n] of arena a of a GPU env, as an env of one arena (what helpers.assert_state_equal reads of it); every field is
    fetched once per comparison."""

    def __init__(self, cache, g, a, n):
        self.cache, self.g, self.a, self.n = cache, g, a, n

    def _cut(self, v):
        return v[self.a:self.a + 1] if v.ndim == 1 else v[self.a:self.a + 1, :self.n]

    def _once(self, key, fn):
        if key not in self.cache:
            self.cache[key] = fn()
        return self.cache[key]

    def get(self, f):
        return self._cut(self._once(f, lambda: self.g.get(f)))

    def neighbor_lists(self):
        c, i = self._once("nb", self.g.neighbor_lists)
        return self._cut(c), self._cut(i)

    def obstacle_neighbor_lists(self):
        c, i = self._once("ob", self.g.obstacle_neighbor_lists)
        return self._cut(c), self._cut(i)


def _same_per_arena(g, rag, what):
    cache = {}
    for a, (n, e) in enumerate(zip(rag.counts, rag.orc)):
        H.assert_state_equal(_Arena(cache, g, a, int(n)), e, "%s arena %d" % (what, a), obs=True)
    absent = ~rag.agent_mask()
    assert not cache[_lib.FLD_OBS][absent].any(), what + ": observation of an absent row"


def _ragged_pair(A, N, counts, seed, radii):
    """A walled box of N-agent arenas, bench_params(N, 5, 10): a radius per arena (ca_set_agent_params) and / or a crowd size per
    arena (ca_set_agent_counts; the absent rows hold copies of the arena's agent 0), and an oracle per arena."""
    p, polys = scenarios.bench_params(N, 5.0, 10), CS.box_world(N)
    sc = CS.draw(A, N, 0.5, scenarios.crowd_envsize(N) - 0.5, seed)
    consts = dict(radius=sc["consts"]["radius"]) if radii else None
    g = H.make_gpu(A, N, None, p, seed=seed, polys=polys)
    if counts is not None:
        g.set_agent_counts(np.asarray(counts, np.int32))
    if radii:
        g.set_agent_params(**consts)
    counts = (N,) * A if counts is None else counts
    CS.set_state(g, _lib, CS.with_decoys(sc, counts))
    rag = CS.RaggedOracleVec(N, counts, p, polys, seed, S_cap=g.S, consts=consts)
    rag.set_scene(sc)
    return g, rag


def _ragged_steps(g, rag, A, N, steps, what):
    rng = np.random.RandomState(6)
    for s in range(steps):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        g.step(act, stats=True); rag.step(act, stats=True)
        _same_per_arena(g, rag, "%s step %d" % (what, s))


@pytest.mark.parametrize("A,N", [(5, 12), (2, 40)], ids=["16 agents of two arenas per workgroup", "40 agents"])
def test_mixed_radii(A, N):
    """An agent is seen as the octagon of ITS radius: the window lane copies the vertices for another agent's group."""
    g, rag = _ragged_pair(A, N, None, 41, radii=True)
    li = g.launch_info()
    assert li["agent_params"] and not li["agent_counts"], li
    _ragged_steps(g, rag, A, N, 6, "radii %d" % N)
    g.close()


@pytest.mark.parametrize("N,counts", [(16, (16, 1, 9, 16, 5, 12, 3, 16)), (12, (12, 3, 7, 1, 12)), (40, (40, 17))],
                         ids=["16 agents", "12 agents: several arenas per workgroup", "40 agents"])
def test_agent_counts_below_n_agents(N, counts):
    """An absent row has no windows and no wall items, and still gets its row of zeros."""
    A = len(counts)
    g, rag = _ragged_pair(A, N, counts, 43, radii=False)
    assert g.launch_info()["agent_counts"]
    _ragged_steps(g, rag, A, N, 6, "counts %d" % N)
    g.close()


def test_observation_after_reset_on_the_previous_steps_lists():
    """ca_reset moves the agents and observes them with the neighbour lists of the last step."""
    A, N = 3, 33
    g, e = _crowd_pair(A, N, 10, seed=9)
    _full_steps(g, e, A, N, 3, "before the reset")
    g.reset(with_obs=True); e.reset(flags=o.F_OBS)
    H.assert_state_equal(g, e, "after the reset", obs=True)
    _full_steps(g, e, A, N, 2, "after the reset")
    g.close()
