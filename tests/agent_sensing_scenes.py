"""Seeded scenes with neighbor_dist and max_neighbors per agent, shared by tests/test_agent_sensing_cpu.py (the oracle's simulator
against a numpy restatement) and tests/test_gpu_agent_sensing.py (the HIP environment with ca_set_agent_sensing against both).

The recipe sits on top of tests/agent_param_scenes.py (16 seeds x 12 agents x 40 ORCA steps, handle values: range 5, 10 neighbours):
for seed s, with rng = RandomState(1000 + s): nd = rng.uniform(1, 5, n) as fp32, K = rng.randint(0, 11, n); then nd[0] = 5, K[0] = 10
(agent 0 carries the handle's values) and K[1] = 0 (an agent that attends to nobody).  The reference hands both values to every
addAgent call (collision_avoidence_env.py:126-133); here they differ by agent.  No tests in here."""
import numpy as np

from oracle import oracle as o
from oracle import rvo2_shim
from tests import agent_param_scenes as S

F = np.float32
SEEDS, N_AGENTS, STEPS = S.SEEDS, S.N_AGENTS, S.STEPS
NEIGHBOR_DIST, MAX_NEIGHBORS = S.NEIGHBOR_DIST, S.MAX_NEIGHBORS      # the handle's values: the capacities


def sensing(seed, n=N_AGENTS):
    """(neighbor_dist [n] f32, max_neighbors [n] i32) of the recipe."""
    rng = np.random.RandomState(1000 + seed)
    nd = rng.uniform(1, 5, n).astype(F)
    K = rng.randint(0, 11, n).astype(np.int32)
    nd[0], K[0] = NEIGHBOR_DIST, MAX_NEIGHBORS
    if n > 1:
        K[1] = 0
    return nd, K


def with_sensing(sc, seed):
    """the scene of agent_param_scenes with the recipe's two arrays added"""
    sc = dict(sc)
    sc["neighbor_dist"], sc["max_neighbors"] = sensing(seed, len(sc["pos"]))
    return sc


def draw(seed):
    return with_sensing(S.draw(seed), seed)


class Sim(S.Sim):
    """agent_param_scenes.Sim whose agents are added with their own neighborDist and maxNeighbors as well (uniform=True: the four
    ORCA parameters are the handle's constants for every agent, the two sensing values stay the agents' own)."""

    def __init__(self, sc, world=None, uniform=False):
        self.sc, self.n = sc, len(sc["pos"])
        d = S.DEFAULTS
        self.sim = rvo2_shim.PyRVOSimulator(S.DT, NEIGHBOR_DIST, MAX_NEIGHBORS, d["time_horizon"], d["time_horizon_obst"], d["radius"],
                                            d["max_speed"])
        for i in range(self.n):
            prm = [float(d[k]) if uniform else float(sc[k][i]) for k in ("time_horizon", "time_horizon_obst", "radius", "max_speed")]
            self.sim.addAgent((float(sc["pos"][i, 0]), float(sc["pos"][i, 1])), float(sc["neighbor_dist"][i]), int(sc["max_neighbors"][i]),
                              prm[0], prm[1], prm[2], prm[3], (float(sc["vel"][i, 0]), float(sc["vel"][i, 1])))
        for poly in (world if world is not None else sc.get("world", S.WORLD)):
            self.sim.addObstacle(poly)
        self.sim.processObstacles()

    def radii(self, uniform):
        return np.full(self.n, S.DEFAULTS["radius"], F) if uniform else self.sc["radius"].astype(F)


def dsq_table(pos):
    """[n,n] f32: fl(fl(dx^2) + fl(dy^2)) with dx = fl(x_i - x_j), as App. A.2 computes it (no fused multiply-add)."""
    pos = np.asarray(pos, F)
    dx, dy = pos[:, None, 0] - pos[None, :, 0], pos[:, None, 1] - pos[None, :, 1]
    d = dx * dx + dy * dy
    assert d.dtype == F
    return d


def ref_lists(pos, nd, K, cap=MAX_NEIGHBORS):
    """The rule in plain numpy fp32: agent i's list is the K_i smallest (dsq, j) keys among j != i with dsq < fl(nd_i * nd_i) (one
    fp32 product), nearest first, ties to the lower index.  Returns (count [n], idx [n, cap] padded with -1) and, for the guards,
    in_range [n]: how many candidates pass agent i's range test."""
    nd, K = np.asarray(nd, F), np.asarray(K)
    n = len(nd)
    d = dsq_table(pos)
    r2 = nd * nd
    assert r2.dtype == F
    cols = np.arange(n)
    cnt, idx, in_range = np.zeros(n, np.int32), np.full((n, cap), -1, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        js = cols[(d[i] < r2[i]) & (cols != i)]
        in_range[i] = js.size
        order = np.lexsort((js, d[i, js]))[:int(K[i])]
        cnt[i] = order.size
        idx[i, :order.size] = js[order]
    return cnt, idx, in_range


def box(side):
    return [[(0.0, 0.0), (0.0, side), (side, side), (side, 0.0)]]


def crowd(seed, n, side):
    """n agents of the agent_param_scenes ranges in a side x side box, with the recipe's sensing arrays"""
    sc = with_sensing(S.draw(seed, n, 0.5, side - 0.5), seed)
    sc["world"] = box(side)
    return sc


# ---- the range and tie boundary --------------------------------------------------------------------------------------------
BOUNDARY_ND, BOUNDARY_OFFSETS = 3.0, (-2, -1, 0, 1)     # an nd_i that is not the handle's; ulps of dsq from fl(nd_i^2)
TIE_AT, TIE_K, TIE_ND = (20.0, 0.0), 3, 4.0


def _at_ulps(target):
    """(dx, dy) f32 with fl(fl(dx^2) + fl(dy^2)) == target exactly: dy near 1, dx searched over the floats around sqrt(target - 1)"""
    from tests import nbr_scenes as NB
    for my in range(0, 64):
        dy = NB.ulps(F(1.0), my)
        x0 = F(np.sqrt(np.float64(target) - np.float64(dy) ** 2))
        for mx in range(-64, 65):
            dx = NB.ulps(x0, mx)
            if F(F(dx * dx) + F(dy * dy)) == target:
                return F(dx), F(dy)
    raise AssertionError("no pair of floats gives dsq = %r" % target)


def boundary_scene(n):
    """One arena of n agents, agents at rest, no walls in reach:
      agent 0 at the origin with nd_0 = 3 (handle: 5), K_0 = 10, and agents 1 .. 4 whose dsq to it lies -2, -1, 0, +1 ulps from
        fl(nd_0^2) = 9 (the first two are its neighbours, the others not); their own range is the handle's, so they all hold agent 0:
        the lists are asymmetric;
      agent 5 at (20, 0) with K_5 = 3, nd_5 = 4: two nearer neighbours at distance 1 (agents 6, 7) and four more at dsq = 4 exactly,
        one per side, whose indices 11, 9, 10, 8 run against the order of any scan: slot 3 goes to index 8;
      the rest: background agents 10 apart, far away (nobody's neighbour), with small ranges and list lengths of their own.
    Returns the scene dict (pos, vel, goal, neighbor_dist, max_neighbors, world)."""
    from tests import nbr_scenes as NB
    assert n >= 13
    pos = np.zeros((n, 2), F)
    nd, K = np.full(n, NEIGHBOR_DIST, F), np.full(n, MAX_NEIGHBORS, np.int32)
    nd[0] = BOUNDARY_ND
    r2 = F(F(BOUNDARY_ND) * F(BOUNDARY_ND))
    for k, off in enumerate(BOUNDARY_OFFSETS):
        dx, dy = _at_ulps(NB.ulps(r2, off))
        pos[1 + k] = ((dx, dy), (-dx, -dy), (dy, dx), (-dy, -dx))[k]     # (four different places: the sum of the squares commutes)
    t = np.asarray(TIE_AT, F)
    pos[5], nd[5], K[5] = t, TIE_ND, TIE_K
    pos[6], pos[7] = t + F([1, 0]), t - F([1, 0])
    for j, d in zip((11, 9, 10, 8), ([2, 0], [0, 2], [-2, 0], [0, -2])):
        pos[j] = t + F(d)
    for j in range(12, n):
        pos[j] = (500.0 + 10.0 * ((j - 12) % 16), 500.0 + 10.0 * ((j - 12) // 16))
        nd[j], K[j] = 1.0 + (j % 5), j % 11
    return dict(pos=pos, vel=np.zeros((n, 2), F), goal=pos.astype(np.float64), neighbor_dist=nd, max_neighbors=K,
                world=[[(-50.0, -50.0), (-50.0, 700.0), (700.0, 700.0), (700.0, -50.0)]])


# ---- the tiled crowd with the three cases the pair count's list shortcut must refuse ------------------------------------------------
def tiled_scene(seed=41, n=150, side=15.0):
    """n agents in a side x side box around a block (tests/tiled_param_scenes.world), the recipe's ranges, plus
      a clump: agents 20 .. 33 (14 > K = 10) packed within 0.6 of agent 20, which has K_20 = 2 (a full list that proves nothing);
      agent 40 with K_40 = 0 on top of agent 41 (an overlap the empty list cannot show);
      agent 50 with nd_50 = 0.5 < 2 r_max next to agent 51, 0.7 away: overlapping at these radii, out of its range."""
    from tests import tiled_param_scenes as T
    sc = with_sensing(T.scene(seed, n, side), seed)
    rng = np.random.RandomState(seed + 1)
    c = np.asarray([3.0, 11.0], F)
    sc["pos"][20] = c
    sc["pos"][21:34] = c + rng.uniform(-0.4, 0.4, (13, 2)).astype(F)
    sc["max_neighbors"][20] = 2
    sc["pos"][40], sc["pos"][41] = F([11.0, 3.0]), F([11.0, 3.25])
    sc["max_neighbors"][40] = 0
    sc["pos"][50], sc["pos"][51] = F([12.0, 12.0]), F([12.7, 12.0])
    sc["neighbor_dist"][50] = 0.5
    sc["radius"][50], sc["radius"][51] = 0.6, 0.6
    sc["vel"][20:34] = 0
    sc["vel"][40:42] = 0
    sc["vel"][50:52] = 0
    return sc


# ---- constants per arena ---------------------------------------------------------------------------------------------------------
def arena_constants(A, seed, nd_cap=NEIGHBOR_DIST, k_cap=MAX_NEIGHBORS):
    """(neighbor_dist [A] f32 in [0.3 cap, cap], max_neighbors [A] i32 in 0 .. cap); arena 0 carries the capacities, arena 1 K = 0"""
    rng = np.random.RandomState(seed)
    nd = rng.uniform(0.3 * nd_cap, nd_cap, A).astype(F)
    K = rng.randint(0, k_cap + 1, A).astype(np.int32)
    nd[0], K[0] = nd_cap, k_cap
    if A > 1:
        K[1] = 0
    return nd, K


class ArenaOracles(object):
    """One OracleEnv per arena (n_arenas = 1, arena_offset = a, n_agents = counts[a]) whose ca_config carries that arena's
    neighbor_dist and max_neighbors: the shape tests/agent_count_scenes.same compares a handle with (.counts, .orc, .agent_steps())."""

    def __init__(self, N, counts, params, polys, seed, nd, K, S_cap):
        self.N, self.counts, self.orc = N, np.asarray(counts, np.int32), []
        for a, n in enumerate(counts):
            pa = dict(params, neighbor_dist=float(nd[a]), max_neighbors=int(K[a]))
            e = o.OracleEnv(o.make_config(n_arenas=1, n_agents=int(n), seed=seed, arena_offset=a, max_obst_neighbors=S_cap, **pa))
            e.set_obstacles(polys)
            self.orc.append(e)

    def agent_steps(self):
        return sum(e.stats()["agent_steps"] for e in self.orc)
