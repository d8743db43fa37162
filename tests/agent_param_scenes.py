"""Seeded scenes with ORCA parameters per agent, shared by tests/test_agent_params_cpu.py (the oracle's simulator alone) and
tests/test_gpu_agent_params.py (the HIP environment against it).

The recipe: for seed s = 100 .. 115, 12 agents with positions and goals uniform in [0.5, 5.5]^2, velocity components uniform
in [-0.5, 0.5], radius in [0.2, 0.8], max_speed in [0.5, 1.5], time_horizon and time_horizon_obst in [0.5, 3] (all fp32; the
goals stay fp64 like the reference's target tuples), neighbor_dist 5, max_neighbors 10, at most 16 obstacle neighbours,
time step 1/60, in the box (0,0),(0,6),(6,6),(6,0) around the block (2.5,2.5) .. (3.5,3.5); 40 ORCA steps, the preferred
velocity being the fp32-rounded pref_dir64 of the current position before every step.  The reference hands all of these to
every addAgent call (collision_avoidence_env.py:126-133); here they differ by agent."""
import numpy as np

from oracle import oracle as o
from oracle import rvo2_shim

SEEDS = tuple(range(100, 116))
N_AGENTS = 12
STEPS = 40
DT = 1 / 60.
NEIGHBOR_DIST, MAX_NEIGHBORS, MAX_OBST_NEIGHBORS = 5.0, 10, 16
DEFAULTS = dict(radius=0.5, max_speed=1.0, time_horizon=1.5, time_horizon_obst=1.5)   # the handle's constants
WORLD = [[(0.0, 0.0), (0.0, 6.0), (6.0, 6.0), (6.0, 0.0)], [(2.5, 2.5), (3.5, 2.5), (3.5, 3.5), (2.5, 3.5)]]
PARAM_NAMES = ("radius", "max_speed", "time_horizon", "time_horizon_obst")
RANGES = dict(radius=(0.2, 0.8), max_speed=(0.5, 1.5), time_horizon=(0.5, 3.0), time_horizon_obst=(0.5, 3.0))


def draw(seed, n=N_AGENTS, lo=0.5, hi=5.5):
    """One scene: dict of pos [n,2] f32, vel [n,2] f32, goal [n,2] f64 and the four parameter arrays [n] f32."""
    rng = np.random.RandomState(seed)
    sc = dict(pos=rng.uniform(lo, hi, (n, 2)).astype(np.float32), goal=rng.uniform(lo, hi, (n, 2)),
              vel=rng.uniform(-0.5, 0.5, (n, 2)).astype(np.float32))
    for name in PARAM_NAMES:
        sc[name] = rng.uniform(RANGES[name][0], RANGES[name][1], n).astype(np.float32)
    return sc


def big_scene(seed=7, n=200, side=20.0):
    """One arena of 200 agents in a side x side box, the same parameter ranges (the 256-lane workgroup and the grid scan)."""
    sc = draw(seed, n, 0.5, side - 0.5)
    sc["world"] = [[(0.0, 0.0), (0.0, side), (side, side), (side, 0.0)]]
    return sc


def pref_of(pos, goal):
    """[n,2] f32: the fp32-rounded pref_dir64 of every agent (env.py:151-154)."""
    return np.asarray([o.pref_dir64(float(pos[i, 0]), float(pos[i, 1]), float(goal[i, 0]), float(goal[i, 1]))
                       for i in range(len(pos))], np.float64).astype(np.float32)


class Sim(object):
    """A scene on the oracle's PyRVOSimulator shim: every agent added with its own parameters, as the reference adds its own."""

    def __init__(self, sc, world=None, uniform=False):
        self.sc, self.n = sc, len(sc["pos"])
        d = DEFAULTS
        self.sim = rvo2_shim.PyRVOSimulator(DT, NEIGHBOR_DIST, MAX_NEIGHBORS, d["time_horizon"], d["time_horizon_obst"],
                                            d["radius"], d["max_speed"])
        for i in range(self.n):
            prm = [float(d[k]) if uniform else float(sc[k][i]) for k in ("time_horizon", "time_horizon_obst", "radius", "max_speed")]
            self.sim.addAgent((float(sc["pos"][i, 0]), float(sc["pos"][i, 1])), NEIGHBOR_DIST, MAX_NEIGHBORS, prm[0], prm[1], prm[2],
                              prm[3], (float(sc["vel"][i, 0]), float(sc["vel"][i, 1])))
        for poly in (world if world is not None else sc.get("world", WORLD)):
            self.sim.addObstacle(poly)
        self.sim.processObstacles()

    def positions(self):
        return np.asarray([self.sim.getAgentPosition(i) for i in range(self.n)], np.float32)

    def velocities(self):
        return np.asarray([self.sim.getAgentVelocity(i) for i in range(self.n)], np.float32)

    def step(self):
        """update_pref_vel (env.py:151-154) + doStep (env.py:447-450)."""
        pref = pref_of(self.positions(), self.sc["goal"])
        for i in range(self.n):
            self.sim.setAgentPrefVelocity(i, (float(pref[i, 0]), float(pref[i, 1])))
        self.sim.doStep()

    def agent_neighbors(self):
        """(count [n], idx [n, K] padded with -1), nearest first."""
        s, cnt, idx = self.sim, np.zeros(self.n, np.int32), np.full((self.n, MAX_NEIGHBORS), -1, np.int32)
        for i in range(self.n):
            cnt[i] = s.getAgentNumAgentNeighbors(i)
            for k in range(cnt[i]):
                idx[i, k] = s.getAgentAgentNeighbor(i, k)
        return cnt, idx

    def obstacle_neighbors(self, cap=64):
        s, cnt, idx = self.sim, np.zeros(self.n, np.int32), np.full((self.n, cap), -1, np.int32)
        for i in range(self.n):
            cnt[i] = s.getAgentNumObstacleNeighbors(i)
            for k in range(min(cnt[i], cap)):
                idx[i, k] = s.getAgentObstacleNeighbor(i, k)
        return cnt, idx

    def obstacle_edges(self):
        """[n_vertices, 4] f32: edge v = vertex v -> its next vertex (env.py:307-311)."""
        s = self.sim
        return np.asarray([s.getObstacleVertex(v) + s.getObstacleVertex(s.getNextObstacleVertexNo(v))
                           for v in range(s.getNumObstacleVertices())], np.float32)


def observation_segments(pos, vel, radius, i, nb, ob, edges, dtype):
    """The segment list of agent i as the oracle's agent_obs builds it (env.py:283-294, 305-315): for every agent neighbour the 8
    chords of the octagon of ITS radius -- octagon_table((double)r_nb), rounded to `dtype` -- moved by the relative position
    taken in `dtype`, with the neighbour's velocity; then the edges of the obstacle neighbours relative to the agent."""
    segs = []
    me = pos[i].astype(dtype)
    for j in nb:
        octa = o.octagon_table(float(np.float32(radius[j]))).astype(dtype)
        rel = pos[j].astype(dtype) - me
        for e in range(8):
            segs.append([octa[e, 0] + rel[0], octa[e, 1] + rel[1], octa[e, 2] + rel[0], octa[e, 3] + rel[1],
                         dtype(vel[j, 0]), dtype(vel[j, 1])])
    for v in ob:
        e = edges[v].astype(dtype)
        segs.append([e[0] - me[0], e[1] - me[1], e[2] - me[0], e[3] - me[1], dtype(0), dtype(0)])
    return np.asarray(segs, dtype).reshape(-1, 6)


def laser(pos, goal, segs, i, dtype):
    """[16,4]: comp_laser on agent i's segments with the 5.0 ray table, oriented by pref_dir64 (env.py:236)."""
    if len(segs) == 0:
        return np.zeros((16, 4), dtype)                                   # env.py:267
    ori = o.pref_dir64(float(pos[i, 0]), float(pos[i, 1]), float(goal[i, 0]), float(goal[i, 1]))
    return o.comp_laser(o.ray_table(NEIGHBOR_DIST), segs, ori, dtype)


OBS_TOL = 3e-5        # the project's absolute tolerance for an fp32 observation
OBS_MAX_LEFT_OUT = 0.01


def excusable_rays(f32, f64):
    """[16] bool: rays where f32 and f64 comp_laser on the SAME segments themselves differ by more than OBS_TOL (a hit that
    flips under rounding): the only rays a comparison may leave out."""
    return np.abs(f32.astype(np.float64) - f64).max(axis=1) > OBS_TOL


def rays_on_agents(pos, goal, segs, n_agent_segs, i, dtype=np.float32):
    """[16] bool: rays of agent i that end on an agent neighbour's octagon -- whose answer changes when the octagons' chords (the
    first n_agent_segs segments) are taken away."""
    full = laser(pos, goal, segs, i, dtype)
    rest = laser(pos, goal, segs[n_agent_segs:], i, dtype)
    return (full != rest).any(axis=1)
