"""ORCA parameters per agent on the GPU (ca_set_agent_params): radius, max_speed, time_horizon and time_horizon_obst as the
reference hands them to every addAgent call (collision_avoidence_env.py:126-133).  The CPU oracle carries them per agent at its
core, so everything here is held bit for bit: arenas with constants of their own against an oracle environment configured with
them, mixed agents against the oracle's PyRVOSimulator (tests/agent_param_scenes.py, whose inputs tests/test_agent_params_cpu.py
checks on the oracle alone).  Every test asserts launch_info(), so that it cannot pass on another kernel."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib, alan, scenarios
from oracle import oracle as o
from tests import agent_param_scenes as S
from tests import helpers as H

pytestmark = pytest.mark.gpu

FLAGS = o.F_OBS | o.F_STATS
_STATE = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "AGENT_DONE", "STEP_COUNT", "ARENA_DONE", "EPISODE",
          "REGOAL_COUNT")


def _is_agent_params(g):
    """launch_info() of a handle with per-agent parameters: the one-lane LDS-line-table kernel of its own (a table of K + S lines, the
    staged arena, the misc ints and the staged radii per lane: no other kernel is launched with that size), T launches per rollout."""
    li = g.launch_info()
    assert li["agent_params"] is True and li["lanes_per_agent"] == 1 and li["rollout_one_launch"] == 0, li
    assert li["lds_bytes"] == li["block"] * ((g.K + g.S) * 16 + 36), (li, g.K, g.S)
    return li


def _set_state(e, fld, pos, vel, goal, goal2=None):
    """positions, velocities, targets and the preferred velocity towards the target, [A,N,2] each, on a GPU or an oracle env"""
    A, N = pos.shape[:2]
    pref = np.stack([S.pref_of(pos[a], goal[a]) for a in range(A)])
    goal2 = goal if goal2 is None else goal2
    for name, v in (("POS_X", pos[..., 0]), ("POS_Y", pos[..., 1]), ("VEL_X", vel[..., 0]), ("VEL_Y", vel[..., 1]),
                    ("PREF_X", pref[..., 0]), ("PREF_Y", pref[..., 1]), ("GOAL_X", goal[..., 0]), ("GOAL_Y", goal[..., 1]),
                    ("GOAL2_X", goal2[..., 0]), ("GOAL2_Y", goal2[..., 1])):
        e.set(getattr(fld, "FLD_" + name), np.ascontiguousarray(v))


# ---- 1. constants per arena: an oracle environment per arena, configured with that arena's values ----------------------------
class _PerArena(object):
    """A GPU handle created with the defaults (0.5, 1, 1.5, 1.5) whose arena a gets seeded constants through set_agent_params, and
    one OracleEnv per arena (n_arenas = 1, arena_offset = a) whose ca_config carries them."""

    def __init__(self, A, N, params, polys, lo, hi, seed, goal2=None, S_cap=None):
        rng = np.random.RandomState(seed)
        self.A, self.N = A, N
        self.consts = dict(radius=rng.uniform(0.3, 0.7, A).astype(np.float32), max_speed=rng.uniform(0.6, 1.4, A).astype(np.float32),
                           time_horizon=rng.uniform(0.75, 3.0, A).astype(np.float32),
                           time_horizon_obst=rng.uniform(0.75, 3.0, A).astype(np.float32))
        pos = rng.uniform(lo, hi, (A, N, 2)).astype(np.float32)
        vel = rng.uniform(-0.5, 0.5, (A, N, 2)).astype(np.float32)
        goal = rng.uniform(lo, hi, (A, N, 2)) if goal2 is None else np.broadcast_to(np.asarray(goal2[0], np.float64), (A, N, 2)).copy()
        g2 = None if goal2 is None else np.broadcast_to(np.asarray(goal2[1], np.float64), (A, N, 2)).copy()
        p = dict(params, **S.DEFAULTS)
        self.g = H.make_gpu(A, N, None, p, seed=seed, polys=polys, max_obst_neighbors=S_cap)
        self.g.set_agent_params(**self.consts)                       # an [A] array: one value per arena
        _set_state(self.g, _lib, pos, vel, goal, g2)
        self.orc = []
        for a in range(A):
            pa = dict(params, **{k: float(v[a]) for k, v in self.consts.items()})
            e = o.OracleEnv(o.make_config(n_arenas=1, n_agents=N, seed=seed, arena_offset=a, max_obst_neighbors=self.g.S, **pa))
            e.set_obstacles(polys)
            _set_state(e, o, pos[a:a + 1], vel[a:a + 1], goal[a:a + 1], None if g2 is None else g2[a:a + 1])
            self.orc.append(e)

    def same(self, what, obs=True, reward=True):
        g = self.g
        got = {n: g.get(getattr(_lib, "FLD_" + n)) for n in _STATE}
        (nc, ni), (oc, oi) = g.neighbor_lists(), g.obstacle_neighbor_lists()
        gobs, grew, gst = g.get(_lib.FLD_OBS), g.get(_lib.FLD_REWARD), g.arena_stats()
        for a, e in enumerate(self.orc):
            w = "%s arena %d" % (what, a)
            for n in _STATE:
                H._eq(got[n][a:a + 1], e.get(getattr(o, "FLD_" + n)), w + " " + n)
            for cnt, idx, fc, fi in ((nc, ni, o.FLD_NB_COUNT, o.FLD_NB_IDX), (oc, oi, o.FLD_OBST_COUNT, o.FLD_OBST_IDX)):
                ec, ei = e.get(fc), e.get(fi)
                H._eq(cnt[a:a + 1], ec, w + " list count")
                mask = np.arange(ei.shape[2])[None, None, :] < ec[:, :, None]
                H._eq(np.where(mask, idx[a:a + 1, :, :ei.shape[2]], -1), np.where(mask, ei, -1), w + " list")
            if obs:
                H._eq(gobs[a:a + 1], e.get(o.FLD_OBS), w + " obs")
            if reward:
                H._eq(grew[a:a + 1], e.get(o.FLD_REWARD), w + " reward")
            s = e.stats()
            for k in ("episodes", "collisions", "obst_collisions", "goals_reached", "obst_overflow"):
                assert int(gst[k][a]) == s[k], (w, k, int(gst[k][a]), s[k])
            assert abs(gst["sum_reward"][a] - s["sum_reward"]) <= 1e-9 * max(1.0, abs(s["sum_reward"])), (w, gst["sum_reward"][a], s["sum_reward"])


def _box(e):
    return [[(0.0, 0.0), (0.0, e), (e, e), (e, 0.0)]]


def test_constants_per_arena_doorway_with_autoreset():
    """6 x 12 in the reference env's own world, CA_DONE_XLESS, max_step 50, CA_F_AUTORESET, 120 steps: the parameters survive the
    resets (three episodes per arena)."""
    A, N = 6, 12
    p = dict(scenarios.env_params(), max_step=50)
    t = _PerArena(A, N, p, scenarios.obstacles("doorway", N), (5.0, 0.5), (9.5, 9.5), seed=31, goal2=((1.0, 5.0), (-10.0, 5.0)), S_cap=16)
    _is_agent_params(t.g)
    rng = np.random.RandomState(5)
    for s in range(120):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        t.g.step(act, stats=True, autoreset=True)
        for a, e in enumerate(t.orc):
            e.step(act[a:a + 1], flags=FLAGS | o.F_AUTORESET)
        if s % 20 == 19 or s in (49, 50):
            t.same("doorway step %d" % s)
    _is_agent_params(t.g)
    assert t.g.stats()["episodes"] >= 2 * A and t.g.stats()["obst_overflow"] == 0
    t.g.close()


@pytest.mark.parametrize("A,N,steps", [(3, 70, 40), (2, 200, 10)], ids=["two waves", "256 lanes, grid scan"])
def test_constants_per_arena_walled_box_with_regoal(A, N, steps):
    p = scenarios.bench_params(N, 5.0, 10)
    e = scenarios.crowd_envsize(N)
    t = _PerArena(A, N, p, _box(e), 0.5, e - 0.5, seed=32)
    li = _is_agent_params(t.g)
    assert li["block"] == (128 if N == 70 else 256)
    rng = np.random.RandomState(6)
    for s in range(steps):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        t.g.step(act, stats=True)
        for a, en in enumerate(t.orc):
            en.step(act[a:a + 1], flags=FLAGS)
        if s % 10 == 9:
            t.same("box %d step %d" % (N, s))
    assert t.g.stats()["collisions"] > 0
    t.g.close()


def test_constants_per_arena_under_alan_step():
    """4 x 12, ca_alan_step with given uniforms, 30 steps: select -> solve (the per-agent kernel) -> update."""
    A, N = 4, 12
    p = scenarios.alan_params(N, "crowd")
    e = scenarios.crowd_envsize(N)
    t = _PerArena(A, N, p, _box(e), 0.5, e - 0.5, seed=33)
    t.g.alan_configure(alan.DEFAULT_ACTIONS)
    for en in t.orc:
        en.alan_configure(alan.DEFAULT_ACTIONS)
    _is_agent_params(t.g)
    rng = np.random.RandomState(7)
    for s in range(30):
        u = rng.uniform(0, 1, (A, N))
        t.g.alan_step(u, with_obs=True, stats=True)
        for a, en in enumerate(t.orc):
            en.alan_step(u[a:a + 1], flags=FLAGS)
        if s % 10 == 9:
            t.same("alan step %d" % s)
            act, w, tm = t.g.get(_lib.FLD_ALAN_ACTION), t.g.get(_lib.FLD_ALAN_WEIGHTS), t.g.get(_lib.FLD_ALAN_TIMES)
            for a, en in enumerate(t.orc):
                H._eq(act[a:a + 1], en.get(o.FLD_ALAN_ACTION), "alan action")
                H._eq(w[a:a + 1], en.get(o.FLD_ALAN_WEIGHTS), "alan weights")
                H._eq(tm[a:a + 1], en.get(o.FLD_ALAN_TIMES), "alan times")
    _is_agent_params(t.g)
    t.g.close()


# ---- 2 - 4. mixed agents against the simulator ------------------------------------------------------------------------------
def _mixed_params():
    p = dict(scenarios.env_params(), neighbor_dist=S.NEIGHBOR_DIST, max_neighbors=S.MAX_NEIGHBORS, time_step=S.DT)
    p.update(S.DEFAULTS)
    return p


def _mixed_gpu(scenes, worlds, S_cap=None):
    A, N = len(scenes), len(scenes[0]["pos"])
    g = H.make_gpu(A, N, None, _mixed_params(), polys=dict(per_arena=worlds), max_obst_neighbors=S_cap)
    _set_state(g, _lib, np.stack([sc["pos"] for sc in scenes]), np.stack([sc["vel"] for sc in scenes]), np.stack([sc["goal"] for sc in scenes]))
    g.set_agent_params(**{k: np.stack([sc[k] for sc in scenes]) for k in S.PARAM_NAMES})
    return g


def _pair_count(pos, radius):
    """pairs i < j with fp32 dx*dx + dy*dy < (r_i + r_j) * (r_i + r_j), the kernel's operation order"""
    pos, r = pos.astype(np.float32), radius.astype(np.float32)
    dx, dy = pos[:, None, 0] - pos[None, :, 0], pos[:, None, 1] - pos[None, :, 1]
    cr = r[:, None] + r[None, :]
    hit = (dx * dx + dy * dy) < cr * cr
    return int(np.triu(hit, 1).sum())


def _against_sims(g, sims, steps, what):
    """orca_step(stats, no_done) x steps: after every step positions, velocities and both neighbour lists equal the simulators'
    bit for bit, and the per-arena collision counter grew by the number of overlapping pairs of the positions read back."""
    A = len(sims)
    coll = g.arena_stats()["collisions"].astype(np.int64)
    for s in range(steps):
        g.orca_step(stats=True, no_done=True)
        for sim in sims:
            sim.step()
        px, py, vx, vy = (g.get(f) for f in (_lib.FLD_POS_X, _lib.FLD_POS_Y, _lib.FLD_VEL_X, _lib.FLD_VEL_Y))
        (nc, ni), (oc, oi) = g.neighbor_lists(), g.obstacle_neighbor_lists()
        now = g.arena_stats()["collisions"].astype(np.int64)
        for a, sim in enumerate(sims):
            w = "%s arena %d step %d" % (what, a, s)
            sp, sv = sim.positions(), sim.velocities()
            H._eq(np.stack([px[a], py[a]], 1), sp, w + " position")
            H._eq(np.stack([vx[a], vy[a]], 1), sv, w + " velocity")
            (snc, sni), (soc, soi) = sim.agent_neighbors(), sim.obstacle_neighbors(cap=g.S)
            H._eq(nc[a], snc, w + " agent-neighbour count")
            H._eq(np.where(np.arange(g.K)[None, :] < snc[:, None], ni[a], -1), sni, w + " agent neighbours")
            H._eq(oc[a], soc, w + " obstacle-neighbour count")
            H._eq(np.where(np.arange(g.S)[None, :] < soc[:, None], oi[a], -1), soi, w + " obstacle neighbours")
            assert now[a] - coll[a] == _pair_count(sp, sim.sc["radius"]), (w, now[a] - coll[a], _pair_count(sp, sim.sc["radius"]))
        coll = now
    return coll


@pytest.fixture(scope="module")
def mixed():
    """The 16 recipe scenes as 16 arenas with a world each, advanced 40 ORCA steps next to 16 simulators (checked step by step),
    then observed once: shared by the tests below."""
    scenes = [S.draw(seed) for seed in S.SEEDS]
    g = _mixed_gpu(scenes, [S.WORLD] * len(scenes), S_cap=S.MAX_OBST_NEIGHBORS)
    li = _is_agent_params(g)
    sims = [S.Sim(sc) for sc in scenes]
    coll = _against_sims(g, sims, S.STEPS, "mixed")
    obs = np.array(g.observe()).reshape(len(scenes), S.N_AGENTS, 16, 4)
    _is_agent_params(g)
    out = dict(sims=sims, obs=obs, collisions=coll, li=li, overflow=g.stats()["obst_overflow"])
    g.close()
    return out


def test_mixed_agents_orca_step_equals_the_simulator(mixed):
    assert mixed["li"]["agent_params"] and mixed["li"]["lanes_per_agent"] == 1
    assert mixed["overflow"] == 0 and mixed["collisions"].sum() > 1000      # (the step-by-step comparison ran in the fixture)


def test_mixed_agents_200_in_one_arena():
    """One arena of 200 agents in a 20 x 20 box, the same ranges, 10 steps: the 256-lane workgroup and the grid scan."""
    sc = S.big_scene()
    g = _mixed_gpu([sc], [sc["world"]])
    li = _is_agent_params(g)
    assert li["block"] == 256
    _against_sims(g, [S.Sim(sc)], 10, "200 agents")
    g.close()


def test_mixed_agents_observation(mixed):
    """Neighbour j is seen as the octagon of ITS radius: for every agent the segment list as agent_obs<float> builds it --
    (float)octagon_table(r_nb) plus the fp32 relative position, then the obstacle neighbours' edges -- through the oracle's fp32
    comp_laser.  Equal bits are expected; the requirement is the project's 3e-5 absolute.  A ray is left out only where fp32 and
    fp64 comp_laser on the same segments themselves differ by more than that, at most 1 % of the rays."""
    rays = left_out = on_agent = unequal = 0
    worst = 0.0
    for a, sim in enumerate(mixed["sims"]):
        pos, vel, goal, rad = sim.positions(), sim.velocities(), sim.sc["goal"], sim.sc["radius"]
        (nc, ni), (oc, oi), edges = sim.agent_neighbors(), sim.obstacle_neighbors(), sim.obstacle_edges()
        for i in range(sim.n):
            seg = S.observation_segments(pos, vel, rad, i, ni[i, :nc[i]], oi[i, :oc[i]], edges, np.float32)
            f32 = S.laser(pos, goal, seg, i, np.float32)
            f64 = S.laser(pos, goal, seg.astype(np.float64), i, np.float64)
            skip = S.excusable_rays(f32, f64)
            got = mixed["obs"][a, i]
            err = np.abs(got.astype(np.float64) - f32.astype(np.float64)).max(axis=1)
            rays += 16
            left_out += int(skip.sum())
            unequal += int((got.view(np.uint32) != f32.view(np.uint32)).any(axis=1).sum())
            on_agent += int(S.rays_on_agents(pos, goal, seg, 8 * nc[i], i).sum())
            worst = max(worst, float(err[~skip].max()) if (~skip).any() else 0.0)
            assert (err[~skip] <= S.OBS_TOL).all(), ("arena %d agent %d" % (a, i), err, skip)
    print("rays", rays, "left out", left_out, "not bit-equal", unequal, "largest error", worst, "on an agent's octagon", on_agent)
    assert left_out <= S.OBS_MAX_LEFT_OUT * rays, (left_out, rays)
    assert on_agent >= 1000, on_agent


def _two_arenas(radius, pos, goal, done_mode):
    """two arenas of one agent each in an empty world, the agent at rest"""
    p = dict(_mixed_params(), done_mode=done_mode, max_step=0)
    g = H.make_gpu(2, 1, None, p, polys=_box(10.0))
    z = np.zeros((2, 1, 2), np.float32)
    _set_state(g, _lib, np.asarray(pos, np.float32).reshape(2, 1, 2), z, np.asarray(goal, np.float64).reshape(2, 1, 2))
    g.set_agent_params(radius=np.asarray(radius, np.float32))
    _is_agent_params(g)
    return g


def test_wall_hits_and_arrival_take_the_agents_radius():
    # 0.45 from the wall x = 0, heading along it: counts with r = 0.5 (0.2025 < 0.25), not with r = 0.4 (0.16)
    g = _two_arenas([0.5, 0.4], [(0.45, 5.0), (0.45, 5.0)], [(0.45, 9.0), (0.45, 9.0)], _lib.DONE_GOAL)
    g.orca_step(stats=True, no_done=True)
    x = g.get(_lib.FLD_POS_X)[:, 0]
    assert (x < 0.5).all() and (x > 0.4).all(), x
    assert list(g.arena_stats()["obst_collisions"]) == [1, 0], g.arena_stats()
    g.close()
    # CA_DONE_GOAL, 0.9 from the goal: r = 0.5 arrives (0.9 < 1.0; the step brings it at most 1 / 60 closer), r = 0.3 does not (0.6)
    g = _two_arenas([0.5, 0.3], [(5.0, 5.0), (5.0, 5.0)], [(5.9, 5.0), (5.9, 5.0)], _lib.DONE_GOAL)
    g.orca_step(stats=True)
    assert list(g.get(_lib.FLD_AGENT_DONE)[:, 0]) == [1, 0] and list(g.arena_stats()["goals_reached"]) == [1, 0]
    g.close()


# ---- 5. boundary behaviour ---------------------------------------------------------------------------------------------------
def _crowd(A=3, N=12, seed=11, **kw):
    return H.make_gpu(A, N, "crowd", scenarios.bench_params(N, 5.0, 10), seed=seed, **kw)


def _same_handles(g1, g2, what):
    for n in _STATE + ("REWARD", "OBS", "NB_COUNT", "OBST_COUNT", "NB_IDX", "OBST_IDX", "ARENA_STATS"):
        a, b = g1.get(getattr(_lib, "FLD_" + n)), g2.get(getattr(_lib, "FLD_" + n))
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, n)


def _five_steps(g, seed=3):
    rng = np.random.RandomState(seed)
    for s in range(5):
        g.step(rng.uniform(-1, 1, (g.A, g.N)).astype(np.float32), stats=True)


def _raw_set(g, arrays, nbytes=None):
    L = _lib.load()
    ptrs = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in arrays]
    rc = L.ca_set_agent_params(g.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], g.A * g.N * 4 if nbytes is None else nbytes, 0)
    return rc, (L.ca_last_error(g.h) or b"").decode()


@pytest.mark.parametrize("configured", [False, True], ids=["uniform handle", "handle with parameters"])
def test_refused_values_and_sizes_leave_the_handle_as_it_was(configured):
    g, ref = _crowd(), _crowd()
    rng = np.random.RandomState(2)
    first = {k: rng.uniform(*S.RANGES[k], size=(g.A, g.N)).astype(np.float32) for k in S.PARAM_NAMES}
    if configured:
        g.set_agent_params(**first); ref.set_agent_params(**first)
    before = g.launch_info()
    good = np.full((g.A, g.N), 0.4, np.float32)
    for k, name in enumerate(S.PARAM_NAMES):
        for bad_value in (np.nan, np.inf, 0.0, -1.0, 1e-4, 2e3):
            arrays = [good.copy() for _ in range(4)]
            arrays[k][1, 7] = bad_value
            rc, msg = _raw_set(g, arrays)
            assert rc == -5 and name + "=" in msg and "arena 1, agent 7" in msg, (name, bad_value, rc, msg)
    for nbytes in (g.A * g.N * 4 - 4, g.A * g.N * 8, 0):
        rc, msg = _raw_set(g, [good] * 4, nbytes)
        assert rc == -4, (nbytes, rc, msg)
    assert g.launch_info() == before
    got = g.agent_params()
    for k in S.PARAM_NAMES:
        want = first[k] if configured else np.full((g.A, g.N), getattr(g.cfg, k), np.float32)
        H._eq(got[k], want, "agent_params() " + k)
    _five_steps(g); _five_steps(ref)
    _same_handles(g, ref, "after refused calls")
    g.close(); ref.close()


def test_not_together_with_wide_obstacle_lists():
    g, ref = _crowd(max_obst_neighbors=17), _crowd(max_obst_neighbors=17)
    before = g.launch_info()
    rc, msg = _raw_set(g, [np.full((g.A, g.N), 0.4, np.float32)] * 4)
    assert rc == -1 and "not together with wide obstacle lists" in msg, (rc, msg)
    assert g.launch_info() == before and not before["agent_params"]
    _five_steps(g); _five_steps(ref)
    _same_handles(g, ref, "wide handle")
    g.close(); ref.close()


def test_a_line_table_that_does_not_fit_is_refused():
    """512 agents with max_neighbors 10 and lists of 16: 512 x (26 x 16 + 36) B = 226 KiB of LDS; the uniform handle runs on
    register lines and keeps doing so."""
    g, ref = _crowd(2, 512, max_obst_neighbors=16), _crowd(2, 512, max_obst_neighbors=16)
    before = g.launch_info()
    rc, msg = _raw_set(g, [np.full((g.A, g.N), 0.4, np.float32)] * 4)
    assert rc == -5 and "does not fit" in msg, (rc, msg)
    assert g.launch_info() == before and not before["agent_params"]
    _five_steps(g); _five_steps(ref)
    _same_handles(g, ref, "512 agents")
    g.close(); ref.close()


@pytest.mark.parametrize("A,N,quad,lanes", [(3, 12, "1", 4), (40, 64, "0", 1)], ids=["from four lanes per agent", "from register lines"])
def test_clear_returns_to_the_uniform_kernels(A, N, quad, lanes, monkeypatch):
    monkeypatch.setenv("CA_QUAD", quad)                                # (latched by ca_create; ignored while the parameters are set)
    g, ref = _crowd(A, N), _crowd(A, N)
    before = g.launch_info()
    assert not before["agent_params"] and before["lanes_per_agent"] == lanes, before
    rng = np.random.RandomState(4)
    prm = {k: rng.uniform(*S.RANGES[k], size=(A, N)).astype(np.float32) for k in S.PARAM_NAMES}
    g.set_agent_params(**prm)
    _is_agent_params(g)
    got = g.agent_params()
    for k in S.PARAM_NAMES:
        H._eq(got[k], prm[k], "agent_params() " + k)
    g.set_agent_params(max_speed=0.8)                                  # a scalar; the three others return to the config values
    _is_agent_params(g)
    got = g.agent_params()
    H._eq(got["max_speed"], np.full((A, N), 0.8, np.float32), "scalar")
    H._eq(got["radius"], np.full((A, N), g.cfg.radius, np.float32), "None = the config value")
    g.clear_agent_params()
    assert g.launch_info() == before
    _five_steps(g); _five_steps(ref)
    _same_handles(g, ref, "after clear_agent_params")
    g.close(); ref.close()


def test_arrays_equal_to_the_config_values_give_the_uniform_bits():
    A, N = 5, 30
    g, ref = _crowd(A, N, seed=12), _crowd(A, N, seed=12)
    g.set_agent_params(**{k: np.full((A, N), getattr(g.cfg, k), np.float32) for k in S.PARAM_NAMES})
    _is_agent_params(g)
    assert not ref.launch_info()["agent_params"]
    for r in range(4):
        _five_steps(g, seed=r); _five_steps(ref, seed=r)
        _same_handles(g, ref, "config values, round %d" % r)
    g.rollout(7, stats=True); ref.rollout(7, stats=True)             # T launches here, whatever the uniform handle takes
    g.observe(); ref.observe()
    _same_handles(g, ref, "config values, rollout")
    g.close(); ref.close()


def test_constructor_takes_agent_params_and_they_survive_init_scenario_and_reset():
    A, N = 3, 12
    prm = {k: np.random.RandomState(9).uniform(*S.RANGES[k], size=(A, N)).astype(np.float32) for k in S.PARAM_NAMES}
    g = _crowd(A, N, agent_params=prm)
    _is_agent_params(g)
    g.init_scenario("crowd"); g.reset(); g.reset_masked(np.asarray([1, 0, 1], np.int32))
    _is_agent_params(g)
    got = g.agent_params()
    for k in S.PARAM_NAMES:
        H._eq(got[k], prm[k], "after reset " + k)
    st = g.get_state()
    assert not any("RADIUS" in k.upper() or "PARAM" in k.upper() for k in st)       # configuration, not state
    g.close()


def test_device_arrays_are_checked_and_copied_like_host_arrays():
    """src_is_device / dst_is_device: the arrays lie in device memory (here: the handle's own reward buffer, f32 [A,N], reached
    through ca_field_ptr); a device array is copied back for the check, so a bad value in it is refused like a host one."""
    g, ref = _crowd(), _crowd()
    L = _lib.load()
    ptr, nbytes = C.c_void_p(), C.c_size_t()
    assert L.ca_field_ptr(g.h, _lib.FLD_REWARD, C.byref(ptr), C.byref(nbytes)) == 0 and nbytes.value == g.A * g.N * 4
    r = np.random.RandomState(8).uniform(0.2, 0.8, (g.A, g.N)).astype(np.float32)
    g.set(_lib.FLD_REWARD, r)
    assert L.ca_set_agent_params(g.h, ptr, None, None, None, nbytes.value, 1) == 0, L.ca_last_error(g.h)
    _is_agent_params(g)
    H._eq(g.agent_params()["radius"], r, "radius from a device array")
    g.set(_lib.FLD_REWARD, np.zeros((g.A, g.N), np.float32))
    assert L.ca_get_agent_params(g.h, None, None, None, ptr, nbytes.value, 1) == 0, L.ca_last_error(g.h)
    H._eq(g.get(_lib.FLD_REWARD), np.full((g.A, g.N), g.cfg.time_horizon_obst, np.float32), "time_horizon_obst into a device array")
    bad = r.copy(); bad[2, 3] = np.nan
    g.set(_lib.FLD_REWARD, bad)
    assert L.ca_set_agent_params(g.h, ptr, None, None, None, nbytes.value, 1) == -5
    assert "radius=" in L.ca_last_error(g.h).decode() and "arena 2, agent 3" in L.ca_last_error(g.h).decode()
    H._eq(g.agent_params()["radius"], r, "the refused call left the radii")
    ref.set_agent_params(radius=r)
    _five_steps(g); _five_steps(ref)
    _same_handles(g, ref, "device arrays")
    g.close(); ref.close()
