"""Arenas of different crowd sizes in one batch on the GPU (ca_set_agent_counts): arena a of a handle whose arena holds n_a agents
against OracleEnv(n_arenas=1, n_agents=n_a, arena_offset=a), bit for bit (tests/agent_count_scenes.py, whose scenes
tests/test_agent_counts_cpu.py checks on the oracle alone).  Every test asserts launch_info(), so that it cannot pass on another
kernel, fills the absent rows with decoys -- copies of the arena's agent 0, which would change a neighbour list, a pair count or an
observation if they leaked -- and asserts at its end that the decoys still hold the same bits and show a zero observation and reward."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from oracle import oracle as o
from tests import agent_count_scenes as S
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _is_agent_counts(g):
    """launch_info() of a handle with counts: one lane per agent on the LDS line table (K + S lines, the staged arena, the misc ints
    and the staged radii per lane), T launches per rollout"""
    li = g.launch_info()
    assert li["agent_counts"] is True and li["lanes_per_agent"] == 1 and li["rollout_one_launch"] == 0, li
    assert li["lds_bytes"] == li["block"] * ((g.K + g.S) * 16 + 36), (li, g.K, g.S)
    return li


class _Decoys(object):
    """The absent rows of g as they are now (after the test wrote its decoys), to be found again at the end."""

    def __init__(self, g):
        self.g, self.absent = g, ~g.agent_mask()
        self.rows = {n: g.get(getattr(_lib, "FLD_" + n))[self.absent] for n in S.ROW_FIELDS}

    def untouched(self, what):
        g = self.g
        for n, v in self.rows.items():
            H._eq(g.get(getattr(_lib, "FLD_" + n))[self.absent], v, "%s: absent rows, %s" % (what, n))
        assert not g.get(_lib.FLD_OBS)[self.absent].any(), what + ": observation of an absent row"
        assert not g.get(_lib.FLD_REWARD)[self.absent].view(np.uint32).any(), what + ": reward of an absent row"
        assert not g.get(_lib.FLD_NB_COUNT)[self.absent].any() and not g.get(_lib.FLD_OBST_COUNT)[self.absent].any(), what


def _pair(N, counts, params, polys, sc, seed, S_cap=None, consts=None):
    """A GPU handle with counts and decoys in its absent rows, and the per-arena oracles, in the same state"""
    A = len(counts)
    g = H.make_gpu(A, N, None, params, seed=seed, polys=polys, max_obst_neighbors=S_cap)
    g.set_agent_counts(np.asarray(counts, np.int32))
    if consts is not None:
        g.set_agent_params(**consts)
    S.set_state(g, _lib, S.with_decoys(sc, counts))
    rag = S.RaggedOracleVec(N, counts, params, polys, seed, S_cap=g.S, consts=consts)
    rag.set_scene(sc)
    H._eq(g.agent_counts(), np.asarray(counts, np.int32), "agent_counts()")
    return g, rag, _Decoys(g)


def _doorway_with_autoreset(counts, N, seed, consts_too):
    A = len(counts)
    p, polys, sc = S.doorway_scene(A, N, seed, max_step=50)
    g, rag, dec = _pair(N, counts, p, polys, sc, seed, S_cap=16, consts=sc["consts"] if consts_too else None)
    li = _is_agent_counts(g)
    assert li["agent_params"] is consts_too
    rng = np.random.RandomState(5)
    for s in range(120 if not consts_too else 60):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        g.step(act, stats=True, autoreset=True)
        rag.step(act, stats=True, autoreset=True)
        if s % 20 == 19 or s in (49, 50):
            S.same(g, rag, "doorway step %d" % s)
    _is_agent_counts(g)
    assert g.stats()["obst_overflow"] == 0
    return g, rag, dec


def test_doorway_with_autoreset():
    """6 x 12 in the reference env's own world, counts 1 .. 12, max_step 50, CA_F_AUTORESET, 120 steps: two episodes per arena
    and the dense observation path; the counts survive the resets."""
    g, rag, dec = _doorway_with_autoreset((1, 3, 12, 7, 2, 10), 12, 31, False)
    assert (g.arena_stats()["episodes"] >= 2).all()
    dec.untouched("doorway")
    g.close()


def test_arrival_scene_every_arena_stops_at_its_own_step():
    """init_scenario(doorway) with counts, reset() with the caller's position arrays, then ONE rollout with CA_F_FREEZE: an arena's
    episode is over when all of ITS agents have arrived, or at the cap."""
    rag, p, px, py = S.arrival_oracles()
    counts = rag.agent_counts()
    g = H.make_gpu(rag.A, rag.N, "doorway", p, seed=S.ARRIVAL_SEED, agent_counts=counts)
    li = _is_agent_counts(g)
    for n in ("POS_X", "POS_Y", "VEL_X", "VEL_Y"):                      # decoys: the arena's agent 0 ...
        v = g.get(getattr(_lib, "FLD_" + n))
        for a, c in enumerate(counts):
            v[a, c:] = v[a, 0]
        g.set(getattr(_lib, "FLD_" + n), v)
    dec = _Decoys(g)
    dpx, dpy = px.copy(), py.copy()
    for a, c in enumerate(counts):
        dpx[a, c:], dpy[a, c:] = px[a, 0], py[a, 0]                       # ... also in the position arrays of the reset
    g.reset(dpx, dpy, with_obs=False)
    g.rollout(400, freeze=True, stats=True)
    for e in rag.orc:
        e.rollout(400, flags=o.F_STATS | o.F_FREEZE)
    S.same(g, rag, "arrival", obs=False, reward=False, fields=S.STATE + S.ARENA + ("ARRIVE_STEP",))
    gs, os_ = g.arena_stats(), rag.arena_stats()
    for k in ("last_episode_steps", "last_episode_arrived"):
        H._eq(gs[k], os_[k], "arrival " + k)
    assert len(set(gs["last_episode_steps"])) >= 3 and (gs["last_episode_arrived"] <= counts).all(), gs
    assert g.get(_lib.FLD_ARENA_DONE).all() and g.launch_info() == li
    dec.untouched("arrival")
    g.close()


@pytest.mark.parametrize("name", sorted(S.BOXES))
def test_walled_boxes_with_regoal(name):
    A, N, counts, p, polys, sc, steps = S.box_scene(name)
    g, rag, dec = _pair(N, counts, p, polys, sc, S.BOXES[name][3])
    li = _is_agent_counts(g)
    assert li["block"] == {16: 64, 70: 128, 200: 256}[N] and li["grid"] == {16: 2, 70: 3, 200: 2}[N], li
    rng = np.random.RandomState(S.BOX_ACTION_SEED)
    for s in range(steps):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        g.step(act, stats=True)
        rag.step(act, stats=True)
        if s % 10 == 9:
            S.same(g, rag, "box %d step %d" % (N, s))
    assert g.stats()["collisions"] > 0
    dec.untouched(name)
    g.close()


_ALL = S.ROW_FIELDS + S.ARENA + ("REWARD", "OBS", "NB_COUNT", "OBST_COUNT", "ARENA_STATS")


@pytest.mark.parametrize("world", ["doorway", "box"])
def test_counts_equal_to_n_give_the_uniform_bits(world):
    if world == "doorway":
        A, N = 4, 12
        p, polys, sc = S.doorway_scene(A, N, 36, max_step=20)
    else:
        A, N = 2, 70
        p, polys, sc = scenarios.bench_params(N, 5.0, 10), S.box_world(N), S.draw(2, 70, 0.5, scenarios.crowd_envsize(70) - 0.5, 37)
    g, ref = (H.make_gpu(A, N, None, p, seed=36, polys=polys, max_obst_neighbors=16 if world == "doorway" else None) for _ in range(2))
    g.set_agent_counts(np.full(A, N, np.int32))
    _is_agent_counts(g)
    assert not ref.launch_info()["agent_counts"] and not g.launch_info()["agent_params"]
    S.set_state(g, _lib, sc); S.set_state(ref, _lib, sc)
    rng = np.random.RandomState(8)
    for s in range(30):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        g.step(act, stats=True, autoreset=True); ref.step(act, stats=True, autoreset=True)
        if s % 10 == 9:
            for n in _ALL:
                a, b = g.get(getattr(_lib, "FLD_" + n)), ref.get(getattr(_lib, "FLD_" + n))
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (world, s, n)
            for lists in ("neighbor_lists", "obstacle_neighbor_lists"):            # (the entries of a list, not what lies behind its end)
                (ca, ia), (cb, ib) = getattr(g, lists)(), getattr(ref, lists)()
                mask = np.arange(ia.shape[2])[None, None, :] < ca[:, :, None]
                assert np.array_equal(ca, cb) and np.array_equal(np.where(mask, ia, -1), np.where(mask, ib, -1)), (world, s, lists)
    assert g.stats() == ref.stats()
    g.close(); ref.close()


def test_with_per_arena_orca_constants():
    """4 x 12 doorway, counts (12, 5, 1, 8), radius / max_speed / horizons per arena through set_agent_params, 60 steps with
    autoreset, against per-arena oracles that carry both; clearing the parameters keeps the counts."""
    g, rag, dec = _doorway_with_autoreset((12, 5, 1, 8), 12, 31, True)
    dec.untouched("constants per arena")
    g.clear_agent_params()
    li = _is_agent_counts(g)
    assert li["agent_params"] is False
    H._eq(g.agent_counts(), np.asarray((12, 5, 1, 8), np.int32), "counts after clear_agent_params")
    H._eq(g.agent_params()["radius"], np.full((4, 12), g.cfg.radius, np.float32), "radius after clear_agent_params")
    g.step(np.zeros((4, 12), np.float32), stats=True)
    dec.untouched("after clear_agent_params")
    g.close()


def _raw_set(g, counts, nbytes=None):
    L = _lib.load()
    c = np.ascontiguousarray(counts, np.int32)
    rc = L.ca_set_agent_counts(g.h, c.ctypes.data_as(C.c_void_p), c.nbytes if nbytes is None else nbytes, 0)
    return rc, (L.ca_last_error(g.h) or b"").decode()


def _crowd(A=3, N=12, **kw):
    return H.make_gpu(A, N, "crowd", scenarios.bench_params(N, 5.0, 10), seed=11, polys=S.box_world(N), **kw)   # (walls: obstacle neighbours)


@pytest.mark.parametrize("configured", [False, True], ids=["uniform handle", "handle with counts"])
def test_the_call_itself(configured):
    g = _crowd()
    g.alan_configure([(1.0, 0.0), (0.0, 1.0)])
    for s in range(3):
        g.orca_step(stats=True)
    assert g.get(_lib.FLD_NB_COUNT).any() and g.get(_lib.FLD_OBST_COUNT).any()
    uniform = g.launch_info()
    assert not uniform["agent_counts"]
    first = np.asarray((12, 4, 7), np.int32)
    if configured:
        g.set_agent_counts(first)
        _is_agent_counts(g)
        assert not g.get(_lib.FLD_NB_COUNT).any() and not g.get(_lib.FLD_OBST_COUNT).any()     # the lists of every arena are empty
        assert not g.get(_lib.FLD_OBS)[~g.agent_mask()].any() and not g.get(_lib.FLD_REWARD)[~g.agent_mask()].any()
    before = g.launch_info()
    for bad, arena in ((0, 1), (g.N + 1, 2), (-3, 0)):
        c = np.full(g.A, 5, np.int32)
        c[arena] = bad
        rc, msg = _raw_set(g, c)
        assert rc == -5 and "arena %d" % arena in msg and str(bad) in msg, (bad, rc, msg)
    for nbytes in (g.A * 4 - 4, g.A * 8, 0):
        rc, msg = _raw_set(g, np.full(g.A, 5, np.int32), nbytes)
        assert rc == -4, (nbytes, rc, msg)
    assert g.launch_info() == before
    H._eq(g.agent_counts(), first if configured else np.full(g.A, g.N, np.int32), "agent_counts() after refused calls")
    if configured:
        L = _lib.load()
        assert L.ca_init_scenario(g.h, _lib.SCN_CROWD) == -1 and "agent counts" in L.ca_last_error(g.h).decode()
        assert L.ca_alan_step(g.h, None, 0, 0) == -1 and "agent counts" in L.ca_last_error(g.h).decode()
        assert L.ca_alan_rollout(g.h, 2, 0) == -1 and L.ca_init_scenario(g.h, _lib.SCN_DOORWAY) == 0
        assert g.launch_info() == before
        with pytest.raises(ValueError):
            g.set_agent_counts(np.zeros((g.A, g.N), np.int32))
        g.orca_step(stats=True)
        g.clear_agent_counts()
        assert g.launch_info() == uniform
        H._eq(g.agent_counts(), np.full(g.A, g.N, np.int32), "agent_counts() after clear_agent_counts")
        g.alan_step()                                                        # works again
    g.close()


def test_not_together_with_wide_obstacle_lists():
    g = _crowd(max_obst_neighbors=24)
    before = g.launch_info()
    rc, msg = _raw_set(g, np.full(g.A, 5, np.int32))
    assert rc == -1 and "wide obstacle lists" in msg, (rc, msg)
    assert g.launch_info() == before and not before["agent_counts"]
    g.close()


def _adapter_gpu():
    g = H.make_gpu(len(S.ADAPTER_COUNTS), S.ADAPTER_N, "doorway", S.adapter_params(), seed=S.ADAPTER_SEED,
                   agent_counts=np.asarray(S.ADAPTER_COUNTS, np.int32))
    for n in ("POS_X", "POS_Y", "VEL_X", "VEL_Y"):
        v = g.get(getattr(_lib, "FLD_" + n))
        for a, c in enumerate(S.ADAPTER_COUNTS):
            v[a, c:] = v[a, 0]
        g.set(getattr(_lib, "FLD_" + n), v)
    _is_agent_counts(g)
    return g, _Decoys(g)


def test_multi_agent_vector_env_on_the_device():
    g, dec = _adapter_gpu()
    S.check_multi_agent_adapter(g)
    _is_agent_counts(g)
    dec.untouched("MultiAgentVectorEnv")
    g.close()


def test_agent_vector_env_on_the_device_equals_the_oracles():
    """AgentVectorEnv over the HIP env: the checks of the CPU test, and the same observations, rewards and dones as the adapter
    over the per-arena oracles (both reset finished arenas inside the step)."""
    from collision_avoidance_amd.adapters import AgentVectorEnv
    g, dec = _adapter_gpu()
    S.check_agent_vector_adapter(g)
    dec.untouched("AgentVectorEnv")
    g.close()
    g, dec = _adapter_gpu()
    rag = S.RaggedOracleVec(S.ADAPTER_N, S.ADAPTER_COUNTS, S.adapter_params(), scenarios.obstacles("doorway", S.ADAPTER_N), S.ADAPTER_SEED,
                            S_cap=g.S, scenario="doorway")
    eg, eo = AgentVectorEnv(g), AgentVectorEnv(rag)
    H._eq(np.asarray(eg.reset()), eo.reset(), "reset observation")
    rng = np.random.RandomState(6)
    for s in range(S.ADAPTER_STEPS):
        act = rng.uniform(-1, 1, eg.num_envs).astype(np.float32)
        og, rg, dg, ig = eg.step(act)
        oo, ro, do, io = eo.step(act)
        H._eq(np.asarray(og), oo, "step %d observation" % s); H._eq(np.asarray(rg), ro, "step %d reward" % s)
        assert np.array_equal(dg, do) and np.array_equal(ig["episode"]["truncated"], io["episode"]["truncated"]), s
    dec.untouched("AgentVectorEnv against the oracles")
    g.close()
