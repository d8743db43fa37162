"""Forking and rewinding arenas on the device (ca_arena_gather, ca_snapshot_*; include/ca_env.h, csrc/ca_fork.h): every test compares
bit patterns (tests.helpers._eq / assert_state_equal) with the CPU oracle, whose expectation after a move is a permutation of its own
arrays along the arena axis -- arena a := arena src[a] for each state field, -1 rows of a load kept, the two clearing rules applied
the same way.  Where a configuration has no multi-arena oracle (per-agent parameters, sensing, counts, ALAN sets per arena) the
oracle is one environment per arena or per set, as in those features' own tests, and rows move between them."""
import ctypes as C
import os

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from oracle import oracle as o
from tests import agent_count_scenes as CS
from tests import agent_param_scenes as PS
from tests import agent_sensing_scenes as SS
from tests import helpers as H
from tests import wide_worlds as W

pytestmark = pytest.mark.gpu

STATE = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "GOAL2_X", "GOAL2_Y", "REWARD", "AGENT_DONE",
         "ARRIVE_STEP", "REGOAL_COUNT", "NB_COUNT", "NB_IDX", "OBST_COUNT", "OBST_IDX", "STEP_COUNT", "ARENA_DONE", "EPISODE")
ALAN = ("ALAN_WEIGHTS", "ALAN_TIMES", "ALAN_ACTION")


def _with_env(over, fn):
    old = {k: os.environ.get(k) for k in over}
    os.environ.update(over)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- the oracle's side of a move -------------------------------------------------------------------------------------------------
def _slots(orcs):
    """[(env, index of the arena inside env)] for arena 0 .. A-1 of a list of oracle environments laid end to end"""
    return [(e, i) for e in orcs for i in range(e.A)]


def _rows(slots, name):
    cache = {}
    out = []
    for e, i in slots:
        if id(e) not in cache:
            cache[id(e)] = e.get(getattr(o, "FLD_" + name))
        out.append(cache[id(e)][i].copy())
    return out


def _record(slots, alan=False):
    """the state of every arena: what a snapshot holds"""
    return {n: _rows(slots, n) for n in STATE + (ALAN if alan else ())}


def _move(slots, src, frm=None, alan=False, clear_obst=False, clear_nb=False, gather=True):
    """arena a := arena src[a] of `frm` (a _record; None: of the state as it is now).  gather: src[a] == a is not written; load:
    src[a] == -1 is not written.  The oracle keeps its lists as the index arrays padded with -1 (the counts follow from them), so a
    clearing rule writes an empty list; its reward is read-only -- a test compares the moved rewards with the record instead."""
    src = [int(v) for v in src]
    frm = _record(slots, alan) if frm is None else frm
    written = [a for a, s in enumerate(src) if (s != a if gather else s >= 0)]
    envs = {}
    for e, i in slots:
        envs.setdefault(id(e), e)
    for n in STATE + (ALAN if alan else ()):
        if n in ("REWARD", "NB_COUNT", "OBST_COUNT"):
            continue
        f = getattr(o, "FLD_" + n)
        cur = {k: e.get(f) for k, e in envs.items()}
        for a in written:
            e, i = slots[a]
            v = frm[n][src[a]]
            if (n == "OBST_IDX" and clear_obst) or (n == "NB_IDX" and clear_nb):
                v = np.full_like(cur[id(e)][i], -1)
            cur[id(e)][i] = v
        for k, e in envs.items():
            e.set(f, cur[k])
    return written


def _broadcast(A):
    """arena 0 into every slot, with one identity entry besides arena 0's own"""
    src = [0] * A
    if A > 2:
        src[A - 1] = A - 1
    return src


def _same(g, orc, what, **kw):
    H.assert_state_equal(g, orc, what, **kw)
    for n, gf, of in (("goal2_x", _lib.FLD_GOAL2_X, o.FLD_GOAL2_X), ("goal2_y", _lib.FLD_GOAL2_Y, o.FLD_GOAL2_Y)):
        H._eq(g.get(gf), orc.get(of), what + " " + n)


def _check_moved(g, st, src, written, frm=None, mask=None, clear_obst=False, clear_nb=False):
    """The move itself, field by field of get_state(), on the device's own bits: a written arena holds the rows of arena src[a] of
    `frm` (None: of st, the state before the call), every other arena -- and, under per-arena counts, every absent row (mask
    [A,N] False) -- what it held in st; a clearing rule zeroes the count of the written arenas."""
    now, frm = g.get_state(), (st if frm is None else frm)
    for k, v in st.items():
        if k == "_shape":
            continue
        want = v.copy()
        for a in written:
            row = frm[k][src[a]].copy()
            if (k == "OBST_COUNT" and clear_obst) or (k == "NB_COUNT" and clear_nb):
                row[...] = 0
            if mask is not None and v.ndim >= 2:
                row = np.where(mask[a], row, v[a])
            want[a] = row
        H._eq(now[k], want, "moved " + k)


def _permuted(st, src):
    """a get_state() dict with its arena axis gathered: what set_state brings a twin to"""
    out = {}
    for k, v in st.items():
        out[k] = v if k == "_shape" else np.ascontiguousarray(v[np.asarray(src)])
    return out


def _field_ptr(g, field):
    p, n = C.c_void_p(), C.c_size_t()
    g._call("ca_field_ptr", g.h, field, C.byref(p), C.byref(n))
    return p.value


# ---- 1. the in-place hazard --------------------------------------------------------------------------------------------------------
def test_overlapping_gather():
    """7 x 10 in the doorway (K = 5: 8-bit ids, rows of 50 bytes): arena 4 takes 6 while 6 takes 5 and 5 takes 3."""
    A, N, src = 7, 10, [3, 3, 0, 1, 6, 3, 5]
    p = dict(scenarios.env_params(), max_step=40)
    g, orc = H.make_gpu(A, N, "doorway", p, seed=11), H.make_oracle(A, N, "doorway", p, seed=11)
    assert g.K == 5 and g.launch_info()["block"] == 64
    rng = np.random.RandomState(3)
    fl = o.F_OBS | o.F_STATS | o.F_AUTORESET
    for s in range(25):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        g.step(act, stats=True, autoreset=True)
        orc.step(act, flags=fl)
    _same(g, orc, "before the fork", obs=True, reward=True)
    st, stats0, astats0 = g.get_state(), g.stats(), g.get(_lib.FLD_ARENA_STATS)
    ptrs = [_field_ptr(g, f) for f in (_lib.FLD_POS_X, _lib.FLD_STEP_COUNT)]
    g.profile(1); g.profile_read()
    obs = g.fork(src, obs=True)
    prof = g.profile_read(); g.profile(0)
    assert prof["reset_kernels"][0] == 2 and prof["obs_kernel"][0] == 1 and prof["step_kernel"][0] == 0, prof   # save, load; one observation
    _move(_slots([orc]), src)
    _same(g, orc, "after the fork")
    H._eq(g.get(_lib.FLD_REWARD), st["REWARD"][src], "after the fork reward")
    assert g.stats() == stats0
    H._eq(g.get(_lib.FLD_ARENA_STATS), astats0, "arena_stats across the fork")
    assert [_field_ptr(g, f) for f in (_lib.FLD_POS_X, _lib.FLD_STEP_COUNT)] == ptrs
    twin = H.make_gpu(A, N, "doorway", p, seed=11)
    twin.set_state(_permuted(st, src))
    H._eq(np.asarray(obs), twin.observe(), "fork(obs=True) against set_state + observe()")
    twin.close()
    for s in range(25):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        g.step(act, stats=True, autoreset=True)
        orc.step(act, flags=fl)
        if s % 6 == 0 or s in (14, 15, 24):
            _same(g, orc, "step %d after the fork" % s, obs=True, reward=True)
    assert (g.arena_stats()["episodes"] >= 1).all()
    H.assert_stats_equal(g, orc, "after the fork")
    g.close()


# ---- 2. one case per kernel family -------------------------------------------------------------------------------------------------
def _crowd_pair(A, N, over=None, env=None, scenario="crowd", **kw):
    p = H.scenario_params(scenario, N, **(over or {}))
    g = _with_env(env or {}, lambda: H.make_gpu(A, N, scenario, p, seed=5, **kw))
    return g, H.make_oracle(A, N, scenario, p, seed=5, max_obst_neighbors=kw.get("max_obst_neighbors"), polys=kw.get("polys"))


def _family(g, orc, A, N, pre=10, post=10, rollout=0):
    rng = np.random.RandomState(9)

    def steps(n, what):
        for s in range(n):
            act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
            g.step(act, stats=True)
            orc.step(act, flags=o.F_OBS | o.F_STATS)
        _same(g, orc, what, obs=True, reward=True)

    steps(pre, "before the fork")
    src, st = _broadcast(A), g.get_state()
    g.fork(src)
    _check_moved(g, st, src, _move(_slots([orc]), src))
    _same(g, orc, "after the fork")
    if rollout:
        g.rollout(rollout, stats=True)
        orc.rollout(rollout, flags=o.F_STATS)
        _same(g, orc, "rollout after the fork")
    steps(post, "steps after the fork")
    H.assert_stats_equal(g, orc, "family")


def test_family_seeded_scan():
    """N = 16 on the one-lane kernel (CA_QUAD=0: a batch this small takes the four-lanes kernel otherwise): the copied lists seed the
    next scan and are sanitised first"""
    g, orc = _crowd_pair(5, 16, env={"CA_QUAD": "0"})
    assert g.nbr_seed_info() is True
    _family(g, orc, 5, 16)
    assert g.nbr_seed_info() is True
    g.close()


def test_family_four_lanes_rollout_stays_one_launch():
    g, orc = _crowd_pair(4, 16, env={"CA_QUAD": "1"})
    li = g.launch_info()
    assert li["lanes_per_agent"] == 4 and li["rollout_one_launch"] == 1, li
    _family(g, orc, 4, 16, rollout=40)
    assert g.launch_info()["rollout_one_launch"] == 1
    g.close()


def test_family_two_lanes():
    g, orc = _crowd_pair(3, 130)
    assert g.K == 10 and g.launch_info()["lanes_per_agent"] == 2, g.launch_info()
    _family(g, orc, 3, 130, pre=6, post=6)
    g.close()


def test_family_16_bit_ids():
    g, orc = _crowd_pair(2, 300)
    assert g.launch_info()["block"] >= 512
    _family(g, orc, 2, 300, pre=5, post=5)
    g.close()


def test_family_wide_lists():
    """S = 32 around tests/wide_worlds.py's ring of 24 edges, one table for all arenas: the lists move intact"""
    A, N = 3, 10
    g, orc = _crowd_pair(A, N, polys=W.ring_world(), max_obst_neighbors=32)
    px, py = W.ring_positions(A, N)
    g.reset(px, py, with_obs=False)
    orc.reset(px, py, flags=0)
    assert g.S == 32 and g.launch_info()["lanes_per_agent"] == 1
    _family(g, orc, A, N)
    assert g.get(_lib.FLD_OBST_COUNT).max() > 16
    g.close()


def _per_arena_params(A, seed):
    rng = np.random.RandomState(seed)
    return {k: rng.uniform(PS.RANGES[k][0], PS.RANGES[k][1], A).astype(np.float32) for k in PS.PARAM_NAMES}


RAGGED_FIELDS = CS.STATE + ("GOAL2_X", "GOAL2_Y") + CS.ARENA


def _ragged_family(g, rag, A, N, src, steps_each=10, clear_nb=False, after=None, obs=True):
    rng = np.random.RandomState(4)

    def steps(n, what):
        for s in range(n):
            act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
            g.step(act, stats=True)
            for a, (c, e) in enumerate(zip(rag.counts, rag.orc)):
                e.step(act[a:a + 1, :c], flags=o.F_OBS | o.F_STATS)
        CS.same(g, rag, what, obs=obs, fields=RAGGED_FIELDS)

    steps(steps_each, "before the fork")
    st = g.get_state()
    g.fork(src)
    written = _move(_slots(rag.orc), src, clear_nb=clear_nb)
    _check_moved(g, st, src, written, mask=g.agent_mask(), clear_nb=clear_nb)
    CS.same(g, rag, "after the fork", obs=False, reward=False, fields=RAGGED_FIELDS)
    if after is not None:
        after()
    steps(steps_each, "after the fork")
    return written


def test_family_agent_params():
    """the world and the parameter ranges of tests/agent_param_scenes.py, a set of constants per arena: the parameters stay with the
    slot, so the copies of arena 0 part ways at once"""
    A, N = 4, PS.N_AGENTS
    p = dict(scenarios.bench_params(N, PS.NEIGHBOR_DIST, PS.MAX_NEIGHBORS), max_step=0)
    consts = _per_arena_params(A, 21)
    sc = CS.draw(A, N, 0.5, 5.5, 22)
    g = H.make_gpu(A, N, None, p, seed=6, polys=PS.WORLD, max_obst_neighbors=16)
    g.set_agent_params(**consts)
    CS.set_state(g, _lib, sc)
    rag = CS.RaggedOracleVec(N, [N] * A, p, PS.WORLD, 6, S_cap=16, consts=consts)
    rag.set_scene(sc)
    assert g.launch_info()["agent_params"] is True
    _ragged_family(g, rag, A, N, _broadcast(A))
    g.close()


@pytest.mark.parametrize("kind", ["tiled", "grid", "tiled_params"])
def test_family_tiled(kind):
    """3 x 200: an arena spans several tiles; 16-bit ids; the sort buffers and the launches' scratch do not move"""
    A, N = 3, 200
    if kind == "tiled_params":
        p = dict(scenarios.bench_params(N, 5.0, 10), max_step=0)
        side = 20.0
        world = [[(0.0, 0.0), (0.0, side), (side, side), (side, 0.0)]]
        consts, sc = _per_arena_params(A, 23), CS.draw(A, N, 0.5, side - 0.5, 24)
        g = H.make_gpu(A, N, None, p, seed=6, polys=world, max_obst_neighbors=4, tiled=True, tiled_params=True)
        g.set_agent_params(**consts)
        CS.set_state(g, _lib, sc)
        rag = CS.RaggedOracleVec(N, [N] * A, p, world, 6, S_cap=4, consts=consts)
        rag.set_scene(sc)
        assert g.tiled_info()["tiles_per_arena"] > 1 and g.launch_info()["agent_params"] is True
        _ragged_family(g, rag, A, N, _broadcast(A), steps_each=5)
    else:
        g, orc = _crowd_pair(A, N, tiled=("grid" if kind == "grid" else True))
        assert g.tiled_info()["tiles_per_arena"] > 1
        _family(g, orc, A, N, pre=5, post=5)
    g.close()


# ---- 3. ALAN -----------------------------------------------------------------------------------------------------------------------
ACTIONS = [(1.0, 0.0), (0.7, 0.7), (0.0, 1.0), (-0.7, 0.7), (0.7, -0.7), (0.0, 0.0)]
ACTIONS_B = [(1.0, 0.0), (0.5, 0.9), (0.9, -0.5), (-1.0, 0.1), (0.2, -1.0), (0.3, 0.3)]


def _alan_same(g, slots, what, reward=True):
    for n in STATE[:10] + (("REWARD",) if reward else ()) + ("AGENT_DONE", "ARRIVE_STEP", "STEP_COUNT", "ARENA_DONE", "EPISODE") + ALAN:
        got = g.get(getattr(_lib, "FLD_" + n))
        for a, row in enumerate(_rows(slots, n)):
            H._eq(got[a], row, "%s arena %d %s" % (what, a, n))


@pytest.mark.parametrize("form", ["quad", "lane", "three", "per_arena"])
def test_alan_state_moves_and_draws_follow_the_destination(form):
    A, N = 5, 16
    env = {"quad": {"CA_QUAD": "1"}, "lane": {"CA_QUAD": "0"}, "three": {"CA_ALAN_FUSED": "0"}, "per_arena": {}}[form]
    p = H.scenario_params("crowd", N, max_step=200)
    g = _with_env(env, lambda: H.make_gpu(A, N, "crowd", p, seed=8))
    if form == "per_arena":
        sets = [ACTIONS if a % 2 == 0 else ACTIONS_B for a in range(A)]
        g.alan_configure_per_arena(sets)
        orcs = []
        for acts in (ACTIONS, ACTIONS_B):
            e = H.make_oracle(A, N, "crowd", p, seed=8)
            e.alan_configure(acts)
            orcs.append(e)
        slots = [(orcs[a % 2], a) for a in range(A)]
    else:
        g.alan_configure(ACTIONS)
        e = H.make_oracle(A, N, "crowd", p, seed=8)
        e.alan_configure(ACTIONS)
        orcs, slots = [e], _slots([e])
    if form in ("quad", "lane"):
        assert g.launch_info()["lanes_per_agent"] == (4 if form == "quad" else 1)
    for s in range(30):
        g.alan_step()
        for e in orcs:
            e.alan_step()
    _alan_same(g, slots, "before the fork")
    src, st = [0, 0, 1, 3, 0], g.get_state()
    g.fork(src)
    _check_moved(g, st, src, _move(slots, src, alan=True))
    _alan_same(g, slots, "after the fork", reward=False)       # (the oracle's reward is read-only: _check_moved has compared it)
    w = g.get(_lib.FLD_ALAN_WEIGHTS)
    assert w[0].any() and np.array_equal(w[1], w[0]) and np.array_equal(w[4], w[0])
    for s in range(30):
        g.alan_step()
        for e in orcs:
            e.alan_step()
    _alan_same(g, slots, "30 steps after the fork")
    pos = g.get(_lib.FLD_POS_X)
    assert not np.array_equal(pos[1], pos[0]) or not np.array_equal(pos[4], pos[0])     # futures of their own
    g.close()


# ---- 4. snapshots ------------------------------------------------------------------------------------------------------------------
def test_snapshot_rewinds_bit_for_bit():
    A, N = 5, 10
    p = dict(scenarios.env_params(), max_step=45)
    g, orc = H.make_gpu(A, N, "doorway", p, seed=13), H.make_oracle(A, N, "doorway", p, seed=13)
    rng = np.random.RandomState(2)
    acts = rng.uniform(-1, 1, (60, A, N)).astype(np.float32)
    for s in range(20):
        g.step(acts[s], autoreset=True)
        orc.step(acts[s], flags=o.F_OBS | o.F_AUTORESET)
    snap = g.snapshot()
    at20 = _record(_slots([orc]))
    first = {}
    for s in range(20, 60):
        obs, rew, _, _ = g.step(acts[s], autoreset=True)
        orc.step(acts[s], flags=o.F_OBS | o.F_AUTORESET)
        if s in (20, 33, 44, 45, 59):
            _same(g, orc, "first pass step %d" % s, obs=True, reward=True)
            first[s] = (g.get_state(), np.array(obs), np.array(rew))
    assert (g.get(_lib.FLD_EPISODE) >= 1).all()            # the cap of 45 reset every arena on the way
    other = g.snapshot()                                    # a later save into another snapshot leaves the first alone
    at60 = _record(_slots([orc]))
    g.restore(snap)
    _move(_slots([orc]), range(A), frm=at20, gather=False)
    _same(g, orc, "restored")
    for s in range(20, 60):
        obs, rew, _, _ = g.step(acts[s], autoreset=True)
        orc.step(acts[s], flags=o.F_OBS | o.F_AUTORESET)
        if s in first:
            st, fobs, frew = first[s]
            now = g.get_state()
            for k in st:
                H._eq(now[k], st[k], "second pass step %d %s" % (s, k))
            H._eq(np.array(obs), fobs, "second pass step %d obs" % s)
            H._eq(np.array(rew), frew, "second pass step %d reward" % s)
    # a partial load: arenas 0 and 3 are kept, the others take arenas of the snapshot
    before = g.get_state()
    src = [-1, 0, 0, -1, 2]
    g.restore(snap, src=src)
    now = g.get_state()
    _move(_slots([orc]), src, frm=at20, gather=False)
    for k in before:
        if k != "_shape":
            H._eq(now[k][[0, 3]], before[k][[0, 3]], "kept arenas " + k)
    _same(g, orc, "partial load")
    # save twice into the same snapshot: the second state counts; `other` still holds step 60
    g.snapshot(into=snap)
    mixed = _record(_slots([orc]))
    g.step(acts[0]); orc.step(acts[0], flags=o.F_OBS)
    g.restore(snap)
    _move(_slots([orc]), range(A), frm=mixed, gather=False)
    _same(g, orc, "second save")
    g.restore(other)
    _move(_slots([orc]), range(A), frm=at60, gather=False)
    _same(g, orc, "the other snapshot")
    g.step(acts[1], autoreset=True); orc.step(acts[1], flags=o.F_OBS | o.F_AUTORESET)
    _same(g, orc, "a step after it", obs=True, reward=True)
    snap.close(); snap.close()
    with pytest.raises(ValueError):
        g.restore(snap)
    g.close()
    assert other.closed


# ---- 5. the clearing rules ---------------------------------------------------------------------------------------------------------
def test_world_per_arena_clears_the_obstacle_lists_of_written_arenas():
    A, N, src = 4, 8, [1, 1, 2, 0]
    p = H.scenario_params("blocks", N, max_step=0)
    g, orc = H.make_gpu(A, N, "blocks", p, seed=4), H.make_oracle(A, N, "blocks", p, seed=4)
    for s in range(40):
        g.orca_step(stats=True)
        orc.orca_step(flags=o.F_STATS)
    _same(g, orc, "before the fork")
    oc = g.get(_lib.FLD_OBST_COUNT)
    assert oc[1].any() and oc[2].any(), "the scene must bring obstacle edges in range"
    st = g.get_state()
    obs = g.fork(src, obs=True)
    _check_moved(g, st, src, _move(_slots([orc]), src, clear_obst=True), clear_obst=True)
    now = g.get(_lib.FLD_OBST_COUNT)
    assert not now[[0, 3]].any() and np.array_equal(now[1], oc[1]) and np.array_equal(now[2], oc[2])
    _same(g, orc, "after the fork")
    twin = H.make_gpu(A, N, "blocks", p, seed=4)
    st2 = _permuted(st, src)
    st2["OBST_COUNT"][[0, 3]] = 0
    twin.set_state(st2)
    H._eq(np.asarray(obs), twin.observe(), "fork(obs=True) against the twin with the same clearing")
    twin.close()
    for s in range(20):
        g.orca_step(stats=True, with_obs=True)
        orc.orca_step(flags=o.F_STATS | o.F_OBS)
    _same(g, orc, "20 steps after the fork", obs=True, reward=True)
    g.close()


def test_agent_sensing_clears_the_agent_lists_of_written_arenas():
    A, N = 4, SS.N_AGENTS
    p = dict(scenarios.bench_params(N, SS.NEIGHBOR_DIST, SS.MAX_NEIGHBORS), max_step=0)
    nd, K = SS.arena_constants(A, 31)
    sc = CS.draw(A, N, 0.5, 5.5, 32)
    g = H.make_gpu(A, N, None, p, seed=6, polys=PS.WORLD, max_obst_neighbors=16)
    g.set_agent_sensing(neighbor_dist=nd, max_neighbors=K)
    CS.set_state(g, _lib, sc)
    rag = SS.ArenaOracles(N, [N] * A, p, PS.WORLD, 6, nd, K, 16)
    for a, e in enumerate(rag.orc):
        CS.set_state(e, o, sc, rows=(a, N))
    assert g.launch_info()["agent_sensing"] is True
    seen = []

    def after():
        seen.append(g.get(_lib.FLD_NB_COUNT))

    # (obs=False: an oracle of one arena takes its neighbor_dist for the laser range too, which stays the handle's on the device)
    _ragged_family(g, rag, A, N, [0, 0, 2, 2], clear_nb=True, after=after, obs=False)
    assert not seen[0][[1, 3]].any() and seen[0][0].any() and seen[0][2].any()     # written: empty; untouched: their lists
    g.close()


# ---- 6. per-arena counts -----------------------------------------------------------------------------------------------------------
def test_agent_counts_move_between_arenas_of_one_size_only():
    counts, N = (5, 8, 5, 8), 8
    A = len(counts)
    p, polys, sc = CS.doorway_scene(A, N, 37, max_step=0)
    g = H.make_gpu(A, N, None, p, seed=37, polys=polys, max_obst_neighbors=16)
    g.set_agent_counts(np.asarray(counts, np.int32))
    CS.set_state(g, _lib, CS.with_decoys(sc, counts))
    rag = CS.RaggedOracleVec(N, counts, p, polys, 37, S_cap=16)
    rag.set_scene(sc)
    absent = ~g.agent_mask()
    sentinel = {}
    for k, n in enumerate(("POS_X", "VEL_Y", "ARRIVE_STEP", "GOAL2_X")):     # a sentinel per arena in the absent rows
        v = g.get(getattr(_lib, "FLD_" + n))
        v[absent] = (1000 * (k + 1) + np.arange(A)[:, None] * np.ones((1, N)))[absent].astype(v.dtype)
        g.set(getattr(_lib, "FLD_" + n), v)
        sentinel[n] = v[absent].copy()
    written = _ragged_family(g, rag, A, N, [2, 3, 0, 1], steps_each=8)
    assert written == [0, 1, 2, 3]
    for n, v in sentinel.items():
        H._eq(g.get(getattr(_lib, "FLD_" + n))[absent], v, "absent rows keep the caller's " + n)
    # a snapshot under counts: the load without an index writes the present rows only
    snap, st0 = g.snapshot(), g.get_state()
    g.step(np.zeros((A, N), np.float32))
    v = g.get(_lib.FLD_POS_X)
    v[absent] = 7777.0
    g.set(_lib.FLD_POS_X, v)
    st1 = g.get_state()
    g.restore(snap)
    _check_moved(g, st1, list(range(A)), list(range(A)), frm=st0, mask=g.agent_mask())
    assert (g.get(_lib.FLD_POS_X)[absent] == 7777.0).all() and not np.array_equal(st1["POS_X"], st0["POS_X"])
    g.set(_lib.FLD_POS_X, st0["POS_X"])
    st = g.get_state()
    src = np.asarray([1, 0, 2, 3], np.int32)
    rc = g.L.ca_arena_gather(g.h, src.ctypes.data_as(C.c_void_p), 16, 0, 0)
    msg = g.L.ca_last_error(g.h).decode()
    assert rc == -1 and "arena 0 " in msg and "5" in msg and "8" in msg, (rc, msg)
    now = g.get_state()
    for k in st:
        H._eq(now[k], st[k], "a refused gather changes nothing: " + k)
    g.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    A, N = 3, 10
    p = scenarios.env_params()
    g, orc = H.make_gpu(A, N, "doorway", p, seed=3), H.make_oracle(A, N, "doorway", p, seed=3)
    other = H.make_gpu(A, N, "doorway", p, seed=3)
    L, vp = g.L, C.c_void_p
    rng = np.random.RandomState(1)

    def refused(rc, code, *words):
        msg = L.ca_last_error(g.h).decode()
        assert rc == code and all(w in msg for w in words), (rc, code, msg, words)
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        g.step(act); orc.step(act)
        _same(g, orc, "a step after the refusal (%s)" % (words,), obs=True, reward=True)

    def idx(v):
        return np.asarray(v, np.int32)

    for bad, pos in ((A, 1), (-1, 2)):
        v = idx([0, 1, 2]); v[pos] = bad
        refused(L.ca_arena_gather(g.h, v.ctypes.data_as(vp), A * 4, 0, 0), -5, "ca_arena_gather", "arena %d " % pos, "arena %d," % bad)
    v = idx([0, 1, 2])
    refused(L.ca_arena_gather(g.h, v.ctypes.data_as(vp), A * 4 - 4, 0, 0), -4, "%d bytes" % (A * 4))
    refused(L.ca_arena_gather(g.h, v.ctypes.data_as(vp), A * 4, 0, _lib.F_STATS), -1, "CA_F_OBS")
    assert L.ca_arena_gather(None, v.ctypes.data_as(vp), A * 4, 0, 0) == -1
    snap, foreign = g.snapshot(), other.snapshot()
    v = idx([0, -2, 1])
    refused(L.ca_snapshot_load(g.h, snap._h, v.ctypes.data_as(vp), A * 4, 0, 0), -5, "ca_snapshot_load", "arena 1 ", "arena -2,")
    refused(L.ca_snapshot_load(g.h, snap._h, v.ctypes.data_as(vp), A * 4 + 4, 0, 0), -4, "bytes")
    refused(L.ca_snapshot_load(g.h, snap._h, None, 0, 0, _lib.F_AUTORESET), -1, "CA_F_OBS")
    refused(L.ca_snapshot_load(g.h, foreign._h, None, 0, 0, 0), -1, "not one of this handle's")
    refused(L.ca_snapshot_save(g.h, foreign._h), -1, "not one of this handle's")
    empty = vp()
    assert L.ca_snapshot_create(g.h, C.byref(empty)) == 0
    refused(L.ca_snapshot_load(g.h, empty, None, 0, 0, 0), -1, "nothing has been saved")
    assert L.ca_snapshot_destroy(g.h, empty) == 0
    g.snapshot(into=snap)                                   # saved before the bandit exists ...
    g.alan_configure(ACTIONS); orc.alan_configure(ACTIONS)
    refused(L.ca_snapshot_load(g.h, snap._h, None, 0, 0, 0), -1, "n_actions=0", "n_actions=%d" % len(ACTIONS))
    g.snapshot(into=snap)                                   # ... and after: the same snapshot takes the new shape
    g.restore(snap)
    _same(g, orc, "restored under the new shape")
    other.close(); g.close()


# ---- 8. the index on the device ----------------------------------------------------------------------------------------------------
def test_device_index_equals_host_index():
    import torch
    A, N, src = 6, 16, [5, 0, 0, 3, 1, 1]
    p = H.scenario_params("crowd", N)
    envs = [H.make_gpu(A, N, "crowd", p, seed=2, use_torch=True) for _ in range(2)]
    for g in envs:
        g.rollout(15)
    snaps = [g.snapshot() for g in envs]
    obs_h = envs[0].fork(src, obs=True)
    obs_d = envs[1].fork(torch.tensor(src, dtype=torch.int32, device="cuda"), obs=True)
    H._eq(obs_h.cpu().numpy(), obs_d.cpu().numpy(), "observation")
    keep = [-1, 2, -1, 0, 0, 4]
    envs[0].restore(snaps[0], src=keep)
    envs[1].restore(snaps[1], src=torch.tensor(keep, dtype=torch.int64, device="cuda"))      # (narrowed on the device)
    with pytest.raises(RuntimeError, match="arena 1 takes arena 6"):
        envs[1].fork(torch.tensor([0, 6, 2, 3, 4, 5], dtype=torch.int64, device="cuda"))
    a, b = envs[0].get_state(), envs[1].get_state()
    for k in a:
        H._eq(a[k], b[k], k)
    for g in envs:
        g.close()
