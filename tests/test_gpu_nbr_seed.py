"""The seeded neighbour scan of arenas of at most 64 agents (csrc/ca_nbr.h, CA_NBR_SEED) against the oracle, bit for bit: counts,
lists (entries up to the count) and the whole state after every step.

The scan starts each agent's list from the one the last step left in memory and runs the insertion network only for candidates
that some lane of the wave can still take, so what is tested here is what the seed can hold and how the crowd can move between
two steps: a fresh handle (zeros), lists left by another crowd (reset, in-kernel auto-reset, set_state), lists written by the
caller (duplicates, ids out of range, counts above K), teleported agents, ties, short lists, newcomers that displace the K-th
entry, and overlaps deep enough for the composite keys to fall back to the exact scan.  Every handle is forced onto the
one-lane-per-agent kernels (CA_QUAD=0: small batches take the four-lanes kernel otherwise) and asserts it; the families that share
the scan are the register-line kernel, the LDS line table (CA_REG_LINES=0) and the ALAN instantiation (the bandit inside the
solve launch): the kernels that have a SeededScan twin.  CA_NBR_SEED=0 in the environment selects the unseeded kernels: one case
runs both handles side by side."""
import os

import numpy as np
import pytest

from collision_avoidance_amd import _lib, alan
from oracle import oracle as o
from tests import agent_count_scenes as S
from tests import helpers as H

pytestmark = pytest.mark.gpu

F = np.float32
FAMILIES = {"reg": dict(CA_QUAD="0"), "table": dict(CA_QUAD="0", CA_REG_LINES="0"), "alan": dict(CA_QUAD="0")}
FLAGS = o.F_OBS | o.F_STATS


def _switched(env, fn):
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


class _Pair(object):
    """A GPU handle of one family and the oracle in the same configuration, stepped together."""

    def __init__(self, family, A, N, K, seed=3, polys=None, **over):
        self.family, self.A, self.N, self.K = family, A, N, K
        p = H.scenario_params("crowd", N, neighbor_dist=5.0, max_neighbors=K, **over)
        kw = {} if polys is None else dict(polys=polys)
        self.g = _switched(FAMILIES[family], lambda: H.make_gpu(A, N, "crowd", p, seed=seed, **kw))
        self.e = H.make_oracle(A, N, "crowd", p, seed=seed, **kw)
        if family == "alan":
            self.g.alan_configure(alan.DEFAULT_ACTIONS)
            self.e.alan_configure(alan.DEFAULT_ACTIONS)
        info = self.g.launch_info()
        assert (info["lanes_per_agent"], info["block"]) == (1, 64), (family, info)
        assert self.g.nbr_seed_info() is True, family        # the launch is a SeededScan kernel
        reg_lds = _switched(FAMILIES["reg"], lambda: H.make_gpu(1, N, "crowd", p, seed=seed, **kw))
        self.reg_lds = reg_lds.launch_info()["lds_bytes"]
        reg_lds.close()
        # (the line table asks for (K + S) KiB of LDS per wave, the register lines for (4 + 5 or 10) / 2 KiB: never equal for the K and S used here)
        assert (info["lds_bytes"] != self.reg_lds) == (family == "table"), (family, info, self.reg_lds)
        self.rng = np.random.RandomState(11)
        self.steps = 0

    def step(self, autoreset=False):
        if self.family == "alan":
            u = self.rng.uniform(0, 1, (self.A, self.N))
            self.g.alan_step(u=u, stats=True, with_obs=True)
            self.e.alan_step(u=u, flags=FLAGS)
        else:
            act = self.rng.uniform(-1, 1, (self.A, self.N)).astype(F)
            self.g.step(act, stats=True, autoreset=autoreset)
            self.e.step(act, flags=FLAGS | (o.F_AUTORESET if autoreset else 0))
        self.steps += 1

    def same(self, what):
        H.assert_state_equal(self.g, self.e, "%s %s, step %d" % (self.family, what, self.steps), obs=True, reward=(self.family != "alan"))
        H.assert_stats_equal(self.g, self.e, "%s %s, step %d" % (self.family, what, self.steps))

    def run(self, n, what, autoreset=False):
        for _ in range(n):
            self.step(autoreset)
            self.same(what)

    def put(self, name, arr):
        """the same field on both sides (positions, velocities, counters: not the lists, which only the GPU handle reads)"""
        self.g.set(getattr(_lib, "FLD_" + name), arr)
        self.e.set(getattr(o, "FLD_" + name), arr)

    def teleport(self, px, py):
        self.put("POS_X", np.asarray(px, F))
        self.put("POS_Y", np.asarray(py, F))

    def lists(self, cnt, idx):
        """overwrite the GPU handle's lists (idx [A, N, K]) through ca_set: the oracle never reads its own before a step"""
        self.g.set(_lib.FLD_NB_COUNT, np.asarray(cnt, np.int32))
        self.g.set(_lib.FLD_NB_IDX, np.ascontiguousarray(np.transpose(np.asarray(idx, np.int32), (0, 2, 1))))

    def close(self):
        self.g.close()


FAMILY = pytest.mark.parametrize("family", sorted(FAMILIES))


@FAMILY
@pytest.mark.parametrize("N,K,A", [(64, 10, 2), (64, 1, 1), (11, 10, 3), (10, 10, 7), (3, 10, 8), (3, 1, 5)])
def test_fresh_handle_then_a_young_crowd(family, N, K, A):
    """The first step of a fresh handle (every seed is zeros: count 0), then the crowd's own lists as seeds.  N = 10: seven arenas
    share a wave at ten lanes each; N = 3 with K = 10: lists that can never fill."""
    q = _Pair(family, A, N, K)
    assert not q.g.get(_lib.FLD_NB_COUNT).any()
    q.run(12 if N == 64 else 25, "young crowd")
    q.close()


@FAMILY
def test_after_reset_and_masked_reset(family):
    """ca_reset leaves the lists of the crowd that was: stale seeds for the first step of the next episode"""
    q = _Pair(family, 4, 64, 10)
    q.run(6, "before reset")
    q.g.reset(); q.e.reset(flags=o.F_OBS)
    q.run(3, "after ca_reset")
    mask = np.array([1, 0, 1, 0], np.int32)
    q.g.reset_masked(mask); q.e.reset_masked(mask, flags=o.F_OBS)
    q.run(3, "after a masked reset")
    q.close()


@pytest.mark.parametrize("family", ["reg", "table"])
def test_in_kernel_auto_reset(family):
    """max_step 9 with CA_F_AUTORESET: the kernel re-spawns the arena in its own epilogue, the next launch is seeded with the old crowd.
    (Not the ALAN family: ca_alan_step takes no CA_F_AUTORESET, its episodes end frozen and are reset by the caller -- the case above.)"""
    q = _Pair(family, 3, 16, 10, max_step=9)
    q.run(30, "auto-reset", autoreset=True)
    assert (q.g.arena_stats()["episodes"] >= 2).all()
    q.close()


STATE_FIELDS = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "GOAL2_X", "GOAL2_Y", "AGENT_DONE",
                "ARRIVE_STEP", "STEP_COUNT", "ARENA_DONE", "EPISODE", "REGOAL_COUNT")   # (the reward is written by every step)


@FAMILY
@pytest.mark.parametrize("keep_lists", [False, True])
def test_set_state_from_a_different_crowd(family, keep_lists):
    """A handle that ran one history takes the state of another: with the snapshot's own lists (true seeds for positions the
    handle never computed), and with the lists the handle had (keep_lists: another crowd's)."""
    a = _Pair(family, 2, 64, 10)
    b = _Pair(family, 2, 64, 10)
    b.rng = np.random.RandomState(12)
    a.run(4, "history a")
    for _ in range(20):
        b.step()
    b.same("history b")
    st = a.g.get_state()
    if keep_lists:
        mine = b.g.get_state()
        st = dict(st, NB_COUNT=mine["NB_COUNT"], NB_IDX=mine["NB_IDX"])
    b.g.set_state(st)
    for name in STATE_FIELDS + (("ALAN_WEIGHTS", "ALAN_TIMES", "ALAN_ACTION") if family == "alan" else ()):
        b.e.set(getattr(o, "FLD_" + name), st[name])
    b.run(3, "after set_state")
    a.close(); b.close()


@FAMILY
@pytest.mark.parametrize("N,K", [(64, 10), (11, 10), (11, 1)])
def test_lists_written_by_the_caller(family, N, K):
    """CA_FLD_NB_IDX / CA_FLD_NB_COUNT are settable: duplicates, ids out of range, the lane's own id and counts above K, then one
    step, and one more from the (correct) lists that step left"""
    A = 4
    q = _Pair(family, A, N, K)
    q.run(3, "before")
    rng = np.random.RandomState(2)
    dup = np.repeat(rng.randint(0, N, (1, N, 1)), K, axis=2)[0]
    idx = np.stack([dup,                                                        # one id K times
                    rng.randint(N, 256, (N, K)),                                 # nothing but ids out of range
                    np.repeat(np.arange(N)[:, None], K, axis=1),                 # the lane itself
                    rng.randint(0, 256, (N, K))])                                # anything a byte holds
    cnt = np.stack([np.full(N, K), np.full(N, 255), np.full(N, K + 1), rng.randint(0, 256, N)])
    q.lists(cnt, idx)
    q.run(2, "after ca_set of the lists")
    q.close()


def _far(N, k):
    """positions far from everything else (more than the range apart from each other, too)"""
    return F(100.0 + 11.0 * k), F(-50.0)


def _scene(A, N, place):
    """[A, N] positions: agent k of every arena parked far away unless place(a) names it"""
    px, py = np.empty((A, N), F), np.empty((A, N), F)
    for a in range(A):
        given = place(a)
        for k in range(N):
            px[a, k], py[a, k] = given.get(k, _far(N, k))
    return px, py


@FAMILY
def test_teleported_agents(family):
    """every position replaced through ca_set between two steps: the seed is a list of agents that are somewhere else now"""
    q = _Pair(family, 3, 64, 10)
    q.run(3, "before")
    px, py = q.g.get(_lib.FLD_POS_X), q.g.get(_lib.FLD_POS_Y)
    perm = np.random.RandomState(4).permutation(64)
    q.teleport(px[:, perm], py[:, perm])
    q.run(2, "after teleport")
    q.close()


@FAMILY
@pytest.mark.parametrize("K", [1, 2])
def test_lattice_with_tie_groups_larger_than_k(family, K):
    """a square lattice (spacing 1.25, exact in fp32): four candidates at a bit-identical distance, eight at the next, for K of 1
    and 2 -- the lower index wins whichever came first, seeded or not"""
    A, N = 2, 11
    q = _Pair(family, A, N, K, polys=[])
    def lattice(a):
        perm = np.random.RandomState(a).permutation(16)[:N]
        return {k: (F(1.25 * (c % 4)), F(1.25 * (c // 4))) for k, c in enumerate(perm)}
    px, py = _scene(A, N, lattice)
    q.g.reset(px, py); q.e.reset(px, py, flags=o.F_OBS)
    q.run(1, "lattice, unseeded")
    q.teleport(px, py)                        # back onto the lattice: the ties again, now with seeds
    q.run(1, "lattice, seeded")
    q.teleport(px[:, ::-1], py[:, ::-1])      # ... and with every index mirrored
    q.run(1, "lattice, mirrored")
    q.close()


@FAMILY
def test_short_lists_and_the_range_boundary(family):
    """N = 3 with K = 10 (a list can never fill; its threshold stays the range): agent 1 crosses the range of 5 outward and inward,
    a step each"""
    A, N = 2, 3
    q = _Pair(family, A, N, 10, polys=[])
    def at(d1):
        return lambda a: {0: (F(0.0), F(0.0)), 1: (F(d1), F(0.0)), 2: (F(0.0), F(3.0 + a))}
    px, py = _scene(A, N, at(4.9))
    q.g.reset(px, py); q.e.reset(px, py, flags=o.F_OBS)
    for d1, n0 in ((4.9, 2), (5.2, 1), (4.9, 2), (5.2, 1)):
        q.teleport(*_scene(A, N, at(d1)))
        q.run(1, "agent 1 at %.1f" % d1)
        assert (q.g.get(_lib.FLD_NB_COUNT)[:, 0] == n0).all(), (d1, q.g.get(_lib.FLD_NB_COUNT))
    q.close()


@FAMILY
def test_two_newcomers_for_one_lane_in_one_step(family):
    """K = 2, agent 0's list is {1, 2} at 1.0 and 1.5; agents 3 and 4 arrive at 0.8 and 1.2 (arena 0) or 1.2 and 0.8 (arena 1: the
    first newcomer in index order displaces the K-th entry and is displaced by the second); arena 2: nobody moves"""
    A, N = 3, 11
    q = _Pair(family, A, N, 2, polys=[])
    base = {0: (F(0.0), F(0.0)), 1: (F(1.0), F(0.0)), 2: (F(0.0), F(1.5))}
    px, py = _scene(A, N, lambda a: base)
    q.g.reset(px, py); q.e.reset(px, py, flags=o.F_OBS)
    q.teleport(px, py)
    q.run(1, "before the newcomers")
    assert (q.g.neighbor_lists()[1][:, 0] == [1, 2]).all()
    def arrive(a):
        d3, d4 = ((0.8, 1.2), (1.2, 0.8), (None, None))[a]
        got = dict(base)
        if d3 is not None:
            got.update({3: (F(-d3), F(0.0)), 4: (F(0.0), F(-d4))})
        return got
    q.teleport(*_scene(A, N, arrive))
    q.run(1, "two newcomers")
    want = np.array([[3, 1], [4, 1], [1, 2]])
    assert (q.g.neighbor_lists()[1][:, 0] == want).all(), q.g.neighbor_lists()[1][:, 0]
    q.close()


@FAMILY
def test_deep_overlap_after_a_seeded_scan(family):
    """two neighbours nearer than sqrt(0.125) share the clamped image 0: the wave falls through to the exact 64-bit scan, after a
    seeded scan of a crowd that had none"""
    A, N = 2, 64
    q = _Pair(family, A, N, 10)
    q.run(3, "before")
    px, py = q.g.get(_lib.FLD_POS_X), q.g.get(_lib.FLD_POS_Y)
    px[0, 5], py[0, 5] = px[0, 40] + F(0.1), py[0, 40]            # arena 0: agents 5 and 7 next to agent 40, nearer 7 first ...
    px[0, 7], py[0, 7] = px[0, 40], py[0, 40] + F(0.05)
    q.teleport(px, py)
    q.run(1, "deep overlap")
    assert (q.g.neighbor_lists()[1][0, 40, :2] == [7, 5]).all()
    q.run(1, "one step on")
    q.close()


def test_arena_counts_handle_with_unequal_counts():
    """ca_set_agent_counts (the ArenaCounts instantiation's seeded twin): absent rows hold decoys -- copies of agent 0 -- that the
    seed must never let in, not even when the caller's lists name them; arenas of 1 .. 16 agents share a wave, four at a time"""
    A, N, counts, params, polys, sc, steps = S.box_scene("one wave, four arenas each")
    g = H.make_gpu(A, N, None, params, seed=34, polys=polys)
    g.set_agent_counts(np.asarray(counts, np.int32))
    S.set_state(g, _lib, S.with_decoys(sc, counts))
    rag = S.RaggedOracleVec(N, counts, params, polys, 34, S_cap=g.S)
    rag.set_scene(sc)
    li = g.launch_info()
    assert li["agent_counts"] is True and (li["lanes_per_agent"], li["block"]) == (1, 64), li
    assert g.nbr_seed_info() is True
    rng = np.random.RandomState(S.BOX_ACTION_SEED)
    for s in range(steps):
        if s == 10:      # every list names the absent rows first (ids n_a .. N - 1), then itself, then anything
            idx = np.tile(np.arange(N - 1, N - 1 - g.K, -1)[None, None, :], (A, N, 1)) % N
            g.set(_lib.FLD_NB_COUNT, np.full((A, N), 255, np.int32))
            g.set(_lib.FLD_NB_IDX, np.ascontiguousarray(np.transpose(idx.astype(np.int32), (0, 2, 1))))
        act = rng.uniform(-1, 1, (A, N)).astype(F)
        g.step(act, stats=True)
        rag.step(act, stats=True)
        if s < 3 or s in (9, 10, 11) or s == steps - 1:
            S.same(g, rag, "counts step %d" % s)
    g.close()


@pytest.mark.parametrize("family", ["reg", "table"])
def test_the_environment_switch_selects_the_unseeded_kernels(family):
    """CA_NBR_SEED=0 when the handle is made: the kernels without the SeededScan tag; the same bits as the seeded handle and the oracle"""
    q = _Pair(family, 2, 64, 10)
    p = H.scenario_params("crowd", 64, neighbor_dist=5.0, max_neighbors=10)
    plain = _switched(dict(FAMILIES[family], CA_NBR_SEED="0"), lambda: H.make_gpu(2, 64, "crowd", p, seed=3))
    assert plain.launch_info() == q.g.launch_info() and plain.nbr_seed_info() is False
    rng = np.random.RandomState(11)
    for s in range(6):
        act = rng.uniform(-1, 1, (2, 64)).astype(F)
        q.step()
        plain.step(act, stats=True)
    q.same("seeded")
    H.assert_state_equal(plain, q.e, family + " unseeded", obs=True, reward=True)
    plain.close(); q.close()


def test_alan_with_an_action_set_per_arena():
    """ca_alan_configure_per_arena (the AlanArenaSets instantiation's seeded twin) with the same set on every arena, which is
    ca_alan_configure's result bit for bit: a fresh handle, then its own lists as seeds.  (Sets of different sizes on this kernel:
    tests/test_gpu_alan_per_arena.py, one oracle per set.)"""
    A, N = 3, 64
    p = H.scenario_params("crowd", N, neighbor_dist=5.0, max_neighbors=10)
    g = _switched(FAMILIES["alan"], lambda: H.make_gpu(A, N, "crowd", p, seed=3))
    e = H.make_oracle(A, N, "crowd", p, seed=3)
    g.alan_configure_per_arena([alan.DEFAULT_ACTIONS] * A)
    e.alan_configure(alan.DEFAULT_ACTIONS)
    assert g.launch_info()["lanes_per_agent"] == 1 and g.nbr_seed_info() is True
    rng = np.random.RandomState(5)
    for s in range(10):
        u = rng.uniform(0, 1, (A, N))
        g.alan_step(u=u, stats=True, with_obs=True)
        e.alan_step(u=u, flags=FLAGS)
        H.assert_state_equal(g, e, "per-arena sets, step %d" % s, obs=True)
    H.assert_stats_equal(g, e, "per-arena sets")
    g.close()
