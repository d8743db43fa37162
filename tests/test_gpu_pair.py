"""Large arenas (129 .. 512 agents): the two-lanes-per-agent solve kernel (csrc/ca_pair.h) is the default there and the
one-lane register-line kernel (CA_PAIR=0) its fallback -- both against the oracle, bit for bit, and against
each other.  The pair kernel works through the arena in the order of its uniform grid, so per-agent results must not
depend on where in that order an agent sits: actions, rewards, observation, auto-reset and per-arena freezing included."""
import os

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from oracle import oracle as o
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _with_pair(value, fn):
    old = os.environ.get("CA_PAIR")
    os.environ["CA_PAIR"] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["CA_PAIR"]
        else:
            os.environ["CA_PAIR"] = old


def test_pair_kernel_is_the_default_for_large_arenas_only():
    for N, lanes in ((512, 2), (300, 2), (192, 2), (129, 2), (1000, 1)):
        g = H.make_gpu(2 if N < 1000 else 1, N, "crowd", H.scenario_params("crowd", N), seed=1)
        assert g.launch_info()["lanes_per_agent"] == lanes, (N, g.launch_info())
        g.close()
    g = _with_pair("0", lambda: H.make_gpu(2, 300, "crowd", H.scenario_params("crowd", 300), seed=1))
    assert g.launch_info()["lanes_per_agent"] == 1
    g.close()
    # K = 16 or more than four obstacle neighbours need the LDS line table: one lane per agent
    g = H.make_gpu(2, 250, "crowd", H.scenario_params("crowd", 250, max_neighbors=16), seed=1)
    assert g.launch_info()["lanes_per_agent"] == 1
    g.close()


@pytest.mark.parametrize("N,K,nd,scenario", [(512, 10, 5.0, "crowd"), (300, 7, 4.0, "crowd"), (200, 3, 2.0, "crowd"),
                                             (256, 10, 5.0, "circle"), (226, 10, 5.0, "incoming")])
def test_pair_and_helper_variants_step_with_actions_obs_autoreset(N, K, nd, scenario):
    """Full steps (actions in, reward and observation out) with statistics and auto-reset, a short episode cap so that the
    reset happens inside the run: the default (pair) kernel, the CA_PAIR=0 one-lane fallback and the oracle agree bit for
    bit.  (The name is from the helper-lane kernel that was the fallback once; it is kept so that the test ids stay.)"""
    A = 3
    p = H.scenario_params(scenario, N, max_neighbors=K, neighbor_dist=nd, max_step=7)
    pair = H.make_gpu(A, N, scenario, p, seed=9)
    one = _with_pair("0", lambda: H.make_gpu(A, N, scenario, p, seed=9))
    orc = H.make_oracle(A, N, scenario, p, seed=9)
    assert pair.launch_info()["lanes_per_agent"] == 2 and one.launch_info()["lanes_per_agent"] == 1
    rng = np.random.RandomState(3)
    for s in range(16):
        act = rng.uniform(-1.0, 1.0, (A, N)).astype(np.float32)
        pair.step(act, stats=True, autoreset=True)
        one.step(act, stats=True, autoreset=True)
        orc.step(act, flags=o.F_OBS | o.F_STATS | o.F_AUTORESET)
        if s % 5 == 4 or s == 15:
            H.assert_state_equal(pair, orc, "pair step %d" % s, obs=True, reward=True)
            H.assert_state_equal(one, orc, "one-lane fallback step %d" % s, obs=True, reward=True)
    H.assert_stats_equal(pair, orc, "pair")
    H.assert_stats_equal(one, orc, "one-lane fallback")
    assert pair.stats()["episodes"] >= 2 * A      # the cap of 7 steps ended (and restarted) every arena at least twice
    np.testing.assert_array_equal(pair.get(_lib.FLD_ARENA_STATS)[:, [0, 1, 2, 3, 4, 6, 7]],
                                  orc.get(o.FLD_ARENA_STATS)[:, [0, 1, 2, 3, 4, 6, 7]])
    pair.close(); one.close()


def test_pair_done_modes_and_freeze():
    """The goal test of ALAN:547-566 (arrival -> second goal, arrival step recorded) and per-arena freezing under the pair
    kernel: a 200-agent circle whose agents arrive at different times, rolled out with CA_F_FREEZE."""
    A, N = 2, 200
    p = H.scenario_params("circle", N, max_step=40)
    g = H.make_gpu(A, N, "circle", p, seed=4)
    e = H.make_oracle(A, N, "circle", p, seed=4)
    assert g.launch_info()["lanes_per_agent"] == 2
    g.set(_lib.FLD_STEP_COUNT, np.array([0, 25], np.int32)); e.set(o.FLD_STEP_COUNT, np.array([0, 25], np.int32))
    for s in range(30):       # arena 1 hits the cap after 15 steps and is frozen from then on
        g.orca_step(stats=True, freeze=True); e.orca_step(flags=o.F_STATS | o.F_FREEZE)
    H.assert_state_equal(g, e, "freeze")
    H.assert_stats_equal(g, e, "freeze")
    assert g.get(_lib.FLD_ARENA_DONE).tolist() == [0, 1] and g.stats()["agent_steps"] == N * (30 + 15)
    np.testing.assert_array_equal(g.get(_lib.FLD_ARRIVE_STEP), e.get(o.FLD_ARRIVE_STEP))
    g.close()


def test_scan_bound_does_not_trust_lists_written_by_the_caller():
    """The pair kernel bounds its neighbour scan with the agent's list of the previous step (any K distinct agents bound the
    K-th nearest).  A list the CALLER wrote through ca_set may name anything -- here the same agent ten times --: the next
    step must ignore it as a bound and still produce the exact lists; after a reset (stale but valid lists) the bound is
    merely looser."""
    A, N, K = 2, 400, 10
    p = H.scenario_params("crowd", N)
    g = H.make_gpu(A, N, "crowd", p, seed=12)
    e = H.make_oracle(A, N, "crowd", p, seed=12)
    assert g.launch_info()["lanes_per_agent"] == 2
    for s in range(5):
        g.orca_step(stats=True); e.orca_step(flags=o.F_STATS)
    H.assert_state_equal(g, e, "before")
    junk = np.zeros((A, K, N), np.int32)
    junk[:, :, :] = (np.arange(N)[None, None, :] + 1) % N          # every entry of agent i names agent i + 1
    cnt = np.full((A, N), K, np.int32)
    g.set(_lib.FLD_NB_IDX, junk); g.set(_lib.FLD_NB_COUNT, cnt)
    e.set(o.FLD_NB_IDX, np.ascontiguousarray(junk.transpose(0, 2, 1)))     # (the oracle keeps [A, N, K]; the count follows)
    g.orca_step(stats=True); e.orca_step(flags=o.F_STATS)
    H.assert_state_equal(g, e, "after a step from junk lists")
    g.reset(with_obs=False); e.reset(flags=0)                       # new positions, the lists stay (env.py:461-488)
    for s in range(3):
        g.orca_step(stats=True); e.orca_step(flags=o.F_STATS)
    H.assert_state_equal(g, e, "after a reset")
    H.assert_stats_equal(g, e, "junk lists")
    g.close()


@pytest.mark.parametrize("pair", [True, False], ids=["two-lanes", "one-lane"])
def test_pair_count_when_an_agent_is_thrown_across_the_arena(pair):
    """The collision statistic of large arenas counts overlapping pairs through the neighbour lists, which is exact as long as
    nobody moves farther in the step than the bound the argument uses.  A reset can drop two agents onto (nearly) the same spot;
    the linear programs then leave one of them at hundreds of times max_speed -- in the oracle as here, bit for bit -- and it
    lands next to agents that were never in its list.  The bound therefore is the arena's LARGEST SPEED OF THIS STEP, measured in
    the kernel; with max_speed in its place this arena (arena 109 of the soak with seeds + 2000) counted 66 pairs instead of 67."""
    import os
    N, seed, arena = 180, 2021, 109
    p = scenarios.bench_params(N, 5.0, 10)
    old = os.environ.get("CA_PAIR")
    if not pair:
        os.environ["CA_PAIR"] = "0"
    try:
        g = H.make_gpu(1, N, "crowd", p, seed=seed, arena_offset=arena)
    finally:
        if not pair:
            if old is None:
                del os.environ["CA_PAIR"]
            else:
                os.environ["CA_PAIR"] = old
    e = H.make_oracle(1, N, "crowd", p, seed=seed, arena_offset=arena)
    assert g.launch_info()["lanes_per_agent"] == (2 if pair else 1)
    g.reset(); e.reset()
    act = np.random.RandomState(seed).uniform(-0.6, 0.6, (256, N)).astype(np.float32)[arena:arena + 1]
    g.step(act, stats=True, autoreset=True)
    e.step(act, flags=o.F_OBS | o.F_STATS | o.F_AUTORESET)
    assert np.hypot(e.get(o.FLD_VEL_X), e.get(o.FLD_VEL_Y)).max() > 100.0       # the degenerate pair is there
    H.assert_state_equal(g, e, "thrown agent", obs=True, reward=True)
    H.assert_stats_equal(g, e, "thrown agent")
    assert e.stats()["collisions"] == 67
    g.close()
