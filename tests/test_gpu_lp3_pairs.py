"""The paired LP3 round of the one-wave register-line solve kernels (csrc/ca_lp.h lp3_pair_lds, the PairedLp3 kernels, CA_LP3_PAIRS)
against the oracle, bit for bit: state, neighbour lists, observation, reward and the per-arena counters after every step of the
scenes of tests/lp3_pair_scenes.py (tests/test_lp3_pairs_cpu.py asserts on the oracle alone that they put 0 .. 16, 17 .. 32 and more
than 32 infeasible agents into a wave, with obstacle lines and with parallel lines of both kinds).  Every handle has three arenas of
64 agents: the scene, the scene again under other actions, and the crowd the handle was made with -- in some step of every scene one
arena has 1 .. 16 infeasible agents while another has more than 16, so the four-lane round and the paired round run in one launch
(asserted on the oracle by tests/test_lp3_pairs_cpu.py).  CA_QUAD=0 keeps the small batch on the one-lane kernel; CA_LP3_PAIRS=1
asks for the twin whatever the library's default is, CA_LP3_PAIRS=0 for the kernel without the tag."""
import os

import numpy as np
import pytest

from collision_avoidance_amd import _lib
from oracle import oracle as o
from tests import helpers as H
from tests import lp3_pair_scenes as S

pytestmark = pytest.mark.gpu

F = np.float32
A = S.BATCH
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


def _gpu(K, pairs):
    g = _switched(dict(CA_QUAD="0", CA_LP3_PAIRS=pairs), lambda: H.make_gpu(A, S.N, "crowd", S.params(K), seed=S.SEED))
    info = g.launch_info()
    assert (info["lanes_per_agent"], info["block"]) == (1, 64), info
    assert g.nbr_seed_info() is True
    assert g.lp3_pairs_info() is (pairs == "1")
    return g


def _place(env, fld, name):
    sc = S.SCENES[name]()
    S.apply(env, fld, sc, arena=0)
    S.apply(env, fld, sc, arena=1)


_actions = S.batch_actions


@pytest.mark.parametrize("K", [10, 5])
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_scene_against_the_oracle(name, K):
    g = _gpu(K, "1")
    e = H.make_oracle(A, S.N, "crowd", S.params(K), seed=S.SEED)
    _place(g, _lib, name)
    _place(e, o, name)
    for s in range(S.STEPS):
        act = _actions(s)
        g.step(act, stats=True)
        e.step(act, flags=FLAGS)
        what = "%s K=%d step %d" % (name, K, s)
        H.assert_state_equal(g, e, what, obs=True, reward=True)
        H.assert_stats_equal(g, e, what)
        gs, cs = g.get(_lib.FLD_ARENA_STATS).astype(np.int64), e.get(o.FLD_ARENA_STATS).astype(np.int64)
        assert np.array_equal(gs[:, 1:5], cs[:, 1:5]), (what, "collisions | obst_collisions | goals_reached | obst_overflow per arena", gs[:, 1:5], cs[:, 1:5])
    g.close()


@pytest.mark.parametrize("name", ["corner", "mirror"])
def test_the_environment_switch_selects_the_kernel_without_the_tag(name):
    """CA_LP3_PAIRS=0 when the handle is made: step_kernel<..., SeededScan>, the same bits as the twin and as the oracle"""
    K = 10
    twin, plain = _gpu(K, "1"), _gpu(K, "0")
    assert plain.launch_info() == twin.launch_info()
    e = H.make_oracle(A, S.N, "crowd", S.params(K), seed=S.SEED)
    for env, fld in ((twin, _lib), (plain, _lib), (e, o)):
        _place(env, fld, name)
    for s in range(20):
        act = _actions(s)
        twin.step(act, stats=True)
        plain.step(act, stats=True)
        e.step(act, flags=FLAGS)
    H.assert_state_equal(twin, e, name + " twin", obs=True, reward=True)
    H.assert_state_equal(plain, e, name + " plain", obs=True, reward=True)
    H.assert_stats_equal(twin, e, name + " twin")
    H.assert_stats_equal(plain, e, name + " plain")
    twin.close(); plain.close()
