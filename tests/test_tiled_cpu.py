"""The scenes of tests/tiled_scenes.py on the CPU oracle alone: each exercises what tests/test_gpu_tiled.py relies on it for.
Plus the header, the binding and the drop-in classes of the tiled path, as far as they go without a GPU."""
import os
import re

import numpy as np
import pytest

from collision_avoidance_amd import _lib
from oracle import oracle as o
from tests import helpers as H
from tests import tiled_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_box(name):
    scenario, A, N, seed, p = S.box_scene(name)
    orc = H.make_oracle(A, N, scenario, p, seed=seed)
    full, pairs = 0, 0
    for act in S.box_actions(name):
        orc.step(act, flags=S.FULL)
        full += int((orc.get(o.FLD_NB_COUNT) == p["max_neighbors"]).sum())
    return orc, p, full / float(S.BOX_STEPS * A * N)


def test_crowd_1025_lists_are_full():
    orc, p, full = _run_box("crowd_1x1025")
    assert full > 0.90, full                       # the search keeps dropping candidates: the K-th key decides
    assert orc.stats()["obst_overflow"] == 0


def test_crowd_1500_collides_with_agents_and_walls():
    orc, p, full = _run_box("crowd_2x1500")
    st = orc.stats()
    assert full > 0.90, full
    assert st["collisions"] > 0 and st["obst_collisions"] > 0 and st["obst_overflow"] == 0, st


def test_circle_1100_runs():
    orc, p, full = _run_box("circle_1x1100")
    assert orc.stats()["agent_steps"] == S.BOX_STEPS * 1100 and orc.stats()["obst_overflow"] == 0


def test_doorway_1300_is_the_dense_case_of_the_pair_count():
    orc, p, full = _run_box("doorway_1x1300")
    st = orc.stats()
    assert st["collisions"] > 1000000 and st["obst_overflow"] == 0, st   # far more overlapping pairs than a list of 5 can name


def test_lattice_ties_and_lists_across_tiles():
    p = S.lattice_params()
    K = p["max_neighbors"]
    orc = H.make_oracle(1, S.LATTICE_N, "crowd", p, seed=3, polys=[])
    S.lattice_place(orc, o)
    px, py = orc.get(o.FLD_POS_X), orc.get(o.FLD_POS_Y)
    orc.orca_step(flags=0)
    cnt, idx = orc.get(o.FLD_NB_COUNT), orc.get(o.FLD_NB_IDX)
    assert (cnt == K).all()
    assert S.lattice_ties(px, py, cnt, idx, K) >= 1000                     # (conditions on the scene, not tolerances)
    tiles = [len(set((idx[0, i, :K] // S.TILE).tolist())) for i in range(S.LATTICE_N)]
    assert min(tiles) >= 3, min(tiles)


def test_largest_arena_on_the_oracle():
    N = _lib.MAX_AGENTS_LARGE
    p = H.scenario_params("crowd", N)
    orc = H.make_oracle(1, N, "crowd", p, seed=5)
    rng = np.random.RandomState(5)
    for _ in range(3):
        orc.step(rng.uniform(-1, 1, (1, N)).astype(np.float32), flags=S.FULL)
    assert orc.stats()["agent_steps"] == 3 * N and (orc.get(o.FLD_NB_COUNT) > 0).any()


def test_ends_scene_each_arena_stops_at_its_own_step():
    p = H.scenario_params("crowd", S.ENDS_N)
    orc = H.make_oracle(2, S.ENDS_N, "crowd", p, seed=9)
    S.ends_setup(orc, o)
    orc.rollout(S.ENDS_STEPS, flags=o.F_STATS | o.F_FREEZE)
    assert orc.get(o.FLD_ARENA_DONE).all()
    st = orc.get(o.FLD_ARENA_STATS)
    steps = (st[:, 7] >> np.uint64(32)).astype(np.int64)
    assert steps[0] != steps[1] and (steps < S.ENDS_STEPS).all() and (st[:, 6] > 0).all(), (steps, st[:, 6])


def test_overflow_scene_has_one_overflowing_agent():
    p = H.scenario_params("crowd", S.OVF_N)
    orc = H.make_oracle(1, S.OVF_N, "crowd", p, seed=2, max_obst_neighbors=1)
    S.overflow_place(orc, o)
    orc.orca_step(flags=0)
    assert orc.stats()["obst_overflow"] == 1 and S.OVF_AGENT > 2047


# ---- header and interface ---------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    assert int(re.search(r"#define\s+CA_MAX_AGENTS_LARGE\s+(\d+)", hdr).group(1)) == _lib.MAX_AGENTS_LARGE == 16384
    assert int(re.search(r"#define\s+CA_CREATE_TILED\s+(\d+)u", hdr).group(1)) == _lib.CREATE_TILED == 1
    assert int(re.search(r"#define\s+CA_MAX_AGENTS\s+(\d+)", hdr).group(1)) == _lib.MAX_AGENTS == 1024
    for name in ("ca_create_ex", "ca_tiled_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and name in _lib.EXPORTS, name


def test_create_ex_validates_before_it_needs_a_device():
    import ctypes as C
    from collision_avoidance_amd import scenarios
    L = _lib.load()
    h = C.c_void_p()
    cfg = lambda n, s=1: _lib.Config(n_arenas=1, n_agents=n, max_obst_neighbors=s, **scenarios.env_params())   # noqa: E731
    assert L.ca_create_ex(C.byref(cfg(8)), 2, 0, None, C.byref(h)) == -1 and not h.value                       # unknown flag bit
    assert L.ca_create_ex(C.byref(cfg(_lib.MAX_AGENTS_LARGE + 1)), _lib.CREATE_TILED, 0, None, C.byref(h)) == -5
    assert b"out of range" in L.ca_last_error(None)
    assert L.ca_create_ex(C.byref(cfg(2000, 17)), _lib.CREATE_TILED, 0, None, C.byref(h)) == -5
    assert b"no tiled form" in L.ca_last_error(None)
    assert L.ca_create_ex(C.byref(cfg(1025)), 0, 0, None, C.byref(h)) == -5 and b"out of range" in L.ca_last_error(None)
    assert L.ca_create(C.byref(cfg(1025)), 0, None, C.byref(h)) == -5 and b"out of range" in L.ca_last_error(None)


def test_vec_env_has_the_tiled_keyword():
    import inspect
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    sig = inspect.signature(VecCollisionAvoidanceEnv.__init__)
    assert sig.parameters["tiled"].default is False and hasattr(VecCollisionAvoidanceEnv, "tiled_info")
    for kw in (dict(agent_params=dict(radius=0.4)), dict(agent_counts=[3])):
        with pytest.raises(ValueError, match="tiled"):
            VecCollisionAvoidanceEnv(1, 8, scenario=None, tiled=True, **kw)


def _no_device():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_device(), reason="needs a machine without a HIP device")
def test_drop_in_classes_accept_more_than_1024_agents():
    """as tests/test_host_cpu.py::test_no_cpu_fallback_is_loud: without a device they fail for the device, not for the size"""
    from collision_avoidance_amd import alan, alan_train, envs
    for make in (lambda: envs.Collision_Avoidance_Env(numAgents=1025),
                 lambda: alan.Collision_Avoidance_Sim(numAgents=1025),
                 lambda: alan_train.MCMC_trainer(numAgents=1025, numRounds=2)):
        with pytest.raises(RuntimeError) as ei:
            make()
        assert "no HIP device" in str(ei.value) and "out of range" not in str(ei.value), str(ei.value)
