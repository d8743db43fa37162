"""CA_CREATE_TILED_WIDE without a device: the header, the binding, the flag validation of ca_create_ex (which runs before a device is
needed), the keyword rules of VecCollisionAvoidanceEnv, the compiled kernels' resources, and the INPUT GUARD of
tests/test_gpu_tiled_wide.py: every sequence of tests/tiled_wide_scenes.py on the oracle alone, over exactly the steps and seeds
the GPU test runs -- lists above 16, and none that overflows unless the scene is there to overflow."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from collision_avoidance_amd import vec_env  # noqa: F401  (PyTorch before the library, the order VecCollisionAvoidanceEnv loads them in)
from oracle import oracle as o
from tests import tiled_wide_scenes as T
from tests import wide_worlds as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -2


def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    assert int(re.search(r"#define\s+CA_CREATE_TILED_WIDE\s+(\d+)u", hdr).group(1)) == _lib.CREATE_TILED_WIDE == 32
    assert T.PLAIN == _lib.CREATE_TILED | _lib.CREATE_TILED_WIDE == 33
    assert T.GRID == _lib.CREATE_TILED | _lib.CREATE_TILED_GRID | _lib.CREATE_TILED_WIDE == 37


def _create(flags, S=1):
    L = _lib.load()
    h = C.c_void_p()
    cfg = _lib.Config(n_arenas=1, n_agents=8, max_obst_neighbors=S, **scenarios.env_params())
    rc = L.ca_create_ex(C.byref(cfg), flags, 0, None, C.byref(h))
    msg = L.ca_last_error(None).decode() if rc else ""
    if rc == 0:
        assert h.value and L.ca_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def test_create_ex_validates_the_flag_before_it_needs_a_device():
    for flags in (33, 37):                                                    # valid: what is left is the device
        for S in (1, 16, 17, 64):
            rc, msg = _create(flags, S)
            assert rc in (0, ENODEV), (flags, S, rc, msg)
    rc, msg = _create(32)
    assert rc == EINVAL and "CA_CREATE_TILED_WIDE" in msg and "without CA_CREATE_TILED" in msg, msg
    for flags in (49, 53):
        rc, msg = _create(flags)
        assert rc == EINVAL and "per-agent parameters go with obstacle lists of up to 16" in msg and "ordinary handles" in msg, (flags, msg)
    for flags in (34, 41, 35, 45, 64, 97, 33 | 128):                          # bit 2, bit 8, bit 64 and above stay unknown
        rc, msg = _create(flags)
        assert rc == EINVAL and "unknown create_flags" in msg, (flags, msg)
    for flags in (1, 5):                                                      # without the flag: today's refusal, a range error
        rc, msg = _create(flags, 17)
        assert rc == -5 and "no tiled form" in msg, (flags, msg)


def test_vec_env_keyword_rules():
    import inspect
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    sig = inspect.signature(VecCollisionAvoidanceEnv.__init__)
    assert sig.parameters["tiled_wide"].default is False
    assert "tiled_wide" in VecCollisionAvoidanceEnv.__doc__
    with pytest.raises(ValueError, match="tiled_wide"):
        VecCollisionAvoidanceEnv(1, 8, scenario=None, tiled_wide=True, max_obst_neighbors=20)
    for tiled in (True, "grid"):
        with pytest.raises(ValueError, match="tiled_wide"):
            VecCollisionAvoidanceEnv(1, 8, scenario=None, tiled=tiled, tiled_wide=True, tiled_params=True)


def test_drop_in_env_asks_for_the_flag_with_wide_lists_above_1024_agents(monkeypatch):
    """Collision_Avoidance_Env asks for the tiled path on its own above 1024 agents, and for the wide lists on it when its
    max_obst_neighbors exceeds 16 (the construction is intercepted: no device)"""
    from collision_avoidance_amd import envs
    seen = []

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.append(kw)
        raise Stop()
    monkeypatch.setattr(envs, "VecCollisionAvoidanceEnv", fake)
    for n, s, want in ((1100, 40, (True, True)), (1100, 16, (True, False)), (1100, None, (True, False)), (64, 40, (False, False))):
        with pytest.raises(Stop):
            envs.Collision_Avoidance_Env(n, max_obst_neighbors=s)
        assert (bool(seen[-1]["tiled"]), bool(seen[-1]["tiled_wide"])) == want, (n, s, seen[-1])


def _rows():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    kr.ensure_asm()
    return kr.parse()


def test_wide_tiled_kernels_are_compiled():
    rows = {r["name"]: r for r in _rows()}
    want = ["tiled_solve_kernel<%d, %d, %d, WideObstLists>" % (k, tile, search) for k in (5, 10, 16) for tile in (64, 128, 256)
            for search in (0, 1, 2)]
    for name in want:
        assert name in rows, name
        # LP3's projected lines: a private array of KMAX + 64 lines of 16 B (by design, as in every table kernel); no spilled register
        k = int(name.split("<")[1].split(",")[0])
        assert rows[name]["scratch"] >= (k + 64) * 16 and rows[name]["vgpr_spill"] == 0, (name, rows[name])
        assert rows[name]["lds"] == 0, (name, rows[name])                     # (all of its LDS is dynamic: the host sizes and checks it)
    name = "obs_kernel<256, true, false, WideObstLists>"
    assert name in rows, name
    assert rows[name]["scratch"] == 0 and rows[name]["vgpr_spill"] == 0 and rows[name]["sgpr_spill"] == 0, rows[name]
    # the tag stands where the issue of the wide lists put it and nowhere else: never beside AgentParams
    tagged = sorted(n for n in rows if "WideObstLists" in n)
    assert tagged == sorted(want + [name, "obs_kernel<256, false, false, WideObstLists>", "obs_kernel<256, false, true, WideObstLists>"]), tagged
    assert not [n for n in tagged if "AgentParams" in n or "ArenaCounts" in n]


def test_tile_arithmetic_of_the_header():
    """tile x ((K + S) x 16 + 8) bytes: the default tile of 64 holds every K and S; 128 holds K = 10 with S = 64 and not K = 16"""
    lds = lambda tile, K, S: tile * ((K + S) * 16 + 8)   # noqa: E731
    assert lds(128, 10, 64) == 152576 <= T.LDS_PER_CU < lds(128, 16, 64) == 164864
    assert max(lds(T.TILE, K, S) for K in range(17) for S in range(17, 65)) == 82432 <= T.LDS_PER_CU


# ---- the input guard ---------------------------------------------------------------------------------------------------------------
def test_guard_halls_have_the_edges_the_scenes_say():
    for name, (N, args, steps, edges) in T.HALLS.items():
        assert T.n_edges(T.hall(name)) == edges, name
    assert T.n_edges(T.dense_hall()) == T.DENSE["edges"]


def test_guard_rings():
    c = T.ring_oracle(64, 64)
    assert T.run_ring([], c) == 64 and c.stats()["obst_overflow"] == 0
    c = T.ring_oracle(24, 20)
    assert T.run_ring([], c) == 20 and c.stats()["obst_overflow"] > 0


@pytest.mark.parametrize("K", [5, 10, 16])
def test_guard_hall_130(K):
    N, _, steps, _ = T.HALLS["130"]
    e = T.make_oracle(2, N, T.hall_worlds("130"), 64, max_neighbors=K)
    top = T.run_alternate([], e, 2, N, steps)
    assert e.stats()["obst_overflow"] == 0 and 16 < top <= 64, top
    print("hall 130, K = %d: largest list %d" % (K, top))


def test_guard_hall_300():
    N, _, steps, _ = T.HALLS["300"]
    e = T.make_oracle(2, N, T.hall_worlds("300"), 64)
    top = T.run_alternate([], e, 2, N, steps)
    assert e.stats()["obst_overflow"] == 0 and 16 < top <= 64, top
    print("hall 300: largest list", top)


def test_guard_hall_1100():
    N, _, steps, _ = T.HALLS["1100"]
    e = T.make_oracle(1, N, T.hall_worlds("1100", 1), 64)
    top = T.run_alternate([], e, 1, N, steps, every=5)
    c = e.get(o.FLD_OBST_COUNT)
    assert e.stats()["obst_overflow"] == 0 and 16 < top <= 64, top
    assert (c[0, 1024:] > 16).any()                                            # agents with ids above 1023 hold wide lists
    print("hall 1100: largest list %d, %d agents above 16" % (top, int((c > 16).sum())))


def test_guard_hall_b_of_the_ordinary_wide_handle():
    e = T.make_oracle(2, 100, W.hall_b_worlds(2), 64)
    top = T.run_alternate([], e, 2, 100, 60, every=60)
    assert e.stats()["obst_overflow"] == 0 and 16 < top <= 64, top


def test_guard_dense_hall_overflows_lists_of_64():
    N = T.DENSE["N"]
    e = T.make_oracle(1, N, [T.dense_hall()], 64)
    top = T.run_alternate([], e, 1, N, T.DENSE["steps"], every=20)
    assert e.stats()["obst_overflow"] > 0 and top == 64, (top, e.stats())


def test_guard_the_rest_of_a_tiled_handle():
    N = 130
    worlds = T.hall_worlds("130")
    e = T.make_oracle(2, N, worlds, 64)                                        # rollout(30), then 5 traced steps
    top = 0
    for s in range(35):
        e.orca_step(flags=o.F_STATS)
        top = max(top, int(e.get(o.FLD_OBST_COUNT).max()))
    assert e.stats()["obst_overflow"] == 0 and 16 < top <= 64, top
    e = T.make_oracle(2, N, worlds, 64)
    top = T.run_alan([], e)
    assert e.stats()["obst_overflow"] == 0 and 16 < top <= 64, top
    e = T.make_oracle(2, N, worlds, 64, max_step=40)
    tops = T.run_resets([], e, 2, N)
    assert e.stats()["obst_overflow"] == 0 and e.stats()["episodes"] >= 2 and all(16 < t <= 64 for t in tops), (tops, e.stats())
    e = T.make_oracle(2, N, worlds, 64)
    tops = T.run_worlds_come_and_go([], e, 2, N, worlds)
    assert e.stats()["obst_overflow"] == 0 and 16 < tops[0] <= 64 and tops[1] <= 4 and 16 < tops[2] <= 64, tops


def test_guard_largest_size():
    L = T.LARGEST
    N, S = L["N"], L["S"]
    p = T.H.scenario_params("crowd", N)
    e = T.H.make_oracle(1, N, "crowd", p, seed=8, polys=T.largest_world(), max_obst_neighbors=S)
    T.largest_place(e, o)
    for s in range(2):
        e.orca_step(flags=o.F_STATS)
        c = e.get(o.FLD_OBST_COUNT)
        assert [int(c[0, i]) for i in L["agents"]] == [24, 24, 24] and c.max() == 24, s
    assert e.stats()["obst_overflow"] == 0
