"""neighbor_dist and max_neighbors per agent, the parts that need no GPU: the oracle's simulator against the plain-numpy rule of
tests/agent_sensing_scenes.py on every agent-step of the recipe (the input guard of tests/test_gpu_agent_sensing.py: each kind of
truncation occurs often), the observation restatement's own cap of excusable rays, and the library's new symbols, its NULL-handle
answer and the Python keyword checks."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from collision_avoidance_amd import _lib
from oracle import oracle as o
from tests import agent_param_scenes as S
from tests import agent_sensing_scenes as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recipe():
    """the 16 scenes on the simulator, 40 steps: per step the positions the lists were built from and the lists"""
    sims = [Z.Sim(Z.draw(seed)) for seed in Z.SEEDS]
    steps = []
    for s in range(Z.STEPS):
        row = []
        for sim in sims:
            before = sim.positions()
            sim.step()
            row.append((before, sim.agent_neighbors()))
        steps.append(row)
    return sims, steps


def test_oracle_equals_the_numpy_rule_on_every_agent_step(recipe):
    sims, steps = recipe
    agent_steps = cut_k = cut_nd = emptied = asym = 0
    for row in steps:
        for sim, (pos, (cnt, idx)) in zip(sims, row):
            nd, K = sim.sc["neighbor_dist"], sim.sc["max_neighbors"]
            rc, ri, in_range = Z.ref_lists(pos, nd, K)
            assert np.array_equal(cnt, rc) and np.array_equal(idx, ri), (cnt, rc)
            _, _, wide = Z.ref_lists(pos, np.full(sim.n, Z.NEIGHBOR_DIST, Z.F), np.full(sim.n, Z.MAX_NEIGHBORS))
            agent_steps += sim.n
            cut_k += int(((in_range > K) & (K > 0)).sum())        # more agents in its range than it attends to
            cut_nd += int((wide > in_range).sum())                # agents within the handle's range that its own range leaves out
            emptied += int(((K == 0) & (in_range > 0)).sum())     # somebody in range, nobody attended to
            held = [set(idx[i, :cnt[i]]) for i in range(sim.n)]
            asym += sum(1 for i in range(sim.n) for j in held[i] if i not in held[j])
    print("agent-steps", agent_steps, "cut by max_neighbors_i", cut_k, "cut by neighbor_dist_i", cut_nd, "emptied by max_neighbors_i = 0", emptied,
          "one-sided list entries", asym)
    assert agent_steps == len(Z.SEEDS) * Z.N_AGENTS * Z.STEPS == 7680
    assert cut_k >= 1000 and cut_nd >= 1000 and emptied >= 1000, (cut_k, cut_nd, emptied)
    assert asym >= 1000, asym                                     # i sees j while j does not see i


def test_share_of_excusable_rays(recipe):
    """What the GPU file compares the observation against -- fp32 comp_laser with the 5.0 ray table on the segments of the agents'
    own lists -- against fp64 comp_laser on the same segments, every fifth step: the rays on which the two differ by more than
    OBS_TOL are the only ones a comparison may leave out, and they are at most OBS_MAX_LEFT_OUT of all."""
    rays = left_out = on_agent = 0
    for seed in Z.SEEDS:
        sim = Z.Sim(Z.draw(seed))
        for s in range(Z.STEPS):
            sim.step()
            if s % 5 != 4:
                continue
            pos, vel, goal, rad = sim.positions(), sim.velocities(), sim.sc["goal"], sim.sc["radius"]
            (nc, ni), (oc, oi), edges = sim.agent_neighbors(), sim.obstacle_neighbors(), sim.obstacle_edges()
            for i in range(sim.n):
                seg = S.observation_segments(pos, vel, rad, i, ni[i, :nc[i]], oi[i, :oc[i]], edges, np.float32)
                f32 = S.laser(pos, goal, seg, i, np.float32)
                f64 = S.laser(pos, goal, seg.astype(np.float64), i, np.float64)
                rays += 16
                left_out += int(S.excusable_rays(f32, f64).sum())
                on_agent += int(S.rays_on_agents(pos, goal, seg, 8 * nc[i], i).sum())
    print("rays", rays, "excusable", left_out, "on an agent's octagon", on_agent)
    assert rays == 16 * 12 * 16 * 8 and left_out <= S.OBS_MAX_LEFT_OUT * rays, (left_out, rays)


def test_boundary_scene_is_what_it_claims():
    """the planted pairs of the range and tie scene, on the numpy rule and on the simulator"""
    sc = Z.boundary_scene(24)
    cnt, idx, in_range = Z.ref_lists(sc["pos"], sc["neighbor_dist"], sc["max_neighbors"])
    d = Z.dsq_table(sc["pos"])
    r2 = Z.F(Z.F(Z.BOUNDARY_ND) * Z.F(Z.BOUNDARY_ND))
    from tests import nbr_scenes as NB
    assert [int(NB._ord(d[0, 1 + k]) - NB._ord(r2)) for k in range(4)] == list(Z.BOUNDARY_OFFSETS)
    assert sorted(idx[0, :cnt[0]]) == [1, 2] and all(0 in idx[j, :cnt[j]] for j in (1, 2, 3, 4))       # asymmetric at the boundary
    assert len({d[5, j].tobytes() for j in (8, 9, 10, 11)}) == 1 and list(idx[5, :cnt[5]]) == [6, 7, 8]
    sim = Z.Sim(dict(sc, **{k: np.full(24, v, Z.F) for k, v in S.DEFAULTS.items()}), uniform=True)
    sim.step()
    scnt, sidx = sim.agent_neighbors()
    assert np.array_equal(scnt, cnt) and np.array_equal(sidx, idx)


# ---- the library on the CPU ----------------------------------------------------------------------------------------------------
def test_library_exports_the_calls_and_a_null_handle_is_einval():
    L = _lib.load()
    for name in ("ca_set_agent_sensing", "ca_get_agent_sensing", "ca_agent_sensing_info"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    nd, k, flag = np.ones(4, np.float32), np.ones(4, np.int32), C.c_int32(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.ca_set_agent_sensing(None, p(nd), p(k), 16, 0) == -1
    assert L.ca_set_agent_sensing(None, None, None, 0, 0) == -1
    assert L.ca_get_agent_sensing(None, p(nd), p(k), 16, 0) == -1
    assert L.ca_agent_sensing_info(None, C.byref(flag)) == -1 and flag.value == 7


def test_header_declares_the_calls():
    h = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    for name in ("ca_set_agent_sensing", "ca_get_agent_sensing", "ca_agent_sensing_info"):
        assert re.search(r"\bint %s\(ca_env\* env," % name, h), name
    doc = h[h.index("The two remaining per-agent arguments of sim.addAgent"):h.index("int ca_set_agent_sensing")]
    for word in ("CAPACITIES", "CA_ESIZE", "CA_EINVAL", "CA_ERANGE", "asymmetric", "laser range stays", "CA_CREATE_TILED_PARAMS"):
        assert word in doc, word
    fields = h[h.index("enum ca_field {"):h.index("CA_FLD__COUNT")]
    assert len(re.findall(r"\bCA_FLD_\w+", fields)) == 26 and "SENSING" not in fields           # configuration, not state


def test_vec_env_interface_and_keyword_checks_need_no_device():
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv as V
    for name in ("set_agent_sensing", "agent_sensing", "clear_agent_sensing"):
        assert callable(getattr(V, name)), name
    assert list(inspect.signature(V.set_agent_sensing).parameters)[1:] == ["neighbor_dist", "max_neighbors"]
    assert "agent_sensing" in inspect.signature(V.__init__).parameters
    sens = dict(neighbor_dist=2.0, max_neighbors=3)
    for kw in (dict(tiled=True), dict(tiled="grid"), dict(tiled=True, tiled_wide=True)):
        with pytest.raises(ValueError, match="agent_sensing"):
            V(1, 1200, agent_sensing=sens, **kw)
    with pytest.raises(ValueError, match="agent_sensing"):
        V(2, 12, agent_sensing=dict(radius=0.3))
    with pytest.raises(ValueError, match="agent_sensing"):
        V(2, 12, agent_sensing=[2.0, 3])


def test_sensing_kernels_are_compiled_as_instantiations_of_their_own():
    """The compiler's metadata (tools/kernel_resources.py): the one-lane LDS-line-table kernel under the AgentSensing tag, alone and
    behind ArenaCounts, for every K class and workgroup size; the tiled solve launch for every K class, tile and search, and the
    close launch.  No spilled register; nothing else carries the tag -- no observation, advance, contact or ALAN kernel needs one:
    lists and counts are their only input from the search."""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    kr.ensure_asm()
    rows = {r["name"]: r for r in kr.parse()}
    want = ["step_kernel<%d, %d, 0, 16, false, %sAgentSensing>" % (k, bs, pre) for k in (5, 10, 16) for bs in (64, 128, 256, 512, 1024)
            for pre in ("", "ArenaCounts, ")]
    want += ["tiled_solve_kernel<%d, %d, %d, AgentSensing>" % (k, tile, search) for k in (5, 10, 16) for tile in (64, 128, 256) for search in (0, 1, 2)]
    want += ["tiled_close_kernel<AgentSensing>"]
    for name in want:
        assert name in rows, name
        assert rows[name]["vgpr_spill"] == 0, (name, rows[name])
    assert sorted(n for n in rows if "AgentSensing" in n) == sorted(want)
    # the twin adds no static LDS: the host's fit test (lds_static_bytes) holds for it as for the kernel it stands beside
    for k in (5, 10, 16):
        for bs in (64, 128, 256, 512, 1024):
            assert rows["step_kernel<%d, %d, 0, 16, false, AgentSensing>" % (k, bs)]["lds"] == rows["step_kernel<%d, %d, 0, 16, false, AgentParams>" % (k, bs)]["lds"]
