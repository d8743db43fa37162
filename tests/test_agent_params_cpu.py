"""The input guard of tests/test_gpu_agent_params.py, on the CPU oracle alone: the seeded scenes of tests/agent_param_scenes.py
(ORCA parameters per agent, as the reference passes them to every addAgent call, collision_avoidence_env.py:126-133) reach the
branches that per-agent parameters enter -- LP3, colliding agents, every obstacle projection -- without overflowing a list of 16
obstacle neighbours, differ from the same scenes with uniform parameters, and their observation restatement (the octagon of
the NEIGHBOUR's radius) stays within its own cap of excusable rays.  Plus the parts of the feature that need no GPU: the
declarations of include/ca_env.h and the ctypes binding."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

from collision_avoidance_amd import _lib
from oracle import oracle as o
from tests import agent_param_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_all(uniform=False):
    sims = [S.Sim(S.draw(seed), uniform=uniform) for seed in S.SEEDS]
    top = 0
    for _ in range(S.STEPS):
        for sim in sims:
            sim.step()
            top = max(top, int(sim.obstacle_neighbors()[0].max()))
    return sims, top


def test_recipe_reaches_the_branches_that_the_parameters_enter():
    o.branch_counts(reset=True)
    sims, top = _run_all()
    br = o.branch_counts(reset=True)
    proj = {k: v for k, v in br.items() if k.startswith("OBST_PROJ_")}
    print("largest obstacle-neighbour list", top, "LP3_ENTERED", br["LP3_ENTERED"], "with obstacle lines", br["LP3_ENTERED_WITH_OBST_LINES"],
          "AGENT_COLLISION", br["AGENT_COLLISION"], proj)
    for sim in sims:
        assert np.isfinite(sim.positions()).all() and np.isfinite(sim.velocities()).all()
    assert top <= S.MAX_OBST_NEIGHBORS, top
    assert br["LP3_ENTERED"] >= 1000 and br["AGENT_COLLISION"] >= 1000, br
    assert len(proj) >= 5 and all(v >= 100 for v in proj.values()), proj


def test_uniform_parameters_end_elsewhere():
    """The parameters matter: the same seeds with the handle's constants for every agent end elsewhere, for every agent."""
    mixed, _ = _run_all()
    uni, _ = _run_all(uniform=True)
    for a, b in zip(mixed, uni):
        assert (np.abs(a.positions() - b.positions()).max(axis=1) > 0).all()


def test_observation_restatement_stays_within_its_flip_cap():
    """What test 3 of the GPU file compares against -- fp32 comp_laser on segments built from (float)octagon_table(r_nb) -- against
    fp64 comp_laser on the same segments: the rays on which the two themselves differ by more than 3e-5 (a hit that flips under
    rounding) are the only ones the GPU comparison may leave out, and they are at most 1 % here; at least 1000 rays end on an
    agent's octagon."""
    sims, _ = _run_all()
    rays = left_out = on_agent = 0
    for sim in sims:
        pos, vel, goal, rad = sim.positions(), sim.velocities(), sim.sc["goal"], sim.sc["radius"]
        (nc, ni), (oc, oi), edges = sim.agent_neighbors(), sim.obstacle_neighbors(), sim.obstacle_edges()
        for i in range(sim.n):
            seg32 = S.observation_segments(pos, vel, rad, i, ni[i, :nc[i]], oi[i, :oc[i]], edges, np.float32)
            f32 = S.laser(pos, goal, seg32, i, np.float32)
            f64 = S.laser(pos, goal, seg32.astype(np.float64), i, np.float64)
            bad = S.excusable_rays(f32, f64)
            rays += 16
            left_out += int(bad.sum())
            on_agent += int(S.rays_on_agents(pos, goal, seg32, 8 * nc[i], i).sum())
    print("rays", rays, "excusable", left_out, "on an agent's octagon", on_agent)
    assert left_out <= S.OBS_MAX_LEFT_OUT * rays, (left_out, rays)
    assert on_agent >= 1000, on_agent


def test_header_declares_the_calls_and_says_what_stays_per_handle():
    h = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    for name in ("ca_set_agent_params", "ca_get_agent_params"):
        assert re.search(r"\bint %s\(ca_env\* env," % name, h) and name in _lib.EXPORTS, name
    doc = h[h.index("Replaces the per-agent arguments of sim.addAgent"):h.index("int ca_set_agent_params")]
    assert "neighbor_dist and max_neighbors stay per handle" in doc and "CA_ESIZE" in doc and "CA_EINVAL" in doc and "CA_ERANGE" in doc
    fields = h[h.index("enum ca_field {"):h.index("CA_FLD__COUNT")]
    assert len(re.findall(r"\bCA_FLD_\w+", fields)) == 26 and "RADIUS" not in fields and "PARAM" not in fields   # configuration, not state


def test_vec_env_has_the_interface():
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv as V
    import inspect
    for name in ("set_agent_params", "agent_params", "clear_agent_params"):
        assert callable(getattr(V, name)), name
    assert list(inspect.signature(V.set_agent_params).parameters)[1:] == list(S.PARAM_NAMES)
    assert "agent_params" in inspect.signature(V.__init__).parameters


def test_per_agent_kernels_are_compiled_as_instantiations_of_their_own():
    """The compiler's metadata (tools/kernel_resources.py): the one-lane LDS-line-table kernel with the AgentParams tag for every
    K class and workgroup size, three observation kernels; no spilled register, no scratch in the observation ones (the table
    kernels keep LP3's projected lines in a private array by design); beside them the tag names the per-agent instantiations of the
    tiled path's three kernel templates (csrc/ca_tiled.h), and nothing else carries it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    kr.ensure_asm()
    rows = {r["name"]: r for r in kr.parse()}
    want = ["step_kernel<%d, %d, 0, 16, false, AgentParams>" % (k, bs) for k in (5, 10, 16) for bs in (64, 128, 256, 512, 1024)]
    obs = ["obs_kernel<256, false, false, AgentParams>", "obs_kernel<256, false, true, AgentParams>", "obs_kernel<256, true, false, AgentParams>"]
    for name in want + obs:
        assert name in rows, name
        assert rows[name]["vgpr_spill"] == 0, (name, rows[name])
    for name in obs:
        assert rows[name]["scratch"] == 0 and rows[name]["sgpr_spill"] == 0, (name, rows[name])
    tiled = ["tiled_solve_kernel<%d, %d, %d, AgentParams>" % (k, tile, search) for k in (5, 10, 16) for tile in (64, 128, 256) for search in (0, 1, 2)] + \
            ["tiled_advance_kernel<false, AgentParams>", "tiled_advance_kernel<true, AgentParams>", "tiled_close_kernel<AgentParams>"]
    assert sorted(n for n in rows if "AgentParams" in n) == sorted(want + obs + tiled)
