"""Neighbour lists at the edge of the neighbour range on every scan path of the kernels (App. A.2), against the oracle
and against the numpy restatement of tests/nbr_scenes.py, on scenes whose pairs sit a few ulps inside or outside
fl(nd^2), next to the cell boundaries of the uniform grid (csrc/ca_nbr.h), tied for the K-th slot across cells, or
coincident, in arenas translated up to 9e4.  Each case asserts the path it runs on; for the pair kernel a second step
runs with the scan bound taken from the previous list (csrc/ca_pair.h)."""
import os

import numpy as np
import pytest

from oracle import oracle as o
from tests import helpers as H
from tests import nbr_scenes as NS

pytestmark = pytest.mark.gpu

# name -> (switches, lanes_per_agent, block)
PATHS = {
    "quad16": (dict(CA_QUAD="1"), 4, 64), "quad64": (dict(CA_QUAD="1"), 4, 256), "quad128": (dict(CA_QUAD="1"), 4, 512),
    "ck16": (dict(CA_QUAD="0"), 1, 64), "ck64": (dict(CA_QUAD="0"), 1, 64),                # 32-bit composite keys
    "scan65": (dict(CA_QUAD="0"), 1, 128), "scan100": (dict(CA_QUAD="0"), 1, 128),          # the 64-bit scan
    "grid32_250_k16": (dict(CA_QUAD="0"), 1, 256),               # one lane, GMAX 32: the LDS line table (K 16)
    "grid32_300_world": (dict(CA_QUAD="0"), 1, 512),             # ... more than four obstacle neighbours (SMX 16)
    "grid32_300_help": (dict(CA_QUAD="0", CA_PAIR="0"), 1, 512),  # one lane, CA_PAIR=0: register lines, SMX 4, GMAX 32
    "grid16_600": (dict(CA_QUAD="0"), 1, 1024), "grid16_1024": (dict(CA_QUAD="0"), 1, 1024),   # one lane, GMAX 16
    "pair192": ({}, 2, 512), "pair300": ({}, 2, 1024), "pair512": ({}, 2, 1024),
}
assert sorted(PATHS) == sorted(NS.CASES)


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


def _lists_equal(gpu, rc, ri, what):
    gc, gi = gpu.neighbor_lists()
    K = ri.shape[2]
    mask = np.arange(K)[None, None, :] < gc[:, :, None]
    bad = np.argwhere(gc != rc)
    assert bad.size == 0, "%s: nb_count differs from App. A.2 for %d agents; first (arena, agent) %s: gpu %d numpy %d" % (
        what, len(bad), tuple(bad[0]), gc[tuple(bad[0])], rc[tuple(bad[0])])
    np.testing.assert_array_equal(np.where(mask, gi, -1), ri, err_msg=what + ": nb_idx differs from App. A.2")


@pytest.mark.parametrize("name", sorted(NS.CASES))
def test_boundary_lists_on_every_scan_path(name):
    N, nd, K, _ = NS.CASES[name]
    env, lanes, block = PATHS[name]
    px, py, feats = NS.case_scenes(name)
    A = px.shape[0]
    p = H.scenario_params("crowd", N, neighbor_dist=nd, max_neighbors=K)
    if name in NS.WORLD_CASES:
        kw = dict(polys=dict(per_arena=NS.two_octagons(px, py, feats, nd)), max_obst_neighbors=16)
    else:
        kw = dict(polys=[])
    gpu = _switched(env, lambda: H.make_gpu(A, N, "crowd", p, seed=3, **kw))
    info = gpu.launch_info()
    assert (info["lanes_per_agent"], info["block"]) == (lanes, block), (name, info)
    orc = H.make_oracle(A, N, "crowd", p, seed=3, **kw)
    gpu.reset(px, py)
    orc.reset(px, py, flags=o.F_OBS)
    gpu.orca_step(with_obs=True, stats=True)
    orc.orca_step(flags=o.F_OBS | o.F_STATS)
    rc, ri = NS.ref_lists(px, py, nd, K)
    _lists_equal(gpu, rc, ri, name + " orca_step")
    H.assert_state_equal(gpu, orc, name + " orca_step", obs=True, reward=True)
    H.assert_stats_equal(gpu, orc, name + " orca_step")
    if name in NS.WORLD_CASES:
        assert gpu.obstacle_neighbor_lists()[0].max() > 4
    rng = np.random.RandomState(7)
    for s in range(2 if lanes == 2 else 1):   # (pair kernel: the second step bounds its scan by the previous list)
        act = rng.uniform(-1.0, 1.0, (A, N)).astype(np.float32)
        gx, gy = gpu.get(H._lib_fld("POS_X")), gpu.get(H._lib_fld("POS_Y"))
        gpu.step(act, stats=True)
        orc.step(act, flags=o.F_OBS | o.F_STATS)
        rc, ri = NS.ref_lists(gx, gy, nd, K)
        _lists_equal(gpu, rc, ri, "%s step %d" % (name, s))
        H.assert_state_equal(gpu, orc, "%s step %d" % (name, s), obs=True, reward=True)
        H.assert_stats_equal(gpu, orc, "%s step %d" % (name, s))
    gpu.close()
