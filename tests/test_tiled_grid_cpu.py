"""The scenes of tests/tiled_grid_scenes.py on the CPU oracle and the numpy model of the cell rule alone: each exercises what
tests/test_gpu_tiled_grid.py relies on it for.  Plus the header, the binding and the keyword of the grid handle, as far as they go
without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from oracle import oracle as o
from tests import helpers as H
from tests import nbr_scenes as NS
from tests import tiled_grid_scenes as G
from tests import tiled_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, K = 5.0, 10
# (agents, side of the table): the tables the GPU tests meet -- one the library picks for the size, and the forced 8 x 8
TABLES = [(300, 16), (1100, 32), (300, 8), (1100, 8)]


def _oracle_lists(N, px, py):
    p = G.params(N)
    assert p["neighbor_dist"] == ND and p["max_neighbors"] == K
    orc = H.make_oracle(1, N, "crowd", p, seed=1, polys=[])
    G.place(orc, o, px, py)
    orc.orca_step(flags=0)
    return orc.get(o.FLD_NB_COUNT)[0], orc.get(o.FLD_NB_IDX)[0]


def _same_lists(cnt, idx, rc, ri, what):
    assert np.array_equal(cnt, rc), what
    mask = np.arange(idx.shape[1])[None, :] < rc[:, None]
    assert np.array_equal(np.where(mask, idx, -1), np.where(mask, ri, -1)), what


def test_model_cell_rule():
    m = G.Model(16, 16, 2.5, ND)
    assert int(m.cell(0.0)) == 0 and int(m.cell(-1e-30)) == -1 and int(m.cell(-2.5)) <= -1 and int(m.cell(2.6)) == 1
    x = np.sort(np.random.RandomState(0).uniform(-300, 300, 4000).astype(np.float32))
    assert (np.diff(m.cell(x)) >= 0).all()                                   # monotone: what the choice of cells rests on
    b = m.bucket(x, x[::-1])
    assert b.min() >= 0 and b.max() < 256
    for v in (-37.3, -0.01, 0.0, 11.9):
        lo, hi = m.span(v)
        assert 4 <= hi - lo <= 5, (v, lo, hi)                                # at most 6 cells: fewer than the smallest side
        assert len(m.scanned(v, v)) == (hi - lo + 1) ** 2
    assert len(G.Model(8, 8, 0.5, ND).scanned(1.0, 1.0)) == 64               # a block wider than the table: every bucket once


@pytest.mark.parametrize("N,g", TABLES)
def test_aliasing_scene(N, g):
    m = G.Model(g, g, 0.5 * ND, ND)
    px, py = G.aliasing_scene(N, m)
    far, strangers = G.aliasing_claims(px, py, m)
    assert far > N and strangers > 0, (far, strangers)
    assert (px < 0).any() and (py < 0).any() and (px > 0).any()
    assert (m.cell(px) == -1).any() and (m.cell(px) == 0).any() and (m.cell(py) == -1).any() and (m.cell(py) == 0).any()
    cnt, idx = _oracle_lists(N, px, py)
    assert (cnt == K).mean() > 0.9
    rc, ri = NS.ref_lists(px[None], py[None], ND, K)
    _same_lists(cnt, idx, rc[0], ri[0], "oracle against App. A.2")
    mc, mi = m.lists(px, py, K)
    _same_lists(mc, mi, rc[0], ri[0], "the scanned buckets hold every neighbour")


@pytest.mark.parametrize("N,g", TABLES)
def test_boundary_scene(N, g):
    m = G.Model(g, g, 0.5 * ND, ND)
    px, py, pairs = G.boundary_scene(N, m)
    assert len(pairs) == 16 and sorted(set(p["off"] for p in pairs)) == [-1, 0]
    assert (px < 0).any() and (py < 0).any()
    assert any(p["c"] == 0 for p in pairs)                                   # the cell border at 0
    cnt, idx = _oracle_lists(N, px, py)
    rc, ri = NS.ref_lists(px[None], py[None], ND, K)
    _same_lists(cnt, idx, rc[0], ri[0], "oracle against App. A.2")
    assert G.boundary_claims(px, py, pairs, m, cnt, idx) == 16
    mc, mi = m.lists(px, py, K)
    _same_lists(mc, mi, rc[0], ri[0], "the scanned buckets hold every neighbour")
    # the planted agents see nobody else; the lattice has full lists
    planted = sorted(set(k for p in pairs for k in (p["i"], p["j"])))
    assert cnt[planted].max() <= 1 and (np.delete(cnt, planted) == K).mean() > 0.8


def test_lattice_has_ties_out_of_index_order():
    p = S.lattice_params()
    orc = H.make_oracle(1, S.LATTICE_N, "crowd", p, seed=3, polys=[])
    S.lattice_place(orc, o)
    px, py = orc.get(o.FLD_POS_X), orc.get(o.FLD_POS_Y)
    orc.orca_step(flags=0)
    cnt, idx = orc.get(o.FLD_NB_COUNT), orc.get(o.FLD_NB_IDX)
    assert S.lattice_ties(px, py, cnt, idx, p["max_neighbors"]) > 0
    m = G.Model(32, 32, 0.5 * p["neighbor_dist"], p["neighbor_dist"])
    # candidates of one cell row arrive with descending indices somewhere: the accept rule cannot rely on index order
    js = m.candidates(px[0], py[0], 0)
    assert (np.diff(js[np.argsort(m.bucket(px[0][js], py[0][js]), kind="stable")]) < 0).any()


def test_one_cell_scene():
    m = G.Model(16, 16, 0.5 * ND, ND)
    px, py = G.one_cell_positions(300, m)
    assert len(np.unique(m.bucket(px, py))) == 1


# ---- header and interface ---------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    assert int(re.search(r"#define\s+CA_CREATE_TILED_GRID\s+(\d+)u", hdr).group(1)) == _lib.CREATE_TILED_GRID == 4
    assert re.search(r"\bint\s+ca_tiled_grid_info\s*\(", hdr) and "ca_tiled_grid_info" in _lib.EXPORTS


def test_create_ex_validates_grid_flags_before_it_needs_a_device():
    L = _lib.load()
    h = C.c_void_p()
    cfg = lambda n, s=1: _lib.Config(n_arenas=1, n_agents=n, max_obst_neighbors=s, **scenarios.env_params())   # noqa: E731
    assert L.ca_create_ex(C.byref(cfg(8)), 4, 0, None, C.byref(h)) == -1 and not h.value
    assert b"tiled" in L.ca_last_error(None)                                 # the grid is the tiled path's
    for flags in (2, 8, 13, 6, 7):
        assert L.ca_create_ex(C.byref(cfg(8)), flags, 0, None, C.byref(h)) == -1 and not h.value, flags
        assert b"unknown create_flags" in L.ca_last_error(None)
    both = _lib.CREATE_TILED | _lib.CREATE_TILED_GRID
    assert both == 5
    assert L.ca_create_ex(C.byref(cfg(_lib.MAX_AGENTS_LARGE + 1)), both, 0, None, C.byref(h)) == -5
    assert b"out of range" in L.ca_last_error(None)
    assert L.ca_create_ex(C.byref(cfg(2000, 17)), both, 0, None, C.byref(h)) == -5
    assert b"no tiled form" in L.ca_last_error(None)


def test_vec_env_takes_tiled_grid():
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    assert hasattr(VecCollisionAvoidanceEnv, "tiled_grid_info")
    for kw in (dict(agent_params=dict(radius=0.4)), dict(agent_counts=[3])):
        with pytest.raises(ValueError, match="tiled"):
            VecCollisionAvoidanceEnv(1, 8, scenario=None, tiled="grid", **kw)
    with pytest.raises(ValueError, match="grid"):
        VecCollisionAvoidanceEnv(1, 8, scenario=None, tiled="cells")
