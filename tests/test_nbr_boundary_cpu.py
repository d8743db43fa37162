"""Neighbour lists at the edge of the neighbour range (App. A.2), CPU only: the oracle against a plain numpy fp32
restatement of App. A.2 on the boundary scenes of tests/nbr_scenes.py (pairs a few ulps inside and outside fl(nd^2),
pairs aimed across the uniform grid's cell boundaries, K-th slot ties, coincident agents, translated arenas), and the
scenes themselves: every aimed pair is a neighbour by App. A.2 and RC + 1 cells apart under the old fixed-block cell
rule -- the pairs that rule's scan never visits (tests/test_gpu_nbr_boundary.py runs the kernels on the same scenes)."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import helpers as H
from tests import nbr_scenes as NS

F = np.float32


@pytest.fixture(scope="module", params=sorted(NS.CASES))
def case(request):
    name = request.param
    px, py, feats = NS.case_scenes(name)
    return name, px, py, feats


def oracle_for(name, px, py, feats):
    N, nd, K, _ = NS.CASES[name]
    A = px.shape[0]
    p = H.scenario_params("crowd", N, neighbor_dist=nd, max_neighbors=K)
    if name in NS.WORLD_CASES:
        return H.make_oracle(A, N, "crowd", p, seed=3, polys=dict(per_arena=NS.two_octagons(px, py, feats, nd)),
                             max_obst_neighbors=16)
    return H.make_oracle(A, N, "crowd", p, seed=3, polys=[])


def test_oracle_lists_equal_numpy_app_a2(case):
    name, px, py, feats = case
    N, nd, K, _ = NS.CASES[name]
    orc = oracle_for(name, px, py, feats)
    orc.reset(px, py)
    np.testing.assert_array_equal(orc.get(o.FLD_POS_X), px)
    np.testing.assert_array_equal(orc.get(o.FLD_POS_Y), py)
    orc.orca_step(flags=o.F_OBS | o.F_STATS)
    rc, ri = NS.ref_lists(px, py, nd, K)
    oc, oi = orc.get(o.FLD_NB_COUNT), orc.get(o.FLD_NB_IDX)
    np.testing.assert_array_equal(oc, rc, err_msg=name + " nb_count")
    mask = np.arange(K)[None, None, :] < oc[:, :, None]
    np.testing.assert_array_equal(np.where(mask, oi, -1), ri, err_msg=name + " nb_idx")
    if name in NS.WORLD_CASES:
        assert orc.get(o.FLD_OBST_COUNT).max() > 4, "no agent has more than four edges in range"
        assert orc.stats()["obst_overflow"] == 0


def test_aimed_pairs_are_neighbours_rc_plus_one_cells_apart(case):
    name, px, py, feats = case
    N, nd, K, regime = NS.CASES[name]
    rc, ri = NS.ref_lists(px, py, nd, K)
    kinds = set()
    for a in range(px.shape[0]):
        g = NS.grid_for(px[a], py[a], nd, regime)
        assert g.RC == (2 if regime == "half" else 1), (name, g.cs, g.RC)
        if a == 0:
            assert abs(float(g.cs) - nd * (0.5 if regime == "half" else 1.0)) <= 4e-7 * nd, (name, g.cs)
        for f in feats[a]:
            if not f["kind"].startswith("aim"):
                continue
            kinds.add(f["kind"])
            i, j = f["idx"]
            assert NS.pair_dsq(px[a, i], py[a, i], px[a, j], py[a, j]) < F(F(nd) * F(nd)), f
            assert j in ri[a, i, :rc[a, i]] and i in ri[a, j, :rc[a, j]], (name, a, f)
            (cxi, cyi), (cxj, cyj) = g.cell(px[a, i], py[a, i]), g.cell(px[a, j], py[a, j])
            if f["kind"] == "aim_y":
                assert abs(cyi - cyj) == g.RC + 1 and cxi == cxj, (name, a, f, g.cell(px[a, i], py[a, i]), g.cell(px[a, j], py[a, j]))
            else:
                assert abs(cxi - cxj) == g.RC + 1, (name, a, f, (cxi, cyi), (cxj, cyj))
                assert abs(cyi - cyj) == (1 if f["kind"] == "aim_diag" else 0), (name, a, f, (cxi, cyi), (cxj, cyj))
    assert kinds == {"aim_x", "aim_y", "aim_diag"}, (name, kinds)


def test_boundary_distances_ties_and_coincident_agents(case):
    name, px, py, feats = case
    N, nd, K, regime = NS.CASES[name]
    r2 = F(F(nd) * F(nd))
    rc, ri = NS.ref_lists(px, py, nd, K)
    offs, kinds = set(), set()
    for a in range(px.shape[0]):
        g = NS.grid_for(px[a], py[a], nd, regime)
        for f in feats[a]:
            kinds.add(f["kind"])
            if f["kind"] == "dsq":
                i, j = f["idx"]
                d = NS.pair_dsq(px[a, i], py[a, i], px[a, j], py[a, j])
                assert NS._ord(d) - NS._ord(r2) == f["off"], f
                offs.add(f["off"])
                inside = f["off"] < 0
                assert (j in ri[a, i, :rc[a, i]]) == inside and (i in ri[a, j, :rc[a, j]]) == inside, (name, a, f)
            elif f["kind"] == "tie":
                c, tied = f["idx"][0], f["idx"][1:5]
                d = {NS.pair_dsq(px[a, c], py[a, c], px[a, t], py[a, t]).view(np.uint32).item() for t in tied}
                assert len(d) == 1, f                                     # bit-identical
                assert len({g.cell(px[a, t], py[a, t]) for t in tied}) == 4, f
                assert rc[a, c] == K and ri[a, c, K - 1] == min(tied), (name, a, f, ri[a, c])
                assert set(ri[a, c, :K - 1]) == set(f["idx"][5:]), f
            elif f["kind"] == "coincident":
                q = f["idx"]
                assert px[a, q[0]] == px[a, q[1]] == px[a, q[2]] and py[a, q[0]] == py[a, q[1]] == py[a, q[2]]
                for t in q:
                    assert set(q) - {t} <= set(ri[a, t, :rc[a, t]]), (name, a, f)
    assert {"tie", "coincident"} <= kinds or N < 64, (name, kinds)
    assert {0, 1, -1} <= offs or N < 64, (name, sorted(offs))
    for a, shift in enumerate(NS.TRANSLATIONS):                   # arena a is translated by about TRANSLATIONS[a]
        assert shift - 0.3 * 31.5 * nd - 1 < float(px[a].min()) < shift and float(px[a].max()) < 1e5


def test_scene_union_covers_every_feature():
    kinds, offs = set(), set()
    for name in ("ck16", "quad16"):
        px, py, feats = NS.case_scenes(name)
        for fa in feats:
            kinds |= {f["kind"] for f in fa}
            offs |= {f["off"] for f in fa if f["kind"] == "dsq"}
    assert {"aim_x", "aim_y", "aim_diag", "dsq", "coincident"} <= kinds, kinds
    assert offs & {0, 1, 2} and offs & set(range(-64, 0)), offs


def test_reference_is_app_a2_by_definition():
    """ref_lists on a hand-made arena: strict range, (distance, index) order, K cut."""
    px = np.array([[0.0, 3.0, -3.0, 0.0, 5.0, 0.0, 0.0]], F)
    py = np.array([[0.0, 4.0, 4.0, -5.0, 0.0, 0.0, 4.999999]], F)
    c, i = NS.ref_lists(px, py, 5.0, 3)
    assert c[0, 0] == 2 and list(i[0, 0]) == [5, 6, -1]      # 1 .. 4 at exactly fl(25): out; 5 at 0, 6 just inside
    c, i = NS.ref_lists(px, py, 5.0000005, 3)
    assert c[0, 0] == 3 and list(i[0, 0]) == [5, 6, 1]       # one ulp more range: four tie at 25, the lowest index wins
    c, i = NS.ref_lists(px, py, 5.0000005, 1)
    assert list(i[0, 5]) == [0] and list(i[0, 0]) == [5]
