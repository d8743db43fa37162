"""The static edge grid's host side, without a device (ca_edge_grid_build; csrc/ca_edge_grid_host.h): the table builder checked by
brute force against a numpy fp32 restatement of the cell expression (include/ca_env.h) and of distSqPointSegment (csrc/ca_math.h),
kept in tests/edge_grid_scenes.py.  For every seeded point the table is walked the way the kernels walk it, with the corner rule:
the walk must meet every edge whose fp32 distance test passes, and no edge twice."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from collision_avoidance_amd import _lib
from tests import edge_grid_scenes as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("ca_tiled_edge_grid", "ca_tiled_edge_grid_info", "ca_edge_grid_build")


# ---- 1. header and binding agree -------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    L = _lib.load()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.EXPORTS and getattr(L, name).restype is C.c_int, name
    m = re.search(r"typedef struct ca_edge_grid_desc \{(.*?)\} ca_edge_grid_desc;", text, re.S)
    fields = re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f for f, _ in _lib.EdgeGridDesc._fields_], fields
    assert "fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1))" in text            # the cell expression, verbatim
    for src in ("ca_edge_grid_host.h", "ca_tiled.h"):
        assert "fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1))" in open(os.path.join(ROOT, "collision_avoidance_amd", "csrc", src)).read(), src
    assert int(re.search(r"#define CA_EDGE_GRID_MAX_EDGES (\d+)", text).group(1)) == _lib.EDGE_GRID_MAX_EDGES
    assert "#define CA_EDGE_GRID_MAX_ENTRIES (1 << 22)" in text and _lib.EDGE_GRID_MAX_ENTRIES == 1 << 22


# ---- 2. the builder by brute force ---------------------------------------------------------------------------------------------------
SETS = E.edge_sets()


@pytest.mark.parametrize("name", sorted(SETS))
def test_walk_meets_every_edge_in_range_once(name):
    edges, R = SETS[name]
    d, cs, en = _lib.edge_grid_build(edges, R)
    if name == "one_line":
        assert d.gy == 1 and d.gx > 1, (d.gx, d.gy)                                     # a degenerate extent: one row of cells
    if name in ("hall", "translated"):
        spans = [(int(w) >> 16 & 0xFF, int(w) >> 24) for w in en if int(w) & 0xFFFF < 4]
        assert (0, 0) in spans and d.n_entries > len(edges) + 2 * (d.gx + d.gy - 4)        # the box's edges run the table's whole sides
    px, py = E.points_for(edges, d, R, n=2000, seed=len(name))
    assert len(px) >= 2000
    rangeSq = F(F(R) * F(R))
    dsq = E.dist_sq_point_segment(edges, px, py)
    inside = dsq < rangeSq
    bits = dsq.view(np.int32).astype(np.int64) - int(rangeSq.view(np.int32))
    assert (np.abs(bits) <= 1).sum() > 50 or name == "translated", "no point within an ulp of the range"
    assert inside.any(axis=1).sum() > 200 and (~inside.any(axis=1)).sum() > 200
    most = 0
    for k in range(len(px)):
        got, ncell = E.walk(d, cs, en, px[k], py[k], R)
        most = max(most, ncell)
        assert len(np.unique(got)) == len(got), "point %d (%r, %r): an edge twice: %s" % (k, px[k], py[k], np.sort(got))
        missed = np.setdiff1d(np.flatnonzero(inside[k]), got)
        assert missed.size == 0, "point %d (%r, %r): edges %s pass the distance test and are not met" % (k, px[k], py[k], missed)
        wall = E.walk(d, cs, en, px[k], py[k], 0.5, dedupe=False)[0]                      # the wall test's walk: radius 0.5 < range
        hit = np.flatnonzero(dsq[k] < F(0.25))
        assert np.setdiff1d(hit, wall).size == 0, "point %d: the wall test misses edges %s" % (k, np.setdiff1d(hit, wall))
    assert most <= 16                                                                       # (3 x 3 but for a rounding of ics: never the table)


def test_points_that_are_no_numbers_stay_inside_the_table():
    edges, R = SETS["hall"]
    d, cs, en = _lib.edge_grid_build(edges, R)
    for x, y in ((np.nan, 1.0), (np.inf, -np.inf), (3e38, -3e38), (-1e30, np.nan)):
        got, ncell = E.walk(d, cs, en, x, y, R)
        assert ncell >= 1 and (got < len(edges)).all()


# ---- 3. CSR consistency ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETS))
def test_csr_is_consistent(name):
    edges, R = SETS[name]
    L = _lib.load()
    sized = _lib.EdgeGridDesc()
    assert L.ca_edge_grid_build(edges.ctypes.data_as(C.c_void_p), len(edges), R, C.byref(sized), None, 0, None, 0) == 0
    d, cs, en = _lib.edge_grid_build(edges, R)
    for f, _ in _lib.EdgeGridDesc._fields_:
        assert getattr(sized, f) == getattr(d, f), f                                      # the NULL-array call sizes the filled one
    assert 1 <= d.gx <= 256 and 1 <= d.gy <= 256 and len(cs) == d.gx * d.gy + 1 and len(en) == d.n_entries
    assert cs[0] == 0 and cs[-1] == d.n_entries and (np.diff(cs.astype(np.int64)) >= 0).all()
    w = en.astype(np.int64)
    assert ((w & 0xFFFF) < len(edges)).all() and (((w >> 16) & 0xFF) < d.gx).all() and ((w >> 24) < d.gy).all()
    cell_of = np.repeat(np.arange(d.gx * d.gy), np.diff(cs.astype(np.int64)))
    assert (((w >> 16) & 0xFF) <= cell_of % d.gx).all() and ((w >> 24) <= cell_of // d.gx).all()   # the corner is the rectangle's low one
    assert sorted(np.unique(w & 0xFFFF)) == list(range(len(edges)))                        # every edge is somewhere
    cs_x, cs_y = 1.0 / d.ics_x, 1.0 / d.ics_y
    assert cs_x >= R * (1 - 1e-6) and cs_y >= R * (1 - 1e-6) and d.margin > 0
    small = np.zeros(2, np.uint32)
    assert L.ca_edge_grid_build(edges.ctypes.data_as(C.c_void_p), len(edges), R, C.byref(sized), small.ctypes.data_as(C.c_void_p), 1,
                                small.ctypes.data_as(C.c_void_p), 1) == -4               # CA_ESIZE: nothing written past the caps


def test_no_edges_is_one_empty_cell():
    d, cs, en = _lib.edge_grid_build(np.zeros((0, 4), F), 2.0)
    assert (d.gx, d.gy, d.n_entries) == (1, 1, 0) and list(cs) == [0, 0] and len(en) == 0


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = _lib.load()
    d = _lib.EdgeGridDesc()
    many = np.zeros((65536, 4), F)
    many[:, 0] = np.arange(65536)
    many[:, 2] = many[:, 0] + 0.5
    assert L.ca_edge_grid_build(many.ctypes.data_as(C.c_void_p), 65536, 2.0, C.byref(d), None, 0, None, 0) == -5
    assert b"at most 65535 edges" in L.ca_last_error(None), L.ca_last_error(None)
    assert L.ca_edge_grid_build(many.ctypes.data_as(C.c_void_p), 65535, 2.0, C.byref(d), None, 0, None, 0) == 0 and d.n_entries >= 65535
    k = np.arange(100, dtype=F)
    walls = np.stack([k, 0 * k, 6000 + k, 6000 + 0 * k], axis=1).astype(F)                # 100 diagonals across a 256 x 256 table
    assert L.ca_edge_grid_build(walls.ctypes.data_as(C.c_void_p), 100, 2.0, C.byref(d), None, 0, None, 0) == -5
    msg = L.ca_last_error(None)
    assert b"subdivide the walls" in msg and str(_lib.EDGE_GRID_MAX_ENTRIES).encode() in msg and d.n_entries > _lib.EDGE_GRID_MAX_ENTRIES, msg
    with pytest.raises(RuntimeError, match="subdivide the walls"):
        _lib.edge_grid_build(walls, 2.0)
    pieces = E.edges_of(E.subdivided([[(float(a), 0.0), (6000.0 + a, 6000.0)] for a in k[:100]], 64))[::2]   # the same walls in 64 pieces each
    d2, _, _ = _lib.edge_grid_build(pieces, 2.0)
    assert len(pieces) == 6400 and d2.n_entries < _lib.EDGE_GRID_MAX_ENTRIES // 4
    for bad in (0.0, -1.0, float("nan")):
        assert L.ca_edge_grid_build(walls.ctypes.data_as(C.c_void_p), 100, bad, C.byref(d), None, 0, None, 0) == -5


# ---- 5. the host header under the sanitizers -------------------------------------------------------------------------------------------
def test_builder_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "edge_grid_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "collision_avoidance_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "abi", "edge_grid_main.cpp")]
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else ["-static-libsan"]
    r = subprocess.run(cmd + static, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)   # (the runtime inside the program: its
    if r.returncode != 0:                                                                            # place among the loaded libraries is moot)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|libclang_rt", r.stdout):
        pytest.skip("the host compiler lacks the sanitizer runtime: " + r.stdout[-300:])
    assert r.returncode == 0, r.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0 and "EDGE_GRID_OK" in run.stdout, run.stdout[-4000:]
    assert "AddressSanitizer" not in run.stdout and "runtime error:" not in run.stdout, run.stdout[-4000:]
