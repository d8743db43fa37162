"""The navigation fields without a device: the host mask builder (ca_nav_mask_build; csrc/ca_nav_host.h) against the numpy restatement of
tests/nav_scenes.py, the uniqueness of the field's definition (label-setting, Jacobi and in-place raster relaxations agree bit for bit),
its plausibility on an empty grid, and its behaviour in front of the CPU oracle's ORCA step: agents leave a trap that holds them
without it.  All bit comparisons are ==, infinities included."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from collision_avoidance_amd import _lib, build
from tests import edge_grid_scenes as E
from tests import nav_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("ca_nav_configure", "ca_nav_clear", "ca_nav_info", "ca_nav_get_field", "ca_nav_pref", "ca_rollout_nav", "ca_nav_mask_build")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- 1. header, binding and sources agree ----------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    L = _lib.load()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.EXPORTS and getattr(L, name).restype is C.c_int, name
    m = re.search(r"typedef struct ca_nav_desc \{(.*?)\} ca_nav_desc;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).replace("*", " ")
    fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [f for f, _ in _lib.NavDesc._fields_], fields
    for macro, val in (("CA_NAV_MAX_CELLS", _lib.NAV_MAX_CELLS), ("CA_NAV_MAX_GOALS", _lib.NAV_MAX_GOALS), ("CA_NAV_MAX_LOOKAHEAD", _lib.NAV_MAX_LOOKAHEAD),
                       ("CA_NAV_STAY", _lib.NAV_STAY), ("CA_NAV_NONE", _lib.NAV_NONE)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == val, macro
    assert _lib.NAV_OFFSETS == S.OFFSETS and (_lib.NAV_STAY, _lib.NAV_NONE) == (S.STAY, S.NONE)
    expr = "fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1))"                        # the cell expression, verbatim
    for src in ("ca_nav_host.h", "ca_nav.h"):
        assert expr in open(os.path.join(ROOT, "collision_avoidance_amd", "csrc", src)).read(), src
    names = {os.path.basename(p) for p in build.SOURCES}
    assert {"ca_nav.h", "ca_nav_host.h"} <= names                                               # source_sha() covers the new files
    hub = open(os.path.join(ROOT, "collision_avoidance_amd", "csrc", "ca_kernels.h")).read()
    assert '#include "ca_nav.h"' in hub


# ---- 2. the mask builder ---------------------------------------------------------------------------------------------------------------
MASK_CASES = {
    "doorway": (S.doorway_world(), S.DOORWAY_GRID, S.DOORWAY_CLEARANCE),
    "doorway_pen": (S.doorway_world(pen=True), S.DOORWAY_GRID, S.DOORWAY_CLEARANCE),
    "doorway_at_clearance": (S.doorway_world(), S.DOORWAY_GRID, 0.5),      # centres of column 3 lie exactly 0.5 from the wall's face
    "blocks": (S.block_world(0), S.BLOCK_GRID, S.BLOCK_CLEARANCE),
    "blocks_1": (S.block_world(1), S.BLOCK_GRID, S.BLOCK_CLEARANCE),
    "one_cell": (S.block_world(0), dict(x0=1.6, y0=1.6, cell=1.0, gx=1, gy=1), 0.3),
    "one_cell_blocked": (S.block_world(0), dict(x0=1.1, y0=1.6, cell=1.0, gx=1, gy=1), 0.3),
    "hall": (S.hall_world(), S.HALL_GRID, S.HALL_CLEARANCE),
    "odd": (S.doorway_world(), dict(x0=-2.5, y0=0.25, cell=1.0, gx=13, gy=7), 0.3),
    "serpentine": (S.serpentine_world(), dict(x0=0.0, y0=0.0, cell=1.0, gx=64, gy=64), S.SERPENTINE_CLEARANCE),
    "trap": (S.trap_world(), S.TRAP_GRID, S.TRAP_CLEARANCE),
}


@pytest.mark.parametrize("name", sorted(MASK_CASES))
def test_mask_build_equals_the_restatement(name):
    polys, grid, clearance = MASK_CASES[name]
    edges, g = E.edges_of(polys), S.Grid(**grid)
    want = S.blocked_mask(edges, g, clearance)
    got = _lib.nav_mask_build(edges, grid["x0"], grid["y0"], grid["cell"], grid["gx"], grid["gy"], clearance)
    assert got.shape == want.shape == (grid["gy"], grid["gx"]) and (got == want).all(), np.argwhere(got != want)[:8]
    assert set(np.unique(got)) <= {0, 1}
    if name == "doorway_at_clearance":
        cx, _ = g.centres()
        assert cx[3] == F(1.5) and not want[:, 3].any() and want[:4, 4].all() and want[4:6, 4].all()   # strict <: 0.5 away is free; the door closes
    if name == "doorway":
        assert want.sum() == 8 and not want[4:6, 4].any()                                          # the door's two cells stay open
    if name == "doorway_pen":
        assert not want[7, 9] and want[6:9, 8:11].sum() == 8                                        # a free cell inside a closed ring
    if name == "one_cell":
        assert want.sum() == 0
    if name == "one_cell_blocked":
        assert want.sum() == 1
    if name == "hall":
        assert want[0].all() and want[:, 0].all() and not want[1:-1, 1:-1].any()


def test_mask_build_refusals():
    L = _lib.load()
    edges = E.edges_of(S.doorway_world())
    buf = np.zeros(200, np.uint8)
    p, b = edges.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
    assert L.ca_nav_mask_build(p, len(edges), -2.0, 0.0, 1.0, 12, 10, 0.05, b, 119) == -4          # CA_ESIZE: cells_cap too small
    assert b"120" in L.ca_last_error(None) and not buf.any()
    assert L.ca_nav_mask_build(p, len(edges), -2.0, 0.0, 1.0, 12, 10, 0.05, b, 120) == 0 and buf[:120].sum() == 8 and not buf[120:].any()
    for gx, gy in ((0, 4), (4, 0), (257, 1), (256, 129), (-1, -1)):
        assert L.ca_nav_mask_build(p, len(edges), 0.0, 0.0, 1.0, gx, gy, 0.05, b, 200) == -1, (gx, gy)
    assert L.ca_nav_mask_build(p, len(edges), 0.0, 0.0, 1.0, 4, 4, 0.05, None, 200) == -1
    assert L.ca_nav_mask_build(None, 0, 0.0, 0.0, 1.0, 4, 4, 0.05, b, 16) == 0                      # no edges: nothing blocked


# ---- 3. one solution, whatever the order ------------------------------------------------------------------------------------------------
def _serpentine():
    g = S.Grid(0.0, 0.0, 1.0, 64, 64)
    return S.blocked_mask(E.edges_of(S.serpentine_world()), g, S.SERPENTINE_CLEARANCE), g, (0, 0)


def _blocks():
    g = S.Grid(**S.BLOCK_GRID)
    return S.blocked_mask(E.edges_of(S.block_world(0)), g, S.BLOCK_CLEARANCE), g, (0, 0)


@pytest.mark.parametrize("world", ["serpentine", "blocks"])
def test_every_relaxation_order_ends_in_the_same_bits(world):
    blk, g, src = _serpentine() if world == "serpentine" else _blocks()
    dist, nxt = S.field(blk, g, src)
    cells = g.gx * g.gy
    jac, sweeps_j = S.jacobi(blk, g, src, max_sweeps=cells + 1)
    fwd, sweeps_f = S.raster(blk, g, src)
    rev, sweeps_r = S.raster(blk, g, src, reverse=True)
    for name, other in (("Jacobi", jac), ("forward raster", fwd), ("reverse raster", rev)):
        assert (_bits(other) == _bits(dist)).all(), (name, np.argwhere(_bits(other) != _bits(dist))[:8])
    assert sweeps_j <= cells + 1 and sweeps_f <= sweeps_j and sweeps_r <= sweeps_j                # in place does at least what Jacobi does
    assert np.isinf(dist[blk == 1]).all() and np.isfinite(dist[blk == 0]).all()
    if world == "serpentine":
        far = (63, 63) if nxt[63, 63] != S.NONE else None
        assert far is not None
        x, y, hops = 63, 63, 0
        while nxt[y, x] != S.STAY:                                                                # the pointers lead to the source
            k = int(nxt[y, x])
            assert k < 8 and dist[y + S.OFFSETS[k][1], x + S.OFFSETS[k][0]] < dist[y, x]
            x, y, hops = x + S.OFFSETS[k][0], y + S.OFFSETS[k][1], hops + 1
        assert (x, y) == src and hops >= 1500, hops
        assert sweeps_j >= 1500


def test_empty_grid_holds_hop_counts_and_octile_distances():
    g = S.Grid(0.0, 0.0, 1.0, 32, 32)
    blk = np.zeros((32, 32), np.uint8)
    src = (11, 20)
    dist, nxt = S.field(blk, g, src)
    xs, ys = np.arange(32), np.arange(32)
    assert (dist[src[1], :] == np.abs(xs - src[0]).astype(F)).all() and (dist[:, src[0]] == np.abs(ys - src[1]).astype(F)).all()
    dx, dy = np.abs(xs[None, :] - src[0]), np.abs(ys[:, None] - src[1])
    octile = np.maximum(dx, dy) + (np.sqrt(2.0) - 1.0) * np.minimum(dx, dy)
    assert (np.abs(dist.astype(np.float64) - octile) <= 1e-5 * np.maximum(octile, 1e-30)).all()
    assert nxt[src[1], src[0]] == S.STAY and nxt[src[1], src[0] + 3] == 2 and nxt[src[1] - 2, src[0]] == 1 and nxt[src[1] + 4, src[0] + 4] == 6


# ---- 4. behaviour in front of the CPU oracle's ORCA step ---------------------------------------------------------------------------------
def test_agents_leave_a_trap_that_holds_them_without_navigation():
    """1 arena x 8 agents left of a cup that opens towards them, goals behind its back wall, CA_DONE_GOAL, T = nav_scenes.TRAP_STEPS = 1200
    steps.  Measured: without navigation 0 of 8 agents arrive (they stand in the cup); with it 8 of 8, no agent ever within its
    radius of a wall."""
    control = S.trap_cpu_run(1, S.TRAP_STEPS, navigate=False)
    print("without navigation: %d of 8 arrived, %d wall overlaps" % (control["done"].sum(), control["obst_collisions"]))
    nav = S.trap_cpu_run(1, S.TRAP_STEPS, navigate=True)
    print("with navigation: %d of 8 arrived, %d wall overlaps" % (nav["done"].sum(), nav["obst_collisions"]))
    assert control["done"].sum() == 0                                                               # the scene is a trap
    assert nav["done"].sum() == 8 and nav["obst_collisions"] == 0


# ---- 5. the host header under the sanitizers ---------------------------------------------------------------------------------------------
def test_mask_builder_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "nav_mask_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "collision_avoidance_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "abi", "nav_mask_main.cpp")]
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else ["-static-libsan"]
    r = subprocess.run(cmd + static, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|libclang_rt", r.stdout):
        pytest.skip("the host compiler lacks the sanitizer runtime: " + r.stdout[-300:])
    assert r.returncode == 0, r.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0 and "NAV_MASK_OK" in run.stdout, run.stdout[-4000:]
    assert "AddressSanitizer" not in run.stdout and "runtime error:" not in run.stdout, run.stdout[-4000:]
