"""Obstacle-neighbour lists of up to 64 edges (RVO2 keeps every edge in range of an agent: collision_avoidence_env.py:249,
301-318): what can be checked without a GPU -- the constants, ca_create's argument check, the compiled kernels' resources,
and the INPUT GUARD of tests/test_gpu_wide_obstacle_lists.py: on the oracle at capacity 64 every world used there has lists
above 16 and none that overflows."""
import ctypes as C
import json
import os
import re
import shutil
import sys

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios, vec_env
from oracle import oracle as o
from tests import wide_worlds as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ENODEV, ERANGE = 0, -2, -5


def test_header_and_binding_say_64_and_the_default_stays_16():
    h = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    assert int(re.search(r"#define CA_MAX_OBST_NEIGHBORS (\d+)", h).group(1)) == 64 == _lib.MAX_OBST_NEIGHBORS
    assert vec_env.DEFAULT_MAX_OBST_NEIGHBORS == 16       # (tests/helpers.py make_oracle assumes it; existing users keep their kernels)


def _create(S, **over):
    L = _lib.load()
    h = C.c_void_p()
    cfg = _lib.Config(n_arenas=2, n_agents=10, max_obst_neighbors=S, **dict(scenarios.env_params(), **over))
    rc = L.ca_create(C.byref(cfg), 0, None, C.byref(h))
    msg = L.ca_last_error(None) if rc else b""
    if rc == OK:
        L.ca_destroy(h)
    return rc, msg, bool(h.value)


def test_ca_create_accepts_1_to_64():
    """Without a device a capacity of 64 gets as far as the device check (CA_ENODEV); 65 and 0 are out of range before that.
    (With a device the handle is created.)"""
    import torch
    want = OK if torch.cuda.is_available() else ENODEV
    for S in (17, 20, 64):
        rc, msg, _ = _create(S)
        assert rc == want, (S, rc, msg)
    for S in (65, 0, -1):
        rc, msg, handle = _create(S)
        assert rc == ERANGE and not handle and b"out of range 1..64" in msg, (S, rc, msg)


def _rows():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    kr.ensure_asm()
    return kr.parse()


def test_wide_kernels_are_compiled_and_the_observation_ones_use_no_scratch():
    rows = {r["name"]: r for r in _rows()}
    for k in (5, 10, 16):
        for bs in (64, 128):
            name = "step_kernel<%d, %d, 0, 64, false>" % (k, bs)
            assert name in rows, name
            # LP3's projected lines: a private array of KMAX + 64 lines of 16 B (by design, as in the 16-entry table kernels)
            assert rows[name]["scratch"] >= (k + 64) * 16 and rows[name]["vgpr_spill"] == 0, (name, rows[name])
    for name in ("obs_kernel<256, false, false, WideObstLists>", "obs_kernel<256, false, true, WideObstLists>"):
        assert name in rows, name
        assert rows[name]["scratch"] == 0 and rows[name]["vgpr_spill"] == 0 and rows[name]["sgpr_spill"] == 0, (name, rows[name])
    # nothing else is wide: no ALAN form, no workgroup above 128 lanes
    wide = [n for n in rows if re.match(r"step_kernel<\d+, \d+, \d+, 64", n)]
    assert len(wide) == 6, wide


def test_kernels_that_existed_before_keep_their_scratch_spills_and_lds():
    """A handle with max_obst_neighbors <= 16 runs the kernels it ran before the wide lists came: every kernel of the library as
    it was then is still there, under its name, with the same scratch, spills and static LDS -- what moves when a template
    gains a parameter carelessly (tests/golden/kernel_resources_before_wide_lists.json).  Registers and code size are not
    pinned here: a compiler update may move them; profiles/wide_obstacle_lists_kernel_resources.txt records that they, too, were
    identical when the wide kernels came.  A change that alters one of these kernels on purpose writes the file again:
      python -c "import json, sys; sys.path.insert(0, 'tools'); import kernel_resources as k; k.ensure_asm(); \
        json.dump([{c: r[c] for c in ('name', 'scratch', 'vgpr_spill', 'sgpr_spill', 'lds')} for r in k.parse() if r['name'] != '?'], \
        open('tests/golden/kernel_resources_before_wide_lists.json', 'w'), indent=0)"
    (and then drops the wide kernels' rows, or keeps them: they are checked by name above)."""
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_before_wide_lists.json")))
    rows = {r["name"]: r for r in _rows()}
    keys = ("scratch", "vgpr_spill", "sgpr_spill", "lds")
    diff = [(b["name"], [(k, b[k], rows[b["name"]][k]) for k in keys if rows[b["name"]][k] != b[k]] if b["name"] in rows else "missing")
            for b in before if b["name"] not in rows or any(rows[b["name"]][k] != b[k] for k in keys)]
    assert len(before) > 100 and not diff, diff


# ---- the input guard: the worlds of the GPU tests, on the oracle at capacity 64 -------------------------------------------
def _largest_list(e):
    return int(e.get(o.FLD_OBST_COUNT).max())


def test_guard_ragged_squares_world():
    _, e = W.make_pair(4, 10, W.ragged_squares_worlds(10), 64, gpu=False)
    top = 0
    for s in range(250):
        e.orca_step(flags=o.F_OBS | o.F_STATS)
        top = max(top, _largest_list(e))
    assert e.stats()["obst_overflow"] == 0 and 16 < top <= 64, top
    print("squares world: largest list", top)


@pytest.mark.parametrize("name,N,worlds,steps", [("A", 64, W.hall_a_worlds, 300), ("B", 100, W.hall_b_worlds, 200)])
def test_guard_pillar_halls(name, N, worlds, steps):
    _, e = W.make_pair(2, N, worlds(2), 64, gpu=False)
    top = [0]
    hist = np.zeros(4, np.int64)

    def look(s):
        c = e.get(o.FLD_OBST_COUNT)[0]
        top[0] = max(top[0], int(c.max()))
        hist[:] += [(c <= 4).sum(), ((c > 4) & (c <= 16)).sum(), ((c > 16) & (c <= 32)).sum(), (c > 32).sum()]
    W.alternate(W.oracle_step(e), 2, N, steps, every=1, check=look)
    assert e.stats()["obst_overflow"] == 0 and 16 < top[0] <= 64, top
    assert hist[2] + hist[3] > hist[0] + hist[1]           # most agent-steps of the hall need a list above 16
    print("pillar hall %s: largest list %d, agent-steps with <= 4 / 5-16 / 17-32 / 33-64 edges: %s" % (name, top[0], hist.tolist()))


@pytest.mark.parametrize("n_edges", [24, 48, 64])
def test_guard_rings(n_edges):
    A, N = 3, 2
    p = scenarios.env_params()
    e = W.H.make_oracle(A, N, "doorway", p, seed=3, arena_offset=40, max_obst_neighbors=64, polys=W.ring_world(n_edges))
    px, py = W.ring_positions(A, N)
    e.set(o.FLD_POS_X, px); e.set(o.FLD_POS_Y, py)
    e.orca_step(flags=o.F_STATS)
    c = e.get(o.FLD_OBST_COUNT)
    assert c[0].tolist() == [n_edges] * N and c[2].tolist() == [n_edges] * N and c[1].max() == 0
    assert e.stats()["obst_overflow"] == 0


def test_guard_come_and_go_sequence():
    A, N = 4, 10
    worlds = W.come_and_go_worlds(N)
    _, e = W.make_pair(A, N, worlds, 64, gpu=False, max_step=90)
    tops = W.come_and_go(None, e, A, N, worlds)
    assert e.stats()["obst_overflow"] == 0 and e.stats()["episodes"] >= A, e.stats()
    assert 16 < tops[0] <= 56 and tops[1] <= 4 and 16 < tops[2] <= 56 and 16 < tops[3] <= 56, tops   # (a margin below 64)
    print("come and go: largest list per stage", tops)


def test_guard_alan_rollout_on_the_squares_world():
    from collision_avoidance_amd import alan
    _, e = W.make_pair(4, 10, W.ragged_squares_worlds(10), 64, gpu=False)
    e.alan_configure(alan.DEFAULT_ACTIONS)
    top = 0
    for s in range(130):
        e.alan_step(flags=o.F_STATS | (o.F_FREEZE if s >= 10 else 0))
        top = max(top, _largest_list(e))
    assert e.stats()["obst_overflow"] == 0 and 16 < top <= 64, top
    print("alan on the squares world: largest list", top)


def test_drop_in_env_takes_the_list_keywords():
    """Collision_Avoidance_Env hands max_obst_neighbors / allow_obst_overflow to the vector env (defaults as before)."""
    import inspect
    from collision_avoidance_amd.envs import Collision_Avoidance_Env
    sig = inspect.signature(Collision_Avoidance_Env.__init__).parameters
    assert sig["max_obst_neighbors"].default is None and sig["allow_obst_overflow"].default is False
    assert list(sig)[:4] == ["self", "numAgents", "device", "seed"]          # the reference's positional arguments first
