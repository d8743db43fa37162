"""CPU-only checks of the host side of forking and rewinding arenas (ca_arena_gather / ca_snapshot_*, include/ca_env.h): the binding
restates the header's prototypes, fork_index accepts and refuses what the library does, the front ends keep their defaults, and the
three statements of what an arena's state is -- the header's list, the library's table of planes, get_state()'s fields -- name the
same fields.  No compute call is made."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from collision_avoidance_amd import _lib, build, vec_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, u32, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t
PROTOTYPES = {
    "ca_arena_gather": ("ca_env* env, const int32_t* src, size_t bytes, int32_t src_is_device, uint32_t flags", [vp, vp, sz, i32, u32]),
    "ca_snapshot_create": ("ca_env* env, ca_snapshot** out", [vp, C.POINTER(vp)]),
    "ca_snapshot_save": ("ca_env* env, ca_snapshot* snap", [vp, vp]),
    "ca_snapshot_load": ("ca_env* env, const ca_snapshot* snap, const int32_t* src, size_t bytes, int32_t src_is_device, uint32_t flags",
                         [vp, vp, vp, sz, i32, u32]),
    "ca_snapshot_destroy": ("ca_env* env, ca_snapshot* snap", [vp, vp]),
    "ca_fork_bytes_per_arena": ("ca_env* env, size_t* bytes", [vp, C.POINTER(sz)]),
}


def _header():
    return open(os.path.join(ROOT, "include", "ca_env.h")).read()


def test_prototypes_exports_and_argtypes_agree():
    h = _header()
    assert re.search(r"^typedef struct ca_snapshot ca_snapshot;", h, re.M)
    L = _lib.load()
    for name, (args, argtypes) in PROTOTYPES.items():
        assert re.search(r"^int %s\(%s\);" % (name, re.escape(args)), h, re.M), name
        assert name in _lib.EXPORTS
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == argtypes, name


def test_kernel_source_is_hashed():
    assert os.path.join(os.path.dirname(build.LIB_PATH), "csrc", "ca_fork.h") in build.SOURCES


@pytest.mark.parametrize("src,A,allow_keep,want", [
    ([3, 3, 0, 1], 4, False, [3, 3, 0, 1]),
    (np.array([1, 2, 0], np.int64), 3, False, [1, 2, 0]),
    (np.array([0, 0, 0], np.uint8), 3, False, [0, 0, 0]),
    ((2, -1, 0), 3, True, [2, -1, 0]),
    (np.arange(5, dtype=np.int16)[::-1], 5, True, [4, 3, 2, 1, 0]),       # not contiguous
    ([0], 1, False, [0]),
])
def test_fork_index_accepts(src, A, allow_keep, want):
    out = vec_env.fork_index(src, A, allow_keep)
    assert out.dtype == np.int32 and out.shape == (A,) and out.flags["C_CONTIGUOUS"] and out.tolist() == want


@pytest.mark.parametrize("src,A,allow_keep", [
    ([0, 1], 3, False),                        # wrong length: CA_ESIZE
    ([[0, 1, 2]], 3, False),                   # wrong shape
    ([0, 1, 3], 3, False),                     # index A: CA_ERANGE
    ([0, -1, 2], 3, False),                    # -1 in a gather: CA_ERANGE
    ([0, -2, 2], 3, True),                     # -2 in a load: CA_ERANGE
    ([0.0, 1.0, 2.0], 3, False),               # not integers
    ([True, False, True], 3, False),
    (np.array([0, 2 ** 40, 1]), 3, False),     # does not fit 32 bits: out of range, not wrapped
    (np.array([0, 2 ** 63, 1], np.uint64), 3, True),
])
def test_fork_index_refuses_what_the_library_refuses(src, A, allow_keep):
    with pytest.raises(ValueError):
        vec_env.fork_index(src, A, allow_keep)


def test_fork_index_takes_a_cpu_tensor():
    import torch
    assert vec_env.fork_index(torch.tensor([1, 0, 1]), 3).tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        vec_env.fork_index(torch.tensor([1.0, 0.0, 1.0]), 3)


def test_front_ends_default_to_no_observation():
    V = vec_env.VecCollisionAvoidanceEnv
    for f in (V.fork, V.restore):
        p = inspect.signature(f).parameters
        assert p["obs"].default is False and p["contacts"].default is False
    assert inspect.signature(V.restore).parameters["src"].default is None
    assert inspect.signature(V.snapshot).parameters["into"].default is None
    assert inspect.signature(vec_env.fork_index).parameters["allow_keep"].default is False
    assert "fork()" in V.get_state.__doc__ and "fork()" in V.set_state.__doc__ and "get_state" in V.fork.__doc__


def test_the_three_lists_of_moved_fields_agree():
    """include/ca_env.h "State that moves", csrc/ca_env.hip state_planes and VecCollisionAvoidanceEnv._STATE_FIELDS (+ the ALAN
    fields get_state() adds after alan_configure)"""
    h = re.search(r"State that moves \(CA_FLD_\*\):(.*?); after ca_alan_configure\*:(.*?)\.\n", _header(), re.S)
    head = re.findall(r"[A-Z][A-Z0-9_]+", h.group(1)), re.findall(r"[A-Z][A-Z0-9_]+", h.group(2))
    src = open(os.path.join(ROOT, "collision_avoidance_amd", "csrc", "ca_env.hip")).read()
    body = src[src.index("static int state_planes("):src.index("static size_t state_plane_bytes(")]
    planes = re.findall(r'^\s*\{"([A-Z0-9_ ]+)", e->\w+, .*?(true|false)\},', body, re.M)
    lib = [n for names, alan in planes if alan == "false" for n in names.split()], \
          [n for names, alan in planes if alan == "true" for n in names.split()]
    V = vec_env.VecCollisionAvoidanceEnv
    assert sorted(head[0]) == sorted(lib[0]) == sorted(V._STATE_FIELDS) and len(set(head[0])) == len(head[0]) == 21
    alan = re.findall(r'st\["(ALAN_\w+)"\] = ', inspect.getsource(V.get_state))
    assert sorted(head[1]) == sorted(lib[1]) == sorted(alan) and len(alan) == 3
    for n in head[0] + head[1]:
        assert re.search(r"\bCA_FLD_%s\b" % n, _header()) and hasattr(_lib, "FLD_" + n), n
