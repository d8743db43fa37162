"""CPU-only checks of the recording rollouts' host side (ca_rollout_trace / ca_alan_rollout_trace, include/ca_env.h): the
binding restates the header's struct, constants and prototypes, trace_shape gives the layout without a device, and the Python
front ends keep their defaults.  No compute call is made."""
import ctypes as C
import inspect
import os
import re

import pytest

from collision_avoidance_amd import _lib, alan, vec_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"void*": C.c_void_p, "size_t": C.c_size_t, "int32_t": C.c_int32, "uint32_t": C.c_uint32}


def _header():
    return open(os.path.join(ROOT, "include", "ca_env.h")).read()


def test_struct_layout_matches_header():
    body = re.search(r"typedef struct ca_trace \{(.*?)\} ca_trace;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s*(void\*|size_t|int32_t|uint32_t)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == ["agents", "agents_bytes", "arenas", "arenas_bytes", "every", "channels"]
    assert [(n, CTYPES[t]) for t, n in fields] == list(_lib.Trace._fields_)
    assert C.sizeof(_lib.Trace) == 2 * C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_size_t) + 8 == 40
    assert _lib.Trace.every.offset == 32 and _lib.Trace.channels.offset == 36


def test_constants_and_exports_match_header():
    h = _header()
    assert int(re.search(r"#define CA_TRACE_POS (\d+)u", h).group(1)) == _lib.TRACE_POS == 1
    assert int(re.search(r"#define CA_TRACE_VEL (\d+)u", h).group(1)) == _lib.TRACE_VEL == 2
    for name in ("ca_rollout_trace", "ca_alan_rollout_trace"):
        assert re.search(r"^int %s\(ca_env\* env, int32_t steps, uint32_t flags, const ca_trace\* tr\);" % name, h, re.M), name
        assert name in _lib.EXPORTS
    L = _lib.load()
    for name in ("ca_rollout_trace", "ca_alan_rollout_trace"):
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(_lib.Trace)]


@pytest.mark.parametrize("steps,every,channels,want_r,want_c", [
    (5, 7, ("pos", "vel"), 0, 4),          # fewer steps than `every`: no record
    (300, 7, ("pos", "vel"), 42, 4),       # `every` does not divide `steps`: the steps beyond 294 are not recorded
    (40, 1, ("pos",), 40, 2),
    (40, 3, ("vel",), 13, 2),
    (40, 3, "pos", 13, 2),                 # a single name
    (40, 40, ("vel", "pos"), 1, 4),        # the order of the names does not matter: the planes' order is fixed
    (0, 1, _lib.TRACE_POS | _lib.TRACE_VEL, 0, 4),
])
def test_trace_shape(steps, every, channels, want_r, want_c):
    assert vec_env.trace_shape(steps, every, channels, 6, 12) == ((want_r, want_c, 6, 12), (want_r, 3, 6))


def test_trace_shape_refuses_what_the_library_refuses():
    for bad in (dict(every=0), dict(every=-3), dict(channels=()), dict(channels=("pos", "action")), dict(channels=4), dict(channels=0)):
        kw = dict(steps=10, every=1, channels=("pos",), A=2, N=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            vec_env.trace_shape(**kw)


def test_front_ends_default_to_no_trace():
    V = vec_env.VecCollisionAvoidanceEnv
    assert inspect.signature(V.rollout).parameters["trace"].default is None
    assert inspect.signature(V.alan_rollout).parameters["trace"].default is None
    sig = inspect.signature(alan.Collision_Avoidance_Sim.run_sim)
    assert sig.parameters["trace_every"].default is None and sig.parameters["mode"].default == 1
