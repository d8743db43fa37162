"""CA_CREATE_TILED_PARAMS without a device: the header, the binding, the flag validation of ca_create_ex (which runs before a device
is needed) and the keyword rules of VecCollisionAvoidanceEnv.  Plus the scenes of tests/tiled_param_scenes.py on the CPU oracle's
simulator, as far as tests/test_gpu_tiled_params.py relies on them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from collision_avoidance_amd import vec_env  # noqa: F401  (PyTorch before the library, the order VecCollisionAvoidanceEnv loads them in:
#                                                          on a machine with a device the create test below initialises the HIP runtime)
from tests import agent_param_scenes as S
from tests import tiled_param_scenes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    assert int(re.search(r"#define\s+CA_CREATE_TILED_PARAMS\s+(\d+)u", hdr).group(1)) == _lib.CREATE_TILED_PARAMS == 16
    assert T.FLAGS_PLAIN == _lib.CREATE_TILED | _lib.CREATE_TILED_PARAMS == 17
    assert T.FLAGS_GRID == _lib.CREATE_TILED | _lib.CREATE_TILED_GRID | _lib.CREATE_TILED_PARAMS == 21


def test_create_ex_validates_the_flag_before_it_needs_a_device():
    L = _lib.load()
    h = C.c_void_p()
    cfg = _lib.Config(n_arenas=1, n_agents=8, max_obst_neighbors=1, **scenarios.env_params())
    for flags in (16, 18, 20, 24, 19):
        assert L.ca_create_ex(C.byref(cfg), flags, 0, None, C.byref(h)) == -1 and not h.value, flags
    assert L.ca_create_ex(C.byref(cfg), 16, 0, None, C.byref(h)) == -1 and b"CA_CREATE_TILED" in L.ca_last_error(None)
    for flags in (17, 21):                                                   # valid: what is left is the device
        rc = L.ca_create_ex(C.byref(cfg), flags, 0, None, C.byref(h))
        if rc == 0:                                                          # (a machine with a device: the handle exists)
            assert h.value and L.ca_destroy(h) == 0
            h = C.c_void_p()
        else:
            assert rc == -2 and not h.value, (flags, rc, L.ca_last_error(None))   # CA_ENODEV


def test_vec_env_keyword_rules():
    import inspect
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    sig = inspect.signature(VecCollisionAvoidanceEnv.__init__)
    assert sig.parameters["tiled_params"].default is False
    with pytest.raises(ValueError, match="tiled_params"):
        VecCollisionAvoidanceEnv(1, 8, scenario=None, tiled_params=True)
    for tiled in (True, "grid"):
        with pytest.raises(ValueError, match="tiled"):                        # without the keyword: today's refusal
            VecCollisionAvoidanceEnv(1, 8, scenario=None, tiled=tiled, agent_params=dict(radius=0.4))
        with pytest.raises(ValueError, match="tiled"):                        # agent counts stay refused with it
            VecCollisionAvoidanceEnv(1, 8, scenario=None, tiled=tiled, tiled_params=True, agent_counts=[3])


def test_scenes_are_what_the_gpu_tests_rely_on():
    """the large scene: full lists with ids beyond 1023; the hall scene: a largest obstacle range above the configuration's 2.0"""
    sc = T.scene(21, 1100, 47.0)
    sim = S.Sim(sc)
    sim.step()
    nc, ni = sim.agent_neighbors()
    oc, _ = sim.obstacle_neighbors()
    assert (nc == S.MAX_NEIGHBORS).all() and ni.max() > 1023 and oc.max() <= 3
    assert T.pair_count(sim.positions(), sc["radius"]) > 100
    e = scenarios.crowd_envsize(200)
    hall = S.draw(23, 200, 0.5, e - 0.5)
    hall["time_horizon_obst"] = np.random.RandomState(5).uniform(0.5, 1.0, 200).astype(np.float32)
    rng = T.obstacle_range(hall)
    assert rng.dtype == np.float32 and 2.25 < rng.max() < 2.26
