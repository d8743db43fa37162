"""Scenes of the tiled handles with ORCA parameters per agent (CA_CREATE_TILED_PARAMS), shared by tests/test_tiled_params_cpu.py
and tests/test_gpu_tiled_params.py.  The recipe is tests/agent_param_scenes.py's (draw, Sim, the observation restatement): neighbour
range 5, max_neighbors 10, obstacle lists of 16, time step 1/60, parameters per agent from its RANGES -- in a clockwise side x side
box around a 3 x 3 block at the centre, at sizes the ordinary handle does not reach.  No tests in here."""
import numpy as np

from collision_avoidance_amd import _lib, scenarios
from tests import agent_param_scenes as S

FLAGS_PLAIN = _lib.CREATE_TILED | 16          # 17: the tiled handle that takes per-agent parameters
FLAGS_GRID = FLAGS_PLAIN | _lib.CREATE_TILED_GRID   # 21: ... with the uniform-grid neighbour search


def world(side):
    """the clockwise box (0, 0) .. (side, side) and a counter-clockwise 3 x 3 block at its centre"""
    c = 0.5 * side
    return [[(0.0, 0.0), (0.0, side), (side, side), (side, 0.0)],
            [(c - 1.5, c - 1.5), (c + 1.5, c - 1.5), (c + 1.5, c + 1.5), (c - 1.5, c + 1.5)]]


def scene(seed, n, side):
    """draw(seed, n, 0.5, side - 0.5) in world(side)"""
    sc = S.draw(seed, n, 0.5, side - 0.5)
    sc["world"] = world(side)
    return sc


def params(**over):
    """the handle's configuration: the recipe's ranges and time step, its constants where no array is given"""
    p = dict(scenarios.env_params(), neighbor_dist=S.NEIGHBOR_DIST, max_neighbors=S.MAX_NEIGHBORS, time_step=S.DT)
    p.update(S.DEFAULTS)
    p.update(over)
    return p


def pair_count(pos, radius):
    """pairs i < j with fp32 dx*dx + dy*dy < (r_i + r_j) * (r_i + r_j), the kernel's operation order; rows at a time, so that 1100
    agents do not need an [n, n] table of every term"""
    pos, r = pos.astype(np.float32), radius.astype(np.float32)
    total = 0
    for i in range(len(pos) - 1):
        dx, dy = pos[i, 0] - pos[i + 1:, 0], pos[i, 1] - pos[i + 1:, 1]
        cr = r[i] + r[i + 1:]
        total += int(((dx * dx + dy * dy) < cr * cr).sum())
    return total


def obstacle_range(sc):
    """[n] f32: tho_i * ms_i + r_i, every operation in fp32 -- what the kernels and the edge-grid builder evaluate"""
    return (sc["time_horizon_obst"].astype(np.float32) * sc["max_speed"].astype(np.float32)).astype(np.float32) + sc["radius"].astype(np.float32)
