"""Worlds that bring MORE than 16 obstacle edges in range of an agent (RVO2 keeps every one: collision_avoidence_env.py:249,
301-318), shared by tests/test_wide_obstacle_lists_cpu.py (the input guard, on the oracle) and
tests/test_gpu_wide_obstacle_lists.py (the HIP path against the oracle at the same capacity).

None of them is denser than listed here on purpose: a grid of squares at a pitch of 0.7 reaches exactly 64 edges in range,
which leaves no margin below the largest supported list."""
import math

import numpy as np

from collision_avoidance_amd import scenarios
from oracle import oracle as o
from tests import helpers as H


squares = scenarios.squares_grid        # k x k squares (counter-clockwise: solid blocks), the lower left one at (x0, y0)


def border(E):
    return [(0.0, 0.0), (0.0, E), (E, E), (E, 0.0)]


def ring_world(n_edges=24, radius=1.2, centre=(5.0, 5.0)):
    """tests/test_gpu_overflow.py's ring: a clockwise polygon of `n_edges` short edges, all of them within range (2) of an
    agent near the centre."""
    th = [-(2 * math.pi * k) / n_edges for k in range(n_edges)]
    return [np.array([[centre[0] + radius * math.cos(t), centre[1] + radius * math.sin(t)] for t in th], np.float32)]


def ring_positions(A, N, seed=5):
    """Agents near the ring's centre; arena 1 stands far away (no edge in range there)."""
    rng = np.random.RandomState(seed)
    px = (5.0 + rng.uniform(-0.3, 0.3, (A, N))).astype(np.float32)
    py = (5.0 + rng.uniform(-0.3, 0.3, (A, N))).astype(np.float32)
    px[1, :] = 40.0
    return px, py


def ragged_squares_worlds(N=10):
    """The four ragged arenas of tests/test_worlds.py::test_per_arena_obstacle_ragged_and_wide_tables: no obstacle, the border,
    a doorway-like world, and the border + 9 x 9 small squares (up to 62 edges in range of an agent)."""
    E = scenarios.envsize("crowd", N)
    b = border(E)
    return [[], [b],
            [b, [(2.0, 0.0), (2.5, 0.0), (2.5, 2.4), (2.0, 2.4)], [(2.0, 3.6), (2.5, 3.6), (2.5, E), (2.0, E)]],
            [b] + squares(9, 0.3, 0.3, 0.65, 0.2)]


def pillar_hall(N, k, pitch):
    """scenarios.pillar_hall: border + the squares of squares(k, 0.4, 0.4, pitch, 0.3) that lie inside the crowd's arena."""
    return scenarios.pillar_hall(N, k, pitch)


def hall_a_worlds(A=2):
    """Pillar hall A, 64 agents: even arenas the hall, odd arenas the border only."""
    hall, plain = pillar_hall(64, 14, 1.0), [border(scenarios.envsize("crowd", 64))]
    return [hall if a % 2 == 0 else plain for a in range(A)]


def hall_b_worlds(A=2):
    """Pillar hall B, 100 agents (a workgroup of 128 lanes)."""
    hall, plain = pillar_hall(100, 16, 1.1), [border(scenarios.envsize("crowd", 100))]
    return [hall if a % 2 == 0 else plain for a in range(A)]


def make_pair(A, N, worlds, S, seed=8, gpu=True, **over):
    """(HIP env or None, oracle) on the crowd scenario with per-arena `worlds` and lists of S."""
    p = H.scenario_params("crowd", N, **over)
    g = H.make_gpu(A, N, "crowd", p, seed=seed, polys=dict(per_arena=worlds), max_obst_neighbors=S) if gpu else None
    e = H.make_oracle(A, N, "crowd", p, seed=seed, polys=dict(per_arena=worlds), max_obst_neighbors=S)
    return g, e


def alternate(envs_step, A, N, steps, seed=2, every=50, check=None):
    """orca_step and step(actions) alternating, observation and statistics on; check(s) every `every` steps."""
    rng = np.random.RandomState(seed)
    for s in range(steps):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32) if s % 2 == 1 else None
        envs_step(act)
        if check is not None and s % every == every - 1:
            check(s)


def oracle_step(e):
    def f(act):
        if act is None:
            e.orca_step(flags=o.F_OBS | o.F_STATS)
        else:
            e.step(act, flags=o.F_OBS | o.F_STATS)
    return f


def come_and_go_worlds(N=10):
    """Like ragged_squares_worlds, the squares at a pitch of 0.85 instead of 0.65: the sequence below drives agents with random
    actions and respawns them, which in the denser grid finds spots with 66 edges in range -- more than any list holds."""
    w = ragged_squares_worlds(N)
    w[3] = [border(scenarios.envsize("crowd", N))] + squares(7, 0.3, 0.3, 0.85, 0.2)
    return w


def come_and_go(g, e, A, N, worlds, same=None, seed=6):
    """One handle through: a many-edge world, the plain border for every arena, the many-edge world again, reset_masked, and 120
    steps with auto-reset (the handle was made with max_step=90: every arena ends an episode and starts another).  g: the HIP env or
    None (the oracle alone: the input guard); same(what): called where the two are compared.  Returns the largest obstacle list
    the oracle saw in each of the four stepping stages."""
    rng = np.random.RandomState(seed)
    F = o.F_OBS | o.F_STATS
    tops = []

    def run(n, what, autoreset=False):
        top = 0
        for s in range(n):
            fl = F | (o.F_AUTORESET if autoreset else 0)
            if s % 2:
                act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
                if g is not None:
                    g.step(act, stats=True, autoreset=autoreset)
                e.step(act, flags=fl)
            else:
                if g is not None:
                    g.orca_step(with_obs=True, stats=True, autoreset=autoreset)
                e.orca_step(flags=fl)
            top = max(top, int(e.get(o.FLD_OBST_COUNT).max()))
        tops.append(top)
        if same is not None:
            same(what)
    run(40, "many edges")
    b = border(scenarios.envsize("crowd", N))
    for env in (g, e):
        if env is not None:
            env.set_obstacles([b])
    run(30, "border only")
    for env in (g, e):
        if env is not None:
            env.set_obstacles_per_arena(worlds)
    run(30, "many edges again")
    mask = np.array([1, 0, 1, 1], np.int32)
    if g is not None:
        g.reset_masked(mask)
    e.reset_masked(mask, flags=o.F_OBS)
    if same is not None:
        same("reset_masked")
    run(120, "auto-reset", autoreset=True)
    return tops
