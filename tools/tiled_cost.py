#!/usr/bin/env python3
"""What the tiled solve path costs (ca_create_ex with CA_CREATE_TILED; csrc/ca_tiled.h): reports, not thresholds.

  python tools/tiled_cost.py [--steps 200] [--warmup 60] [--out profiles/tiled_cost.txt]
  python tools/tiled_cost.py --grid [--steps 100] [--warmup 30] [--repeats 3] [--out profiles/tiled_grid_cost.txt]
  python tools/tiled_cost.py --grid-kernels          (one handle, for a kernel trace of its own)
  python tools/tiled_cost.py --edges [--parent-lib OTHER/libcaenv.so] [--repeats 5] [--out profiles/edge_grid_cost.txt]

The synthetic crowd of bench.py (scenarios.bench_params: range 5, K = 10, a new goal whenever one is reached, walls), a FULL step
per call: ca_step with CA_F_OBS | CA_F_STATS on device actions -- three solve launches and the observation on a tiled handle.
  1. one large crowd per arena: 8 x 2048, 4 x 4096, 1 x 16384 at the library's TILE;
  2. the three TILE sizes (CA_TILE = 64 | 128 | 256, the diagnostic switch ca_create_ex latches) at 4 x 4096;
  3. at 64 x 512 and 32 x 1024 the tiled handle next to the ordinary one, alternated in this one call (blocks of --steps steps,
     tiled, ordinary, tiled, ...; the median block of three each).  The ordinary handle's kernels are the ones every earlier
     commit ran, so that column is the baseline.
--grid: only the uniform-grid neighbour search (CA_CREATE_TILED | CA_CREATE_TILED_GRID) next to the plain tiled handle of the same
library -- the baseline: its kernels are the parent commit's, byte for byte --, alternated block by block in this one call,
--repeats blocks each, the full step and the ORCA-only step (ca_rollout with CA_F_STATS: the solve sequence without observation)
at 8 x 2048, 4 x 4096, 1 x 16384, 64 x 512 and 1 x 1100; every block's figure is printed, so the spread of the baseline's own
repeats stands next to the difference.  Then the launches of one step at 1 x 16384 by ca_profile: launches per step and their
mean, plain and grid.  --grid-kernels: 1 x 16384 on a grid handle and on a plain one, 20 ORCA-only steps each and nothing else,
for `rocprofv3 --kernel-trace --stats -- python tools/tiled_cost.py --grid-kernels` (per-kernel times: bin, scan, scatter, solve,
advance, close).
--edges: only the static edge grid (ca_tiled_edge_grid) of a grid handle.  Shapes 1 x 16384 and 4 x 4096; worlds of the crowd's box
alone (4 edges) and the box with a lattice of 0.5 x 0.5 pillars of about 500, 5000 and -- every edge cut in four -- 20000 edges;
lists of 16 with the truncation allowed (the cut walls overflow them, alike in every variant).  Variants, alternated block by block
in this one process, --repeats blocks of at least a second each (the block length is calibrated per variant): (i) the library given
by --parent-lib (the parent commit's build; left out without it), (ii) this library with the edge grid off -- the same kernel bytes
as (i), so it should lie inside the spread of (i)'s repeats --, (iii) this library with the edge grid on.  Per variant the ORCA-only
step with statistics (ca_rollout with CA_F_STATS: the six launches, wall test included) in us per step, every block and the median,
and ca_profile's mean over the six launches of a step (it does not tell the launches apart) times six.
Needs a GPU and PyTorch (for the device action pool and the synchronisation only).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(A, N, tiled, tile=None):
    from collision_avoidance_amd import scenarios
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    if tile is None:
        os.environ.pop("CA_TILE", None)
    else:
        os.environ["CA_TILE"] = str(tile)     # (read once, by ca_create_ex)
    p = scenarios.bench_params(N, 5.0, 10)
    env = VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=p, seed=0, use_torch=True, tiled=tiled)
    os.environ.pop("CA_TILE", None)
    return env


def block(env, pool, steps, first):
    """seconds per step over `steps` full steps"""
    import torch
    from collision_avoidance_amd import _lib
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        env._call("ca_step", env.h, pool[(first + i) % 16].data_ptr(), _lib.F_STATS | _lib.F_OBS)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def orca_block(env, steps):
    """seconds per step over `steps` ORCA-only steps: one ca_rollout, which on a tiled handle is `steps` times the solve sequence"""
    import torch
    from collision_avoidance_amd import _lib
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    env._call("ca_rollout", env.h, int(steps), _lib.F_STATS)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


GRID_SHAPES = ((8, 2048), (4, 4096), (1, 16384), (64, 512), (1, 1100))


def grid_table(args, lines):
    def say(text=""):
        lines.append(text)
        print(text, flush=True)

    say("plain tiled handle (baseline: the parent's kernels) next to the grid handle, alternated block by block, %d blocks of %d "
        "steps each; us per step, every block, then the median" % (args.repeats, args.steps))
    for A, N in GRID_SHAPES:
        envs = {"plain": make(A, N, True), "grid": make(A, N, "grid")}
        gi = envs["grid"].tiled_grid_info()
        pool = pool_for(A, N)
        for mode in ("full step", "ORCA only"):
            run = (lambda e, first: block(e, pool, args.steps, first)) if mode == "full step" else (lambda e, first: orca_block(e, args.steps))
            times = {k: [] for k in envs}
            for e in envs.values():
                (block(e, pool, args.warmup, 0) if mode == "full step" else orca_block(e, args.warmup))
            for r in range(args.repeats):
                for k, e in envs.items():
                    times[k].append(run(e, args.warmup + r * args.steps) * 1e6)
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            spread = max(times["plain"]) - min(times["plain"])
            for k in ("plain", "grid"):
                say("%5d x %-6d %-10s %-6s %s   median %10.1f us/step" % (A, N, mode, k, " ".join("%10.1f" % t for t in times[k]), med[k]))
            say("%5d x %-6d %-10s grid / plain = %.3f   (plain - grid = %.1f us, spread of plain's repeats %.1f us; table %d x %d cells)"
                % (A, N, mode, med["grid"] / med["plain"], med["plain"] - med["grid"], spread, gi["cells_x"], gi["cells_y"]))
        if (A, N) == (1, 16384):
            for k, e in envs.items():
                e.profile(1)
                orca_block(e, 20)
                n, ms = e.profile_read()["step_kernel"]
                say("%5d x %-6d ca_profile, ORCA only, %-6s %d launches per step, mean %.1f us per launch, %.1f us of kernels per step"
                    % (A, N, k, e.tiled_info()["launches_per_step"], ms * 1e3, ms * 1e3 * e.tiled_info()["launches_per_step"]))
                e.profile(0)
        for e in envs.values():
            e.close()
        say()


EDGE_SHAPES = ((1, 16384), (4, 4096))
EDGE_WORLDS = (4, 500, 5000, 20000)


def edge_world(N, target):
    """the crowd's box, clockwise, and a lattice of counter-clockwise 0.5 x 0.5 pillars, about `target` edges (20000: every edge of
    the 5000-edge world cut in four)"""
    from collision_avoidance_amd import scenarios
    e = scenarios.crowd_envsize(N)
    cut = 4 if target >= 20000 else 1
    side = 0 if target <= 4 else max(1, int(round(((target / cut - 4) / 4.0) ** 0.5)))
    polys = [[(0.0, 0.0), (0.0, e), (e, e), (e, 0.0)]]
    for j in range(side):
        for i in range(side):
            x, y = (i + 0.5) * e / side - 0.25, (j + 0.5) * e / side - 0.25
            polys.append([(x, y), (x + 0.5, y), (x + 0.5, y + 0.5), (x, y + 0.5)])
    if cut > 1:
        polys = [[(a[0] + (b[0] - a[0]) * k / cut, a[1] + (b[1] - a[1]) * k / cut) for a, b in zip(q, q[1:] + q[:1]) for k in range(cut)]
                 for q in polys]
    return polys


def other_library(path):
    """a second libcaenv.so in this process, bound like the first wherever it has the call"""
    import ctypes as C
    from collision_avoidance_amd import _lib
    L, P = _lib.load(), C.CDLL(path)
    for name in _lib.EXPORTS:
        if hasattr(P, name):
            getattr(P, name).argtypes, getattr(P, name).restype = getattr(L, name).argtypes, getattr(L, name).restype
    return P


def make_edges(A, N, polys, lib=None, edge_grid=False):
    from collision_avoidance_amd import _lib, scenarios
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    mine = _lib._lib
    if lib is not None:
        _lib._lib = lib
    try:
        return VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, 5.0, 10), seed=0, use_torch=True,
                                        tiled="grid", obstacles=polys, max_obst_neighbors=16, allow_obst_overflow=True,
                                        edge_grid=edge_grid)
    finally:
        _lib._lib = mine


def edges_table(args, lines):
    def say(text=""):
        lines.append(text)
        print(text, flush=True)

    parent = other_library(args.parent_lib) if args.parent_lib else None
    say("ORCA-only step with statistics on a grid handle, us per step; variants alternated block by block, %d blocks of at least 1 s each" % args.repeats)
    say("(i) parent = %s; (ii) off = this library, edge grid off; (iii) on = this library, edge grid on" % (args.parent_lib or "not given: left out"))
    for A, N in EDGE_SHAPES:
        for target in EDGE_WORLDS:
            polys = edge_world(N, target)
            n_edges = sum(len(q) for q in polys)
            envs = {}
            if parent is not None:
                envs["parent"] = make_edges(A, N, polys, lib=parent)
            envs["off"] = make_edges(A, N, polys)
            envs["on"] = make_edges(A, N, polys, edge_grid=True)
            info = envs["on"].edge_grid_info()
            steps, times = {}, {k: [] for k in envs}
            for k, e in envs.items():
                orca_block(e, 10)
                steps[k] = max(10, int(1.05 / orca_block(e, 10)) + 1)
            for r in range(args.repeats):
                for k, e in envs.items():
                    times[k].append(orca_block(e, steps[k]) * 1e6)
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            for k in envs:
                envs[k].profile(1)
                orca_block(envs[k], 20)
                n, ms = envs[k].profile_read()["step_kernel"]
                envs[k].profile(0)
                say("%2d x %-6d %6d edges  %-6s %s   median %10.1f us/step   (%5d steps per block; ca_profile: %.1f us of kernels per step)"
                    % (A, N, n_edges, k, " ".join("%10.1f" % t for t in times[k]), med[k], steps[k], ms * 1e3 * 6))
            base = "parent" if "parent" in envs else "off"
            say("%2d x %-6d %6d edges  on / off = %.3f   off - on = %.1f us   spread of %s's repeats %.1f us%s   (edge grid %d x %d cells, %d entries)"
                % (A, N, n_edges, med["on"] / med["off"], med["off"] - med["on"], base, max(times[base]) - min(times[base]),
                   "   off - parent = %.1f us" % (med["off"] - med["parent"]) if "parent" in envs else "",
                   info["cells_x"], info["cells_y"], info["entries"]))
            for e in envs.values():
                e.close()
            say()


def grid_kernels():
    for tiled in ("grid", True):
        env = make(1, 16384, tiled)
        orca_block(env, 20)
        env.close()


def pool_for(A, N):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(1234)
    return torch.rand((16, A, N), device="cuda", generator=gen) - 0.5


def row(label, A, N, sec):
    return "%-34s %7d x %-6d %12.1f us/step %14.3e agent-steps/s" % (label, A, N, sec * 1e6, A * N / sec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=None)
    ap.add_argument("--grid", action="store_true", help="only the grid handle next to the plain tiled one")
    ap.add_argument("--grid-kernels", action="store_true", help="only 20 ORCA-only steps at 1 x 16384, grid then plain: for a kernel trace")
    ap.add_argument("--edges", action="store_true", help="only the static edge grid of a grid handle: off, on, and the parent's library")
    ap.add_argument("--parent-lib", default=None, help="--edges: a libcaenv.so built from the parent commit, variant (i)")
    ap.add_argument("--repeats", type=int, default=None, help="blocks per variant (--grid: 3, --edges: 5)")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # PyTorch opens the device before the library does: the other way round it found no device
    if args.repeats is None:
        args.repeats = 5 if args.edges else 3
    if args.grid_kernels:
        return grid_kernels()
    from collision_avoidance_amd import build as b
    lines = ["tiled_cost.py %s--steps %d --warmup %d   (library source hash %s)" % ("--grid " if args.grid else "", args.steps, args.warmup, b.loaded_sha()), ""]
    if args.edges:
        lines[0] = "tiled_cost.py --edges --repeats %d   (library source hash %s)" % (args.repeats, b.loaded_sha())
        edges_table(args, lines)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if args.grid:
        grid_table(args, lines)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return

    def single(label, A, N, tiled, tile=None):
        env = make(A, N, tiled, tile)
        pool = pool_for(A, N)
        block(env, pool, args.warmup, 0)
        sec = sorted(block(env, pool, args.steps, args.warmup + k * args.steps) for k in range(3))[1]
        info = env.tiled_info()
        env.close()
        lines.append(row(label + (" (TILE %d)" % info["tile_agents"] if tiled else ""), A, N, sec))
        print(lines[-1], flush=True)

    lines.append("1. one large crowd per arena, full step (solve, advance, close, observation), median of 3 blocks")
    for A, N in ((8, 2048), (4, 4096), (1, 16384)):
        single("tiled", A, N, True)
    lines += ["", "2. the TILE sizes at 4 x 4096"]
    for tile in (64, 128, 256):
        single("tiled", 4, 4096, True, tile)
    lines += ["", "3. ordinary sizes: tiled next to the ordinary handle, alternated block by block"]
    for A, N in ((64, 512), (32, 1024)):
        envs = {"tiled": make(A, N, True), "ordinary": make(A, N, False)}
        pool = pool_for(A, N)
        times = {k: [] for k in envs}
        for k, e in envs.items():
            block(e, pool, args.warmup, 0)
        for rep in range(3):
            for k, e in envs.items():
                times[k].append(block(e, pool, args.steps, args.warmup + rep * args.steps))
        for k, e in envs.items():
            lines.append(row(k + (" (TILE %d)" % e.tiled_info()["tile_agents"] if k == "tiled" else ""), A, N, sorted(times[k])[1]))
            print(lines[-1], flush=True)
            e.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
