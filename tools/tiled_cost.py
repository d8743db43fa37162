#!/usr/bin/env python3
"""What the tiled solve path costs (ca_create_ex with CA_CREATE_TILED; csrc/ca_tiled.h): reports, not thresholds.

  python tools/tiled_cost.py [--steps 200] [--warmup 60] [--out profiles/tiled_cost.txt]
  python tools/tiled_cost.py --grid [--steps 100] [--warmup 30] [--repeats 3] [--out profiles/tiled_grid_cost.txt]
  python tools/tiled_cost.py --grid-kernels          (one handle, for a kernel trace of its own)

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
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # PyTorch opens the device before the library does: the other way round it found no device
    if args.grid_kernels:
        return grid_kernels()
    from collision_avoidance_amd import build as b
    lines = ["tiled_cost.py %s--steps %d --warmup %d   (library source hash %s)" % ("--grid " if args.grid else "", args.steps, args.warmup, b.loaded_sha()), ""]
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
