#!/usr/bin/env python3
"""What the tiled solve path costs (ca_create_ex with CA_CREATE_TILED; csrc/ca_tiled.h): reports, not thresholds.

  python tools/tiled_cost.py [--steps 200] [--warmup 60] [--out profiles/tiled_cost.txt]

The synthetic crowd of bench.py (scenarios.bench_params: range 5, K = 10, a new goal whenever one is reached, walls), a FULL step
per call: ca_step with CA_F_OBS | CA_F_STATS on device actions -- three solve launches and the observation on a tiled handle.
  1. one large crowd per arena: 8 x 2048, 4 x 4096, 1 x 16384 at the library's TILE;
  2. the three TILE sizes (CA_TILE = 64 | 128 | 256, the diagnostic switch ca_create_ex latches) at 4 x 4096;
  3. at 64 x 512 and 32 x 1024 the tiled handle next to the ordinary one, alternated in this one call (blocks of --steps steps,
     tiled, ordinary, tiled, ...; the median block of three each).  The ordinary handle's kernels are the ones every earlier
     commit ran, so that column is the baseline.
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
    args = ap.parse_args()
    from collision_avoidance_amd import build as b
    lines = ["tiled_cost.py --steps %d --warmup %d   (library source hash %s)" % (args.steps, args.warmup, b.loaded_sha()), ""]

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
