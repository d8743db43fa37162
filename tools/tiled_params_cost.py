#!/usr/bin/env python3
"""What per-agent parameters cost on a tiled grid handle (CA_CREATE_TILED_PARAMS; csrc/ca_tiled.h's AgentParams instantiations): a
report, no threshold.

  python tools/tiled_params_cost.py [--steps 100] [--warmup 30] [--repeats 5] [--out profiles/tiled_params_cost.txt]

Two handles of create flags 21 (tiled, grid, parameters allowed) in the synthetic crowd of bench.py (scenarios.bench_params: range 5,
K = 10, a new goal whenever one is reached, walls), the same seed: one without parameters -- it launches the uniform tiled kernels
-- and one whose four arrays equal the ca_config values, which launches the parameter kernels on the same simulation, bit for bit.
Alternated block by block in this one call, --repeats blocks each, at 1 x 16384 and 4 x 4096: the full step (ca_step with
CA_F_OBS | CA_F_STATS on device actions) and the ORCA-only step (ca_rollout with CA_F_STATS); us per step, every block and the
median, so the spread of the uniform handle's own repeats stands next to the difference.  Needs a GPU and PyTorch (for the device
action pool and the synchronisation only).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = ((1, 16384), (4, 4096))


def make(A, N, with_params):
    import numpy as np
    from collision_avoidance_amd import scenarios
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    env = VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, 5.0, 10), seed=0, use_torch=True,
                                   tiled="grid", tiled_params=True)
    if with_params:
        env.set_agent_params(**{k: np.full((A, N), getattr(env.cfg, k), np.float32)
                                for k in ("radius", "max_speed", "time_horizon", "time_horizon_obst")})
    assert env.launch_info()["agent_params"] is bool(with_params)
    return env


def main():
    import torch  # noqa: F401  (before the library is loaded: PyTorch brings a HIP runtime of its own)
    import tiled_cost as tc
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text=""):
        lines.append(text)
        print(text, flush=True)

    from collision_avoidance_amd import build as b
    say("# tools/tiled_params_cost.py, sources %s: uniform tiled grid kernels next to the per-agent-parameter kernels (arrays equal to the "
        "ca_config values: the same simulation), alternated block by block, %d blocks of %d steps each; us per step, every block, then "
        "the median" % (b.loaded_sha(), args.repeats, args.steps))
    for A, N in SHAPES:
        envs = {"uniform": make(A, N, False), "params": make(A, N, True)}
        pool = tc.pool_for(A, N)
        for mode in ("full step", "ORCA only"):
            full = mode == "full step"
            for e in envs.values():
                (tc.block(e, pool, args.warmup, 0) if full else tc.orca_block(e, args.warmup))
            times = {k: [] for k in envs}
            for r in range(args.repeats):
                for k, e in envs.items():
                    sec = tc.block(e, pool, args.steps, args.warmup + r * args.steps) if full else tc.orca_block(e, args.steps)
                    times[k].append(sec * 1e6)
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            for k in ("uniform", "params"):
                say("%5d x %-6d %-10s %-8s %s   median %10.1f us/step" % (A, N, mode, k, " ".join("%10.1f" % t for t in times[k]), med[k]))
            say("%5d x %-6d %-10s params / uniform = %.3f   (params - uniform = %.1f us, spread of uniform's repeats %.1f us)"
                % (A, N, mode, med["params"] / med["uniform"], med["params"] - med["uniform"], max(times["uniform"]) - min(times["uniform"])))
        same = all((envs["uniform"].get(f) == envs["params"].get(f)).all() for f in (0, 1, 2, 3))
        say("%5d x %-6d positions and velocities of the two handles after the run: %s" % (A, N, "equal" if same else "DIFFERENT"))
        for e in envs.values():
            e.close()
        say()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
