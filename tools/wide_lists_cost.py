#!/usr/bin/env python3
"""Cost of obstacle-neighbour lists above 16: ORCA-only and full-step agent-steps/s of a pillar hall.

The world is scenarios.pillar_hall(64, 14, 1.0), "pillar hall A" of the tests: the crowd arena of 64 agents (16 x 16), its
border and 14 x 14 pillars of side 0.3 at a pitch of 1.0 (788 edges, up to 34 of them in range of an agent).  One table for
every arena, the bench's rules around it (a new goal whenever one is reached, no episode cap: the load stays what it is).

  python tools/wide_lists_cost.py [--arenas 1024] [--cap 64] [--accept-overflow] [--steps 200] [--warmup 50] [--repeats 3]

--cap 16 --accept-overflow is the only form a library without the wide kernels can run: every list is cut to its nearest 16
edges, which is a DIFFERENT simulation (agents walk through the pillars' far edges' constraints), not a slower or faster form of
the same one.  Prints one JSON line: agent-steps/s (median of the repeats) of ca_orca_step and of ca_step with the
observation, the per-kernel means of ca_profile for a sampled run, the launch geometry and the overflow count.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--arenas", type=int, default=1024)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--accept-overflow", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    from collision_avoidance_amd import scenarios, build
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    A, N = args.arenas, 64
    p = scenarios.bench_params(N, 5.0, 10)
    env = VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=p, seed=8, max_obst_neighbors=args.cap, use_torch=True,
                                   obstacles=scenarios.pillar_hall(N, 14, 1.0), allow_obst_overflow=args.accept_overflow)
    act = (torch.rand((A, N), device="cuda") * 2 - 1).contiguous()

    def orca():
        env.orca_step(stats=True)

    def full():
        env.step(act, with_obs=True, stats=True)

    def rate(fn):
        for _ in range(args.warmup):
            fn()
        env.sync()
        out = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            env.sync()
            out.append(A * N * args.steps / (time.perf_counter() - t0))
        return out
    r_orca, r_full = rate(orca), rate(full)
    env.profile(1)
    for _ in range(20):
        full()
    prof = env.profile_read()
    env.profile(0)
    st = env.stats()
    print(json.dumps(dict(world="pillar hall A (788 edges, one table)", arenas=A, n_agents=N, max_neighbors=10, max_obst_neighbors=args.cap,
                          truncation_accepted=bool(args.accept_overflow), obst_overflow=int(st["obst_overflow"]),
                          agent_steps=int(st["agent_steps"]),
                          orca_agent_steps_per_s=float(np.median(r_orca)), orca_runs=[round(v) for v in r_orca],
                          step_obs_agent_steps_per_s=float(np.median(r_full)), step_obs_runs=[round(v) for v in r_full],
                          kernels_ms={k: round(v[1], 5) for k, v in prof.items() if v[0]},
                          launch=env.launch_info(), source_sha=build.loaded_sha())), flush=True)
    env.close()


if __name__ == "__main__":
    main()
