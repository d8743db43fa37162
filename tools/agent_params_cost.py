#!/usr/bin/env python3
"""What per-agent ORCA parameters (ca_set_agent_params) cost: agent-steps/s of the full step and of the ORCA-only step on one
handle shape, three ways --

  per-agent      the AgentParams kernels, the arrays set EQUAL to the config values (the same simulation, bit for bit)
  uniform/table  the same handle with uniform parameters on the LDS-line-table kernel (CA_REG_LINES=0 CA_QUAD=0): the
                 like-for-like cost of loading the parameters per lane
  uniform        the same handle as ca_create chooses it by default (register lines / four lanes per agent): what a user gives up

  python tools/agent_params_cost.py [--shapes 4096x64,1024x16] [--steps 300] [--warmup 60] [--repeat 3] [--out FILE]

The crowd workload of bench.py (random starts and goals, a new goal whenever one is reached), max_neighbors 10, neighbor_dist 5.
Each figure is the best of --repeat timed runs of --steps steps (wall clock around the loop, the stream drained at both ends).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collision_avoidance_amd import build as b, scenarios  # noqa: E402
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv  # noqa: E402

PARAMS = ("radius", "max_speed", "time_horizon", "time_horizon_obst")


def make(A, N, mode):
    switches = {"CA_REG_LINES": "0", "CA_QUAD": "0"} if mode == "uniform/table" else {}
    old = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)                      # (latched by ca_create)
    try:
        g = VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, 5.0, 10), seed=0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    if mode == "per-agent":
        g.set_agent_params(**{k: np.full((A, N), getattr(g.cfg, k), np.float32) for k in PARAMS})
    return g


def rate(g, full, steps, warmup, repeat):
    act = None
    if full:
        rng = np.random.RandomState(0)
        act = rng.uniform(-1, 1, (g.A, g.N)).astype(np.float32)
        if g.use_torch:
            import torch
            act = torch.as_tensor(act, device=torch.device("cuda", g.device))

    def run(n):
        for _ in range(n):
            if full:
                g.step(act, with_obs=True)
            else:
                g.orca_step()
    run(warmup)
    g.sync()
    best = 0.0
    for _ in range(repeat):
        t0 = time.perf_counter()
        run(steps)
        g.sync()
        best = max(best, g.A * g.N * steps / (time.perf_counter() - t0))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x64,1024x16")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["sources %s; steps %d, warmup %d, best of %d; agent-steps/s in G" % (b.source_sha(), a.steps, a.warmup, a.repeat),
             "%-10s %-14s %6s %5s %9s %10s %10s" % ("shape", "handle", "lanes", "block", "LDS B", "full step", "ORCA only")]
    for shape in a.shapes.split(","):
        A, N = (int(v) for v in shape.split("x"))
        res = {}
        for mode in ("per-agent", "uniform/table", "uniform"):
            g = make(A, N, mode)
            li = g.launch_info()
            assert li["agent_params"] == (mode == "per-agent"), li
            res[mode] = (rate(g, True, a.steps, a.warmup, a.repeat), rate(g, False, a.steps, a.warmup, a.repeat))
            lines.append("%-10s %-14s %6d %5d %9d %10.3f %10.3f" % (shape, mode, li["lanes_per_agent"], li["block"], li["lds_bytes"],
                                                                   res[mode][0] / 1e9, res[mode][1] / 1e9))
            g.close()
        for other in ("uniform/table", "uniform"):
            lines.append("%-10s per-agent / %-13s full step %.3f, ORCA only %.3f" % (shape, other, res["per-agent"][0] / res[other][0],
                                                                                   res["per-agent"][1] / res[other][1]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
