#!/usr/bin/env python3
"""What per-agent sensing costs (ca_set_agent_sensing): microseconds per step of ONE handle in three configurations,
alternated, every timed run at least --seconds long, --repeat runs of each, medians:

  params          set_agent_params with the ca_config values (the AgentParams kernels): the baseline
  + sensing same  ... and set_agent_sensing with the handle's own neighbor_dist and max_neighbors for every agent: the lists are the
                  same, so the difference is the cost of the tag
  + sensing mixed ... and neighbor_dist_i uniform in [1, 5], max_neighbors_i uniform in 0 .. 10: shorter lists, fewer ORCA lines

  python tools/agent_sensing_cost.py [--shapes 4096x64,256x512,grid:1x16384] [--repeat 3] [--seconds 1.0] [--no-stats] [--out FILE]

The workload is bench.py's crowd (scenarios.bench_params: range 5, K = 10), a full step per call: ca_step with CA_F_OBS | CA_F_STATS on
device actions.  `grid:AxN` is a tiled handle with the uniform grid made with tiled_params=True.  A shape whose per-agent line table
does not fit a CU is reported as such and skipped.  The three configurations share the handle and so its evolving state.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collision_avoidance_amd import build as b, scenarios  # noqa: E402
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv  # noqa: E402

MODES = ("params", "+ sensing same", "+ sensing mixed")


def make(shape):
    tiled = False
    if ":" in shape:
        kind, shape = shape.split(":", 1)
        tiled = {"tiled": True, "grid": "grid"}[kind]
    A, N = (int(v) for v in shape.split("x"))
    env = VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, 5.0, 10), seed=0, use_torch=True, tiled=tiled,
                                   tiled_params=bool(tiled))
    return env, A, N


def apply(env, mode, mixed):
    if mode == "params":
        env.clear_agent_sensing()
    elif mode == "+ sensing same":
        env.set_agent_sensing(neighbor_dist=float(env.cfg.neighbor_dist), max_neighbors=int(env.cfg.max_neighbors))
    else:
        env.set_agent_sensing(**mixed)
    assert env.launch_info()["agent_sensing"] is (mode != "params") and env.launch_info()["agent_params"]


STATS = True   # --no-stats: steps without CA_F_STATS (no pair count: on a tiled handle the close launch's share)


def timed(env, act, seconds):
    """steps until `seconds` have passed, the stream drained at both ends -> microseconds per step"""
    env.sync()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(16):
            env.step(act, stats=STATS)
        n += 16
        env.sync()
        if time.perf_counter() - t0 >= seconds:
            break
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x64,256x512,grid:1x16384")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-stats", action="store_true", help="steps without CA_F_STATS: no pair count, no wall test")
    a = ap.parse_args()
    global STATS
    STATS = not a.no_stats
    lines = ["sources %s; a full step (observation, %s) per call on one handle, %d alternated repeats of at least %.1f s each; "
             "us per step: median (min .. max); ratio = median / median of `params`" % (b.source_sha(), "statistics" if STATS else "NO statistics", a.repeat, a.seconds),
             "%-16s %-16s %30s %8s" % ("shape", "configuration", "us per step", "ratio")]
    for shape in a.shapes.split(","):
        env, A, N = make(shape)
        cfgv = {k: float(getattr(env.cfg, k)) for k in ("radius", "max_speed", "time_horizon", "time_horizon_obst")}
        try:
            env.set_agent_params(**cfgv)
        except RuntimeError as err:
            lines.append("%-16s the per-agent line table does not fit: %s" % (shape, str(err)[:120]))
            env.close()
            continue
        rng = np.random.RandomState(0)
        mixed = dict(neighbor_dist=rng.uniform(1, 5, (A, N)).astype(np.float32), max_neighbors=rng.randint(0, 11, (A, N)).astype(np.int32))
        act = (torch.rand((A, N), device="cuda") - 0.5)
        runs = {m: [] for m in MODES}
        for _ in range(a.repeat):
            for m in MODES:
                apply(env, m, mixed)
                for _ in range(8):                                   # warm-up: the lists of this configuration
                    env.step(act, stats=STATS)
                runs[m].append(timed(env, act, a.seconds))
        med = {m: sorted(runs[m])[len(runs[m]) // 2] for m in MODES}
        for m in MODES:
            lines.append("%-16s %-16s %30s %8.3f" % (shape, m, "%9.2f (%.2f .. %.2f)" % (med[m], min(runs[m]), max(runs[m])), med[m] / med["params"]))
        env.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
