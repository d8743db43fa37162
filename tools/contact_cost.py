#!/usr/bin/env python3
"""What the per-agent contact report costs (CA_F_CONTACT): microseconds per step of step(contacts=True) against
step() on the SAME handle, the two alternated, every timed run at least --seconds long, --repeat runs of each; and the mean
duration of contact_kernel itself from ca_profile (kind 3: on such a step the only kind-3 launch).

  python tools/contact_cost.py [--shapes 4096x64,16384x10,256x512,grid:1x16384] [--repeat 5] [--seconds 1.0] [--out FILE]

The flagless step is the parent's: the report is a kernel of its own behind the step, and no other kernel changed
(profiles/contact_kernel_resources.txt).  The workload is bench.py's crowd (scenarios.bench_params: range 5, K = 10; range 1.5,
K = 5 at 10 agents, the reference env's own constants), a full step per call: ca_step with CA_F_OBS | CA_F_STATS on device
actions.  `grid:AxN` is a tiled handle with the uniform grid.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collision_avoidance_amd import build as b, scenarios  # noqa: E402
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv  # noqa: E402


def make(shape):
    tiled = False
    if ":" in shape:
        kind, shape = shape.split(":", 1)
        tiled = {"tiled": True, "grid": "grid"}[kind]
    A, N = (int(v) for v in shape.split("x"))
    nd, K = (1.5, 5) if N <= 16 else (5.0, 10)
    env = VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, nd, K), seed=0, use_torch=True, tiled=tiled)
    return env, A, N, nd, K


def timed(env, act, contacts, seconds):
    """steps until `seconds` have passed, the stream drained at both ends -> microseconds per step"""
    env.sync()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(16):
            env.step(act, stats=True, contacts=contacts)
        n += 16
        env.sync()
        if time.perf_counter() - t0 >= seconds:
            break
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x64,16384x10,256x512,grid:1x16384")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["sources %s; a full step (observation, statistics) per call on one handle, %d alternated repeats of at least %.1f s each; "
             "us per step: median (min .. max)" % (b.source_sha(), a.repeat, a.seconds),
             "%-22s %28s %28s %10s %26s" % ("shape", "step()", "step(contacts=True)", "difference", "contact_kernel (ca_profile)")]
    for shape in a.shapes.split(","):
        env, A, N, nd, K = make(shape)
        act = (torch.rand((A, N), device="cuda") - 0.5)
        for c in (False, True):                                   # warm-up, and the report's buffer
            for _ in range(8):
                env.step(act, stats=True, contacts=c)
        env.sync()
        runs = {False: [], True: []}
        for _ in range(a.repeat):
            for c in (False, True):
                runs[c].append(timed(env, act, c, a.seconds))
        env.profile(1)
        env.profile_read()
        for _ in range(32):
            env.step(act, stats=True, contacts=True)
        n3, ms3 = env.profile_read()["reset_kernels"]
        env.profile(0)
        med = {c: sorted(runs[c])[len(runs[c]) // 2] for c in runs}
        cell = lambda c: "%9.2f (%.2f .. %.2f)" % (med[c], min(runs[c]), max(runs[c]))
        lines.append("%-22s %28s %28s %10.2f %17.2f us x %d" % (shape, cell(False), cell(True), med[True] - med[False], ms3 * 1e3, n3))
        env.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
