#!/usr/bin/env python3
"""What a rollout under an action tensor costs (ca_rollout_actions): three ways of running the same T = 64 steps on
the same handle -- rollout_actions(); T step(with_obs=False) calls with a torch accumulate of the rewards behind each, which is what
a planner had to write before; rollout() (ORCA-only, no actions and no rewards: the floor) -- in ONE process, the variants
alternated, every timed run at least --seconds long, --repeat runs of each.  Then one planning round: fork arena 0 into every slot,
rollout_actions() with a sequence per slot, pick the best, restore.

  python tools/action_rollout_cost.py [--shapes 1024x16,4096x64] [--repeat 5] [--seconds 0.5] [--plan 1024x16] [--out FILE]

The workload is bench.py's crowd (bench_params: a new goal whenever one is reached); the action tensor, the discounts and the
outputs live on the device and are made once.  1024 x 16 takes the one-launch form (ca_solver_info: rollout_one_launch), 4096 x 64
the per-step form; the header line of each table says which.
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

T = 64


def make(A, N):
    nd, K = (1.5, 5) if N <= 16 else (5.0, 10)
    return VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, nd, K), use_torch=True), nd, K


def variants(env, hold=1):
    dev = torch.device("cuda", env.device)
    g = torch.Generator(device=dev).manual_seed(1)
    actions = (torch.rand((T // hold, env.A, env.N), generator=g, device=dev, dtype=torch.float32) * 2 - 1) * np.pi
    weights = torch.pow(torch.tensor(0.99, device=dev), torch.arange(T, device=dev, dtype=torch.float32))
    acc = torch.zeros((env.A, env.N), device=dev, dtype=torch.float32)

    def seq():
        return env.rollout_actions(actions, hold=hold, weights=weights)["returns"]

    w_host = weights.cpu().tolist()

    def steps_discounted():   # (one torch op per step: acc += w[t] * reward)
        acc.zero_()
        for t in range(T):
            _, rew, _, _ = env.step(actions[t // hold], with_obs=False)
            acc.add_(rew, alpha=w_host[t])
        return acc

    def floor():
        env.rollout(T)
    return [("rollout_actions(T, weights)", seq), ("T x step(with_obs=False) + torch add_ per step", steps_discounted),
            ("rollout(T): ORCA-only, the floor", floor)]


def timed(env, call, seconds):
    """calls of `call` until `seconds` have passed (the stream drained at both ends) -> agent-steps/s"""
    env.sync()
    n, t0 = 0, time.perf_counter()
    while True:
        call()
        n += 1
        env.sync()
        if time.perf_counter() - t0 >= seconds:
            break
    return env.A * env.N * T * n / (time.perf_counter() - t0)


def fmt(name, runs, unit=1e9):
    r = sorted(runs)
    return "%-52s %9.4f  %9.4f .. %-9.4f  %s" % (name, r[len(r) // 2] / unit, r[0] / unit, r[-1] / unit, " ".join("%.4f" % (v / unit) for v in runs))


def measure(env, vs, repeat, seconds):
    res = {name: [] for name, _ in vs}
    for _, call in vs:                   # warm-up: one call each
        call(); env.sync()
    for _ in range(repeat):              # alternated: one run of every variant per round
        for name, call in vs:
            res[name].append(timed(env, call, seconds))
    return res


def planning_round(env, repeat):
    """fork / rollout_actions / pick / restore, timed as one round trip to the host (the pick is an argmax read back): ms per round"""
    dev = torch.device("cuda", env.device)
    g = torch.Generator(device=dev).manual_seed(2)
    actions = (torch.rand((T, env.A, env.N), generator=g, device=dev, dtype=torch.float32) * 2 - 1) * np.pi
    src = torch.zeros(env.A, dtype=torch.int32, device=dev)
    snap = env.snapshot()
    out = []
    for r in range(repeat + 1):
        env.sync()
        t0 = time.perf_counter()
        env.snapshot(into=snap)
        env.fork(src)
        ret = env.rollout_actions(actions)["returns"]
        best = int(ret.sum(1).argmax().item())
        env.restore(snap)
        env.sync()
        if r:                            # (the first round is the warm-up)
            out.append((time.perf_counter() - t0) * 1e3)
    snap.close()
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x16,4096x64")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--plan", default="1024x16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_rollout_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("action_rollout_cost.py measures on the GPU: no device found")
    lines = ["sources %s; T = %d steps per call, %d alternated repeats of at least %.1f s each; G agent-steps/s: median, min .. max, every repeat"
             % (b.source_sha(), T, a.repeat, a.seconds)]
    for shape in a.shapes.split(","):
        A, N = (int(v) for v in shape.split("x"))
        env, nd, K = make(A, N)
        form = "one launch per 256 steps" if env.launch_info()["rollout_one_launch"] else "a launch sequence per step + the accumulate kernel"
        vs = variants(env)
        res = measure(env, vs, a.repeat, a.seconds)
        lines.append("")
        lines.append("%d x %d agents (neighbor_dist %.1f, max_neighbors %d): %s" % (A, N, nd, K, form))
        lines += [fmt(name, res[name]) for name, _ in vs]
        env.profile(1); env.profile_read()          # one profiled call: every launch timed on its own dispatch (ca_profile)
        vs[0][1](); prof = env.profile_read(); env.profile(0)
        lines.append("one profiled rollout_actions(T): solve launches %d, %.2f us per step; small kernels (set-up, accumulate: kind 3) %d x %.2f us"
                     % (prof["step_kernel"][0], prof["step_kernel"][1] * 1e3, prof["reset_kernels"][0], prof["reset_kernels"][1] * 1e3))
        env.close()
    if a.plan:
        A, N = (int(v) for v in a.plan.split("x"))
        env, nd, K = make(A, N)
        ms, best = planning_round(env, a.repeat)
        lines.append("")
        lines.append("planning round at %d x %d: snapshot, fork arena 0 into %d slots, rollout_actions(T = %d), argmax read back, restore; ms per round"
                     % (A, N, A, T))
        lines.append(fmt("one round", ms, unit=1.0))
        env.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
