#!/usr/bin/env python3
"""What a closed-loop policy rollout costs (ca_rollout_policy): two ways of running the same T = 64 steps of a 64-64
ReLU MLP policy on the same handle -- rollout_policy(T) with returns; and what the library offered before: a Python loop of
step(with_obs=True), the same MLP as a torch fp32 nn.Sequential on the device, and a torch add_ for the return -- in ONE process,
the variants alternated, every timed run at least --seconds long, --repeat runs of each.  Then one profiled rollout_policy(T): the
policy kernel's own time from ca_profile, next to the paper estimate of the f32 matrix peak.

  python tools/policy_rollout_cost.py [--shapes 1024x16,4096x64] [--repeat 5] [--seconds 0.5] [--out FILE]

The workload is bench.py's crowd (bench_params: a new goal whenever one is reached).  Both variants hold their buffers on the device;
rollout_policy() writes returns only in the timed runs (record=()), like the loop.
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
HIDDEN = (64, 64)
PEAK_F32_MATRIX = 157.3e12   # FLOP/s: the f32-input MFMA runs at the f32 vector peak


def make(A, N):
    nd, K = (1.5, 5) if N <= 16 else (5.0, 10)
    return VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, nd, K), use_torch=True), nd, K


def variants(env):
    dev = torch.device("cuda", env.device)
    torch.manual_seed(1)
    widths = (64,) + HIDDEN + (1,)
    mods = []
    for i, o in zip(widths[:-1], widths[1:]):
        mods += [torch.nn.Linear(i, o), torch.nn.ReLU()]
    net = torch.nn.Sequential(*mods[:-1]).to(dev).float().requires_grad_(False)
    env.set_policy(net)
    acc = torch.zeros((env.A, env.N), device=dev, dtype=torch.float32)

    def one_call():
        return env.rollout_policy(T, record=(), returns=True)["returns"]

    def loop():   # (per step: step with the observation, the MLP in torch, one add_ for the return)
        acc.zero_()
        obs = env.observe()
        with torch.no_grad():
            for _ in range(T):
                act = net(obs).reshape(env.A, env.N)
                obs, rew, _, _ = env.step(act, with_obs=True)
                acc.add_(rew)
        return acc
    return [("rollout_policy(T): one call", one_call), ("T x (torch MLP + step(with_obs=True) + add_)", loop)], net


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


def policy_kernel_us(env):
    """the policy kernel alone: ca_policy_actions with every launch timed on its own dispatch (kind 3 holds nothing else here)"""
    env.observe()
    env.profile(1); env.profile_read()
    for _ in range(20):
        env.policy_actions()
    prof = env.profile_read(); env.profile(0)
    return prof["reset_kernels"][0], prof["reset_kernels"][1] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x16,4096x64")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_rollout_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_rollout_cost.py measures on the GPU: no device found")
    lines = ["sources %s; policy 64-%s-1 (fp32), T = %d steps per call, %d alternated repeats of at least %.1f s each; G agent-steps/s: median, min .. max, every repeat"
             % (b.source_sha(), "-".join(str(h) for h in HIDDEN), T, a.repeat, a.seconds)]
    widths = (64,) + HIDDEN + (1,)
    macs = sum(i * o for i, o in zip(widths[:-1], widths[1:]))
    for shape in a.shapes.split(","):
        A, N = (int(v) for v in shape.split("x"))
        env, nd, K = make(A, N)
        vs, net = variants(env)
        # the two variants run the same policy: the kernel's chain and torch's GEMM differ in the order of their sums only
        env.observe()
        diff = (env.policy_actions() - net(env._obs_t).reshape(A, N)).abs().max().item()
        res = measure(env, vs, a.repeat, a.seconds)
        lines.append("")
        lines.append("%d x %d agents (neighbor_dist %.1f, max_neighbors %d); largest |policy kernel - torch nn.Sequential| on one observation: %.2e"
                     % (A, N, nd, K, diff))
        lines += [fmt(name, res[name]) for name, _ in vs]
        m = {name: sorted(res[name])[len(res[name]) // 2] for name, _ in vs}
        lines.append("one call / loop (medians): %.3f" % (m[vs[0][0]] / m[vs[1][0]]))
        env.profile(1); env.profile_read()          # one profiled call: every launch timed on its own dispatch (ca_profile)
        vs[0][1](); prof = env.profile_read(); env.profile(0)
        lines.append("one profiled rollout_policy(T): solve launches %d x %.2f us; observation launches %d x %.2f us; small kernels (set-up, policy, "
                     "record: kind 3) %d x %.2f us" % (prof["step_kernel"][0], prof["step_kernel"][1] * 1e3, prof["obs_kernel"][0],
                                                       prof["obs_kernel"][1] * 1e3, prof["reset_kernels"][0], prof["reset_kernels"][1] * 1e3))
        n, us = policy_kernel_us(env)
        est = 2.0 * macs * A * N / PEAK_F32_MATRIX * 1e6
        lines.append("policy_kernel<false> alone (%d profiled ca_policy_actions launches): %.2f us; %.2f G multiply-adds per launch = %.2f us at the f32 "
                     "matrix peak of %.1f TF (paper figure): %.0f %% of it" % (n, us, macs * A * N / 1e9, est, PEAK_F32_MATRIX / 1e12, 100.0 * est / us))
        env.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
