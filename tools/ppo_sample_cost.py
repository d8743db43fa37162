#!/usr/bin/env python3
"""What collecting a PPO batch costs (ca_rollout_policy_sample): two ways of getting the same batch of T = 64 steps of a
64-64 ReLU policy with a value head and a state-independent log-std on the same handle -- rollout_policy_sample(T) with every record
and its GAE launch; and what the library offered before: rollout_policy(T) with its four records, one batched torch forward over the
recorded observations for the values (and one more for the bootstrap row), torch log-probabilities, and GAE as a reverse Python
loop over the rows -- in ONE process, the variants alternated, every timed run at least --seconds long, --repeat runs of each.  Then
one profiled call, and the heads kernel's own time (policy_kernel<true>) beside policy_kernel<false>'s from ca_profile on the same handle.

  python tools/ppo_sample_cost.py [--shapes 1024x16,4096x64] [--repeat 5] [--seconds 0.5] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/ppo_sample_cost.py --probe 4096x64
      (a run of its own: 50 launches each of policy_kernel<false> and policy_kernel<true> on one handle, for the trace's per-launch times)

The workload is bench.py's crowd (bench_params: a new goal whenever one is reached).  The bar: the new call's median no lower than the
composition's median minus the composition's own spread (max - min of its repeats).
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

T = 64
HIDDEN = (64, 64)
GAMMA, LAM = 0.95, 0.95


def make(A, N):
    nd, K = (1.5, 5) if N <= 16 else (5.0, 10)
    return VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, nd, K), use_torch=True), nd, K


def variants(env):
    dev = torch.device("cuda", env.device)
    torch.manual_seed(1)
    mods, w = [], 64
    for h in HIDDEN:
        mods += [torch.nn.Linear(w, h), torch.nn.ReLU()]
        w = h
    trunk = torch.nn.Sequential(*mods).to(dev).float().requires_grad_(False)
    mean_head = torch.nn.Linear(w, 1).to(dev).requires_grad_(False)
    value_head = torch.nn.Linear(w, 1).to(dev).requires_grad_(False)
    log_std = torch.full((1,), -0.5, device=dev)
    lin = [m for m in trunk if isinstance(m, torch.nn.Linear)] + [mean_head]
    env.set_policy([(m.weight, m.bias) for m in lin])
    env.set_policy_heads(value=value_head, log_std=(None, log_std))
    eps = torch.randn((T, env.A, env.N), device=dev)
    noise = eps * torch.exp(log_std)          # what rollout_policy adds to the mean

    def sample():
        return env.rollout_policy_sample(T, noise=eps, gamma=GAMMA, lam=LAM, record=("obs", "actions", "logp", "dist", "values", "row_rewards",
                                                                                     "row_dones", "row_valid", "advantages", "targets"))

    def composed():
        out = env.rollout_policy(T, noise=noise, record=("obs", "actions", "rewards", "dones"), returns=False)
        with torch.no_grad():
            h = trunk(out["obs"].reshape(-1, 64))
            values = value_head(h).reshape(T, env.A, env.N)
            mean = mean_head(h).reshape(T, env.A, env.N)
            boot = value_head(trunk(env.observe().reshape(-1, 64))).reshape(1, env.A, env.N)
            values = torch.cat([values, boot], 0)
            z = (out["actions"] - mean) * torch.exp(-log_std)
            logp = -0.5 * z * z - log_std - 0.918938533
            adv = torch.empty_like(out["rewards"])
            nd = (out["dones"] == 0).to(torch.float32)[:, :, None]
            last = torch.zeros_like(values[0])
            for r in range(T - 1, -1, -1):          # the reverse GAE loop: five small kernels a row
                delta = out["rewards"][r] + GAMMA * values[r + 1] * nd[r] - values[r]
                last = delta + GAMMA * LAM * nd[r] * last
                adv[r] = last
            targets = adv + values[:T]
        return out, logp, values, adv, targets
    return [("rollout_policy_sample(T): one call, every record, GAE", sample),
            ("rollout_policy(T) + torch values, log-probabilities, GAE loop", composed)]


def timed(env, call, seconds):
    env.sync()
    n, t0 = 0, time.perf_counter()
    while True:
        call()
        n += 1
        env.sync()
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= seconds:
            break
    return env.A * env.N * T * n / (time.perf_counter() - t0)


def fmt(name, runs, unit=1e9):
    r = sorted(runs)
    return "%-62s %9.4f  %9.4f .. %-9.4f  %s" % (name, r[len(r) // 2] / unit, r[0] / unit, r[-1] / unit, " ".join("%.4f" % (v / unit) for v in runs))


def kernel_us(env, call, n=20):
    env.observe()
    env.profile(1); env.profile_read()
    for _ in range(n):
        call()
    prof = env.profile_read(); env.profile(0)
    return prof["reset_kernels"][0], prof["reset_kernels"][1] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x16,4096x64")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_sample_cost.txt"))
    ap.add_argument("--probe", default=None, help="AxN: only launch policy_kernel<false> and policy_kernel<true> 50 times each (for a kernel trace)")
    a = ap.parse_args()
    if a.probe:
        A, N = (int(v) for v in a.probe.split("x"))
        env, _, _ = make(A, N)
        variants(env)
        env.observe()
        for _ in range(50):
            env.policy_actions()
        for _ in range(50):
            env.policy_evaluate()
        env.sync()
        env.close()
        return
    if not torch.cuda.is_available():
        raise SystemExit("ppo_sample_cost.py measures on the GPU: no device found")
    lines = ["sources %s; policy 64-%s-1 with a value head and a state-independent log-std (fp32), T = %d steps per call, %d alternated repeats of "
             "at least %.1f s each; G agent-steps/s: median, min .. max, every repeat" % (b.source_sha(), "-".join(str(h) for h in HIDDEN), T, a.repeat, a.seconds)]
    for shape in a.shapes.split(","):
        A, N = (int(v) for v in shape.split("x"))
        env, nd, K = make(A, N)
        vs = variants(env)
        res = {name: [] for name, _ in vs}
        for _, call in vs:
            call(); env.sync()
        for _ in range(a.repeat):
            for name, call in vs:
                res[name].append(timed(env, call, a.seconds))
        lines.append("")
        lines.append("%d x %d agents (neighbor_dist %.1f, max_neighbors %d)" % (A, N, nd, K))
        lines += [fmt(name, res[name]) for name, _ in vs]
        med = {name: sorted(res[name])[len(res[name]) // 2] for name, _ in vs}
        comp = res[vs[1][0]]
        bar = med[vs[1][0]] - (max(comp) - min(comp))
        lines.append("one call / composition (medians): %.3f; the bar (composition's median minus its spread): %.4f G -- %s"
                     % (med[vs[0][0]] / med[vs[1][0]], bar / 1e9, "held" if med[vs[0][0]] >= bar else "MISSED"))
        env.profile(1); env.profile_read()
        vs[0][1](); prof = env.profile_read(); env.profile(0)
        lines.append("one profiled rollout_policy_sample(T): solve launches %d x %.2f us; observation launches %d x %.2f us; small kernels (set-up, "
                     "heads, record, GAE: kind 3) %d x %.2f us" % (prof["step_kernel"][0], prof["step_kernel"][1] * 1e3, prof["obs_kernel"][0],
                                                                   prof["obs_kernel"][1] * 1e3, prof["reset_kernels"][0], prof["reset_kernels"][1] * 1e3))
        n1, us1 = kernel_us(env, env.policy_actions)
        n2, us2 = kernel_us(env, env.policy_evaluate)
        lines.append("per launch on this handle (ca_profile, %d launches each): policy_kernel<false> %.2f us, policy_kernel<true> %.2f us" % (n1, us1, us2))
        rew, val = torch.randn((T, A, N), device="cuda"), torch.randn((T + 1, A, N), device="cuda")
        done = torch.zeros((T, A), dtype=torch.int32, device="cuda")
        n3, us3 = kernel_us(env, lambda: env.gae(rew, val, done, gamma=GAMMA, lam=LAM))
        lines.append("gae_kernel alone, %d rows (%d launches): %.2f us" % (T, n3, us3))
        env.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
