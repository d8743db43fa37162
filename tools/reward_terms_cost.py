#!/usr/bin/env python3
"""What shaping the reward on the device costs (ca_reward_configure).  Three ways of collecting a PPO batch of T = 64
steps of a 64-64 ReLU policy with a value head and a state-independent log-std, alternated in ONE process, every timed run at least
--seconds long, --repeat runs of each:
  on           rollout_policy_sample(T) on a handle with collision, wall, near and step terms: one call;
  composition  what the library offered for the same result before the terms: the Python loop of observe / policy_evaluate /
               step(contacts=True) on a handle without terms, torch arithmetic on the reward (the contact report has no count within
               a margin: its `near` term is nearest_d2 < sqr(2 r + margin), 0 or 1), and GAE as a reverse torch loop over the rows;
  off          rollout_policy_sample(T) on the handle without terms.
The bar, set before measuring: `on` no slower than the composition's median minus the composition's own spread (max - min of its
repeats).  Then one profiled call of `on` and of `off`: the kind-3 launches and their time, whose difference over 2 T launches is the
two reward kernels' own time per step.

  python tools/reward_terms_cost.py [--shapes 1024x16,4096x64] [--repeat 5] [--seconds 0.5] [--out FILE]

The workload is bench.py's crowd (bench_params: a new goal whenever one is reached).
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collision_avoidance_amd import _lib, build as b, scenarios  # noqa: E402
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv  # noqa: E402

T = 64
HIDDEN = (64, 64)
GAMMA, LAM = 0.95, 0.95
TERMS = dict(base=1.0, collision=-0.5, wall=-0.5, near=-0.05, step=-0.01, margin=0.3)
RECORDS = ("obs", "actions", "logp", "dist", "values", "row_rewards", "row_dones", "row_valid", "advantages", "targets")


def make(A, N, terms):
    nd, K = (1.5, 5) if N <= 16 else (5.0, 10)
    env = VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, nd, K), use_torch=True, reward_terms=terms)
    return env, nd, K


def install(env):
    torch.manual_seed(1)
    dev = torch.device("cuda", env.device)
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


def variants(on, off):
    dev = torch.device("cuda", on.device)
    eps = torch.randn((T, on.A, on.N), device=dev)
    near2 = (2.0 * off.cfg.radius + TERMS["margin"]) ** 2

    def sample_on():
        return on.rollout_policy_sample(T, noise=eps, gamma=GAMMA, lam=LAM, record=RECORDS)

    def sample_off():
        return off.rollout_policy_sample(T, noise=eps, gamma=GAMMA, lam=LAM, record=RECORDS)

    def composed():
        env = off
        rewards, values, dones, logps = [], [], [], []
        done_t = env.field_tensor(_lib.FLD_AGENT_DONE)
        for t in range(T):
            env.observe()
            ev = env.policy_evaluate(eps[t])
            stepping = (done_t == 0).to(torch.float32)
            _, rew, done, info = env.step(ev["actions"], with_obs=False, contacts=True)
            c = info["contacts"]
            r = TERMS["base"] * rew + TERMS["collision"] * c["agents"].to(torch.float32) + TERMS["wall"] * c["wall"].to(torch.float32) \
                + TERMS["near"] * (c["nearest_d2"] < near2).to(torch.float32) + TERMS["step"] * stepping
            rewards.append(r); values.append(ev["value"].clone()); logps.append(ev["logp"].clone()); dones.append(done.clone())
        env.observe()
        values.append(env.policy_evaluate()["value"].clone())
        rewards, values, dones = torch.stack(rewards), torch.stack(values), torch.stack(dones)
        adv = torch.empty_like(rewards)
        nd = (dones == 0).to(torch.float32)[:, :, None]
        last = torch.zeros_like(values[0])
        for r in range(T - 1, -1, -1):
            delta = rewards[r] + GAMMA * values[r + 1] * nd[r] - values[r]
            last = delta + GAMMA * LAM * nd[r] * last
            adv[r] = last
        return rewards, adv, adv + values[:T], logps
    return [("on: rollout_policy_sample(T) under collision, wall, near, step terms", sample_on, on),
            ("composition: observe / policy_evaluate / step(contacts) loop + torch", composed, off),
            ("off: rollout_policy_sample(T) without terms", sample_off, off)]


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
    return "%-72s %9.4f  %9.4f .. %-9.4f  %s" % (name, r[len(r) // 2] / unit, r[0] / unit, r[-1] / unit, " ".join("%.4f" % (v / unit) for v in runs))


def profiled(env, call):
    env.profile(1); env.profile_read()
    call()
    prof = env.profile_read(); env.profile(0)
    return prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x16,4096x64")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reward_terms_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reward_terms_cost.py measures on the GPU: no device found")
    lines = ["sources %s; policy 64-%s-1 with a value head and a state-independent log-std (fp32), T = %d steps per call, terms %r, %d alternated "
             "repeats of at least %.1f s each; G agent-steps/s: median, min .. max, every repeat"
             % (b.source_sha(), "-".join(str(h) for h in HIDDEN), T, TERMS, a.repeat, a.seconds)]
    for shape in a.shapes.split(","):
        A, N = (int(v) for v in shape.split("x"))
        on, nd, K = make(A, N, TERMS)
        off, _, _ = make(A, N, None)
        for e in (on, off):
            install(e)
        vs = variants(on, off)
        res = {name: [] for name, _, _ in vs}
        for _, call, env in vs:
            call(); env.sync()
        for _ in range(a.repeat):
            for name, call, env in vs:
                res[name].append(timed(env, call, a.seconds))
        lines.append("")
        lines.append("%d x %d agents (neighbor_dist %.1f, max_neighbors %d)" % (A, N, nd, K))
        lines += [fmt(name, res[name]) for name, _, _ in vs]
        med = {name: sorted(res[name])[len(res[name]) // 2] for name, _, _ in vs}
        comp = res[vs[1][0]]
        bar = med[vs[1][0]] - (max(comp) - min(comp))
        lines.append("on / composition (medians): %.3f; the bar (composition's median minus its spread): %.4f G -- %s"
                     % (med[vs[0][0]] / med[vs[1][0]], bar / 1e9, "held" if med[vs[0][0]] >= bar else "MISSED"))
        lines.append("on / off (medians): %.3f" % (med[vs[0][0]] / med[vs[2][0]]))
        p_on, p_off = profiled(on, vs[0][1]), profiled(off, vs[2][1])
        n_on, ms_on = p_on["reset_kernels"]
        n_off, ms_off = p_off["reset_kernels"]
        lines.append("one profiled call: kind-3 launches on %d x %.2f us, off %d x %.2f us; solve launches on %d x %.2f us, off %d x %.2f us"
                     % (n_on, ms_on * 1e3, n_off, ms_off * 1e3, p_on["step_kernel"][0], p_on["step_kernel"][1] * 1e3, p_off["step_kernel"][0],
                        p_off["step_kernel"][1] * 1e3))
        if n_on > n_off:
            lines.append("the reward kernels: %d launches more, %.2f us per launch (reward_begin_kernel and reward_terms_kernel averaged), %.2f us per step"
                         % (n_on - n_off, (n_on * ms_on - n_off * ms_off) * 1e3 / (n_on - n_off), (n_on * ms_on - n_off * ms_off) * 1e3 / T))
        on.close(); off.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
