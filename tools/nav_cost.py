#!/usr/bin/env python3
"""What the navigation fields cost (ca_nav_*), measured in ONE process, variants alternated, median and range:

  (a) ca_nav_configure: wall time of the call and the field kernel's own time (ca_profile), with sweeps_max, for the two block sizes
      of nav_field_kernel (CA_NAV_BLOCK = 256 | 1024, the diagnostic switch ca_create latches) -- 1 set x 4 goals x 256 x 128 cells in
      scenarios.pillar_hall(300, 40, 1.0), and 4096 sets x 1 goal x 32 x 32 cells in scenarios.blocks_worlds(4096, 16);
  (b) nav_pref_kernel per launch at 4096 x 64 and at 1 x 16384 (tiled, grid), beside the launches of the ORCA-only step it precedes;
  (c) rollout_nav(64) against what a caller could do before: a Python loop that computes the same preferred velocities with torch
      gathers on the device, writes them into PREF_X / PREF_Y and calls orca_step -- at 1024 x 16 and 4096 x 64;
  (e) the navigated action step (ca_nav_step): rollout_nav_policy(64) against (i) the Python loop of observe /
      policy_actions / step_nav and (ii) rollout_policy(64) on the same handle, at 1024 x 16 and 4096 x 64, and the two new kernels'
      own times (ca_profile).  Not among the default parts: --only e --out profiles/nav_step_cost.txt.

  python tools/nav_cost.py [--repeat 5] [--seconds 0.5] [--only a,b,c] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collision_avoidance_amd import _lib, build as b, scenarios  # noqa: E402
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv  # noqa: E402

T = 64


def stat(runs, unit, fmt="%.3f"):
    r = sorted(runs)
    return (fmt + "  " + fmt + " .. " + fmt + "  (%s)") % (r[len(r) // 2] / unit, r[0] / unit, r[-1] / unit, " ".join(fmt % (v / unit) for v in runs))


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------
def configure_cases():
    hall = scenarios.pillar_hall(300, 40, 1.0)
    e = scenarios.envsize("crowd", 300)
    cell = e / 256.0
    yield ("1 set x 4 goals x 256 x 128 cells, pillar_hall(300, 40, 1.0): %d edges" % sum(len(q) for q in hall),
           dict(n_arenas=1, n_agents=64, obstacles=hall, max_obst_neighbors=16),
           dict(targets=[(1.05, 1.05), (30.05, 1.05), (1.05, 16.05), (30.05, 16.05)], agent_class=0, cell=cell, origin=(0.0, 0.0), shape=(256, 128),
                clearance=0.1))
    A, N = 4096, 16
    worlds = scenarios.blocks_worlds(A, N)
    e = scenarios.envsize("blocks", N)
    yield ("%d sets x 1 goal x 32 x 32 cells, blocks_worlds(%d, %d): %d edges per arena" % (A, A, N, sum(len(q) for q in worlds[0])),
           dict(n_arenas=A, n_agents=N, obstacles=dict(per_arena=worlds), max_obst_neighbors=16),
           dict(targets=np.full((A, 1, 2), 1.2, np.float32), agent_class=0, cell=e / 32.0, origin=(0.0, 0.0), shape=(32, 32), clearance=0.3))   # (cell (1, 1): no block reaches it)


def part_a(args, say):
    say("(a) ca_nav_configure: wall ms of the call | the field kernel's own ms (one launch, ca_profile) -- median  min .. max  (every repeat)")
    for name, mk, nav in configure_cases():
        say(name)
        envs = {}
        for blk in (256, 1024):
            os.environ["CA_NAV_BLOCK"] = str(blk)
            envs[blk] = VecCollisionAvoidanceEnv(scenario=None, params=scenarios.bench_params(mk["n_agents"], 1.5, 5), use_torch=True, **mk)
        os.environ.pop("CA_NAV_BLOCK", None)
        wall, kern, sweeps = {k: [] for k in envs}, {k: [] for k in envs}, {}
        for rep in range(args.repeat + 1):
            for blk, env in envs.items():
                env.profile(1); env.profile_read()
                env.sync()
                t0 = time.perf_counter()
                env.set_navigation(**nav)
                dt = time.perf_counter() - t0
                n, ms = env.profile_read()["reset_kernels"]
                env.profile(0)
                assert n == 1, n
                if rep:                      # (the first round warms up)
                    wall[blk].append(dt * 1e3); kern[blk].append(ms)
                sweeps[blk] = env.navigation_info()["sweeps_max"]
        for blk in envs:
            say("  block %4d: sweeps_max %5d   configure %s ms   field kernel %s ms" % (blk, sweeps[blk], stat(wall[blk], 1.0), stat(kern[blk], 1.0)))
        for env in envs.values():
            env.close()


# ---- (b), (c) --------------------------------------------------------------------------------------------------------------------------
def crowd_env(A, N, **kw):
    nd, K = (1.5, 5) if N <= 16 else (5.0, 10)
    env = VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, nd, K), use_torch=True, **kw)
    e = scenarios.envsize("crowd", N)
    cell = 0.5 if e <= 64 else e / 128.0
    side = int(np.ceil(e / cell))
    targets = np.asarray([(0.25 * e, 0.25 * e), (0.75 * e, 0.25 * e), (0.25 * e, 0.75 * e), (0.75 * e, 0.75 * e)], np.float32)
    cls = (np.arange(A * N).reshape(A, N) % 4).astype(np.int32)
    env.set_navigation(targets, cls, cell, origin=(0.0, 0.0), shape=(side, side), clearance=0.0, lookahead=2)
    return env, dict(cell=cell, side=side, targets=targets, cls=cls)


def part_b(args, say):
    say("")
    say("(b) nav_pref_kernel per launch beside the ORCA-only step it precedes (ca_profile, 40 steps, every launch timed on its own dispatch)")
    for A, N, kw in ((4096, 64, {}), (1, 16384, dict(tiled="grid"))):
        env, nav = crowd_env(A, N, **kw)
        for _ in range(5):
            env.nav_pref(); env.orca_step()
        env.profile(1); env.profile_read()
        for _ in range(40):
            env.nav_pref(); env.orca_step()
        prof = env.profile_read(); env.profile(0)
        sn, sms = prof["step_kernel"]
        say("  %5d x %-5d %s grid %d x %d: nav_pref_kernel %d x %.2f us; solve launches %d x %.2f us = %.2f us per step"
            % (A, N, "(tiled, grid)" if kw else "", nav["side"], nav["side"], prof["reset_kernels"][0], prof["reset_kernels"][1] * 1e3, sn, sms * 1e3,
               sn * sms * 1e3 / 40))
        env.close()


def torch_pref(env, nav):
    """the same preferred velocities with torch gathers on the device (one set, lookahead 2, nobody done / absent)"""
    dev = torch.device("cuda", env.device)
    side, cell = nav["side"], float(np.float32(nav["cell"]))
    ics = float(np.float32(1.0) / np.float32(nav["cell"]))
    nxt = torch.stack([torch.as_tensor(env.nav_field(0, k)[1].astype(np.int64)).reshape(-1) for k in range(4)]).to(dev)     # [G, cells]
    cls = torch.as_tensor(nav["cls"].astype(np.int64)).to(dev)
    off = torch.as_tensor(np.asarray([dx + side * dy for dx, dy in _lib.NAV_OFFSETS] + [0, 0], np.int64)).to(dev)
    px, py = env.field_tensor(_lib.FLD_POS_X), env.field_tensor(_lib.FLD_POS_Y)
    gx, gy = env.field_tensor(_lib.FLD_GOAL_X), env.field_tensor(_lib.FLD_GOAL_Y)
    prx, pry = env.field_tensor(_lib.FLD_PREF_X), env.field_tensor(_lib.FLD_PREF_Y)
    base = cls * (side * side)
    flat = nxt.reshape(-1)

    def call():
        cx = torch.clamp(torch.floor(px * ics), 0, side - 1).long()
        cy = torch.clamp(torch.floor(py * ics), 0, side - 1).long()
        w = cy * side + cx
        k1 = flat[base + w]
        w1 = w + off[k1]
        k2 = flat[base + w1]
        w2 = w1 + off[k2]
        own = (k1 >= 8) | (k2 == 8)
        tx = torch.where(own, gx, (((w2 % side).float() + 0.5) * cell).double())
        ty = torch.where(own, gy, ((torch.div(w2, side, rounding_mode="floor").float() + 0.5) * cell).double())
        dx, dy = tx - px.double(), ty - py.double()
        ln = torch.sqrt(dx * dx + dy * dy)
        zero = ln == 0
        prx.copy_(torch.where(zero, torch.ones_like(dx), dx / ln).float())
        pry.copy_(torch.where(zero, torch.zeros_like(dy), dy / ln).float())
    return call


def timed(env, call, seconds):
    env.sync()
    n, t0 = 0, time.perf_counter()
    while True:
        call(); n += 1
        env.sync()
        if time.perf_counter() - t0 >= seconds:
            break
    return env.A * env.N * T * n / (time.perf_counter() - t0)


def part_c(args, say):
    say("")
    say("(c) %d navigated steps: rollout_nav(%d) | a Python loop of torch gathers + PREF writes + orca_step -- G agent-steps/s: median  min .. max  (every repeat)" % (T, T))
    for A, N in ((1024, 16), (4096, 64)):
        env, nav = crowd_env(A, N)
        pref = torch_pref(env, nav)
        pref(); a = env.get(_lib.FLD_PREF_X)
        env.nav_pref(); bb = env.get(_lib.FLD_PREF_X)
        same = float((a == bb).mean())

        def loop():
            for _ in range(T):
                pref(); env.orca_step()
        vs = [("rollout_nav(T): one call", lambda: env.rollout_nav(T)), ("T x (torch gathers + orca_step)", loop)]
        res = {n: [] for n, _ in vs}
        for _, c in vs:
            c(); env.sync()
        for _ in range(args.repeat):
            for n, c in vs:
                res[n].append(timed(env, c, args.seconds))
        say("  %d x %d agents, grid %d x %d, 4 targets (the torch loop's PREF_X equals the kernel's in %.1f %% of the rows)" % (A, N, nav["side"], nav["side"], 100 * same))
        for n, _ in vs:
            say("    %-36s %s" % (n, stat(res[n], 1e9, "%.4f")))
        med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
        say("    one call / loop (medians): %.2f" % (med[vs[0][0]] / med[vs[1][0]]))
        env.close()


# ---- (e) -------------------------------------------------------------------------------------------------------------------------------
def part_e(args, say):
    say("")
    say("(e) %d policy steps (64-64-1): rollout_nav_policy | the Python loop observe / policy_actions / step_nav | rollout_policy -- "
        "G agent-steps/s: median  min .. max  (every repeat)" % T)
    rs = np.random.RandomState(0)
    layers = [((rs.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32), np.zeros(o, np.float32)) for i, o in ((64, 64), (64, 64), (64, 1))]
    for A, N in ((1024, 16), (4096, 64)):
        env, nav = crowd_env(A, N)
        env.set_policy(layers, out="clip", limit=float(np.pi / 4))

        def loop():
            for _ in range(T):
                env.observe()
                env.step_nav(env.policy_actions(), with_obs=False)
        vs = [("rollout_nav_policy(T): one call", lambda: env.rollout_nav_policy(T, record=(), returns=False)),
              ("T x (observe, policy_actions, step_nav)", loop),
              ("rollout_policy(T): one call", lambda: env.rollout_policy(T, record=(), returns=False))]
        res = {n: [] for n, _ in vs}
        for _, c in vs:
            c(); env.sync()
        for _ in range(args.repeat):
            for n, c in vs:
                res[n].append(timed(env, c, args.seconds))
        say("  %d x %d agents, grid %d x %d, 4 targets" % (A, N, nav["side"], nav["side"]))
        for n, _ in vs:
            say("    %-42s %s" % (n, stat(res[n], 1e9, "%.4f")))
        med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
        say("    one call / loop (medians): %.2f;  navigated / straight-line policy rollout (medians): %.2f"
            % (med[vs[0][0]] / med[vs[1][0]], med[vs[0][0]] / med[vs[2][0]]))
        # the two kernels on their own dispatches: nav_act alone, then both round the step (the mean of the two: reward = 2 x mean - act)
        act = torch.zeros((A, N), dtype=torch.float32, device=torch.device("cuda", env.device))
        env.profile(1); env.profile_read()
        for _ in range(40):
            env.nav_act(act)
        n_a, ms_a = env.profile_read()["reset_kernels"]
        for _ in range(40):
            env.step_nav(act, with_obs=False, stats=True)
        prof = env.profile_read(); env.profile(0)
        n_b, ms_b = prof["reset_kernels"]
        sn, sms = prof["step_kernel"]
        assert n_a == 40 and n_b == 80, (n_a, n_b)
        say("    nav_act_kernel %d x %.2f us; nav_reward_kernel (CA_F_STATS) %d x %.2f us; solve launches %d x %.2f us = %.2f us per step"
            % (n_a, ms_a * 1e3, n_b - n_a, (2 * ms_b - ms_a) * 1e3, sn, sms * 1e3, sn * sms * 1e3 / 40))
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nav_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nav_cost.py measures on the GPU: no device found")
    lines = ["sources %s; %d alternated repeats" % (b.source_sha(), args.repeat)]

    def say(text=""):
        print(text, flush=True)
        lines.append(text)
    for part, fn in (("a", part_a), ("b", part_b), ("c", part_c), ("e", part_e)):
        if part in args.only.split(","):
            try:
                fn(args, say)
            except RuntimeError as ex:          # (a part the library refuses is reported, the others still run)
                say("(%s) not measured: %s" % (part, ex))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
