#!/usr/bin/env python3
"""What per-arena agent counts (ca_set_agent_counts) cost: time per step and agent-steps/s over the PRESENT agents, of the full
step and of the ORCA-only step on one handle shape, three ways, alternated --

  params = config   the AgentParams kernels with the arrays set equal to the config values: the baseline (the kernels a handle
                    with counts builds on, without the counts)
  counts = N        the ArenaCounts kernels with every count equal to n_agents: the same simulation, bit for bit -- the cost of
                    the count itself (a load per arena, a compare per candidate)
  counts 16..N      counts drawn uniformly from [16, n_agents] (seeded): what idle lanes cost, per present agent

  python tools/agent_counts_cost.py [--shape 4096x64] [--steps 300] [--warmup 60] [--repeat 3] [--out FILE]

The crowd workload of bench.py's rules (bench_params: a new goal whenever one is reached, max_neighbors 10, neighbor_dist 5) in
the walled box of the crowd arena; the crowd generator's geometry is a function of n_agents and is refused with counts, so the
states of all three handles are drawn uniformly in the box, like the box tests'.  The three handles are timed in turn, --repeat
rounds; every timed run is --steps steps, wall clock around the loop, the stream drained at both ends; all repeats are printed.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collision_avoidance_amd import _lib, build as b, scenarios  # noqa: E402
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv  # noqa: E402

PARAMS = ("radius", "max_speed", "time_horizon", "time_horizon_obst")
MODES = ("params = config", "counts = N", "counts 16..N")


def make(A, N, mode, seed=0):
    e = scenarios.crowd_envsize(N)
    box = [[(0.0, 0.0), (0.0, e), (e, e), (e, 0.0)]]
    g = VecCollisionAvoidanceEnv(A, N, scenario=None, params=scenarios.bench_params(N, 5.0, 10), seed=seed, obstacles=box)
    rng = np.random.RandomState(seed)
    pos, goal = rng.uniform(0.5, e - 0.5, (2, A, N, 2))
    d = goal - pos
    pref = d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-9)
    for name, v in (("POS_X", pos[..., 0]), ("POS_Y", pos[..., 1]), ("PREF_X", pref[..., 0]), ("PREF_Y", pref[..., 1]),
                    ("GOAL_X", goal[..., 0]), ("GOAL_Y", goal[..., 1]), ("GOAL2_X", goal[..., 0]), ("GOAL2_Y", goal[..., 1])):
        g.set(getattr(_lib, "FLD_" + name), v)
    if mode == "params = config":
        g.set_agent_params(**{k: np.full((A, N), getattr(g.cfg, k), np.float32) for k in PARAMS})
    elif mode == "counts = N":
        g.set_agent_counts(np.full(A, N, np.int32))
    else:
        g.set_agent_counts(np.random.RandomState(seed + 1).randint(min(16, N), N + 1, A).astype(np.int32))
    li = g.launch_info()
    assert li["agent_counts"] == (mode != "params = config") and li["lanes_per_agent"] == 1, li
    return g


def timed(g, full, steps, act):
    t0 = time.perf_counter()
    for _ in range(steps):
        if full:
            g.step(act, with_obs=True)
        else:
            g.orca_step()
    g.sync()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="4096x64")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    A, N = (int(v) for v in a.shape.split("x"))
    envs = {m: make(A, N, m) for m in MODES}
    present = {m: int(g.agent_counts().sum()) for m, g in envs.items()}
    act = np.random.RandomState(0).uniform(-1, 1, (A, N)).astype(np.float32)
    if envs[MODES[0]].use_torch:
        import torch
        act = torch.as_tensor(act, device=torch.device("cuda", envs[MODES[0]].device))
    res = {(m, full): [] for m in MODES for full in (True, False)}
    for full in (True, False):
        for m in MODES:
            timed(envs[m], full, a.warmup, act)
        for _ in range(a.repeat):            # alternated: one run of each handle per round
            for m in MODES:
                res[(m, full)].append(timed(envs[m], full, a.steps, act))
    lines = ["sources %s; shape %s, steps %d, warmup %d, %d alternated repeats; us per step (every repeat) and G agent-steps/s over the present "
             "agents (best repeat)" % (b.source_sha(), a.shape, a.steps, a.warmup, a.repeat),
             "%-16s %9s  %-34s %8s  %-34s %8s" % ("handle", "present", "full step us", "G/s", "ORCA only us", "G/s")]
    for m in MODES:
        f, o = res[(m, True)], res[(m, False)]
        lines.append("%-16s %9d  %-34s %8.3f  %-34s %8.3f" % (m, present[m], " ".join("%.1f" % (t * 1e6) for t in f), present[m] / min(f) / 1e9,
                                                              " ".join("%.1f" % (t * 1e6) for t in o), present[m] / min(o) / 1e9))
    base_f, base_o = res[(MODES[0], True)], res[(MODES[0], False)]
    lines.append("spread of the baseline's own repeats: full step %.2f %%, ORCA only %.2f %%" %
                 (100 * (max(base_f) / min(base_f) - 1), 100 * (max(base_o) / min(base_o) - 1)))
    for m in MODES[1:]:
        lines.append("%-16s time per step / baseline (best repeats): full step %.4f, ORCA only %.4f" %
                     (m, min(res[(m, True)]) / min(base_f), min(res[(m, False)]) / min(base_o)))
    for g in envs.values():
        g.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
