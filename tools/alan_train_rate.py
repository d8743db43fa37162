#!/usr/bin/env python3
"""Rate of the action-space trainer's evaluations (Train_ALAN_action_space.py:53-67; collision_avoidance_amd/alan_train.py):
rounds/s and agent-steps/s (ca_stats.agent_steps) of the reference's own configurations -- blocks / 20 agents, crowd / 40,
circle / 40 (Train_ALAN_action_space.py:152-168) -- with n_chains chains evaluated side by side.

A round is what one MCMC round costs: every chain's proposal scored over `num` fresh worlds, i.e. ONE
Collision_Avoidance_Sim(n_arenas=n_chains*num) episode set run to its end (run_sim(mode=1)); each chain gets a random action
set of 2..8 actions of its own (ca_alan_configure_per_arena).  n_chains = 1 uses one set for the handle (ca_alan_configure):
the evaluation loop a caller of Collision_Avoidance_Sim runs without per-arena sets.

  python tools/alan_train_rate.py [--chains 1,64,512] [--rounds 3] [--num 3] [--configs blocks:20,crowd:40,circle:40]

Prints one JSON line per (configuration, n_chains).
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


def random_sets(rng, n):
    out = []
    for _ in range(n):
        k = int(rng.randint(2, 9))
        ang = rng.uniform(-np.pi, np.pi, k - 1)
        out.append([(1.0, 0.0)] + [(float(np.cos(a)), float(np.sin(a))) for a in ang])
    return out


def measure(scenario, n_agents, n_chains, rounds, num, seed=0):
    from collision_avoidance_amd.alan import Collision_Avoidance_Sim
    rng = np.random.RandomState(seed)
    A = n_chains * num

    def sets_for_round():
        s = random_sets(rng, n_chains)
        if n_chains == 1:
            return dict(online_actions=s[0])
        return dict(arena_actions=[a for a in s for _ in range(num)])

    sim = Collision_Avoidance_Sim(numAgents=n_agents, scenario=scenario, seed=seed, n_arenas=A, **sets_for_round())
    sim.run_sim(1)                                          # warm-up round (first launches, LDS attributes)
    t_total, steps, ok = 0.0, 0, 0
    for _ in range(rounds):
        sim.reset(**sets_for_round())
        sim.vec.sync()
        s0 = sim.vec.stats()["agent_steps"]
        t0 = time.perf_counter()
        res = sim.run_sim(1)
        sim.vec.sync()
        t_total += time.perf_counter() - t0
        steps += sim.vec.stats()["agent_steps"] - s0
        ok += int(np.sum(res[0]))
    info = sim.vec.launch_info()
    sim.vec.close()
    return dict(scenario=scenario, n_agents=n_agents, n_chains=n_chains, num=num, arenas=A, rounds=rounds,
                seconds=round(t_total, 4), rounds_per_s=round(rounds / t_total, 4),
                proposals_per_s=round(rounds * n_chains / t_total, 3), agent_steps_per_s=round(steps / t_total, 1),
                agent_steps=int(steps), arenas_finished=ok, lanes_per_agent=info["lanes_per_agent"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chains", default="1,64,512")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--num", type=int, default=3)
    ap.add_argument("--configs", default="blocks:20,crowd:40,circle:40")
    args = ap.parse_args()
    for cfg in args.configs.split(","):
        scen, n = cfg.split(":")
        for c in (int(x) for x in args.chains.split(",")):
            print(json.dumps(measure(scen, int(n), c, args.rounds, args.num)), flush=True)


if __name__ == "__main__":
    main()
