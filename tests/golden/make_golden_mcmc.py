#!/usr/bin/env python3
"""Generate tests/golden/mcmc_trainer.npz: the decisions of the reference's action-space trainer
(collision_avoidance/ALAN/Train_ALAN_action_space.py:7-135), by IMPORTING the reference's own module.

Runs only where the reference exists (the build container); none of its source is copied.  `ALAN_true` is replaced by a stub
whose run_sim() returns a deterministic TTime that is a function of the action set (`stub_ttime`) and draws nothing, so the
recorded decisions are those of the trainer alone.  apply_modification is patched to pass `list(actions)`: the intended
algorithm without the reference's aliasing (proposals are copies, a rejection keeps the previous set), on the
reference's own code.  Per seed, after `random.seed(seed); np.random.seed(seed)`, one run of numRounds rounds records per
round: the modification, dist, the proposal, the likelihood, the accept decision, eval and eval_opt.

Usage: python tests/golden/make_golden_mcmc.py REFERENCE_ROOT   (the checkout holding collision_avoidance/ALAN/)
"""
import contextlib
import importlib.util
import io
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (0, 1, 7)
ROUNDS = 60
MAXA = 40   # proposal rows stored (padded with NaN)


def stub_ttime(actions):
    """A deterministic score of an action set (no draws): the stand-in for the TTime of run_sim(mode=1)."""
    s = 0.0
    for k, a in enumerate(actions):
        s += (0.37 * a[0] - 0.61 * a[1] + 0.05 * k) ** 2
    return 12.0 + 1.7 * s / len(actions) + 0.05 * (len(actions) - 5) ** 2


def main(ref_root):
    class Sim(object):
        def __init__(self, numAgents=50, scenario="crowd", online_actions=None, visualize=False):
            self.actions = None

        def reset(self, online_actions=None):
            self.actions = list(online_actions)

        def run_sim(self, mode=1):
            return True, 1.0, stub_ttime(self.actions), 1.0

    stub = types.ModuleType("ALAN_true")
    stub.Collision_Avoidance_Sim = Sim
    sys.modules["ALAN_true"] = stub
    spec = importlib.util.spec_from_file_location(
        "ref_train", os.path.join(ref_root, "collision_avoidance/ALAN/Train_ALAN_action_space.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)

    class Rec(T.MCMC_trainer):
        def __init__(self, *a, **kw):
            self.rec = []
            super().__init__(*a, **kw)
            self.init_actions = list(self.actions)
            self.init_eval = self.eval

        def _close_round(self):
            if self.rec and "accepted" not in self.rec[-1]:
                r = self.rec[-1]
                r["accepted"] = self.actions is r["obj"]
                r["eval"] = self.eval             # the chain's current score after the round
                r["eval_opt"] = self.eval_opt

        def select_modification(self, actions, i):
            self._close_round()
            return super().select_modification(actions, i)

        def apply_modification(self, actions, modification):
            dist, new = super().apply_modification(list(actions), modification)
            self.rec.append(dict(mod=int(modification), dist=float(dist), obj=new, proposal=list(new)))
            return dist, new

        def evaluate_action(self, actions, i=0):
            v = super().evaluate_action(actions, i)
            if self.rec and "new_eval" not in self.rec[-1]:
                self.rec[-1]["new_eval"] = v
            return v

        def symmetric_likelihood(self, dist):
            v = super().symmetric_likelihood(dist)
            self.rec[-1]["lik"] = float(v)
            return v

    out = {"seeds": np.array(SEEDS, np.int64), "rounds": np.int64(ROUNDS)}
    for seed in SEEDS:
        random.seed(seed)
        np.random.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            t = Rec(numAgents=20, scenario="blocks", numRounds=ROUNDS)
            best = t.train()
        t._close_round()
        assert len(t.rec) == ROUNDS
        prop = np.full((ROUNDS, MAXA, 2), np.nan)
        for i, r in enumerate(t.rec):
            prop[i, :len(r["proposal"])] = np.asarray(r["proposal"], np.float64)
        k = "s%d_" % seed
        out[k + "init_actions"] = np.asarray(t.init_actions, np.float64)
        out[k + "init_eval"] = np.float64(t.init_eval)
        out[k + "mod"] = np.array([r["mod"] for r in t.rec], np.int64)
        out[k + "dist"] = np.array([r["dist"] for r in t.rec], np.float64)
        out[k + "n_prop"] = np.array([len(r["proposal"]) for r in t.rec], np.int64)
        out[k + "proposal"] = prop
        out[k + "lik"] = np.array([r["lik"] for r in t.rec], np.float64)
        out[k + "accepted"] = np.array([r["accepted"] for r in t.rec], np.bool_)
        out[k + "new_eval"] = np.array([r["new_eval"] for r in t.rec], np.float64)
        out[k + "eval"] = np.array([r["eval"] for r in t.rec], np.float64)
        out[k + "eval_opt"] = np.array([r["eval_opt"] for r in t.rec], np.float64)
        out[k + "best"] = np.asarray(best, np.float64)
        print("seed %d: %d accepted of %d, eval_opt %.6f, best set of %d"
              % (seed, int(out[k + "accepted"].sum()), ROUNDS, t.eval_opt, len(best)))
    path = os.path.join(HERE, "mcmc_trainer.npz")
    np.savez_compressed(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
