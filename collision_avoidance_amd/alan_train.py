"""The ALAN action-space trainer (reference collision_avoidance/ALAN/Train_ALAN_action_space.py:7-135) on the batched HIP
environment: the reference's simulated annealing over action sets, run for `n_chains` independent chains at once.

Every round evaluates ONE proposal per chain, and all chains' proposals are evaluated together: round r is one episode set of
`n_chains * num` arenas, chain c on arenas c*num .. c*num+num-1, each arena with its chain's action set
(`ca_alan_configure_per_arena`).  Through `Collision_Avoidance_Sim.reset()` those are the global arenas
r*n_chains*num + c*num + j of the seed: every evaluation sees fresh worlds, as every reset() of the reference does.  The
accept / reject step is per chain and stays on the host.

Decision streams: chain c draws from its own `random.Random(seed + c)` (the reference's `random.uniform`) and
`np.random.RandomState(seed + c)` (its `np.random.choice` / `np.random.normal`), in the reference's order, so chain 0 makes the
reference's decisions under `random.seed(seed); np.random.seed(seed)`.  In the reference the worlds draw from the same global
`random` as these decisions; here the worlds come from the device's counter-based streams (seed, global arena), so the two are
independent: a chain's decisions do not depend on the worlds it was scored in, nor on how many chains run beside it.

Deliberate deviation: the reference edits `self.actions` in place -- `apply_modification` returns the list
it was given, and `actions_opt` aliases it (:17-19, :84-125) --, so a rejected proposal is never undone and train() returns
the final random-walk state.  Here proposals are copies, a rejection keeps the previous set and `actions_opt` is a snapshot of
the best set evaluated.  A proposal of more than 32 actions (CA_ALAN_MAX_ACTIONS) is rejected without an evaluation; the
draws it would have consumed (the acceptance uniform) are consumed all the same, so the streams stay aligned.
"""
import math
import random

import numpy as np

MAX_ACTIONS = 32   # CA_ALAN_MAX_ACTIONS


def symmetric_likelihood(dist):
    """Train_ALAN_action_space.py:132-135: scipy.stats.norm.pdf(dist) / 0.5, restated without scipy.  norm.pdf evaluates
    exp(-x**2/2) / sqrt(2 pi) with numpy's exp on an ARRAY (its vector loop): math.exp, and numpy's exp of a scalar, differ
    from that in the last bit on some inputs, so the same array form is used here."""
    x = np.array([dist], np.float64)
    return float((np.exp(-x ** 2 / 2.0) / np.sqrt(2 * np.pi))[0]) / 0.5


def action_dist(p1, p2):
    """Train_ALAN_action_space.py:129-130."""
    return math.sqrt((p1[0] - p2[0]) ** 2 + (p1[1] - p2[1]) ** 2)


def save_act(path, actions):
    """Write an action set in the reference's `.act` format (Train_ALAN_action_space.py:153-156: `str(actions)`, the repr
    of a list of tuples); tools/alan_actions.load_actions reads it back."""
    with open(path, "w") as f:
        f.write(str([tuple(a) for a in actions]))


class _Chain(object):
    """One annealing chain: the state of one reference MCMC_trainer."""

    def __init__(self, seed):
        self.rng = random.Random(seed)              # the reference's `random.uniform`
        self.nrng = np.random.RandomState(seed)     # the reference's `np.random.*`
        self.actions = [(1, 0), self.random_action()]   # :16
        self.eval = self.eval_opt = None
        self.actions_opt = list(self.actions)
        self.history = []

    def random_action(self):                        # :50-52
        angle = self.rng.uniform(-math.pi, math.pi)
        return math.cos(angle), math.sin(angle)

    def select_modification(self):                  # :70-74 (0 edit, 1 remove, 2 add)
        if len(self.actions) <= 1:
            return 2
        return int(self.nrng.choice(3, p=[0.8, 0.1, 0.1]))

    def propose(self, modification):
        """:77-126 on a copy of the current set: returns (dist, proposal)."""
        actions = list(self.actions)
        if modification == 1:                       # :100-112
            index = self.nrng.choice(range(1, len(actions)))
            old_action = actions[index]
            actions.remove(old_action)
            min_dist = 10
            for act in actions:
                d = action_dist(act, old_action)
                if d < min_dist:
                    min_dist = d
            return min_dist, actions
        # :86-97 edit (action 0 stays), :115-126 add (any action may be the parent)
        index = self.nrng.choice(range(0 if modification == 2 else 1, len(actions)))
        angle = np.arctan2(actions[index][1], actions[index][0])
        new_angle = self.nrng.normal(angle, math.pi)
        new_action = (math.cos(new_angle), math.sin(new_angle))
        d = action_dist(actions[index], new_action)
        if modification == 2:
            actions.append(new_action)
        else:
            actions[index] = new_action
        return d, actions


class MCMC_trainer(object):
    """Train_ALAN_action_space.py:7-47 for `n_chains` chains at once; `.train()` returns the best action set (of chain
    `best_chain`) as a list of tuples.

    Attributes after train(): eval_opt / actions_opt (best over all chains), chains[c].eval_opt / .actions_opt, and
    history[c]: one dict per round (round 0 = the initial evaluation) with the evaluation (None for a proposal rejected for
    its size), the accepted flag and the size of the evaluated set, plus the modification, dist, likelihood and the set.

    evaluate_ttimes: a hook for tests -- called as evaluate_ttimes(action_sets, round) with one set per chain, it returns
    the TTimes [n_chains][num] of the `num` runs of each; default: the batched HIP episode set described in the module doc.
    """

    def __init__(self, numAgents=50, scenario="crowd", numRounds=10, *, n_chains=1, num=3, seed=0, device=0,
                 evaluate_ttimes=None):
        if numRounds < 2:   # (the reference divides by numRounds - 1, :25)
            raise ValueError("MCMC_trainer: numRounds must be at least 2 (got %r)" % (numRounds,))
        if n_chains < 1 or num < 1:
            raise ValueError("MCMC_trainer: n_chains and num must be positive")
        self.numAgents, self.scenario, self.numRounds = numAgents, scenario, int(numRounds)
        self.n_chains, self.num, self.seed, self.device = int(n_chains), int(num), seed, device
        self._evaluate_ttimes = evaluate_ttimes or self._gpu_ttimes
        self._sim = None
        self.rounds_done = 0
        self.chains = [_Chain(seed + c) for c in range(self.n_chains)]
        # :19-20 the initial evaluation = round 0
        evals = self._scores([ch.actions for ch in self.chains], 0)
        for ch, ev in zip(self.chains, evals):
            ch.eval = ch.eval_opt = ev
            ch.history.append(dict(round=0, modification=None, dist=None, likelihood=None, eval=ev, accepted=True,
                                   n_actions=len(ch.actions), actions=list(ch.actions)))
        self.init_temp, self.final_temp = 0.9, 0.1    # :22-25
        self.temp = self.init_temp
        self.delta_temp = (self.final_temp - self.init_temp) / (self.numRounds - 1)

    # ---- evaluation ------------------------------------------------------------------------------
    def _gpu_ttimes(self, action_sets, r):
        """One episode set of n_chains * num arenas; chain c's set on arenas c*num .. c*num+num-1 (:55-67)."""
        from .alan import Collision_Avoidance_Sim
        arena_sets = [list(s) for s in action_sets for _ in range(self.num)]
        if self._sim is None:   # (any numAgents: above 1024 the simulator asks for a tiled handle on its own, alan.py)
            self._sim = Collision_Avoidance_Sim(numAgents=self.numAgents, scenario=self.scenario, device=self.device,
                                                seed=self.seed, n_arenas=self.n_chains * self.num, arena_actions=arena_sets)
        else:
            self._sim.reset(arena_actions=arena_sets)
        tt = np.atleast_1d(self._sim.run_sim(mode=1)[2])
        return tt.reshape(self.n_chains, self.num)

    def _scores(self, action_sets, r):
        tts = self._evaluate_ttimes(action_sets, r)
        out = []
        for c in range(len(action_sets)):
            total_score = 0                         # :56-67, summed in order
            for j in range(self.num):
                total_score += float(tts[c][j])
            out.append(total_score / self.num)
        return out

    # ---- annealing -------------------------------------------------------------------------------
    def train(self):
        """:27-47, every chain once per round."""
        for _ in range(self.numRounds):
            r = self.rounds_done + 1
            mods, dists, props = [], [], []
            for ch in self.chains:
                m = ch.select_modification()
                d, p = ch.propose(m)
                mods.append(m); dists.append(d); props.append(p)
            fits = [len(p) <= MAX_ACTIONS for p in props]
            # a proposal too large to evaluate keeps its arenas busy with the chain's current set (result unused)
            evals = self._scores([p if ok else ch.actions for p, ok, ch in zip(props, fits, self.chains)], r)
            for c, ch in enumerate(self.chains):
                new_eval = evals[c] if fits[c] else None
                if fits[c] and new_eval < ch.eval_opt:     # :37-39
                    ch.actions_opt, ch.eval_opt = list(props[c]), new_eval
                u = ch.rng.uniform(0, 1)                    # :41 (drawn whether or not the proposal was evaluated)
                lik = symmetric_likelihood(dists[c])
                accepted = False
                if fits[c]:
                    try:
                        bound = lik * math.exp((ch.eval - new_eval) / self.temp)
                    except OverflowError:
                        bound = math.inf
                    accepted = u < bound
                if accepted:                                # :42-43
                    ch.actions, ch.eval = props[c], new_eval
                ch.history.append(dict(round=r, modification=mods[c], dist=dists[c], likelihood=lik, eval=new_eval,
                                       accepted=accepted, n_actions=len(props[c]), actions=list(props[c])))
            self.temp -= self.delta_temp                    # :45
            self.rounds_done = r
        return self.actions_opt

    @property
    def best_chain(self):
        return int(np.argmin([ch.eval_opt for ch in self.chains]))

    @property
    def eval_opt(self):
        return self.chains[self.best_chain].eval_opt

    @property
    def actions_opt(self):
        return [tuple(a) for a in self.chains[self.best_chain].actions_opt]

    @property
    def history(self):
        return [ch.history for ch in self.chains]

    def close(self):
        if self._sim is not None and self._sim.vec is not None:
            self._sim.vec.close()
            self._sim.vec = None
