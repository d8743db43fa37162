"""The action-space trainer's decisions (collision_avoidance_amd/alan_train.py) against the reference's own trainer
(Train_ALAN_action_space.py:7-135) recorded by tests/golden/make_golden_mcmc.py: with the same stub scores injected through
the evaluation hook, chain 0 makes the reference's decisions under the same seed, value for value."""
import importlib.util
import os

import numpy as np
import pytest

from collision_avoidance_amd import alan_train
from tools import alan_actions

HERE = os.path.dirname(os.path.abspath(__file__))


def _stub_ttime():
    spec = importlib.util.spec_from_file_location("make_golden_mcmc", os.path.join(HERE, "golden", "make_golden_mcmc.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.stub_ttime


def _stub_hook(num, calls=None):
    f = _stub_ttime()

    def hook(action_sets, r):
        if calls is not None:
            calls.append((r, [list(s) for s in action_sets]))
        return [[f(s)] * num for s in action_sets]
    return hook


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "mcmc_trainer.npz"))


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_decisions_match_the_reference_trainer(golden, seed):
    rounds = int(golden["rounds"])
    k = "s%d_" % seed
    t = alan_train.MCMC_trainer(20, "blocks", rounds, n_chains=1, num=3, seed=seed, evaluate_ttimes=_stub_hook(3))
    ch = t.chains[0]
    np.testing.assert_array_equal(np.asarray(ch.history[0]["actions"], np.float64), golden[k + "init_actions"])
    assert ch.history[0]["eval"] == float(golden[k + "init_eval"])
    best = t.train()
    h = ch.history[1:]
    assert len(h) == rounds
    for i, r in enumerate(h):
        what = "seed %d round %d" % (seed, i)
        assert r["modification"] == int(golden[k + "mod"][i]), what
        assert r["dist"] == float(golden[k + "dist"][i]), what
        n = int(golden[k + "n_prop"][i])
        assert r["n_actions"] == n, what
        np.testing.assert_array_equal(np.asarray(r["actions"], np.float64), golden[k + "proposal"][i, :n], err_msg=what)
        # scipy's norm.pdf (np.exp) against math.exp: the same value to the last bit on these inputs
        assert r["likelihood"] == float(golden[k + "lik"][i]), (what, r["likelihood"], float(golden[k + "lik"][i]))
        assert r["eval"] == float(golden[k + "new_eval"][i]), what
        assert r["accepted"] == bool(golden[k + "accepted"][i]), what
    assert ch.eval == float(golden[k + "eval"][-1])
    assert t.eval_opt == float(golden[k + "eval_opt"][-1])
    np.testing.assert_array_equal(np.asarray(best, np.float64), golden[k + "best"])
    # the running values, round by round (re-run: the trainer keeps only the final ones)
    t2 = alan_train.MCMC_trainer(20, "blocks", rounds, n_chains=1, num=3, seed=seed, evaluate_ttimes=_stub_hook(3))
    cur, opt = t2.chains[0].eval, t2.chains[0].eval_opt
    for i, r in enumerate(t.chains[0].history[1:]):
        if r["eval"] < opt:
            opt = r["eval"]
        if r["accepted"]:
            cur = r["eval"]
        assert cur == float(golden[k + "eval"][i]) and opt == float(golden[k + "eval_opt"][i]), i


def test_chains_are_independent_streams():
    """Chain c draws from seed + c alone: chain 1 of a two-chain run is chain 0 of a run seeded one higher."""
    a = alan_train.MCMC_trainer(20, "crowd", 25, n_chains=3, num=2, seed=4, evaluate_ttimes=_stub_hook(2))
    b = alan_train.MCMC_trainer(20, "crowd", 25, n_chains=1, num=2, seed=5, evaluate_ttimes=_stub_hook(2))
    a.train(); b.train()
    assert a.history[1] == b.history[0]
    assert a.history[0] != a.history[1]
    assert a.eval_opt == min(ch.eval_opt for ch in a.chains)
    for hist in a.history:
        opts = np.minimum.accumulate([r["eval"] for r in hist])
        assert (np.diff(opts) <= 0).all()


def test_batched_evaluation_layout():
    """Every round evaluates every chain's proposal in one call (round 0 = the initial sets), in chain order."""
    calls = []
    t = alan_train.MCMC_trainer(20, "crowd", 5, n_chains=4, num=3, seed=0, evaluate_ttimes=_stub_hook(3, calls))
    t.train()
    assert [r for r, _ in calls] == list(range(6))
    for r, sets in calls:
        assert len(sets) == 4
        for c in range(4):
            assert sets[c] == t.history[c][r]["actions"]


def test_score_is_the_ordered_mean_over_num_runs():
    vals = [[0.1, 0.2, 0.7], [1e16, 1.0, -1e16]]
    t = alan_train.MCMC_trainer(20, "crowd", 2, n_chains=2, num=3, seed=0, evaluate_ttimes=lambda s, r: vals)
    assert t.chains[0].eval == (0 + 0.1 + 0.2 + 0.7) / 3 and t.chains[1].eval == ((0 + 1e16) + 1.0 - 1e16) / 3


@pytest.mark.parametrize("rounds", [1, 0, -3])
def test_num_rounds_below_two_is_an_error(rounds):
    with pytest.raises(ValueError, match="numRounds"):
        alan_train.MCMC_trainer(20, "crowd", rounds, evaluate_ttimes=_stub_hook(3))


def test_proposal_over_32_actions_is_rejected_unevaluated():
    """A proposal beyond CA_ALAN_MAX_ACTIONS is rejected without an evaluation; the draws the reference would make for
    it (the acceptance uniform) are consumed all the same: after every round the chain's `random` stream stands where the
    reference's stands -- the initial random_action and one uniform per round (:16, :41)."""
    import random
    calls = []
    t = alan_train.MCMC_trainer(20, "crowd", 40, n_chains=1, num=3, seed=3, evaluate_ttimes=_stub_hook(3, calls))
    ch = t.chains[0]
    ch.actions = [(1, 0)] + [(float(np.cos(0.1 * k)), float(np.sin(0.1 * k))) for k in range(1, 32)]
    ch.eval = 1e9          # from here the chain accepts nearly every proposal it may evaluate: it stays at 31 .. 32
    t.train()
    expect = random.Random(3)
    expect.uniform(-np.pi, np.pi)
    for _ in range(40):
        expect.uniform(0, 1)
    assert ch.rng.getstate() == expect.getstate()
    big = [r for r in ch.history[1:] if r["n_actions"] > 32]
    assert big, "no proposal over 32 actions in this run (pick another seed)"
    for r in big:
        assert r["modification"] == 2 and r["eval"] is None and not r["accepted"]
    assert all(len(s) <= 32 for _, sets in calls for s in sets)
    assert all(h["n_actions"] <= 32 for h in ch.history if h["accepted"])
    assert len(ch.actions) <= 32


def test_act_file_round_trip(tmp_path):
    acts = [(1, 0), (0.47793668363831737, -0.8783942887068465), (-0.9934856438219436, 0.11395734078899142)]
    p = tmp_path / "blocks_actions.act"
    alan_train.save_act(str(p), acts)
    assert p.read_text() == str(acts)                     # the reference's own format (Train_ALAN_action_space.py:153-156)
    assert alan_actions.load_actions(str(p)) == acts
    t = alan_train.MCMC_trainer(20, "crowd", 4, n_chains=2, num=1, seed=2, evaluate_ttimes=_stub_hook(1))
    best = t.train()
    alan_train.save_act(str(p), best)
    assert alan_actions.load_actions(str(p)) == [tuple(map(float, a)) for a in best] == t.actions_opt
