"""Per-arena ALAN action sets (ca_alan_configure_per_arena) in every form of the ALAN step -- the four-lanes kernel, the lane
kernel's ALAN instantiation, the three-launch form -- against the oracle, bit for bit; per-arena sets equal to one set equal
ca_alan_configure; ca_alan_actions_arena; and the batched action-space trainer (alan_train.MCMC_trainer) against one-set
Collision_Avoidance_Sim runs of the same worlds."""
import os
import re

import numpy as np
import pytest

from collision_avoidance_amd import _lib, alan, alan_train
from oracle import oracle as o
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _set(n, seed):
    r = np.random.RandomState(seed)
    ang = r.uniform(-np.pi, np.pi, n)
    acts = [(1.0, 0.0)] + [(float(2 * np.cos(x)), float(2 * np.sin(x))) for x in ang[1:]]   # (lengths != 1: normalised)
    if n >= 3:
        acts[2] = (0.0, 0.0)        # the zero-length rule: no rotation
    return acts


SETS = {n: _set(n, 10 + n) for n in (1, 2, 3, 8, 9, 32)}


def _make(over, fn):
    old = {k: os.environ.get(k) for k in over}
    os.environ.update(over)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


FORMS = {"quad": {"CA_QUAD": "1"}, "lane": {"CA_QUAD": "0"}, "three": {"CA_ALAN_FUSED": "0"}}


def _assert_arenas_equal(g, e, arenas, n, what):
    """The GPU handle on `arenas` against an oracle handle configured with that arenas' set of n actions (all its arenas)."""
    pairs = [("pos_x", _lib.FLD_POS_X, o.FLD_POS_X), ("pos_y", _lib.FLD_POS_Y, o.FLD_POS_Y),
             ("vel_x", _lib.FLD_VEL_X, o.FLD_VEL_X), ("vel_y", _lib.FLD_VEL_Y, o.FLD_VEL_Y),
             ("pref_x", _lib.FLD_PREF_X, o.FLD_PREF_X), ("pref_y", _lib.FLD_PREF_Y, o.FLD_PREF_Y),
             ("agent_done", _lib.FLD_AGENT_DONE, o.FLD_AGENT_DONE), ("arrive_step", _lib.FLD_ARRIVE_STEP, o.FLD_ARRIVE_STEP),
             ("step_count", _lib.FLD_STEP_COUNT, o.FLD_STEP_COUNT), ("arena_done", _lib.FLD_ARENA_DONE, o.FLD_ARENA_DONE),
             ("reward", _lib.FLD_REWARD, o.FLD_REWARD), ("action", _lib.FLD_ALAN_ACTION, o.FLD_ALAN_ACTION)]
    for name, gf, of in pairs:
        H._eq(g.get(gf)[arenas], e.get(of)[arenas], "%s %s" % (what, name))
    # CA_F_STATS per-arena counters: exact, but the reward sum (column 5, f64 bits), which the kernels add up atomically
    gs, es = g.get(_lib.FLD_ARENA_STATS)[arenas], e.get(o.FLD_ARENA_STATS)[arenas]
    cols = [0, 1, 2, 3, 4, 6, 7]
    H._eq(gs[:, cols], es[:, cols], what + " arena_stats")
    np.testing.assert_allclose(gs[:, 5].view(np.float64), es[:, 5].view(np.float64), rtol=1e-12, atol=1e-9,
                               err_msg=what + " arena sum_reward")
    for name, gf, of in (("weights", _lib.FLD_ALAN_WEIGHTS, o.FLD_ALAN_WEIGHTS), ("times", _lib.FLD_ALAN_TIMES, o.FLD_ALAN_TIMES)):
        gw, ew = g.get(gf)[arenas], e.get(of)[arenas]             # [arenas, N, n_max] / [arenas, N, n]
        H._eq(gw[..., :n], ew, "%s %s" % (what, name))
        assert not gw[..., n:].any(), what + " " + name + ": rows beyond the arena's set were touched"


def _ragged_run(form, scenario, A, N, sizes, one_launch):
    p = H.scenario_params(scenario, N, max_step=90)
    g = _make(FORMS[form], lambda: H.make_gpu(A, N, scenario, p, seed=8))
    of = [sizes[a % len(sizes)] for a in range(A)]
    g.alan_configure_per_arena([SETS[n] for n in of])
    assert g.n_actions == max(sizes)
    lanes = g.launch_info()["lanes_per_agent"]
    if form != "three":
        assert lanes == (4 if form == "quad" else 1)
    orcs = {}
    for n in sizes:
        e = H.make_oracle(A, N, scenario, p, seed=8)
        e.alan_configure(SETS[n])
        orcs[n] = e
    arenas = {n: np.array([a for a in range(A) if of[a] == n]) for n in sizes}

    def check(what):
        for n in sizes:
            _assert_arenas_equal(g, orcs[n], arenas[n], n, "%s %s n=%d" % (form, what, n))

    rng = np.random.RandomState(6)
    g.profile(1); g.profile_read()
    for s in range(10):                              # the uniforms numpy's choice would consume (ALAN:585)
        u = rng.uniform(0, 1, (A, N))
        g.alan_step(u=u, stats=True)
        for e in orcs.values():
            e.alan_step(u=u, flags=o.F_STATS)
    prof = g.profile_read(); g.profile(0)
    launches = prof["reset_kernels"][0]      # the select / update launches of the three-launch form
    assert launches in ((0, 20) if one_launch is None else ((0,) if one_launch else (20,))), prof
    check("given uniforms")
    for s in range(8):
        g.alan_step(stats=True, with_obs=(s == 7))
        for e in orcs.values():
            e.alan_step(flags=o.F_STATS | (o.F_OBS if s == 7 else 0))
    check("own draws")
    for n in sizes:
        H._eq(g.get(_lib.FLD_OBS)[arenas[n]], orcs[n].get(o.FLD_OBS)[arenas[n]], "%s obs n=%d" % (form, n))
    sc = (np.arange(A) % 31).astype(np.int32) + g.get(_lib.FLD_STEP_COUNT)     # the arenas end at different steps
    g.set(_lib.FLD_STEP_COUNT, sc)
    for e in orcs.values():
        e.set(o.FLD_STEP_COUNT, sc)
    g.alan_rollout(300, stats=True, freeze=True)     # 256 + 44 steps
    for e in orcs.values():
        for s in range(300):
            e.alan_step(flags=o.F_STATS | o.F_FREEZE)
    check("frozen rollout")
    assert g.get(_lib.FLD_ARENA_DONE).all()
    g.close()


@pytest.mark.parametrize("form", ["quad", "lane", "three"])
def test_ragged_sets_fused_sizes(form):
    """Sets of 1, 2, 3, 8 and 9 actions mixed in one handle: each fused form runs them in its one launch."""
    _ragged_run(form, "crowd", 20, 16, [1, 2, 3, 8, 9], one_launch=(form != "three"))   # (lane kernel: 4 arenas per wave)


@pytest.mark.parametrize("form", ["quad", "lane", "three"])
def test_ragged_sets_with_32_actions(form):
    """A 32-action set among them: more than the lane kernel's register-line pool holds, so that handle falls back to the
    three-launch form (as a 32-action set on its own does); the four-lanes kernel keeps it in one launch when its LDS (sized
    by the largest set) fits.  Results unchanged either way."""
    _ragged_run(form, "crowd", 24, 16, [1, 2, 3, 8, 9, 32], one_launch={"quad": None, "lane": False, "three": False}[form])


def test_ragged_sets_lane_kernel_line_table():
    """The lane kernel with the LDS line table ("deadlock": 42 edges) holds 32 actions per lane: one launch, a 32-action set
    beside small ones."""
    _ragged_run("lane", "deadlock", 6, 40, [32, 1, 9], one_launch=True)


def _state(env):
    st = env.get_state()
    return {k: np.asarray(v) for k, v in st.items()}


@pytest.mark.parametrize("form", ["quad", "lane", "three"])
def test_per_arena_with_one_set_equals_configure(form):
    """The same set on every arena through ca_alan_configure_per_arena == ca_alan_configure, bit for bit; and a handle
    switched configure -> per-arena -> configure runs as one that only ever had one set."""
    A, N = 16, 12
    p = H.scenario_params("circle", N, max_step=200)
    a = _make(FORMS[form], lambda: H.make_gpu(A, N, "circle", p, seed=4))
    b = _make(FORMS[form], lambda: H.make_gpu(A, N, "circle", p, seed=4))
    s1, s2, s3 = SETS[8], SETS[3], SETS[9]
    a.alan_configure(s1); b.alan_configure(s1)
    for env in (a, b):
        env.alan_rollout(30, stats=True, freeze=True)
    a.alan_configure_per_arena([s2] * A); b.alan_configure(s2)
    for env in (a, b):
        env.alan_rollout(40, stats=True, freeze=True)
        env.alan_step(stats=True)
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        H._eq(sa[k], sb[k], "%s per-arena == one set: %s" % (form, k))
    a.alan_configure(s3); b.alan_configure(s3)
    for env in (a, b):
        env.alan_rollout(300, stats=True, freeze=True)
    sa, sb = _state(a), _state(b)
    for k in sa:
        H._eq(sa[k], sb[k], "%s back to one set: %s" % (form, k))
    assert a.stats() == b.stats()
    a.close(); b.close()


def _unit(acts):
    xy = np.asarray(acts, np.float64)
    ln = np.sqrt(xy[:, 0] * xy[:, 0] + xy[:, 1] * xy[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ln[:, None] == 0.0, np.array([1.0, 0.0]), xy / ln[:, None])


def test_actions_arena_and_errors():
    A, N = 4, 6
    env = H.make_gpu(A, N, "crowd", H.scenario_params("crowd", N))
    with pytest.raises(RuntimeError, match="configure first"):
        env.alan_actions(0)
    sets = [SETS[3], SETS[1], SETS[32], SETS[9]]
    env.alan_configure_per_arena(sets)
    for a in range(A):
        H._eq(env.alan_actions(a), _unit(sets[a]), "arena %d" % a)
    assert env.get(_lib.FLD_ALAN_WEIGHTS).shape == (A, N, 32)
    env.alan_step()
    w = env.get(_lib.FLD_ALAN_WEIGHTS)
    assert not w[1, :, 1:].any() and not w[0, :, 3:].any()
    env.alan_configure(SETS[8])                             # back to one set for every arena
    for a in range(A):
        H._eq(env.alan_actions(a), _unit(SETS[8]), "one set, arena %d" % a)
    L = _lib.load()
    xy = np.zeros((64, 2)); n = np.ones(A, np.int32)
    n0, n33 = np.array([1, 0, 1, 1], np.int32), np.array([1, 1, 33, 1], np.int32)     # (alive across the calls)
    for args, msg in [((None, n.ctypes.data, 0.2, 2.0, 1 / 60.), "null argument"),
                      ((xy.ctypes.data, None, 0.2, 2.0, 1 / 60.), "null argument"),
                      ((xy.ctypes.data, n0.ctypes.data, 0.2, 2.0, 1 / 60.), r"n_actions\[1\]=0 out of range"),
                      ((xy.ctypes.data, n33.ctypes.data, 0.2, 2.0, 1 / 60.), r"n_actions\[2\]=33 out of range"),
                      ((xy.ctypes.data, n.ctypes.data, 0.0, 2.0, 1 / 60.), "positive"),
                      ((xy.ctypes.data, n.ctypes.data, 0.2, -1.0, 1 / 60.), "positive"),
                      ((xy.ctypes.data, n.ctypes.data, 0.2, 2.0, 0.0), "positive")]:
        rc = L.ca_alan_configure_per_arena(env.h, *args)
        assert rc != 0 and re.search(msg, L.ca_last_error(env.h).decode()), (msg, rc)
    with pytest.raises(RuntimeError, match="arena 4 of 4"):
        env.alan_actions(4)
    with pytest.raises(ValueError, match="3 action sets for 4 arenas"):
        env.alan_configure_per_arena(sets[:3])
    with pytest.raises(RuntimeError, match="out of range"):
        env.alan_configure_per_arena([SETS[1], [], SETS[1], SETS[1]])
    env.alan_step()                                         # the handle still runs its last good configuration
    env.close()


def test_trainer_scores_equal_one_set_runs():
    """Each chain's score in every round == the score of a one-set Collision_Avoidance_Sim(n_arenas=n_chains*num) run of that
    chain's set after as many resets, on that chain's arenas; the same seed gives the same history; eval_opt never grows."""
    C, num, rounds, N = 4, 3, 4, 8
    t = alan_train.MCMC_trainer(N, "crowd", rounds, n_chains=C, num=num, seed=5)
    best = t.train()
    t2 = alan_train.MCMC_trainer(N, "crowd", rounds, n_chains=C, num=num, seed=5)
    t2.train()
    assert t.history == t2.history and best == t2.actions_opt
    t.close(); t2.close()
    for r in range(rounds + 1):
        for c in range(C):
            h = t.history[c][r]
            if h["eval"] is None:
                continue
            sim = alan.Collision_Avoidance_Sim(numAgents=N, scenario="crowd", seed=5, n_arenas=C * num,
                                               online_actions=h["actions"])
            for _ in range(r):
                sim.reset(h["actions"])
            tt = sim.run_sim(1)[2]
            total = 0
            for j in range(num):
                total += float(tt[c * num + j])
            assert h["eval"] == total / num, (r, c, h["eval"], total / num)
            sim.vec.close()
    for c in range(C):
        opts = [t.history[c][0]["eval"]]
        for h in t.history[c][1:]:
            opts.append(min(opts[-1], h["eval"]) if h["eval"] is not None else opts[-1])
        assert opts[-1] == t.chains[c].eval_opt and all(x >= y for x, y in zip(opts, opts[1:]))
    assert t.eval_opt == min(ch.eval_opt for ch in t.chains) and len(best) >= 1
