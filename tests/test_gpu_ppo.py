"""PPO sample collection on the GPU (ca_policy_set_heads, ca_policy_evaluate, ca_rollout_policy_sample, ca_gae; include/ca_env.h).
Everything is compared bit for bit:
  * ca_policy_evaluate against the numpy restatement (tests/ppo_scenes.py) -- the shapes, width classes and weight sets of
    tests/test_gpu_policy.py, every combination of heads, both clamps, noise on and off, both out modes;
  * ca_rollout_policy_sample against a twin handle driven call by call through observe / policy_evaluate / step: every field, the
    statistics and every record, on one handle of every form a step is launched in; its advantages and targets against
    gae_reference fed with the call's own records;
  * ca_gae alone on synthetic tensors, and at the row counts around its unroll with done, valid, gamma, lambda and the values at
    their extremes; the heads stay with the slot under fork(); set_policy drops them; refusals advance nothing;
  * the trainer (collision_avoidance_amd/ppo.py): two iterations, and the reinstalled weights against the restatement."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib
from tests import agent_count_scenes as CS
from tests import helpers as H
from tests import policy_scenes as PS
from tests import ppo_scenes as PP
from tests import test_gpu_policy as TP

pytestmark = pytest.mark.gpu
f32 = np.float32
_layers, _sets, _np = TP._layers, TP._sets, TP._np
OUTS = ("actions", "logp", "value", "mean", "log_std")


def _heads(K, P, seed, which="both", state_free=False):
    """(value, log_std) per weight set: value (w [P, K], b [P]) or None, log_std (w [P, K] or None, b [P]) or None"""
    rs = np.random.RandomState(seed)
    n = P or 1
    value = ((rs.standard_normal((n, K)) / np.sqrt(K)).astype(f32), (0.2 * rs.standard_normal(n)).astype(f32))
    lw = (0.5 * rs.standard_normal((n, K)) / np.sqrt(K)).astype(f32)
    log_std = (None if state_free else lw, (-0.5 + 0.2 * rs.standard_normal(n)).astype(f32))
    return (value if which in ("both", "value") else None), (log_std if which in ("both", "log_std") else None)


def _wide_log_std(obs, layers, sets, seed):
    """a log-std head whose rows spread over [-34, 16] on the observations `obs` of the arenas that play them: both clamps are hit"""
    Ws, bs = _sets(layers)
    P, K = Ws[0].shape[0], Ws[-1].shape[2]
    rs = np.random.RandomState(seed)
    lw, lb = rs.standard_normal((P, K)), np.zeros(P)
    for p in range(P):
        rows = obs if sets is None else obs[np.asarray(sets) == p]
        h = PP.hidden_reference(rows.reshape(-1, 64), [W[p] for W in Ws], [b[p] for b in bs]).astype(np.float64)
        raw = h @ lw[p]
        assert raw.max() > raw.min()
        lw[p] *= 50.0 / (raw.max() - raw.min())
        raw = h @ lw[p]
        lb[p] = -9.0 - 0.5 * (raw.max() + raw.min())
    return lw.astype(f32), lb.astype(f32)


def _check_evaluate(g, layers, sets, obs, value, log_std, what, seed=0, clamps=False):
    Ws, bs = _sets(layers)
    A, N = obs.shape[:2]
    mean, ls_raw, val = PP.heads_reference(obs, Ws, bs, sets, value, log_std)
    if clamps:
        assert (ls_raw < -20).any() and (ls_raw > 2).any(), what
    eps = np.random.RandomState(seed + 100).standard_normal((A, N)).astype(f32)
    u = PP.sample_reference(mean, ls_raw, eps, log_std is not None)["u"]
    lim = f32(np.median(np.abs(u)))
    for out, limit in (("identity", np.pi), ("clip", float(lim))):
        g.set_policy(layers, sets=sets, out=out, limit=limit)
        assert g.policy_heads_info() == dict(value=False, log_std=False), what           # set_policy drops the heads
        g.set_policy_heads(value=value, log_std=log_std)
        assert g.policy_heads_info() == dict(value=value is not None, log_std=log_std is not None), what
        for nz in (None, eps):
            got = g.policy_evaluate(nz)
            s = PP.sample_reference(mean, ls_raw, nz, log_std is not None, out, limit)
            want = dict(actions=s["actions"], logp=s["logp"], value=val, mean=mean, log_std=s["log_std"])
            for n in OUTS:
                H._eq(_np(got[n]), want[n], "%s: %s, out=%s, noise %s" % (what, n, out, "off" if nz is None else "on"))
        if out == "clip":
            a = _np(g.policy_evaluate(eps)["actions"])
            assert (a != u).any() and (a == u).any(), what                                   # the limit clips some rows and leaves some
        # with heads installed, policy_actions() returns the bits it always did: the mean row alone, noise added as it is
        H._eq(_np(g.policy_actions(eps)), PS.out_reference((mean + eps).astype(f32), out, limit), what + ": policy_actions, heads installed")


@pytest.mark.parametrize("P", [None, 2], ids=["one_set", "two_sets"])
@pytest.mark.parametrize("hidden", [(64, 64), (16,), (128, 32, 48)], ids=["64-64", "16", "128-32-48"])
def test_policy_evaluate_equals_the_definition(hidden, P):
    """3 x 10 doorway after 5 steps: the 32-row tile is ragged and crosses arenas"""
    A, N = 3, 10
    p = H.scenario_params("doorway", N)
    g = H.make_gpu(A, N, "doorway", p, seed=3)
    layers = _layers(hidden, P, seed=len(hidden))
    sets = None if P is None else np.asarray([1, 0, 1], np.int32)
    act = np.random.RandomState(1).uniform(-np.pi, np.pi, (5, A, N)).astype(f32)
    for t in range(5):
        obs, *_ = g.step(act[t])
    assert np.abs(obs).max() > 0
    K = hidden[-1]
    for which, kw in (("both, both clamps hit", {}), ("value", {}), ("log_std", {}), ("both", dict(state_free=True))):
        value, log_std = _heads(K, P, seed=7, which=which.split(",")[0], **kw)
        clamps = "clamps" in which
        if clamps:
            log_std = _wide_log_std(obs, layers, sets, seed=8)
        _check_evaluate(g, layers, sets, obs, value, log_std, "heads: %s %s" % (which, kw), clamps=clamps)
    g.clear_policy_heads()
    assert g.policy_heads_info() == dict(value=False, log_std=False)
    with pytest.raises(RuntimeError, match="ca_policy_set_heads"):
        g.policy_evaluate()
    g.close()


def test_policy_evaluate_on_a_tiled_handle_with_a_bound_observation():
    """1 x 80 on the tiled path, torch mode: three tiles, the last with 16 rows; one set, and a set per arena"""
    A, N = 1, 80
    p = H.scenario_params("crowd", N)
    g = H.make_gpu(A, N, "crowd", p, seed=2, tiled=True, use_torch=True)
    assert g.tiled_info()["tiled"]
    for _ in range(2):
        obs, *_ = g.step(np.zeros((A, N), f32))
    obs = _np(obs).copy()
    value, log_std = _heads(64, None, seed=3)
    _check_evaluate(g, _layers((64, 64), None, seed=5), None, obs, value, log_std, "tiled, one set")
    value, log_std = _heads(64, 2, seed=4)
    _check_evaluate(g, _layers((64, 64), 2, seed=6), np.asarray([1], np.int32), obs, value, log_std, "tiled, a set per arena")
    g.close()


# ---- ca_rollout_policy_sample against a twin handle driven call by call ---------------------------------------------------------------
RECORDS = ("obs", "actions", "rewards", "dones", "logp", "dist", "values", "row_rewards", "row_dones", "row_valid", "advantages", "targets")


def _sample_case(g, twin, layers, sets, heads, what, steps, hold, weights=None, noise=True, present=None, exact_sum=True,
                 out="identity", limit=np.pi, gamma=0.95, lam=0.9, **kw):
    A, N = g.A, g.N
    R = (steps + hold - 1) // hold
    for e in (g, twin):
        e.set_policy(layers, sets=sets, out=out, limit=limit)
        e.set_policy_heads(value=heads[0], log_std=heads[1])
    nz = np.random.RandomState(17).standard_normal((R, A, N)).astype(f32) if noise else None
    freeze, stats = bool(kw.get("freeze")), bool(kw.get("stats"))
    res = g.rollout_policy_sample(steps, hold=hold, noise=nz, weights=weights, gamma=gamma, lam=lam, record=RECORDS, returns=True,
                                  first_done=True, **kw)
    res = {n: (None if v is None else _np(v)) for n, v in res.items()}
    gf = (_lib.F_STATS if stats else 0) | (_lib.F_AUTORESET if kw.get("autoreset") else 0) | (_lib.F_FREEZE if freeze else 0)
    entry = twin.get(_lib.FLD_ARENA_DONE).copy()
    ev = []
    def act(o, n):
        ev.append({k: _np(v).copy() for k, v in twin.policy_evaluate(n).items()})
        return ev[-1]["actions"]
    rec = PS.rollout_records(twin.observe, act, lambda a: TP._gpu_step(twin, a, gf),
                             lambda: (twin.get(_lib.FLD_REWARD), twin.get(_lib.FLD_ARENA_DONE)), steps, hold, nz)
    twin.observe()
    boot = _np(twin.policy_evaluate()["value"]).copy()
    for name in ("obs", "actions", "rewards", "dones"):
        H._eq(res[name], rec[name].reshape(res[name].shape), "%s: the %s record against the twin's loop" % (what, name))
    if R:
        H._eq(res["logp"], np.asarray([e["logp"] for e in ev]), what + ": logp")
        H._eq(res["dist"], np.asarray([[e["mean"], e["log_std"]] for e in ev]), what + ": dist")
    H._eq(res["values"], np.asarray([e["value"] for e in ev] + [boot]), what + ": values, the bootstrap row included")
    rr, rd, rv = PP.row_records(entry, rec["rewards"].reshape(steps, A, N), rec["dones"].reshape(steps, A), hold, freeze)
    H._eq(res["row_rewards"], rr, what + ": row_rewards")
    H._eq(res["row_dones"], rd, what + ": row_dones")
    H._eq(res["row_valid"], rv, what + ": row_valid")
    ret, fd = PS.returns_and_first_done(entry, rec["rewards"].reshape(steps, A, N), rec["dones"].reshape(steps, A), weights, freeze, present)
    H._eq(res["returns"], ret, what + ": returns")
    H._eq(res["first_done"], fd, what + ": first_done")
    adv, tgt = PP.gae_reference(res["row_rewards"], res["values"], res["row_dones"], res["row_valid"], gamma, lam)
    H._eq(res["advantages"], adv, what + ": advantages against gae_reference on the call's own records")
    H._eq(res["targets"], tgt, what + ": targets")
    TP._same_handles(g, twin, what + ": the call against the loop", stats, exact_sum)
    H._eq(g.get(_lib.FLD_OBS), twin.get(_lib.FLD_OBS), what + ": the observation buffer holds the final state's observation")
    return res


def _both_heads(P=None, seed=9):
    return _heads(64, P, seed)


def _one_call(g, twin, what, sets=None, P=None, **kw):
    """7 steps with hold 3: the last row is held for one step; weights, noise and statistics"""
    layers = _layers((64, 64), P, seed=4)
    w = (f32(0.9) ** np.arange(7)).astype(f32)
    res = _sample_case(g, twin, layers, sets, _both_heads(P), what + ", 7 / 3", 7, 3, weights=w, stats=True, **kw)
    assert np.abs(res["actions"]).max() > 0 and np.abs(res["advantages"]).max() > 0 and np.abs(res["values"][-1]).max() > 0
    g.close(); twin.close()


@pytest.mark.parametrize("quad", ["1", "0"], ids=["four_lanes", "one_lane"])
def test_sample_four_lanes_and_one_lane(monkeypatch, quad):
    monkeypatch.setenv("CA_QUAD", quad)
    A, N = 4, 16
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=11) for _ in range(2))
    assert g.launch_info()["lanes_per_agent"] == (4 if quad == "1" else 1), g.launch_info()
    if quad == "0":   # ca_profile counts the new kernels under kind 3: set-up, 3 heads launches, 7 record launches, the bootstrap, GAE
        layers = _layers((64, 64), None, seed=4)
        for e in (g, twin):
            e.set_policy(layers); e.set_policy_heads(*_both_heads())
        g.profile(1); g.profile_read()
        g.rollout_policy_sample(7, hold=3); twin.rollout_policy_sample(7, hold=3)
        prof = g.profile_read(); g.profile(0)
        assert prof["reset_kernels"][0] == 1 + 3 + 7 + 1 + 1, prof
        assert prof["obs_kernel"][0] == 3 + 1, prof
    _one_call(g, twin, "crowd 4 x 16, CA_QUAD=%s" % quad, sets=np.asarray([1, 0, 0, 1], np.int32), P=2)


def test_sample_per_arena_counts():
    N, counts = 16, (10, 3, 16, 1)
    A = len(counts)
    p, polys, sc = CS.doorway_scene(A, N, 33, max_step=50)
    g, twin = (H.make_gpu(A, N, None, p, seed=33, polys=polys, max_obst_neighbors=16) for _ in range(2))
    for e in (g, twin):
        e.set_agent_counts(np.asarray(counts, np.int32))
        CS.set_state(e, _lib, CS.with_decoys(sc, counts))
    _one_call(g, twin, "per-arena counts", present=g.agent_mask())


def test_sample_tiled_grid():
    A, N = 1, 80
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=21, tiled="grid") for _ in range(2))
    assert g.tiled_info()["tiled"] and g.tiled_grid_info()["grid"]
    _one_call(g, twin, "tiled grid 1 x 80", exact_sum=False)


def test_sample_per_agent_parameters():
    A, N = 4, 20
    p = H.scenario_params("crowd", N)
    radius = np.random.RandomState(3).uniform(0.3, 0.6, (A, N)).astype(f32)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=9, agent_params=dict(radius=radius)) for _ in range(2))
    assert g.launch_info()["agent_params"]
    _one_call(g, twin, "per-agent parameters")


def test_sample_autoreset_an_episode_ends_inside_the_call():
    g, twin = TP._doorway_pair()
    res = _sample_case(g, twin, _layers((64, 64), None, seed=4), None, _both_heads(), "doorway, autoreset", 7, 3, stats=True, autoreset=True)
    assert res["first_done"].tolist() == [4] * 4 and res["row_dones"].tolist() == [[0] * 4, [1] * 4, [0] * 4] and res["row_valid"].all()
    # the row the episode ended in bootstraps from nothing: its advantage is its own delta
    H._eq(res["advantages"][1], (res["row_rewards"][1] - res["values"][1]).astype(f32), "the done row's advantage")
    g.close(); twin.close()


def test_sample_freeze_with_an_arena_frozen_at_entry():
    g, twin = TP._doorway_pair()
    ad = np.asarray([0, 0, 1, 0], np.int32)
    for e in (g, twin):
        e.set(_lib.FLD_ARENA_DONE, ad)
    res = _sample_case(g, twin, _layers((64, 64), None, seed=4), None, _both_heads(), "doorway, freeze", 7, 3,
                       weights=(f32(0.5) ** np.arange(7)).astype(f32), stats=True, freeze=True)
    assert res["first_done"].tolist() == [4, 4, -1, 4]
    assert res["row_valid"].tolist() == [[1, 1, 0, 1], [1, 1, 0, 1], [0, 0, 0, 0]] and res["row_dones"][:, 2].all()
    assert not res["row_rewards"][:, 2].any() and not res["row_rewards"][2].any() and res["row_rewards"][0, 0].any()
    assert not res["advantages"][:, 2].any() and not res["advantages"][2].any()
    H._eq(res["targets"][2], res["values"][2], "a row that is not valid: the target is the value")
    g.close(); twin.close()


def test_sample_zero_steps_and_the_fields_of_rollout_policy():
    """steps = 0: returns, first_done and the bootstrap row alone.  Without a log-std head std = 1, so the effective actions are
    rollout_policy's under the same noise: the fields and the four records are its bits"""
    A, N = 4, 12
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=6) for _ in range(2))
    layers = _layers((64, 64), None, seed=4)
    value, _ = _heads(64, None, 5, which="value")
    for e in (g, twin):
        e.set_policy(layers)
    g.set_policy_heads(value=value)
    before = {n: g.get(getattr(_lib, "FLD_" + n)) for n in TP.STATE}
    out = g.rollout_policy_sample(0, hold=2, returns=True, first_done=True, record=RECORDS)
    for n in TP.STATE:
        H._eq(g.get(getattr(_lib, "FLD_" + n)), before[n], "after zero steps: %s" % n)
    assert not out["returns"].any() and (out["first_done"] == -1).all() and out["obs"].shape == (0, A, N, 64) and out["advantages"].shape == (0, A, N)
    obs0 = g.observe()
    H._eq(out["values"], PP.heads_reference(obs0, *_sets(layers), None, value)[2][None], "zero steps: the bootstrap row")
    nz = (0.3 * np.random.RandomState(2).standard_normal((3, A, N))).astype(f32)
    a = g.rollout_policy_sample(7, hold=3, noise=nz, record=RECORDS, returns=True, first_done=True, stats=True)
    b = twin.rollout_policy(7, hold=3, noise=nz, returns=True, first_done=True, stats=True)
    for n in ("obs", "actions", "rewards", "dones", "returns", "first_done"):
        H._eq(a[n], b[n], "the %s of rollout_policy under the same effective actions" % n)
    TP._same_handles(g, twin, "rollout_policy_sample against rollout_policy", True)
    assert not a["dist"][:, 1].any() and (a["logp"] == ((f32(-0.5) * (nz * nz)).astype(f32) - f32(0.918938533)).astype(f32)).all()
    g.close(); twin.close()


def test_values_only_launch_on_a_ragged_tile_with_a_set_per_arena():
    """3 x 10 doorway after 5 steps, two weight sets, sets = [1, 0, 1]: 10-row padded tiles with a set per arena.  The bootstrap row
    of a call of zero steps is the values-only launch alone: its bits are policy_evaluate()'s value and the definition's"""
    A, N = 3, 10
    p = H.scenario_params("doorway", N)
    g = H.make_gpu(A, N, "doorway", p, seed=3)
    layers = _layers((64, 64), 2, seed=2)
    sets = np.asarray([1, 0, 1], np.int32)
    act = np.random.RandomState(1).uniform(-np.pi, np.pi, (5, A, N)).astype(f32)
    for t in range(5):
        obs, *_ = g.step(act[t])
    assert np.abs(obs).max() > 0
    value, log_std = _heads(64, 2, seed=7)
    g.set_policy(layers, sets=sets)
    g.set_policy_heads(value=value, log_std=log_std)
    out = g.rollout_policy_sample(0, record=("values",))
    assert out["values"].shape == (1, A, N) and out["logp"] is None
    H._eq(out["values"][0], _np(g.policy_evaluate()["value"]), "values only: the bootstrap row against policy_evaluate")
    H._eq(out["values"][0], PP.heads_reference(obs, *_sets(layers), sets, value, log_std)[2], "values only: the bootstrap row against the definition")
    g.close()


# ---- ca_gae alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,A,N", [(5, 3, 10), (6, 2, 70), (1, 3, 10)], ids=["5x3x10", "6x2x70_a_wave_spans_arenas", "one_row"])
def test_gae_on_synthetic_tensors(R, A, N):
    rs = np.random.RandomState(R + N)
    g = H.make_gpu(A, N, "crowd", H.scenario_params("crowd", N), seed=1)
    rew, val = rs.standard_normal((R, A, N)).astype(f32), rs.standard_normal((R + 1, A, N)).astype(f32)
    done = (rs.uniform(size=(R, A)) < 0.3).astype(np.int32)
    valid = (rs.uniform(size=(R, A)) < 0.7).astype(np.int32)
    done[R - 1, 0] = 1
    for v, gamma, lam in ((valid, 0.95, 0.9), (None, 0.99, 1.0)):
        adv, tgt = g.gae(rew, val, done, v, gamma=gamma, lam=lam)
        wa, wt = PP.gae_reference(rew, val, done, v, gamma, lam)
        H._eq(adv, wa, "advantages, valid %s" % (v is not None))
        H._eq(tgt, wt, "targets, valid %s" % (v is not None))
    assert np.abs(adv).max() > 0
    with pytest.raises(ValueError, match="values must be"):
        g.gae(rew, val[:R], done)
    g.close()


def _gae_nan_eq(got, want, what):
    """the same elements are NaN (the header defines no payload or sign for one); every other element has the same bits"""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, np.argwhere(gn)[:8].tolist(), np.argwhere(wn)[:8].tolist())
    H._eq(np.where(gn, f32(0.0), got), np.where(wn, f32(0.0), want), what)


def _gae_case(g, rew, val, done, valid, gamma, lam, what, eq=H._eq):
    with np.errstate(all="ignore"):
        wa, wt = PP.gae_reference(rew, val, done, valid, gamma, lam)
    adv, tgt = g.gae(rew, val, done, valid, gamma=gamma, lam=lam)
    eq(adv, wa, what + ": advantages")
    eq(tgt, wt, what + ": targets")
    return wa, wt


@pytest.mark.parametrize("R", [2, 3, 4, 7, 8, 9])
def test_gae_row_counts_around_the_unroll_and_edge_values(R):
    """R below, at, beside and at twice the kernel's unroll of four rows; 2 x 70 so that a wave spans both arenas.  done and valid at
    their extremes, gamma and lambda at 0 and 1, values at the ends of fp32, and non-finite values behind done and valid, which the
    definition selects away (a product with 0 would keep them)."""
    A, N = 2, 70
    rs = np.random.RandomState(40 + R)
    g = H.make_gpu(A, N, "crowd", H.scenario_params("crowd", N), seed=1)
    rew, val = rs.standard_normal((R, A, N)).astype(f32), rs.standard_normal((R + 1, A, N)).astype(f32)
    rnd_done = (rs.uniform(size=(R, A)) < 0.3).astype(np.int32)
    rnd_valid = (rs.uniform(size=(R, A)) < 0.7).astype(np.int32)
    zeros, ones = np.zeros((R, A), np.int32), np.ones((R, A), np.int32)
    last, first = zeros.copy(), zeros.copy()
    last[R - 1], first[0] = 1, 1
    for done, valid, what in ((rnd_done, rnd_valid, "random done and valid"), (rnd_done, zeros, "valid all zero"), (ones, rnd_valid, "done all one"),
                              (last, None, "done at the last row only"), (first, ones, "done at row 0 only"), (zeros, None, "never done")):
        wa, _ = _gae_case(g, rew, val, done, valid, 0.95, 0.9, "R = %d, %s" % (R, what))
        assert what == "valid all zero" or np.abs(wa).max() > 0
    for gamma, lam in ((0.0, 0.9), (1.0, 0.9), (0.95, 0.0), (0.95, 1.0), (0.0, 0.0), (1.0, 1.0)):
        _gae_case(g, rew, val, rnd_done, rnd_valid, gamma, lam, "R = %d, gamma %g, lambda %g" % (R, gamma, lam))
    # the ends of fp32: subnormal values and rewards, -0, and 1e38, where gamma * v is finite and the sum is not
    tiny = (rs.standard_normal((R + 1, A, N)) * 2.0 ** -135).astype(f32)
    wa, wt = _gae_case(g, (rs.standard_normal((R, A, N)) * 2.0 ** -136).astype(f32), tiny, last, rnd_valid, 0.95, 0.9, "R = %d, subnormal" % R)
    sub = lambda v: ((np.abs(v) > 0) & (np.abs(v) < np.finfo(f32).tiny)).sum()
    assert sub(wa) >= A * N // 2 and sub(wt) >= A * N // 2
    nz = np.where(rs.uniform(size=(R + 1, A, N)) < 0.5, f32(-0.0), f32(0.0)).astype(f32)
    wa, wt = _gae_case(g, nz[:R].copy(), nz, rnd_done, rnd_valid, 0.95, 0.9, "R = %d, signed zeros" % R)
    assert not wa.view(np.uint32).any() and not wt.view(np.uint32).any()                  # gamma lambda * (+0) is +0: every -0 ends as +0
    big_v = (f32(1e38) * rs.choice([-1.0, 1.0], (R + 1, A, N))).astype(f32)
    big_r = (f32(3e38) * rs.choice([-1.0, 1.0], (R, A, N))).astype(f32)
    wa, _ = _gae_case(g, big_r, big_v, last, None, 0.95, 0.9, "R = %d, sums that overflow" % R, eq=_gae_nan_eq)
    assert np.isinf(wa).any() and np.isfinite(wa).any()
    # non-finite values that the definition never reads: the bootstrap row behind done[R - 1], a reward under valid = 0
    for bad in (np.nan, np.inf, -np.inf):
        v2, r2, d2, k2 = val.copy(), rew.copy(), rnd_done.copy(), ones.copy()
        v2[R] = bad
        d2[R - 1] = 1
        r0 = R // 2
        r2[r0, 1], k2[r0, 1] = bad, 0
        with np.errstate(all="ignore"):
            wa, wt = PP.gae_reference(r2, v2, d2, k2, 0.95, 0.9)
        assert np.isfinite(wa).all() and np.isfinite(wt).all(), bad
        _gae_case(g, r2, v2, d2, k2, 0.95, 0.9, "R = %d, %r behind done and valid" % (R, bad))
        # ... and one in the middle: values[r0 + 1] behind done[r0]; row r0 + 1 itself reads it (its advantage is 0 under valid = 0, its
        # target is not a number), the rows at and below r0 do not
        v3, d3, k3 = val.copy(), zeros.copy(), ones.copy()
        v3[r0 + 1, 0] = bad
        d3[r0, 0] = 1
        if r0 + 1 < R:
            k3[r0 + 1, 0] = 0
        with np.errstate(all="ignore"):
            wa, wt = PP.gae_reference(rew, v3, d3, k3, 0.95, 0.9)
        assert np.isfinite(wa[:r0 + 1]).all() and np.isfinite(wt[:r0 + 1]).all() and np.isfinite(wa).all(), bad
        _gae_case(g, rew, v3, d3, k3, 0.95, 0.9, "R = %d, %r in values[%d] behind done[%d]" % (R, bad, r0 + 1, r0), eq=_gae_nan_eq)
    g.close()


def test_gae_of_zero_rows():
    A, N = 3, 10
    g = H.make_gpu(A, N, "crowd", H.scenario_params("crowd", N), seed=1)
    adv, tgt = g.gae(np.zeros((0, A, N), f32), np.ones((1, A, N), f32), np.zeros((0, A), np.int32), np.zeros((0, A), np.int32))
    assert adv.shape == (0, A, N) and tgt.shape == (0, A, N) and adv.dtype == f32 and tgt.dtype == f32
    rew, val = np.ones((1, A, N), f32), np.ones((2, A, N), f32)                            # and the handle computes afterwards
    _gae_case(g, rew, val, np.zeros((1, A), np.int32), None, 0.95, 0.9, "after zero rows")
    g.close()


# ---- configuration, refusals ------------------------------------------------------------------------------------------------------------
def test_heads_stay_with_the_slot_under_fork():
    A, N = 4, 12
    p = H.scenario_params("crowd", N)
    g = H.make_gpu(A, N, "crowd", p, seed=13)
    layers = _layers((64, 64), 4, seed=8)
    sets = np.asarray([2, 0, 3, 1], np.int32)
    heads = _heads(64, 4, seed=2)
    g.set_policy(layers, sets=sets)
    g.set_policy_heads(value=heads[0], log_std=heads[1])
    for _ in range(3):
        g.orca_step()
    g.fork(np.zeros(A, np.int32))
    g.reset_stats()
    obs = g.observe()
    for a in range(1, A):
        H._eq(obs[a], obs[0], "the four slots start from arena 0's state")
    got = g.policy_evaluate()
    want = PP.evaluate_reference(obs, *_sets(layers), sets, heads[0], heads[1])
    for n in OUTS:
        H._eq(got[n], want[n], "after fork: %s, arena a plays set sets[a]" % n)
    assert all((got["value"][a] != got["value"][b]).any() for a in range(A) for b in range(a))
    assert g.policy_heads_info() == dict(value=True, log_std=True)
    g.close()


def test_refusals_advance_nothing():
    import torch
    A, N, steps, hold, R = 4, 12, 7, 3, 3
    p = H.scenario_params("crowd", N)
    g = H.make_gpu(A, N, "crowd", p, seed=6)
    fields = TP.STATE + ("ARENA_STATS",)
    before = {n: g.get(getattr(_lib, "FLD_" + n)) for n in fields}
    dev = torch.device("cuda", g.device)
    t = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device=dev)
    bufs = dict(noise=t((R, A, N), torch.float32, 0.0), returns=t((A, N), torch.float32, -7.5), first_done=t((A,), torch.int32, -7),
                obs_out=t((R, A, N, 64), torch.float32, -7.5), actions_out=t((R, A, N), torch.float32, -7.5),
                logp_out=t((R, A, N), torch.float32, -7.5), dist_out=t((R, 2, A, N), torch.float32, -7.5),
                values_out=t((R + 1, A, N), torch.float32, -7.5), row_rewards_out=t((R, A, N), torch.float32, -7.5),
                row_done_out=t((R, A), torch.int32, -7), row_valid_out=t((R, A), torch.int32, -7),
                advantages_out=t((R, A, N), torch.float32, -7.5), targets_out=t((R, A, N), torch.float32, -7.5))
    full = dict(hold=hold, gamma=0.95)
    full["lambda"] = 1.0
    for n, b in bufs.items():
        full[n], full[n + "_bytes"] = b.data_ptr(), b.numel() * 4
    torch.cuda.synchronize()
    EINVAL, ESIZE, ERANGE = -1, -4, -5
    err = lambda: g.L.ca_last_error(g.h).decode()
    roll = lambda n_steps, flags, kw: g.L.ca_rollout_policy_sample(g.h, n_steps, flags, C.byref(_lib.PolicySampleSeq(**kw)) if kw is not None else None)
    ev = _lib.PolicyEval(value=bufs["returns"].data_ptr())
    keep = []

    def hd(K=64, P=1, **edit):
        vw, vb, lw, lb = np.full((P, K), 0.01, f32), np.zeros(P, f32), np.full((P, K), 0.01, f32), np.zeros(P, f32)
        for name, (idx, v) in edit.get("poke", {}).items():
            dict(value_w=vw, value_b=vb, logstd_w=lw, logstd_b=lb)[name].reshape(-1)[idx] = v
        keep.extend([vw, vb, lw, lb])
        d = _lib.PolicyHeads(value_w=vw.ctypes.data, value_w_bytes=vw.nbytes, value_b=vb.ctypes.data, value_b_bytes=vb.nbytes,
                             logstd_w=lw.ctypes.data, logstd_w_bytes=lw.nbytes, logstd_b=lb.ctypes.data, logstd_b_bytes=lb.nbytes)
        for k, v in edit.get("set", {}).items():
            setattr(d, k, v)
        return d
    # no policy: nothing to put heads on
    assert g.L.ca_policy_set_heads(g.h, C.byref(hd())) == EINVAL and "ca_policy_configure" in err()
    assert roll(steps, 0, full) == EINVAL and "ca_policy_configure" in err()
    assert g.L.ca_policy_evaluate(g.h, None, C.byref(ev)) == EINVAL and "ca_policy_configure" in err()
    layers = _layers((64, 32), None, seed=4)
    g.set_policy(layers)
    # a policy without heads
    assert roll(steps, 0, full) == EINVAL and "ca_policy_set_heads" in err()
    assert g.L.ca_policy_evaluate(g.h, None, C.byref(ev)) == EINVAL and "ca_policy_set_heads" in err()
    bad = [(hd(32, set=dict(value_w=None, value_b=None, logstd_w=None, logstd_b=None)), EINVAL, "neither head"),
           (hd(32, set=dict(value_w=None)), EINVAL, "value_b without value_w"), (hd(32, set=dict(logstd_b=None)), EINVAL, "logstd_w without logstd_b"),
           (hd(32, set=dict(value_w_bytes=32 * 4 - 1)), ESIZE, "value_w needs 128"), (hd(32, set=dict(logstd_b_bytes=3)), ESIZE, "logstd_b needs 4"),
           (hd(32, poke=dict(value_w=(5, np.nan))), ERANGE, "value head, set 0: weight [5]"),
           (hd(32, poke=dict(logstd_b=(0, np.inf))), ERANGE, "logstd head, set 0: the bias")]
    for stage in range(2):
        for d, code, word in bad:
            rc = g.L.ca_policy_set_heads(g.h, C.byref(d))
            assert rc == code and word in err(), (stage, word, rc, err())
        if stage == 0:
            assert g.policy_heads_info() == dict(value=False, log_std=False)
            g.set_policy_heads(*_heads(32, None, seed=1))
        else:
            assert g.policy_heads_info() == dict(value=True, log_std=True)
    size = {n: b.numel() * 4 for n, b in bufs.items()}
    cases = [(steps, 0, None, EINVAL, "null"), (steps, 0, dict(full, hold=0), EINVAL, "hold"), (-1, 0, full, EINVAL, "steps"),
             (steps, _lib.F_NODONE, full, EINVAL, "CA_F_NODONE"), (steps, 64, full, EINVAL, "flags"),
             (steps, 0, dict(full, obs_out=full["obs_out"] + 4), EINVAL, "aligned"),
             (steps, 0, dict(full, values_out=None), EINVAL, "need values_out")]
    cases += [(steps, 0, dict(full, **{n + "_bytes": size[n] - 1}), ESIZE, "%s buffer needs %d" % (n, size[n])) for n in bufs]
    for n_steps, flags, kw, code, word in cases:
        rc = roll(n_steps, flags, kw)
        assert rc == code and word in err() and "ca_rollout_policy_sample:" in err(), (n_steps, flags, word, rc, err())
    gd = _lib.GaeDesc(rewards=full["logp_out"], rewards_bytes=size["logp_out"], values=full["values_out"], values_bytes=size["values_out"] - 1,
                      done=full["row_done_out"], done_bytes=size["row_done_out"], advantages=full["advantages_out"], advantages_bytes=size["advantages_out"])
    assert g.L.ca_gae(g.h, R, C.byref(gd)) == ESIZE and "values buffer needs %d" % size["values_out"] in err()
    assert g.L.ca_gae(g.h, -1, C.byref(gd)) == EINVAL and g.L.ca_gae(g.h, R, None) == EINVAL
    g.sync()
    for n in fields:
        H._eq(g.get(getattr(_lib, "FLD_" + n)), before[n], "after the refusals: %s" % n)
    assert not g.get(_lib.FLD_STEP_COUNT).any()
    assert all((b == (-7 if b.dtype == torch.int32 else -7.5)).all().item() for n, b in bufs.items() if n != "noise")
    assert roll(steps, 0, full) == 0, err()                                               # and the handle samples afterwards
    g.sync()
    assert (g.get(_lib.FLD_STEP_COUNT) == steps).all() and torch.isfinite(bufs["advantages_out"]).all().item()
    g.close()


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def test_ppo_trainer_two_iterations():
    import torch
    from collision_avoidance_amd import ppo
    A, N, T = 8, 10, 16
    p = H.scenario_params("doorway", N)
    g = H.make_gpu(A, N, "doorway", p, seed=4, use_torch=True)
    torch.manual_seed(0)
    tr = ppo.PPOTrainer(g, hidden=(64, 64), gamma=0.95, lam=0.95, clip=0.2, lr=3e-4, sgd_iters=2, minibatch=A * N * T // 2)
    start = [q.detach().clone() for q in tr.parameters()]
    for it in range(2):
        batch = tr.collect(T)
        assert batch["obs"].shape == (T, A, N, 64) and batch["eps"].shape == (T, A, N) and batch["advantages"].shape == (T, A, N)
        assert batch["values"].shape == (T + 1, A, N) and batch["dist"].shape == (T, 2, A, N)
        info = tr.update(batch)
        print("iteration %d: %s" % (it, info))
        assert all(np.isfinite(v) for v in info.values()), info
    assert any((a != b.detach()).any().item() for a, b in zip(start, tr.parameters()))
    # the weights the update left are the ones installed: policy_evaluate against the restatement under them
    layers, value, log_std = tr.layers()
    obs = _np(g.observe()).copy()
    got = g.policy_evaluate()
    want = PP.evaluate_reference(obs, *_sets([(W.astype(f32), b.astype(f32)) for W, b in layers]), None, value, log_std)
    for n in OUTS:
        H._eq(_np(got[n]), want[n], "after the update: %s" % n)
    g.close()
