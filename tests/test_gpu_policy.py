"""The policy on the GPU (ca_policy_*, ca_rollout_policy; include/ca_env.h).  Everything is compared bit for bit:
  * ca_policy_actions against the numpy restatement of the definition (tests/policy_scenes.py: the k-ordered fmaf chain from the
    bias) -- 30 rows in 3 arenas, so that the 32-row tile is ragged and crosses arenas, every width class, one and two weight sets;
  * ca_rollout_policy against a twin handle driven call by call through observe / policy_actions / step: every field, the
    statistics, returns, first_done, the four records, and the recorded actions against the restatement fed with the recorded
    observations -- one handle of every form in which a step is launched;
  * configuration stays with the slot under fork(); refusals advance nothing; zero steps."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib
from tests import agent_count_scenes as CS
from tests import helpers as H
from tests import policy_scenes as PS

pytestmark = pytest.mark.gpu

STATE = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "AGENT_DONE", "ARRIVE_STEP", "REGOAL_COUNT",
         "NB_COUNT", "NB_IDX", "OBST_COUNT", "OBST_IDX", "STEP_COUNT", "ARENA_DONE", "EPISODE", "REWARD")
f32 = np.float32


def _layers(hidden, P=None, seed=0):
    """[(W, b)] of a policy 64 -> hidden ... -> 1; with P: a leading set axis.  Weights ~ 1 / sqrt(fan-in): activations stay O(1)"""
    rs = np.random.RandomState(seed)
    widths = (64,) + tuple(hidden) + (1,)
    lead = () if P is None else (P,)
    return [((rs.standard_normal(lead + (o, i)) / np.sqrt(i)).astype(f32), (0.3 * rs.standard_normal(lead + (o,))).astype(f32))
            for i, o in zip(widths[:-1], widths[1:])]


def _sets(layers):
    """the layers as the restatement takes them: Ws[l] [P, out, in], bs[l] [P, out]"""
    Ws = [W if W.ndim == 3 else W[None] for W, _ in layers]
    bs = [b if b.ndim == 2 else b[None] for _, b in layers]
    return Ws, bs


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


# ---- 1. ca_policy_actions against the restatement --------------------------------------------------------------------------------------
def _check_actions(g, layers, sets, obs, what, seed=0):
    """identity / clip x noise off / on for the observation the handle holds (obs: its host copy)"""
    Ws, bs = _sets(layers)
    A, N = obs.shape[:2]
    mean = PS.actions_reference(obs, Ws, bs, sets)
    noise = (0.5 * np.random.RandomState(seed + 100).standard_normal((A, N))).astype(f32)
    noisy = (mean + noise).astype(f32)
    lim = f32(np.median(np.abs(noisy)))
    clipped = PS.out_reference(noisy, "clip", lim)
    assert (clipped != noisy).any() and (clipped == noisy).any(), what          # the limit clips some rows and leaves some
    g.set_policy(layers, sets=sets)
    H._eq(_np(g.policy_actions()), mean, what + ": identity, no noise")
    H._eq(_np(g.policy_actions(noise)), noisy, what + ": identity, noise")
    g.set_policy(layers, sets=sets, out="clip", limit=float(lim))
    H._eq(_np(g.policy_actions(noise)), clipped, what + ": clip, noise")
    H._eq(_np(g.policy_actions()), PS.out_reference(mean, "clip", lim), what + ": clip, no noise")
    return mean


@pytest.mark.parametrize("P", [None, 2], ids=["one_set", "two_sets"])
@pytest.mark.parametrize("hidden", [(64, 64), (16,), (128, 32, 48)], ids=["64-64", "16", "128-32-48"])
def test_policy_actions_equal_the_definition(hidden, P):
    A, N = 3, 10
    p = H.scenario_params("doorway", N)
    g = H.make_gpu(A, N, "doorway", p, seed=3)
    layers = _layers(hidden, P, seed=len(hidden))
    sets = None if P is None else np.asarray([1, 0, 1], np.int32)
    act = np.random.RandomState(1).uniform(-np.pi, np.pi, (5, A, N)).astype(f32)
    for t in range(5):
        obs, *_ = g.step(act[t])
    assert np.abs(obs).max() > 0
    mean = _check_actions(g, layers, sets, obs, "after 5 doorway steps")
    assert len(np.unique(mean)) > A * N // 2
    info = g.policy_info()
    assert info == dict(configured=True, n_layers=len(hidden) + 1, widths=[64] + list(hidden) + [1], n_sets=P or 1), info
    # an observation of the caller's: normals, a row of zeros (the chain of the biases alone), a row of negatives
    rs = np.random.RandomState(9)
    obs2 = rs.standard_normal((A, N, 64)).astype(f32)
    obs2[0, 0] = 0.0
    obs2[1, 3] = -np.abs(obs2[1, 3])
    g.set(_lib.FLD_OBS, obs2)
    _check_actions(g, layers, sets, obs2, "an observation written through ca_set", seed=1)
    g.clear_policy()
    assert g.policy_info() == dict(configured=False, n_layers=0, widths=[], n_sets=0)
    g.close()


def test_policy_actions_on_a_tiled_handle_with_a_bound_observation():
    """1 x 80 on the tiled path, torch mode (the observation lies in a tensor bound with ca_bind_obs): three tiles, the last with 16
    rows; with one set (tiles of consecutive rows) and with a set per arena (tiles of one arena, padded)"""
    A, N = 1, 80
    p = H.scenario_params("crowd", N)
    g = H.make_gpu(A, N, "crowd", p, seed=2, tiled=True, use_torch=True)
    assert g.tiled_info()["tiled"]
    for _ in range(2):
        obs, *_ = g.step(np.zeros((A, N), f32))
    obs = _np(obs).copy()
    _check_actions(g, _layers((64, 64), None, seed=5), None, obs, "tiled, one set")
    _check_actions(g, _layers((64, 64), 2, seed=6), np.asarray([1], np.int32), obs, "tiled, a set per arena")
    g.close()


# ---- 2. ca_rollout_policy against a twin handle driven call by call ----------------------------------------------------------------------
def _gpu_step(g, act, flags):
    a = np.ascontiguousarray(act, f32)
    g._call("ca_step_host", g.h, a.ctypes.data_as(C.c_void_p), flags)


def _same_handles(a, b, what, stats, exact_sum=True):
    for n in STATE:
        f = getattr(_lib, "FLD_" + n)
        H._eq(a.get(f), b.get(f), "%s: %s" % (what, n))
    if not stats:
        return
    sa, sb = a.stats(), b.stats()
    ra, rb = a.get(_lib.FLD_ARENA_STATS), b.get(_lib.FLD_ARENA_STATS)
    if exact_sum:
        assert sa == sb, (what, sa, sb)
        assert np.array_equal(ra, rb), what + ": per-arena counters"
    else:   # more than 64 agents: the arena's sum of rewards is added up from several waves in the order they arrive
        assert {k: v for k, v in sa.items() if k != "sum_reward"} == {k: v for k, v in sb.items() if k != "sum_reward"}, (what, sa, sb)
        assert abs(sa["sum_reward"] - sb["sum_reward"]) <= 1e-9 * max(1.0, abs(sb["sum_reward"])), (what, sa, sb)
        cols = [c for c in range(ra.shape[1]) if c != 5]
        assert np.array_equal(ra[:, cols], rb[:, cols]), what + ": per-arena counters"


def _case(g, twin, layers, sets, what, steps, hold, weights=None, noise=False, present=None, exact_sum=True, tail=False,
          out="identity", limit=np.pi, **kw):
    """the call on g, the loop of the definition on twin; returns the call's dict"""
    A, N = g.A, g.N
    R = (steps + hold - 1) // hold
    for e in (g, twin):
        e.set_policy(layers, sets=sets, out=out, limit=limit)
    nz = (0.3 * np.random.RandomState(17).standard_normal((R, A, N))).astype(f32) if noise else None
    freeze, stats = bool(kw.get("freeze")), bool(kw.get("stats"))
    res = g.rollout_policy(steps, hold=hold, noise=nz, weights=weights, returns=True, first_done=True, with_obs=tail, contacts=tail, **kw)
    gf = (_lib.F_STATS if stats else 0) | (_lib.F_AUTORESET if kw.get("autoreset") else 0) | (_lib.F_FREEZE if freeze else 0)
    entry = twin.get(_lib.FLD_ARENA_DONE).copy()
    rec = PS.rollout_records(twin.observe, lambda o, n: twin.policy_actions(n), lambda a: _gpu_step(twin, a, gf),
                             lambda: (twin.get(_lib.FLD_REWARD), twin.get(_lib.FLD_ARENA_DONE)), steps, hold, nz)
    for name in ("obs", "actions", "rewards", "dones"):
        H._eq(res[name], rec[name], "%s: the %s record against the twin's loop" % (what, name))
    ret, fd = PS.returns_and_first_done(entry, rec["rewards"], rec["dones"], weights, freeze, present)
    H._eq(res["returns"], ret, what + ": returns")
    H._eq(res["first_done"], fd, what + ": first_done")
    _same_handles(g, twin, what + ": the call against the loop", stats, exact_sum)
    Ws, bs = _sets(layers)
    for r in range(R):
        want = PS.actions_reference(res["obs"][r], Ws, bs, sets, None if nz is None else nz[r], out, limit)
        H._eq(res["actions"][r], want, "%s: the actions of row %d against the restatement" % (what, r))
    if tail:
        H._eq(res["obs_last"], twin.observe(), what + ": with_obs against a trailing observe()")
        got, want = g.last_contacts(), twin.contacts()
        for k in want:
            H._eq(got[k], want[k], what + ": contacts=True against a trailing contacts(): " + k)
    return res


def _two_calls(g, twin, what, sets=None, P=None, **kw):
    """7 steps with hold 3 (the last row is held for one step), weights, noise and statistics; then 4 steps with hold 1, neither,
    with the observation and the contact report of the final state"""
    layers = _layers((64, 64), P, seed=4)
    w = (f32(0.9) ** np.arange(7)).astype(f32)
    res = _case(g, twin, layers, sets, what + ", 7 / 3", 7, 3, weights=w, noise=True, stats=True, **kw)
    assert np.abs(res["actions"]).max() > 0 and np.abs(res["returns"]).max() > 0
    _case(g, twin, layers, sets, what + ", 4 / 1", 4, 1, tail=True, out="clip", limit=0.4, **kw)
    g.close(); twin.close()


@pytest.mark.parametrize("quad", ["1", "0"], ids=["four_lanes", "one_lane"])
def test_rollout_four_lanes_and_one_lane(monkeypatch, quad):
    monkeypatch.setenv("CA_QUAD", quad)
    A, N = 4, 16
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=11) for _ in range(2))
    assert g.launch_info()["lanes_per_agent"] == (4 if quad == "1" else 1), g.launch_info()
    if quad == "0":   # both new kernels are small kernels to ca_profile: the set-up launch, one policy launch per row, one record launch per step
        layers = _layers((64, 64), None, seed=4)
        g.set_policy(layers); twin.set_policy(layers)
        g.profile(1); g.profile_read()
        g.rollout_policy(7, hold=3); twin.rollout_policy(7, hold=3)
        prof = g.profile_read(); g.profile(0)
        assert prof["reset_kernels"][0] == 1 + 3 + 7, prof
        assert prof["obs_kernel"][0] == 3, prof
    _two_calls(g, twin, "crowd 4 x 16, CA_QUAD=%s" % quad, sets=np.asarray([1, 0, 0, 1], np.int32), P=2)


def test_rollout_per_arena_counts():
    """counts [10, 3, 16, 1] of 16 rows: absent rows return 0 and record the policy of a zero observation"""
    N, counts = 16, (10, 3, 16, 1)
    A = len(counts)
    p, polys, sc = CS.doorway_scene(A, N, 33, max_step=50)
    g, twin = (H.make_gpu(A, N, None, p, seed=33, polys=polys, max_obst_neighbors=16) for _ in range(2))
    for e in (g, twin):
        e.set_agent_counts(np.asarray(counts, np.int32))
        CS.set_state(e, _lib, CS.with_decoys(sc, counts))
    assert g.launch_info()["agent_counts"]
    present = g.agent_mask()
    layers = _layers((64, 64), None, seed=4)
    res = _case(g, twin, layers, None, "per-arena counts", 7, 3, weights=(f32(0.9) ** np.arange(7)).astype(f32), noise=True, stats=True,
                present=present)
    assert not res["returns"][~present].any() and res["returns"][present].any()
    assert not res["obs"][:, ~present].any()
    zero = PS.actions_reference(np.zeros((1, 1, 64), f32), *_sets(layers))[0, 0]
    nz = (0.3 * np.random.RandomState(17).standard_normal((3, A, N))).astype(f32)
    H._eq(res["actions"][:, ~present], (zero + nz[:, ~present]).astype(f32), "absent rows: the policy of the zero observation")
    _case(g, twin, layers, None, "per-arena counts, 4 / 1", 4, 1, tail=True, present=present)
    g.close(); twin.close()


def test_rollout_tiled_grid():
    A, N = 1, 80
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=21, tiled="grid") for _ in range(2))
    assert g.tiled_info()["tiled"] and g.tiled_grid_info()["grid"]
    _two_calls(g, twin, "tiled grid 1 x 80", exact_sum=False)


def test_rollout_per_agent_parameters():
    A, N = 4, 20
    p = H.scenario_params("crowd", N)
    radius = np.random.RandomState(3).uniform(0.3, 0.6, (A, N)).astype(f32)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=9, agent_params=dict(radius=radius)) for _ in range(2))
    assert g.launch_info()["agent_params"]
    _two_calls(g, twin, "per-agent parameters")


def _doorway_pair(max_step=5):
    A, N = 4, 10
    p = H.scenario_params("doorway", N, max_step=max_step)
    return [H.make_gpu(A, N, "doorway", p, seed=5) for _ in range(2)]


def test_rollout_autoreset_an_episode_ends_inside_the_call():
    g, twin = _doorway_pair()
    res = _case(g, twin, _layers((64, 64), None, seed=4), None, "doorway, autoreset", 7, 3, noise=True, stats=True, autoreset=True)
    assert res["first_done"].tolist() == [4] * 4 and res["dones"][4].all() and not res["dones"][:4].any()
    assert (g.get(_lib.FLD_EPISODE) == 1).all() and (g.get(_lib.FLD_STEP_COUNT) == 2).all()   # respawned at step 4, two steps since
    g.close(); twin.close()


def test_rollout_freeze_with_an_arena_frozen_at_entry():
    g, twin = _doorway_pair()
    ad = np.asarray([0, 0, 1, 0], np.int32)
    for e in (g, twin):
        e.set(_lib.FLD_ARENA_DONE, ad)
    res = _case(g, twin, _layers((64, 64), None, seed=4), None, "doorway, freeze", 7, 3, weights=(f32(0.5) ** np.arange(7)).astype(f32),
                stats=True, freeze=True)
    assert res["first_done"].tolist() == [4, 4, -1, 4] and not res["returns"][2].any()
    assert res["dones"][:, 2].all() and res["dones"][3:, 0].tolist() == [0, 1, 1, 1]
    H._eq(res["obs"][0, 2], res["obs"][2, 2], "a frozen arena repeats its observation")
    H._eq(res["rewards"][0, 2], res["rewards"][6, 2], "a frozen arena records the reward its field holds")
    assert (res["obs"][0, 0] != res["obs"][1, 0]).any()
    g.close(); twin.close()


# ---- 3. configuration stays with the slot -----------------------------------------------------------------------------------------------
def test_fork_leaves_every_slot_its_own_weight_set():
    A, N = 4, 12
    p = H.scenario_params("crowd", N)
    g = H.make_gpu(A, N, "crowd", p, seed=13)
    layers = _layers((64, 64), 4, seed=8)
    sets = np.asarray([2, 0, 3, 1], np.int32)
    g.set_policy(layers, sets=sets)
    for _ in range(3):
        g.orca_step()
    g.fork(np.zeros(A, np.int32))
    res = g.rollout_policy(3, hold=1)
    for a in range(1, A):
        H._eq(res["obs"][0, a], res["obs"][0, 0], "the four slots start from arena 0's state")
    Ws, bs = _sets(layers)
    for r in range(3):
        H._eq(res["actions"][r], PS.actions_reference(res["obs"][r], Ws, bs, sets), "row %d: arena a plays set sets[a]" % r)
    first = res["actions"][0]
    assert all((first[a] != first[b]).any() for a in range(A) for b in range(a)), first
    assert g.policy_info()["n_sets"] == 4
    g.close()


# ---- 4. refusals, 5. zero steps ---------------------------------------------------------------------------------------------------------
def _desc(hidden, P=1, sets=None, out_mode=0, limit=1.0, n_layers=None, keep=None, **edit):
    """a ca_policy_desc over host arrays (kept alive in `keep`); edit: weights_bytes / bias_bytes as (layer, bytes), poke = (layer, flat
    index, value) into the weights"""
    widths = (64,) + tuple(hidden) + (1,)
    d = _lib.PolicyDesc(n_layers=len(widths) - 1 if n_layers is None else n_layers, n_sets=P, out_mode=out_mode, out_limit=limit)
    for l, (i, o) in enumerate(zip(widths[:-1], widths[1:])):
        if l >= 4:
            break
        W, b = np.full((P, o, i), 0.01, f32), np.zeros((P, o), f32)
        if edit.get("poke") and edit["poke"][0] == l:
            W.reshape(-1)[edit["poke"][1]] = edit["poke"][2]
        keep += [W, b]
        d.weights[l], d.weights_bytes[l], d.bias[l], d.bias_bytes[l] = W.ctypes.data, W.nbytes, b.ctypes.data, b.nbytes
    for l, w in enumerate(widths[:5]):
        d.width[l] = w
    for key in ("weights_bytes", "bias_bytes"):
        if key in edit:
            getattr(d, key)[edit[key][0]] = edit[key][1]
    if sets is not None:
        s = np.asarray(sets, np.int32)
        keep.append(s)
        d.set_of_arena, d.set_of_arena_bytes = s.ctypes.data, edit.get("set_bytes", s.nbytes)
    return d


def test_refusals_advance_nothing_and_zero_steps():
    import torch
    A, N, steps, hold = 4, 12, 7, 3
    R = 3
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=6) for _ in range(2))
    fields = STATE + ("ARENA_STATS",)
    before = {n: g.get(getattr(_lib, "FLD_" + n)) for n in fields}
    dev = torch.device("cuda", g.device)
    t = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device=dev)
    bufs = dict(noise=t((R, A, N), torch.float32, 0.0), weights=t((steps,), torch.float32, 1.0), returns=t((A, N), torch.float32, -7.5),
                first_done=t((A,), torch.int32, -7), obs_out=t((R, A, N, 64), torch.float32, -7.5), actions_out=t((R, A, N), torch.float32, -7.5),
                rewards_out=t((steps, A, N), torch.float32, -7.5), done_out=t((steps, A), torch.int32, -7))
    full = dict(hold=hold)
    for n, b in bufs.items():
        full[n], full[n + "_bytes"] = b.data_ptr(), b.numel() * 4
    torch.cuda.synchronize()
    EINVAL, ESIZE, ERANGE = -1, -4, -5
    err = lambda: g.L.ca_last_error(g.h).decode()

    def roll(n_steps, flags, kw):
        return g.L.ca_rollout_policy(g.h, n_steps, flags, C.byref(_lib.PolicySeq(**kw)) if kw is not None else None)
    # no policy
    assert roll(steps, 0, full) == EINVAL and "ca_policy_configure" in err()
    assert g.L.ca_policy_actions(g.h, None, bufs["returns"].data_ptr()) == EINVAL and "ca_policy_configure" in err()
    # configurations that are refused change nothing
    keep = []
    bad = [(_desc((20,), keep=keep), EINVAL, "width[1]=20"), (_desc((144,), keep=keep), EINVAL, "width[1]=144"),
           (_desc((16,), n_layers=1, keep=keep), EINVAL, "n_layers=1"), (_desc((16, 16, 16), n_layers=5, keep=keep), EINVAL, "n_layers=5"),
           (_desc((16,), out_mode=2, keep=keep), EINVAL, "out_mode=2"), (_desc((16,), P=0, keep=keep), EINVAL, "n_sets=0"),
           (_desc((16,), P=2, keep=keep), EINVAL, "set_of_arena"),
           (_desc((16, 32), poke=(1, 16 * 3 + 5, np.nan), keep=keep), ERANGE, "layer 1, set 0: weight [3, 5]"),
           (_desc((16,), P=2, poke=(0, 16 * 64 + 64 * 2 + 7, np.inf), sets=[0, 1, 0, 1], keep=keep), ERANGE, "layer 0, set 1: weight [2, 7]"),
           (_desc((16,), P=2, sets=[0, 1, 2, 1], keep=keep), ERANGE, "arena 2 asks for set 2"),
           (_desc((16,), P=2, sets=[0, -1, 0, 1], keep=keep), ERANGE, "arena 1"),
           (_desc((16,), weights_bytes=(0, 16 * 64 * 4 - 1), keep=keep), ESIZE, "weights[0] needs %d" % (16 * 64 * 4)),
           (_desc((16,), bias_bytes=(1, 3), keep=keep), ESIZE, "bias[1] needs 4"),
           (_desc((16,), P=2, sets=[0, 1, 0, 1], set_bytes=15, keep=keep), ESIZE, "set_of_arena needs 16")]
    for stage in range(2):
        for d, code, word in bad:
            rc = g.L.ca_policy_configure(g.h, C.byref(d))
            assert rc == code and word in err(), (stage, word, rc, err())
        if stage == 0:
            assert not g.policy_info()["configured"]
            layers = _layers((64, 64), None, seed=4)
            g.set_policy(layers); twin.set_policy(layers)
        else:
            assert g.policy_info() == dict(configured=True, n_layers=3, widths=[64, 64, 64, 1], n_sets=1)
    # the rollout's own refusals
    size = {n: b.numel() * 4 for n, b in bufs.items()}
    cases = [(steps, 0, None, EINVAL, "null"), (steps, 0, dict(full, hold=0), EINVAL, "hold"), (-1, 0, full, EINVAL, "steps"),
             (steps, _lib.F_NODONE, full, EINVAL, "CA_F_NODONE"), (steps, 64, full, EINVAL, "flags"),
             (steps, 0, dict(full, obs_out=full["obs_out"] + 4), EINVAL, "aligned")]
    cases += [(steps, 0, dict(full, **{n + "_bytes": size[n] - 1}), ESIZE, "%s buffer needs %d" % (n, size[n])) for n in bufs]
    cases += [(steps + 3, 0, full, ESIZE, "noise buffer needs %d" % (4 * A * N * 4))]
    for n_steps, flags, kw, code, word in cases:
        rc = roll(n_steps, flags, kw)
        assert rc == code and word in err(), (n_steps, flags, word, rc, err())
        # the refusal names the call that was made, and none of the calls that share its checks
        assert "ca_rollout_policy:" in err() and not any(n in err() for n in ("ca_rollout_nav_policy:", "ca_rollout_actions:", "ca_rollout_nav_actions:")), err()
    g.sync()
    for n in fields:
        H._eq(g.get(getattr(_lib, "FLD_" + n)), before[n], "after the refusals: %s" % n)
    assert not g.get(_lib.FLD_STEP_COUNT).any()
    assert all((b == (-7 if b.dtype == torch.int32 else -7.5)).all().item() for n, b in bufs.items() if n not in ("noise", "weights"))
    # steps == 0: zeros to returns, -1 to first_done, nothing else
    assert roll(0, 0, full) == 0, err()
    g.sync()
    for n in fields:
        H._eq(g.get(getattr(_lib, "FLD_" + n)), before[n], "after zero steps: %s" % n)
    assert np.array_equal(bufs["returns"].cpu().numpy().view(np.uint32), np.zeros((A, N), np.uint32)) and (bufs["first_done"] == -1).all().item()
    assert all((bufs[n] == (-7 if n == "done_out" else -7.5)).all().item() for n in ("obs_out", "actions_out", "rewards_out", "done_out"))
    out = g.rollout_policy(0, hold=2, first_done=True)                                    # the front end
    assert not out["returns"].any() and (out["first_done"] == -1).all() and out["obs"].shape == (0, A, N, 64) and out["dones"].shape == (0, A)
    _case(g, twin, layers, None, "after the refusals", steps, hold)                      # the handle rolls out correctly afterwards
    g.close(); twin.close()
