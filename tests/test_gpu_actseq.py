"""Action-sequence rollouts on the GPU (ca_rollout_actions, include/ca_env.h): the call is `steps` ca_step calls under the caller's
[R, A, N] action tensor, row t // hold driving step t.  Every test runs three handles of one seed: one makes the call, a twin makes
the single steps and is read after each (reward, arena_done), the CPU oracle does the same in at least one case per form.  Compared
bit for bit: the returns and first_done of the call against the restatement of tests/actseq_scenes.py fed with what the twin's steps
left, the fields the call left against the twin's, the statistics where they were asked for.  Shapes are the smallest at which each
mechanism can go wrong: a launch boundary in the middle of a hold, a last row held for one step, arenas that share a wave, arenas
that freeze or respawn inside a launch, one handle for every form in which a step is a launch sequence of its own."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib, alan, scenarios
from oracle import oracle as o
from tests import actseq_scenes as S
from tests import agent_count_scenes as CS
from tests import helpers as H
from tests import wide_worlds as W

pytestmark = pytest.mark.gpu

STATE = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "AGENT_DONE", "ARRIVE_STEP", "REGOAL_COUNT",
         "NB_COUNT", "NB_IDX", "OBST_COUNT", "OBST_IDX", "STEP_COUNT", "ARENA_DONE", "EPISODE", "REWARD")
f32 = np.float32


def _actions(R, A, N, seed):
    return np.random.RandomState(seed).uniform(-np.pi, np.pi, (R, A, N)).astype(f32)


def _flags(fld, stats=False, autoreset=False, freeze=False, with_obs=False):
    return (fld.F_OBS if with_obs else 0) | (fld.F_STATS if stats else 0) | (fld.F_AUTORESET if autoreset else 0) | \
        (fld.F_FREEZE if freeze else 0)


def _gpu_step(g, act, flags):
    a = np.ascontiguousarray(act, f32)
    g._call("ca_step_host", g.h, a.ctypes.data_as(C.c_void_p), flags)


def _single_steps(step, env, fld, actions, steps, hold):
    """step(actions[t // hold]) `steps` times; (arena_done at entry, rewards [T, A, N], arena_done [T, A]) as get() reads them"""
    entry = env.get(fld.FLD_ARENA_DONE).copy()
    rew, done = [], []
    for t in range(steps):
        step(actions[t // hold])
        rew.append(env.get(fld.FLD_REWARD).copy())
        done.append(env.get(fld.FLD_ARENA_DONE).copy())
    A, N = actions.shape[1:]
    return entry, np.asarray(rew, f32).reshape(steps, A, N), np.asarray(done, np.int32).reshape(steps, A)


def _want(entry, rew, done, weights, freeze, present=None):
    adv = S.advanced_reference(entry, done, freeze)
    return S.returns_reference(rew, adv, weights, present), S.first_done_reference(done, adv), adv


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


def _case(g, twin, orc, what, steps, hold, weights=None, seed=3, one_launch=None, present=None, exact_sum=True, with_obs=False, **kw):
    """the call on g, the single steps on twin (and the oracle); returns (out, want_returns, want_first_done, advanced)"""
    if one_launch is not None:
        assert bool(g.launch_info()["rollout_one_launch"]) is one_launch, (what, g.launch_info())
    R = (steps + hold - 1) // hold
    actions = _actions(R, g.A, g.N, seed)
    freeze, stats = bool(kw.get("freeze")), bool(kw.get("stats"))
    out = g.rollout_actions(actions, hold=hold, weights=weights, returns=True, first_done=True, steps=steps, with_obs=with_obs, **kw)
    gf = _flags(_lib, **kw)
    last = [0]

    def twin_step(act):
        last[0] += 1
        _gpu_step(twin, act, gf | (_lib.F_OBS if with_obs and last[0] == steps else 0))
    entry, rew, done = _single_steps(twin_step, twin, _lib, actions, steps, hold)
    ret, fd, adv = _want(entry, rew, done, weights, freeze, present)
    H._eq(out["returns"], ret, what + ": returns against the twin's rewards")
    H._eq(out["first_done"], fd, what + ": first_done against the twin's flags")
    _same_handles(g, twin, what + ": the call against single steps", stats, exact_sum)
    if with_obs:
        H._eq(out["obs"], twin.get(_lib.FLD_OBS), what + ": the observation of the last step")
    if orc is not None:
        of = _flags(o, **kw)
        oentry, orew, odone = _single_steps(lambda act: orc.step(act, flags=of), orc, o, actions, steps, hold)
        oret, ofd, _ = _want(oentry, orew, odone, weights, freeze, present)
        H._eq(out["returns"], oret, what + ": returns against the oracle's rewards")
        H._eq(out["first_done"], ofd, what + ": first_done against the oracle's flags")
        H.assert_state_equal(g, orc, what + ": final state against the oracle", reward=True)
        if stats:
            H.assert_stats_equal(g, orc, what)
    return out, ret, fd, adv


# ---- the four-lanes kernel: the T-step launch with actions ----------------------------------------------------------------------------
def _two_launches(monkeypatch, steps, hold, n_rows):
    monkeypatch.setenv("CA_QUAD", "1")
    A, N = 37, 16
    p = H.scenario_params("crowd", N, neighbor_dist=1.5, max_neighbors=5)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=11) for _ in range(2))
    orc = H.make_oracle(A, N, "crowd", p, seed=11)
    w = (f32(0.99) ** np.arange(steps)).astype(f32)
    out, ret, fd, _ = _case(g, twin, orc, "37x16", steps, hold, weights=w, one_launch=True, stats=True)
    assert np.abs(ret).max() > 1.0 and S.rows(steps, hold)[0] == n_rows
    g.close(); twin.close()


def test_quad_two_launches_boundary_inside_a_hold(monkeypatch):
    """259 steps are two launches (256 + 3); hold = 3: step 255 is the first of row 85's three, so the boundary falls inside a hold,
    and row 86 is held for one step; weights 0.99^t"""
    _two_launches(monkeypatch, 259, 3, 87)


def test_quad_two_launches_remainder_of_one(monkeypatch):
    """257 steps are two launches (256 + 1), the second of a single step: its block starts at row 128 with a full countdown (hold = 2),
    and the row is held for that one step; the same comparison"""
    _two_launches(monkeypatch, 257, 2, 129)


@pytest.mark.parametrize("scenario,A,N", [("circle", 5, 12), ("crowd", 70, 1)], ids=["circle5x12", "crowd70x1"])
def test_quad_arena_layouts(monkeypatch, scenario, A, N):
    """N no power of two with several arenas per wave; one agent per arena"""
    monkeypatch.setenv("CA_QUAD", "1")
    p = H.scenario_params(scenario, N)
    g, twin = (H.make_gpu(A, N, scenario, p, seed=4) for _ in range(2))
    orc = H.make_oracle(A, N, scenario, p, seed=4)
    _case(g, twin, orc, scenario, 21, 4, one_launch=True, stats=True)
    g.close(); twin.close()


def _doorway(monkeypatch, **kw):
    """doorway 40 x 10, max_step = 20, the arenas' step counters staggered by 0 .. 6: they end at steps 13 .. 19 of 30; arena 3 has
    its done flag set at entry"""
    monkeypatch.setenv("CA_QUAD", "1")
    A, N = 40, 10
    p = H.scenario_params("doorway", N, max_step=20)
    g, twin = (H.make_gpu(A, N, "doorway", p, seed=5) for _ in range(2))
    orc = H.make_oracle(A, N, "doorway", p, seed=5)
    sc = (np.arange(A) % 7).astype(np.int32)
    ad = np.zeros(A, np.int32); ad[3] = 1
    for e in (g, twin):
        e.set(_lib.FLD_STEP_COUNT, sc); e.set(_lib.FLD_ARENA_DONE, ad)
    orc.set(o.FLD_STEP_COUNT, sc); orc.set(o.FLD_ARENA_DONE, ad)
    res = _case(g, twin, orc, "doorway %s" % (kw,), 30, 2, one_launch=True, stats=True, **kw)
    g.close(); twin.close()
    return res, sc


def test_quad_arenas_freeze_inside_the_launch(monkeypatch):
    (out, ret, fd, adv), sc = _doorway(monkeypatch, freeze=True)
    want = 19 - sc
    want[3] = -1                                                      # frozen at entry: its flag was there to see
    assert fd.tolist() == want.tolist(), (fd, want)
    assert not ret[3].any() and not adv[:, 3].any()
    assert (adv.sum(0) == np.where(want < 0, 0, want + 1)).all()      # the returns stopped growing at the step that froze the arena


def test_quad_sum_crosses_a_respawn(monkeypatch):
    (out, ret, fd, adv), sc = _doorway(monkeypatch, autoreset=True)
    assert adv.all() and (fd >= 0).all() and fd[0] == 19 and fd[3] == 19 - sc[3]      # (no freeze: arena 3 is stepped like the others)


def test_quad_512_lanes(monkeypatch):
    """3 x 128, K = 5: the 512-lane workgroup, one arena each"""
    monkeypatch.setenv("CA_QUAD", "1")
    A, N = 3, 128
    p = H.scenario_params("crowd", N, max_neighbors=5)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=6) for _ in range(2))
    assert g.launch_info()["lanes_per_agent"] == 4, g.launch_info()
    _case(g, twin, H.make_oracle(A, N, "crowd", p, seed=6), "3x128", 9, 2, one_launch=True, stats=True, exact_sum=False)
    g.close(); twin.close()


def test_quad_with_observation(monkeypatch):
    monkeypatch.setenv("CA_QUAD", "1")
    A, N = 6, 12
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=6) for _ in range(2))
    orc = H.make_oracle(A, N, "crowd", p, seed=6)
    out, *_ = _case(g, twin, None, "with the observation", 10, 3, one_launch=True, with_obs=True)
    for t, act in enumerate(_actions(4, A, N, 3)[[0, 0, 0, 1, 1, 1, 2, 2, 2, 3]]):
        orc.step(act, flags=o.F_OBS if t == 9 else 0)
    H._eq(out["obs"], orc.get(o.FLD_OBS), "the observation against the oracle's")
    g.close(); twin.close()


def test_quad_alan_configured_handle(monkeypatch):
    """ca_step on an ALAN-configured handle runs without the bandit; so does the call, and the bandit's state stays as it was"""
    monkeypatch.setenv("CA_QUAD", "1")
    A, N = 7, 12
    p = H.scenario_params("circle", N)
    g, twin = (H.make_gpu(A, N, "circle", p, seed=8) for _ in range(2))
    for e in (g, twin):
        e.alan_configure(alan.DEFAULT_ACTIONS)
        e.alan_rollout(5)
    before = g.get(_lib.FLD_ALAN_WEIGHTS), g.get(_lib.FLD_ALAN_TIMES)
    _case(g, twin, None, "ALAN handle", 14, 5, one_launch=True, stats=True)
    H._eq(g.get(_lib.FLD_ALAN_WEIGHTS), before[0], "ALAN weights untouched")
    H._eq(g.get(_lib.FLD_ALAN_TIMES), before[1], "ALAN times untouched")
    H._eq(g.get(_lib.FLD_ALAN_WEIGHTS), twin.get(_lib.FLD_ALAN_WEIGHTS), "ALAN weights as the twin's")
    g.close(); twin.close()


# ---- the per-step form: the launches of ca_step and the accumulate kernel behind them ---------------------------------------------------
def test_per_step_one_lane_per_agent(monkeypatch):
    monkeypatch.setenv("CA_QUAD", "0")
    A, N = 6, 64
    p = H.scenario_params("crowd", N, neighbor_dist=5.0, max_neighbors=10)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=7) for _ in range(2))
    assert g.launch_info()["lanes_per_agent"] == 1
    g.profile(1); g.profile_read()
    w = (f32(0.9) ** np.arange(12)).astype(f32)
    _case(g, twin, H.make_oracle(A, N, "crowd", p, seed=7), "one lane per agent", 12, 2, weights=w, one_launch=False, stats=True)
    prof = g.profile_read(); g.profile(0)
    assert prof["reset_kernels"][0] == 12 + 1, prof          # the set-up launch and one accumulate launch per step: kind 3
    g.close(); twin.close()


def test_per_step_two_lanes_per_agent():
    A, N = 2, 130
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=1) for _ in range(2))
    assert g.launch_info()["lanes_per_agent"] == 2
    _case(g, twin, H.make_oracle(A, N, "crowd", p, seed=1), "pair kernel", 12, 2, one_launch=False, stats=True, exact_sum=False)
    g.close(); twin.close()


def test_per_step_freeze_with_an_arena_frozen_at_entry(monkeypatch):
    """the accumulate kernel's own freeze logic: staggered ends and a flag set at entry, on the one-lane kernel"""
    monkeypatch.setenv("CA_QUAD", "0")
    A, N = 9, 10
    p = H.scenario_params("doorway", N, max_step=8)
    g, twin = (H.make_gpu(A, N, "doorway", p, seed=5) for _ in range(2))
    orc = H.make_oracle(A, N, "doorway", p, seed=5)
    sc = (np.arange(A) % 4).astype(np.int32)
    ad = np.zeros(A, np.int32); ad[2] = 1
    for e in (g, twin):
        e.set(_lib.FLD_STEP_COUNT, sc); e.set(_lib.FLD_ARENA_DONE, ad)
    orc.set(o.FLD_STEP_COUNT, sc); orc.set(o.FLD_ARENA_DONE, ad)
    out, ret, fd, adv = _case(g, twin, orc, "per-step freeze", 12, 2, one_launch=False, stats=True, freeze=True)
    want = 7 - sc
    want[2] = -1
    assert fd.tolist() == want.tolist() and not ret[2].any()
    g.close(); twin.close()


def test_per_step_per_agent_parameters():
    A, N = 4, 20
    p = H.scenario_params("crowd", N)
    radius = np.random.RandomState(3).uniform(0.3, 0.6, (A, N)).astype(f32)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=9, agent_params=dict(radius=radius)) for _ in range(2))
    assert g.launch_info()["agent_params"]
    _case(g, twin, None, "per-agent parameters", 12, 2, one_launch=False, stats=True)
    g.close(); twin.close()


def test_per_step_per_arena_counts():
    """counts [20, 7, 1, 13] of 20 rows: absent rows return 0"""
    N, counts = 20, (20, 7, 1, 13)
    A = len(counts)
    p, polys, sc = CS.doorway_scene(A, N, 33, max_step=50)
    g, twin = (H.make_gpu(A, N, None, p, seed=33, polys=polys, max_obst_neighbors=16) for _ in range(2))
    for e in (g, twin):
        e.set_agent_counts(np.asarray(counts, np.int32))
        CS.set_state(e, _lib, CS.with_decoys(sc, counts))
    assert g.launch_info()["agent_counts"]
    present = g.agent_mask()
    out, ret, fd, adv = _case(g, twin, None, "per-arena counts", 12, 2, one_launch=False, present=present, stats=True)
    assert not out["returns"][~present].any() and out["returns"][present].any()
    g.close(); twin.close()


def test_per_step_per_agent_sensing():
    A, N = 3, 12
    sens = dict(neighbor_dist=np.random.RandomState(9).uniform(1, 5, (A, N)).astype(f32), max_neighbors=np.asarray([2, 0, 7], np.int32))
    p = scenarios.bench_params(N, 5.0, 10)          # neighbor_dist 5 and max_neighbors 10 are the capacities
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=2, agent_sensing=sens) for _ in range(2))
    assert g.launch_info()["agent_sensing"]
    _case(g, twin, None, "per-agent sensing", 12, 2, one_launch=False, stats=True)
    g.close(); twin.close()


def test_per_step_wide_obstacle_lists():
    worlds = W.ragged_squares_worlds(10)
    g, orc = W.make_pair(4, 10, worlds, 64)
    twin, _ = W.make_pair(4, 10, worlds, 64)
    assert g.launch_info()["lanes_per_agent"] == 1 and g.S == 64
    _case(g, twin, orc, "wide lists", 12, 2, one_launch=False, stats=True)
    g.close(); twin.close()


@pytest.mark.parametrize("tiled", [True, "grid"], ids=["tiled", "grid"])
def test_per_step_tiled(tiled):
    A, N = 2, 100
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=21, tiled=tiled) for _ in range(2))
    assert g.tiled_info()["tiled"]
    _case(g, twin, H.make_oracle(A, N, "crowd", p, seed=21), "tiled %s" % (tiled,), 12, 2, one_launch=False, stats=True, exact_sum=False)
    g.close(); twin.close()


# ---- refusals, zero steps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad", ["1", "0"])
def test_refusals_advance_nothing(monkeypatch, quad):
    import torch
    monkeypatch.setenv("CA_QUAD", quad)
    A, N, steps, hold = 6, 12, 10, 3
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=6) for _ in range(2))
    fields = STATE + ("ARENA_STATS",)
    before = {n: g.get(getattr(_lib, "FLD_" + n)) for n in fields}
    dev = torch.device("cuda", g.device)
    act = torch.as_tensor(_actions(4, A, N, 3)).to(dev)
    wt = torch.ones(steps, dtype=torch.float32, device=dev)
    ret = torch.full((A, N), -7.5, dtype=torch.float32, device=dev)
    fd = torch.full((A,), -7, dtype=torch.int32, device=dev)
    full = dict(actions=act.data_ptr(), actions_bytes=act.numel() * 4, hold=hold, weights=wt.data_ptr(), weights_bytes=steps * 4,
                returns=ret.data_ptr(), returns_bytes=A * N * 4, first_done=fd.data_ptr(), first_done_bytes=A * 4)
    torch.cuda.synchronize()                        # (the handle runs on a stream of its own)
    EINVAL, ESIZE = -1, -4
    cases = [(steps, 0, None, EINVAL, "null"),
             (steps, 0, dict(full, actions=None), EINVAL, "null"),
             (steps, 0, dict(full, hold=0), EINVAL, "hold"),
             (steps, 0, dict(full, hold=-3), EINVAL, "hold"),
             (-1, 0, full, EINVAL, "steps"),
             (steps, _lib.F_NODONE, full, EINVAL, "CA_F_NODONE"),
             (steps, 64, full, EINVAL, "flags"),
             (steps, 0x100 | _lib.F_STATS, full, EINVAL, "flags"),
             (steps, 0, dict(full, actions_bytes=4 * A * N * 4 - 1), ESIZE, "actions buffer needs %d" % (4 * A * N * 4)),
             (steps, 0, dict(full, weights_bytes=steps * 4 - 1), ESIZE, "weights buffer needs %d" % (steps * 4)),
             (steps, 0, dict(full, returns_bytes=A * N * 4 - 1), ESIZE, "returns buffer needs %d" % (A * N * 4)),
             (steps, 0, dict(full, first_done_bytes=A * 4 - 1), ESIZE, "first_done buffer needs %d" % (A * 4)),
             (steps + 3, 0, full, ESIZE, "actions buffer needs %d" % (5 * A * N * 4))]
    for n_steps, flags, kw, code, word in cases:
        seq = _lib.ActionSeq(**kw) if kw is not None else None
        rc = g.L.ca_rollout_actions(g.h, n_steps, flags, C.byref(seq) if seq is not None else None)
        assert rc == code, (n_steps, flags, kw, rc)
        assert word in g.L.ca_last_error(g.h).decode(), (kw, g.L.ca_last_error(g.h))
        # the refusal names the call that was made, and none of the calls that share its checks
        msg = g.L.ca_last_error(g.h).decode()
        assert "ca_rollout_actions:" in msg and not any(n in msg for n in ("ca_rollout_nav_actions:", "ca_rollout_policy:", "ca_rollout_nav_policy:")), msg
    g.sync()
    for n in fields:
        H._eq(g.get(getattr(_lib, "FLD_" + n)), before[n], "after the refusals: %s" % n)
    assert (ret == -7.5).all().item() and (fd == -7).all().item()
    # steps == 0 advances nothing and still writes zeros and -1
    rc = g.L.ca_rollout_actions(g.h, 0, 0, C.byref(_lib.ActionSeq(**dict(full, actions_bytes=0, weights=None, weights_bytes=0))))
    assert rc == 0, g.L.ca_last_error(g.h)
    g.sync()
    for n in fields:
        H._eq(g.get(getattr(_lib, "FLD_" + n)), before[n], "after zero steps: %s" % n)
    assert np.array_equal(ret.cpu().numpy().view(np.uint32), np.zeros((A, N), np.uint32)) and (fd == -1).all().item()
    out = g.rollout_actions(np.zeros((0, A, N), f32), hold=2, first_done=True)          # the front end
    assert not out["returns"].any() and (out["first_done"] == -1).all()
    _case(g, twin, None, "after the refusals", steps, hold)                              # the handle steps correctly afterwards
    g.close(); twin.close()


# ---- step_repeat, the planning round ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad", ["1", "0"])
def test_step_repeat_is_four_steps(monkeypatch, quad):
    monkeypatch.setenv("CA_QUAD", quad)
    A, N = 5, 12
    p = H.scenario_params("crowd", N)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=12) for _ in range(2))
    act = _actions(1, A, N, 5)[0]
    obs, rew, dones, info = g.step_repeat(act, 4)
    total = np.zeros((A, N), f32)
    for _ in range(4):
        tobs, trew, tdone, _ = twin.step(act)
        total = (total + trew).astype(f32)
    H._eq(rew, total, "summed rewards")
    H._eq(obs, tobs, "the observation of the fourth step")
    assert dones.dtype == bool and not dones.any() and (info["first_done"] == -1).all()
    _same_handles(g, twin, "step_repeat", stats=False)
    g.close(); twin.close()


def test_step_repeat_reports_an_episode_end(monkeypatch):
    monkeypatch.setenv("CA_QUAD", "1")
    A, N = 4, 10
    p = H.scenario_params("doorway", N, max_step=6)
    g = H.make_gpu(A, N, "doorway", p, seed=5)
    g.set(_lib.FLD_STEP_COUNT, np.asarray([0, 3, 0, 4], np.int32))
    obs, rew, dones, info = g.step_repeat(_actions(1, A, N, 1)[0], 3, autoreset=True)
    assert dones.tolist() == [False, True, False, True] and info["first_done"].tolist() == [-1, 2, -1, 1]
    g.close()


def test_planning_round(monkeypatch):
    """fork arena 0 into all 16 slots, roll each copy out under its own sequence, rewind, replay the best with step(): the replay
    yields exactly the return that was reported"""
    monkeypatch.setenv("CA_QUAD", "1")
    A, N, T, hold = 16, 16, 10, 2
    p = H.scenario_params("crowd", N)
    g = H.make_gpu(A, N, "crowd", p, seed=13)
    for _ in range(3):
        g.orca_step()
    snap = g.snapshot()
    real = {n: g.get(getattr(_lib, "FLD_" + n)) for n in STATE}
    g.fork(np.zeros(A, np.int32))
    actions = _actions(T // hold, A, N, 17)
    w = (f32(0.95) ** np.arange(T)).astype(f32)
    out = g.rollout_actions(actions, hold=hold, weights=w)
    score = out["returns"].astype(np.float64).sum(1)
    best = int(np.argmax(score))
    assert len(set(score.tolist())) == A                         # sixteen different futures of one arena
    g.restore(snap)
    for n in STATE:
        H._eq(g.get(getattr(_lib, "FLD_" + n)), real[n], "rewound: %s" % n)
    # replay: arena 0 takes the best sequence.  (A slot draws its futures from its own random streams; this world draws nothing
    # inside the horizon -- arrivals draw no new goal in done_mode 1, and no episode ends --, so arena 0 retraces arena `best` exactly.)
    assert p["done_mode"] == 1
    ret = np.zeros(N, f32)
    for t in range(T):
        act = np.zeros((A, N), f32)
        act[0] = actions[t // hold, best]
        _, rew, _, _ = g.step(act, with_obs=False)
        ret = (ret + (w[t] * rew[0]).astype(f32)).astype(f32)
    assert not g.get(_lib.FLD_ARENA_DONE).any()
    H._eq(ret, out["returns"][best], "the replayed return of the best sequence")
    g.close()
