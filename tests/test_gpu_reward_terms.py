"""The reward terms on the GPU (ca_reward_configure, ca_reward_parts; include/ca_env.h, csrc/ca_reward.h).  Everything is compared bit
for bit (==) against the numpy restatement of tests/reward_scenes.py or against a twin handle; the one tolerance is ca_stats.sum_reward,
whose order of addition is not defined: 1e-9 * sum(|r|), as the header states.
  1. identity: weights (1, 0, ...) on one handle of every form a step is launched in, against a twin without terms;
  2. the parts at the boundaries of every count, on every geometry of the kernel;
  3. steps in the doorway world against the restatement and a twin in lockstep;
  4. episode ends: the respawning step, a frozen arena, CA_DONE_REGOAL;
  5. the rollouts against the loop of shaped step() calls on a twin;
  6. ca_step_packed; 7. fork; 8. refusals; 9. launch counts."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from tests import agent_count_scenes as ACS
from tests import contact_scenes as CS
from tests import helpers as H
from tests import nav_scenes as S
from tests import reward_scenes as RS
from tests import test_gpu_actseq as TA
from tests import test_gpu_policy as TP
from tests import test_gpu_ppo as PP

pytestmark = pytest.mark.gpu

F = np.float32
R = 0.5
IDENTITY = dict(base=1.0)
ALL = dict(base=0.75, collision=-0.5, wall=-0.25, near=-0.125, wall_near=-0.0625, arrival=3.0, step=-0.01, margin=0.3)   # every scan is made
STATE = TP.STATE


def _per_arena(A, seed=4):
    """all seven weights non-zero and different in every arena"""
    rs = np.random.RandomState(seed)
    kw = {n: (rs.uniform(0.1, 1.0, A) * (1.0 if n in ("base", "arrival") else -1.0)).astype(F) for n in RS.TERMS}
    kw["margin"] = 0.3
    return kw


def _weights(g):
    return g.reward_terms_info()["weights"]


def _get(g, n):
    return g.get(getattr(_lib, "FLD_" + n))


def _assert_parts(got, want, what, rows=None):
    rows = want["written"] if rows is None else rows
    H._eq(np.asarray(got["ref"])[rows], want["ref"][rows], what + ": ref")
    for n in RS.COUNTS:
        H._eq(np.asarray(got[n])[rows], want[n][rows], "%s: %s" % (what, n))


def _radius(g, radius=None):
    return g.cfg.radius if radius is None else radius


def _shaped_step(g, twin, act, what, flags=0, radius=None, counts=None, stepper=None):
    """one step of both handles under `act`; g's reward and parts against the restatement fed with the twin's reward; returns it"""
    regoal = g.cfg.done_mode == _lib.DONE_REGOAL
    word = "REGOAL_COUNT" if regoal else "AGENT_DONE"
    saved, entry = _get(twin, word).copy(), _get(twin, "ARENA_DONE").copy()
    for e in (g, twin):
        (stepper or TP._gpu_step)(e, act, flags)
    done = _get(twin, "ARENA_DONE")
    adv = ~((entry != 0) & bool(flags & _lib.F_FREEZE))
    resp = (done != 0) & bool(flags & _lib.F_AUTORESET) & adv
    le = (twin.get(_lib.FLD_ARENA_STATS)[:, 7] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    c5, c6 = RS.arrival_counts(regoal, saved, _get(twin, word), counts, resp, le)
    m = g.reward_terms_info()["margin"]
    want = RS.shaped_reference(_get(g, "POS_X"), _get(g, "POS_Y"), _radius(g, radius), CS.tables_of(g, g.A), _get(twin, "REWARD"), _weights(g), m,
                               c5, c6, counts, adv, resp)
    H._eq(_get(g, "REWARD")[want["written"]], want["reward"][want["written"]], what + ": the shaped reward")
    _assert_parts(g.last_reward_parts(), want, what)
    for n in STATE:
        if n != "REWARD":
            H._eq(_get(g, n), _get(twin, n), "%s: %s" % (what, n))
    return want


# ---- 1. identity ------------------------------------------------------------------------------------------------------------------------
def _form(name, monkeypatch):
    """(g, twin, keywords of _one_call) of one form a step is launched in"""
    kw = {}
    if name in ("four_lanes", "one_lane"):
        monkeypatch.setenv("CA_QUAD", "1" if name == "four_lanes" else "0")
        pair = [H.make_gpu(4, 16, "crowd", H.scenario_params("crowd", 16), seed=11) for _ in range(2)]
        assert pair[0].launch_info()["lanes_per_agent"] == (4 if name == "four_lanes" else 1)
    elif name == "two_lanes":
        pair = [H.make_gpu(1, 129, "crowd", H.scenario_params("crowd", 129), seed=1) for _ in range(2)]
        assert pair[0].launch_info()["lanes_per_agent"] == 2
        kw = dict(exact_sum=False)
    elif name == "wide_lists":
        pair = [H.make_gpu(2, 40, "doorway", H.scenario_params("doorway", 40), seed=3, max_obst_neighbors=40) for _ in range(2)]
    elif name == "agent_params":
        radius = np.random.RandomState(3).uniform(0.3, 0.6, (4, 20)).astype(F)
        pair = [H.make_gpu(4, 20, "crowd", H.scenario_params("crowd", 20), seed=9, agent_params=dict(radius=radius)) for _ in range(2)]
    elif name == "counts":
        N, counts = 16, (10, 3, 16, 1)
        p, polys, sc = ACS.doorway_scene(len(counts), N, 33, max_step=50)
        pair = [H.make_gpu(len(counts), N, None, p, seed=33, polys=polys, max_obst_neighbors=16) for _ in range(2)]
        for e in pair:
            e.set_agent_counts(np.asarray(counts, np.int32))
            ACS.set_state(e, _lib, ACS.with_decoys(sc, counts))
        kw = dict(present=pair[0].agent_mask())
    elif name == "sensing":
        A, N = 3, 12
        sens = dict(neighbor_dist=np.random.RandomState(9).uniform(1, 5, (A, N)).astype(F), max_neighbors=np.asarray([2, 0, 7], np.int32))
        p = scenarios.bench_params(N, 5.0, 10)          # neighbor_dist 5 and max_neighbors 10 are the capacities
        pair = [H.make_gpu(A, N, "crowd", p, seed=2, agent_sensing=sens) for _ in range(2)]
    else:   # tiled1 / tiled5 / tiled17 / tiled33: the create flags
        flags = int(name[5:])
        tk = dict(tiled="grid" if flags & 4 else True, tiled_params=bool(flags & 16), tiled_wide=bool(flags & 32))
        pair = [H.make_gpu(1, 80, "crowd", H.scenario_params("crowd", 80), seed=21, **tk) for _ in range(2)]
        assert pair[0].tiled_info()["tiled"]
        kw = dict(exact_sum=False)
    return pair[0], pair[1], kw


@pytest.mark.parametrize("form", ["four_lanes", "one_lane", "two_lanes", "wide_lists", "agent_params", "counts", "sensing", "tiled1", "tiled5",
                                  "tiled17", "tiled33"])
def test_identity_terms_change_nothing(form, monkeypatch):
    """rollout_policy_sample under (1, 0, 0, 0, 0, 0, 0) against a twin without terms driven step by step: every field, the reward,
    the statistics and every record; then three more single steps"""
    g, twin, kw = _form(form, monkeypatch)
    g.set_reward_terms(**IDENTITY)
    assert g.reward_terms_info()["configured"] and not twin.reward_terms_info()["configured"]
    exact = kw.get("exact_sum", True)
    layers = TP._layers((64, 64), None, seed=4)
    w = (F(0.9) ** np.arange(7)).astype(F)
    PP._sample_case(g, twin, layers, None, PP._both_heads(), form + ", identity, 7 / 3", 7, 3, weights=w, stats=True, **kw)
    rs = np.random.RandomState(5)
    for s in range(3):
        act = rs.uniform(-1, 1, (g.A, g.N)).astype(F)
        for e in (g, twin):
            TP._gpu_step(e, act, _lib.F_STATS)
        TP._same_handles(g, twin, "%s: single step %d" % (form, s), True, exact)
    parts = g.last_reward_parts()
    present = kw.get("present", np.ones((g.A, g.N), bool))
    H._eq(parts["ref"][present], _get(twin, "REWARD")[present], form + ": plane 0 is the reference reward")
    assert all(not parts[n].any() for n in RS.COUNTS)                     # no weight anywhere: no scan, every count plane reads 0
    g.close(); twin.close()


# ---- 2. the parts at the boundaries ---------------------------------------------------------------------------------------------------
SHAPES = [(27, 10, {}), (3, 64, {}), (1, 256, {}), (1, 300, {}), (2, 600, dict(tiled=True, tiled_params=True))]


@pytest.mark.parametrize("A,N,kw", SHAPES, ids=["27x10", "3x64", "1x256", "1x300", "tiled2x600"])
def test_parts_at_the_boundaries(A, N, kw):
    m = ALL["margin"]
    g = H.make_gpu(A, N, None, scenarios.env_params(), seed=5, polys=CS.WALL, **kw)
    g.set_reward_terms(**ALL)
    tabs = CS.tables_of(g, A)
    done = (np.arange(A * N).reshape(A, N) % 3 == 0).astype(np.int32)
    g.set(_lib.FLD_AGENT_DONE, done)

    def check(px, py, what, radius=R):
        X, Y = RS.tile_scene(px, py, A, N, spread=3.0)
        g.set(_lib.FLD_POS_X, X); g.set(_lib.FLD_POS_Y, Y)
        before = _get(g, "REWARD").copy()
        got = g.reward_parts()
        rad = R
        if not np.isscalar(radius):
            rad = np.full((A, N), R, F)
            rad[:, :radius.shape[1]] = radius[0]
        want = RS.shaped_reference(X, Y, rad, tabs, before, _weights(g), m, np.zeros((A, N), np.int32), (done == 0).astype(np.int32))
        _assert_parts(got, want, "%d x %d: %s" % (A, N, what))
        H._eq(_get(g, "REWARD"), before, what + ": ca_reward_parts does not write the reward")
        return got

    px, py = RS.boundary_pairs(R, m)
    got = check(px, py, "pairs at (r_i + r_j) + margin")
    assert got["near"][A - 1, :9].tolist() == [0, 0, 1, 1, 0, 0, 2, 2, 2] and got["collision"][A - 1, :9].tolist() == [0, 0, 0, 0, 0, 0, 2, 2, 2]
    px, py = CS.boundary_pairs(R)
    got = check(px, py, "pairs at r_i + r_j")
    assert got["collision"][0, :9].tolist() == [0, 0, 1, 1, 0, 0, 2, 2, 2] and got["near"][0, :9].tolist() == [1, 1, 1, 1, 1, 1, 2, 2, 2]
    px, py = RS.wall_cases(R, m)
    got = check(px, py, "walls at r_i + margin")
    assert got["wall_near"][A - 1, :9].tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0] and not got["wall"].any()
    px, py = CS.wall_cases(R)
    got = check(px, py, "walls at r_i")
    assert got["wall"][0, :9].tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0] and got["wall_near"][0, :9].all()
    assert got["arrival"].sum() == 0 and (got["step"] == (done == 0)).all()
    px, py, rad = CS.nearest_cases()
    g.set_agent_params(radius=np.broadcast_to(np.pad(rad, ((0, 0), (0, N - 6)), constant_values=R), (A, N)).copy())
    got = check(px, py, "per-agent radii", radius=rad)
    assert got["collision"][A - 1, :6].tolist() == [0, 0, 0, 1, 0, 1]
    g.clear_agent_params()
    # a crowded state: every chunk of a large arena holds candidates that count
    px, py = CS.random_state(A, N, 100 + N, centre=(2.0, 0.5))
    g.set(_lib.FLD_POS_X, px); g.set(_lib.FLD_POS_Y, py)
    got = g.reward_parts()
    want = RS.shaped_reference(px, py, R, tabs, _get(g, "REWARD"), _weights(g), m, np.zeros((A, N), np.int32), (done == 0).astype(np.int32))
    _assert_parts(got, want, "%d x %d: a crowd" % (A, N))
    assert got["near"].sum() > got["collision"].sum() > 0 and got["wall_near"].sum() > got["wall"].sum() > 0
    g.close()


# ---- 3. steps ---------------------------------------------------------------------------------------------------------------------------
def test_steps_in_the_doorway_world():
    A, N, T = 4, 10, 30
    p = H.scenario_params("doorway", N)
    g, twin = (H.make_gpu(A, N, "doorway", p, seed=3) for _ in range(2))
    g.set_reward_terms(**_per_arena(A))
    assert g.reward_terms_info()["per_arena"] and (_weights(g) != 0).all()
    seq, mag = np.zeros(A), np.zeros(A)
    shaped = 0
    for s, act in CS.doorway_actions(A, N, 3, T):
        want = _shaped_step(g, twin, act, "step %d" % s, _lib.F_STATS)
        for a in range(A):                                       # the sequential float64 sum of the shaped rewards
            for v in want["reward"][a]:
                seq[a] += float(v); mag[a] += abs(float(v))
        got = g.arena_stats()["sum_reward"]
        print("step %d: sum_reward %r, sequential %r" % (s, got.tolist(), seq.tolist()))
        assert (np.abs(got - seq) <= 1e-9 * mag).all(), (s, got, seq, mag)
        shaped += int(want["collision"].sum() + want["wall"].sum())
    assert shaped > 0 and (_get(g, "REWARD") != _get(twin, "REWARD")).any()
    sg, st = g.stats(), twin.stats()
    assert {k: v for k, v in sg.items() if k != "sum_reward"} == {k: v for k, v in st.items() if k != "sum_reward"}
    g.close(); twin.close()


# ---- 4. episode ends --------------------------------------------------------------------------------------------------------------------
def test_autoreset_at_the_step_cap():
    A, N = 4, 6
    p = H.scenario_params("doorway", N, max_step=3)
    g, twin = (H.make_gpu(A, N, "doorway", p, seed=2) for _ in range(2))
    g.set_reward_terms(**ALL)
    px = _get(g, "POS_X"); px[:, 1] = px[:, 0] + F(0.25)         # a touching pair that the respawn dissolves
    py = _get(g, "POS_Y"); py[:, 1] = py[:, 0]
    for e in (g, twin):
        e.set(_lib.FLD_POS_X, px); e.set(_lib.FLD_POS_Y, py)
    for s in range(3):
        want = _shaped_step(g, twin, np.zeros((A, N), F), "cap, step %d" % s, _lib.F_STATS | _lib.F_AUTORESET)
        if s < 2:
            assert want["collision"][:, :2].all()
    assert (_get(g, "EPISODE") == 1).all() and _get(g, "ARENA_DONE").all()
    for n in ("collision", "wall", "near", "wall_near", "arrival"):
        assert not want[n].any(), n                                # the positions are the next episode's; the cap credits nobody
    assert want["step"].all()
    g.close(); twin.close()


def test_autoreset_when_every_agent_arrives_in_one_step():
    A, N = 3, 6
    p = H.scenario_params("doorway", N, done_x_thresh=100.0)       # CA_DONE_XLESS: every agent is left of the threshold at once
    g, twin = (H.make_gpu(A, N, "doorway", p, seed=2) for _ in range(2))
    g.set_reward_terms(**ALL)
    want = _shaped_step(g, twin, np.zeros((A, N), F), "all arrive", _lib.F_STATS | _lib.F_AUTORESET)
    assert _get(g, "ARENA_DONE").all() and not _get(g, "AGENT_DONE").any()      # respawned: the flags are cleared
    assert want["arrival"].all() and want["step"].all() and not want["collision"].any() and not want["wall_near"].any()
    la = g.arena_stats()["last_episode_arrived"]
    assert (la == N).all()
    g.close(); twin.close()


def test_freeze_leaves_a_frozen_arena_its_reward():
    A, N = 4, 10
    p = H.scenario_params("doorway", N)
    g, twin = (H.make_gpu(A, N, "doorway", p, seed=5) for _ in range(2))
    g.set_reward_terms(**ALL)
    act = np.random.RandomState(1).uniform(-1, 1, (A, N)).astype(F)
    _shaped_step(g, twin, act, "before the freeze", _lib.F_FREEZE)
    ad = np.asarray([0, 0, 1, 0], np.int32)
    for e in (g, twin):
        e.set(_lib.FLD_ARENA_DONE, ad)
    held, parts = _get(g, "REWARD")[2].copy(), {k: v[2].copy() for k, v in g.last_reward_parts().items()}
    for s in range(2):
        want = _shaped_step(g, twin, act, "frozen at entry, step %d" % s, _lib.F_FREEZE | _lib.F_STATS)
        assert not want["written"][2].any() and want["written"][[0, 1, 3]].all()
        H._eq(_get(g, "REWARD")[2], held, "the frozen arena's reward")
        for k, v in g.last_reward_parts().items():
            H._eq(v[2], parts[k], "the frozen arena's parts: " + k)
    g.close(); twin.close()


def test_regoal_arrival_follows_regoal_count():
    A, N = 3, 12
    p = scenarios.bench_params(N, 5.0, 10)
    assert p["done_mode"] == _lib.DONE_REGOAL
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=2) for _ in range(2))
    g.set_reward_terms(**ALL)
    gx, gy = _get(g, "GOAL_X"), _get(g, "GOAL_Y")
    gx[:, ::3], gy[:, ::3] = _get(g, "POS_X")[:, ::3], _get(g, "POS_Y")[:, ::3]     # every third agent stands on its goal
    for e in (g, twin):
        e.set(_lib.FLD_GOAL_X, gx); e.set(_lib.FLD_GOAL_Y, gy)
    before = _get(g, "REGOAL_COUNT").copy()
    want = _shaped_step(g, twin, np.zeros((A, N), F), "regoal", _lib.F_STATS)
    assert (want["arrival"] == (_get(g, "REGOAL_COUNT") != before)).all() and want["arrival"][:, ::3].all() and not want["arrival"].all()
    assert want["step"].all()
    before = _get(g, "REGOAL_COUNT").copy()
    want = _shaped_step(g, twin, np.zeros((A, N), F), "regoal, the step after", _lib.F_STATS)
    assert (want["arrival"] == (_get(g, "REGOAL_COUNT") != before)).all() and not want["arrival"].all() and want["step"].all()
    g.close(); twin.close()


# ---- 5. the rollouts against the loop of shaped steps on a twin -----------------------------------------------------------------------
def test_rollout_actions_takes_the_per_step_form(monkeypatch):
    monkeypatch.setenv("CA_QUAD", "1")
    A, N, T, hold = 4, 16, 40, 3
    p = H.scenario_params("crowd", N, neighbor_dist=1.5, max_neighbors=5)
    g, twin = (H.make_gpu(A, N, "crowd", p, seed=11) for _ in range(2))
    assert g.launch_info()["rollout_one_launch"] == 1
    for e in (g, twin):
        e.set_reward_terms(**_per_arena(A))
    w = (F(0.99) ** np.arange(T)).astype(F)
    g.profile(1); g.profile_read()
    out, ret, fd, _ = TA._case(g, twin, None, "4 x 16 under terms", T, hold, weights=w, one_launch=True, stats=True)
    prof = g.profile_read(); g.profile(0)
    assert prof["step_kernel"][0] == T and prof["reset_kernels"][0] == 1 + 3 * T, prof      # set-up; begin, terms, accumulate per step
    assert np.abs(ret).max() > 0 and g.last_reward_parts()["step"].any()
    g.close(); twin.close()


def test_rollout_policy_and_sample_records():
    A, N = 4, 10
    g, twin = TP._doorway_pair(max_step=50)
    for e in (g, twin):
        e.set_reward_terms(**_per_arena(A))
    layers = TP._layers((64, 64), None, seed=4)
    w = (F(0.9) ** np.arange(7)).astype(F)
    res = TP._case(g, twin, layers, None, "rollout_policy under terms, 7 / 3", 7, 3, weights=w, noise=True, stats=True)
    parts = g.last_reward_parts()
    H._eq(res["rewards"][6], RS.weighted_sum(parts["ref"], [parts[n] for n in RS.COUNTS], _weights(g)), "the last reward record is the shaped one")
    assert (res["rewards"][6] != parts["ref"]).all()                  # the time term alone moves every row
    res = PP._sample_case(g, twin, layers, None, PP._both_heads(), "rollout_policy_sample under terms, 7 / 3", 7, 3, weights=w, stats=True)
    parts = g.last_reward_parts()
    H._eq(res["rewards"][6], RS.weighted_sum(parts["ref"], [parts[n] for n in RS.COUNTS], _weights(g)), "sample: the last reward record")
    assert np.abs(res["advantages"]).max() > 0 and np.abs(res["row_rewards"]).max() > 0
    g.close(); twin.close()


def _trap(A, N, terms):
    p = {k: v for k, v in S.trap_params().items() if k != "max_obst_neighbors"}
    g = H.make_gpu(A, N, "doorway", p, polys=S.trap_world(), max_obst_neighbors=16)
    S.trap_setup(g, _lib, A, N)
    gr = S.TRAP_GRID
    g.set_navigation([S.TRAP_TARGET], 0, gr["cell"], origin=(gr["x0"], gr["y0"]), shape=(gr["gx"], gr["gy"]), clearance=S.TRAP_CLEARANCE,
                     lookahead=S.TRAP_LOOKAHEAD)
    if terms:
        g.set_reward_terms(**terms)
    return g


def _nav_stepper(e, act, flags):
    e.step_nav(act, with_obs=False, stats=bool(flags & _lib.F_STATS))


def test_step_nav_and_rollout_nav_policy_on_the_trap():
    A, N, T = 2, 8, 12
    terms = _per_arena(A)
    g, plain, twin = _trap(A, N, terms), _trap(A, N, None), _trap(A, N, terms)
    actions = np.random.RandomState(21).uniform(-0.5, 0.5, (T, A, N)).astype(F)
    g.profile(1); g.profile_read(); plain.profile(1); plain.profile_read()
    for t in range(T):
        _shaped_step(g, plain, actions[t], "step_nav %d" % t, _lib.F_STATS, stepper=_nav_stepper)
        _nav_stepper(twin, actions[t], _lib.F_STATS)
    pg, pp = g.profile_read(), plain.profile_read()
    assert pg["reset_kernels"][0] == pp["reset_kernels"][0] + 2 * T == 4 * T, (pg, pp)      # a navigated step: begin and terms more
    g.profile(0)
    # the rollout on g, the loop of observe / policy_actions / shaped step_nav on the twin
    layers = TP._layers((64, 64), None, seed=4)
    steps, hold = 6, 2
    for e in (g, twin):
        e.set_policy(layers, out="clip", limit=0.5)
    g.profile(1); g.profile_read()
    res = g.rollout_nav_policy(steps, hold=hold, returns=True, first_done=True, stats=True)
    prof = g.profile_read()
    assert prof["reset_kernels"][0] == 1 + 3 + 5 * steps, prof      # set-up, a policy launch per row; begin, nav_act, nav_reward, terms, record per step
    ret = np.zeros((A, N), F)
    for t in range(steps):
        if t % hold == 0:
            twin.observe()
            act = TP._np(twin.policy_actions(None)).copy()
            H._eq(res["actions"][t // hold], act, "row %d: actions" % (t // hold))
        _nav_stepper(twin, act, _lib.F_STATS)
        H._eq(res["rewards"][t], _get(twin, "REWARD"), "step %d: the reward record is the shaped reward" % t)
        ret = (ret + _get(twin, "REWARD")).astype(F)
    H._eq(res["returns"], ret, "returns")
    for n in STATE:
        H._eq(_get(g, n), _get(twin, n), "rollout_nav_policy: " + n)
    assert (_get(g, "REWARD") != _get(plain, "REWARD")).any()
    sg, st = g.stats(), twin.stats()
    assert abs(sg["sum_reward"] - st["sum_reward"]) <= 1e-9 * max(1.0, abs(st["sum_reward"]))
    for e in (g, plain, twin):
        e.close()


# ---- 6. ca_step_packed ------------------------------------------------------------------------------------------------------------------
def test_step_packed_reward_block_is_the_shaped_one():
    A, N = 3, 10
    p = H.scenario_params("doorway", N)
    g, twin = (H.make_gpu(A, N, "doorway", p, seed=1) for _ in range(2))
    g.set_reward_terms(**_per_arena(A))
    rs = np.random.RandomState(1)
    for s in range(3):
        act = rs.uniform(-1, 1, (A, N)).astype(F)
        obs, rew, done, _ = g.step_packed(act, stats=True)
        obs_t, rew_t, done_t, _ = twin.step_packed(act, stats=True)
        parts = g.last_reward_parts()
        H._eq(parts["ref"], rew_t, "step %d: plane 0 is the twin's packed reward" % s)
        H._eq(rew, RS.weighted_sum(rew_t, [parts[n] for n in RS.COUNTS], _weights(g)), "step %d: the packed reward block" % s)
        H._eq(rew, _get(g, "REWARD"), "step %d: ... and the field" % s)
        H._eq(obs, obs_t, "step %d: the packed observation" % s)
        assert (rew != rew_t).all()
    g.close(); twin.close()


# ---- 7. fork ----------------------------------------------------------------------------------------------------------------------------
def test_per_arena_weights_stay_with_the_slot_under_fork():
    A, N = 4, 10
    p = H.scenario_params("doorway", N)
    g, twin = (H.make_gpu(A, N, "doorway", p, seed=5) for _ in range(2))
    g.set_reward_terms(**_per_arena(A))
    w = _weights(g).copy()
    act = np.random.RandomState(2).uniform(-1, 1, (A, N)).astype(F)
    _shaped_step(g, twin, act, "before the fork")
    snap = g.snapshot()
    for e in (g, twin):
        e.fork(np.ones(A, np.int32))
    H._eq(_weights(g), w, "the weights after fork")
    act[:] = act[1]
    want = _shaped_step(g, twin, act, "after the fork")
    for a in range(A):                                              # one state in every slot, the slot's own weights
        H._eq(want["ref"][a], want["ref"][1], "arena %d: the reference reward" % a)
    assert all((_get(g, "REWARD")[a] != _get(g, "REWARD")[b]).any() for a in range(A) for b in range(a))
    g.restore(snap, np.asarray([2, 2, 2, 2], np.int32))
    H._eq(_weights(g), w, "the weights after restore")
    info = g.reward_terms_info()
    assert info["configured"] and info["per_arena"] and info["margin"] == F(0.3)
    g.close(); twin.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    A, N = 3, 10
    p = H.scenario_params("doorway", N)
    g, twin = (H.make_gpu(A, N, "doorway", p, seed=7) for _ in range(2))
    L = g.L
    EINVAL, ESIZE, ERANGE = -1, -4, -5
    err = lambda: L.ca_last_error(g.h).decode()
    buf = np.zeros((A, N), F)
    assert L.ca_reward_parts(g.h) == EINVAL and "ca_reward_configure" in err()
    assert L.ca_get_reward_parts(g.h, buf.ctypes.data_as(C.c_void_p), None, buf.nbytes, 0, 0) == EINVAL
    assert L.ca_reward_get_weights(g.h, buf.ctypes.data_as(C.c_void_p), A * 7 * 4) == EINVAL
    with pytest.raises(RuntimeError):
        g.last_reward_parts()
    dev, nbytes = C.c_void_p(), C.c_size_t()
    assert L.ca_reward_parts_ptr(g.h, C.byref(dev), C.byref(nbytes)) == 0 and dev.value and nbytes.value == 7 * A * N * 4
    assert L.ca_get_reward_parts(g.h, buf.ctypes.data_as(C.c_void_p), None, buf.nbytes, 0, 0) == EINVAL     # the buffer alone is no result
    g.set_reward_terms(**_per_arena(A))
    w, info = _weights(g).copy(), g.reward_terms_info()

    def desc(weights, per_arena=1, margin=0.3, nbytes=None):
        weights = np.ascontiguousarray(weights, F)
        d = _lib.RewardDesc(weights=weights.ctypes.data, weights_bytes=weights.nbytes if nbytes is None else nbytes, per_arena=per_arena, margin=margin)
        return d, weights
    bad = w.copy(); bad[1, 3] = np.nan
    inf = w.copy(); inf[2, 6] = np.inf
    cases = [(None, EINVAL, "null"), (desc(w, per_arena=2), EINVAL, "per_arena"), (desc(w, per_arena=-1), EINVAL, "per_arena"),
             (desc(w, nbytes=w.nbytes - 4), ESIZE, "bytes"), (desc(w, per_arena=0), ESIZE, "bytes"), (desc(w[0], per_arena=1), ESIZE, "bytes"),
             (desc(bad), ERANGE, "arena 1, term 3"), (desc(inf), ERANGE, "arena 2, term 6"),
             (desc(w, margin=-0.5), ERANGE, "margin"), (desc(w, margin=float("nan")), ERANGE, "margin"),
             (desc(w, margin=float("inf")), ERANGE, "margin"), (desc(w, margin=1000.5), ERANGE, "margin")]
    d0 = _lib.RewardDesc(weights=None, weights_bytes=w.nbytes, per_arena=1, margin=0.3)
    cases.append(((d0, None), EINVAL, "null"))
    for c, code, word in cases:
        rc = L.ca_reward_configure(g.h, C.byref(c[0]) if c is not None else None)
        assert rc == code and word in err(), (rc, code, word, err())
        now = g.reward_terms_info()
        H._eq(now.pop("weights"), w, "the weights after a refusal (%s)" % word)
        assert now == {k: v for k, v in info.items() if k != "weights"}
    act = np.random.RandomState(3).uniform(-1, 1, (A, N)).astype(F)
    _shaped_step(g, twin, act, "after the refusals")
    cnt = np.zeros((6, A, N), np.int32)
    assert L.ca_get_reward_parts(g.h, buf.ctypes.data_as(C.c_void_p), None, buf.nbytes - 4, 0, 0) == ESIZE
    assert L.ca_get_reward_parts(g.h, None, cnt.ctypes.data_as(C.c_void_p), 0, cnt.nbytes + 4, 0) == ESIZE
    assert L.ca_reward_get_weights(g.h, buf.ctypes.data_as(C.c_void_p), 4) == ESIZE
    assert L.ca_get_reward_parts(g.h, buf.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), buf.nbytes, cnt.nbytes, 0) == 0
    H._eq(buf, _get(twin, "REWARD"), "ca_get_reward_parts: plane 0")
    g.clear_reward_terms()
    assert g.reward_terms_info() == dict(configured=False, per_arena=False, margin=0.0, weights=None)
    for e in (g, twin):
        TP._gpu_step(e, act, 0)
    H._eq(_get(g, "REWARD"), _get(twin, "REWARD"), "after clear_reward_terms the reward is the reference's")
    g.close(); twin.close()


def test_constructor_keyword_and_torch_views():
    torch = pytest.importorskip("torch")
    A, N = 3, 10
    p = H.scenario_params("doorway", N)
    g = H.make_gpu(A, N, "doorway", p, seed=1, use_torch=True, reward_terms=dict(ALL))
    twin = H.make_gpu(A, N, "doorway", p, seed=1)
    info = g.reward_terms_info()
    assert info["configured"] and not info["per_arena"] and info["margin"] == F(0.3) and (info["weights"] == info["weights"][0]).all()
    act = np.random.RandomState(3).uniform(-1, 1, (A, N)).astype(F)
    _, rew, _, _ = g.step(act)
    twin.step(act)
    parts = g.last_reward_parts()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and tuple(v.shape) == (A, N) for v in parts.values())
    assert parts["ref"].dtype == torch.float32 and parts["step"].dtype == torch.int32
    assert parts["collision"].data_ptr() - parts["ref"].data_ptr() == A * N * 4          # planes of the one [7, A, N] buffer
    g.sync()
    host = {k: v.cpu().numpy() for k, v in parts.items()}
    H._eq(host["ref"], _get(twin, "REWARD"), "torch views: plane 0")
    H._eq(rew.cpu().numpy(), RS.weighted_sum(host["ref"], [host[n] for n in RS.COUNTS], info["weights"]), "torch: the reward tensor is shaped")
    g.close(); twin.close()


# ---- 9. launch counts -------------------------------------------------------------------------------------------------------------------
def test_launch_counts(monkeypatch):
    """kind 3 of ca_profile: a handle without terms launches what it always did; with terms every step of a plain call adds two"""
    monkeypatch.setenv("CA_QUAD", "0")
    A, N = 4, 16
    p = H.scenario_params("crowd", N)
    g, plain = (H.make_gpu(A, N, "crowd", p, seed=11) for _ in range(2))
    layers = TP._layers((64, 64), None, seed=4)
    for e in (g, plain):
        e.set_policy(layers); e.set_policy_heads(*PP._both_heads())
        e.profile(1); e.profile_read()
    g.set_reward_terms(**ALL)
    act = np.zeros((A, N), F)
    seq = np.zeros((14, A, N), F)
    calls = [("step", lambda e: e.step(act, with_obs=False), 1, 0),
             ("rollout_actions", lambda e: e.rollout_actions(seq, hold=3, steps=40), 40, 1 + 40),
             ("rollout_policy", lambda e: e.rollout_policy(7, hold=3), 7, 1 + 3 + 7),
             ("rollout_policy_sample", lambda e: e.rollout_policy_sample(7, hold=3), 7, 1 + 3 + 7 + 1 + 1)]
    for name, call, steps, parent in calls:
        call(g); call(plain)
        pg, pp = g.profile_read(), plain.profile_read()
        assert pp["reset_kernels"][0] == parent, (name, pp)                       # the parent's count
        assert pg["reset_kernels"][0] == parent + 2 * steps, (name, pg)
        assert pg["step_kernel"][0] == pp["step_kernel"][0] == steps and pg["obs_kernel"][0] == pp["obs_kernel"][0], (name, pg, pp)
    g.reward_parts()
    assert g.profile_read()["reset_kernels"][0] == 1
    g.orca_step(); g.rollout(5)                                                   # no reward is written: nothing new
    assert g.profile_read()["reset_kernels"][0] == 0
    g.close(); plain.close()
