"""The navigated action step on the GPU (ca_nav_act, ca_nav_step, ca_rollout_nav_actions, ca_rollout_nav_policy; include/ca_env.h).
Everything is compared bit for bit (==; no tolerance anywhere but the one sum noted below):
  * ca_nav_act against the numpy restatement (tests/nav_step_scenes.py), row kinds placed by hand; rows that are not steered keep
    their bits, and no other field moves;
  * ca_nav_step against the CPU loop on the trap, and -- with no row navigated -- against a twin handle driven by ca_step;
  * the two rollouts against a twin handle driven call by call through step_nav (and observe / policy_actions), one handle of every
    form in which an ORCA-only step is launched.  ca_stats.sum_reward is added up by the kernel behind the step in an order that is not
    defined: it is compared to 1e-9 relative, the project's tolerance for tiled handles, every other figure exactly;
  * every refusal leaves the handle working; the adapters' navigate=True."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib
from collision_avoidance_amd.adapters import AgentVectorEnv, MultiAgentVectorEnv
from tests import edge_grid_scenes as E
from tests import helpers as H
from tests import nav_scenes as S
from tests import nav_step_scenes as NS

pytestmark = pytest.mark.gpu

F = np.float32
STATE = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "GOAL2_X", "GOAL2_Y", "AGENT_DONE", "ARRIVE_STEP",
         "REGOAL_COUNT", "NB_COUNT", "NB_IDX", "OBST_COUNT", "OBST_IDX", "STEP_COUNT", "ARENA_DONE", "EPISODE", "REWARD")
EINVAL, ESIZE = -1, -4


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _nav(g, grid, clearance, targets, cls, lookahead=2):
    g.set_navigation(targets, cls, grid["cell"], origin=(grid["x0"], grid["y0"]), shape=(grid["gx"], grid["gy"]), clearance=clearance,
                     lookahead=lookahead)


def _same_handles(a, b, what, skip=()):
    """every field, and the statistics: sum_reward to 1e-9 relative (see above), everything else exactly"""
    for n in STATE:
        if n not in skip:
            H._eq(a.get(getattr(_lib, "FLD_" + n)), b.get(getattr(_lib, "FLD_" + n)), "%s: %s" % (what, n))
    sa, sb = a.stats(), b.stats()
    ra, rb = a.get(_lib.FLD_ARENA_STATS), b.get(_lib.FLD_ARENA_STATS)
    assert {k: v for k, v in sa.items() if k != "sum_reward"} == {k: v for k, v in sb.items() if k != "sum_reward"}, (what, sa, sb)
    assert abs(sa["sum_reward"] - sb["sum_reward"]) <= 1e-9 * max(1.0, abs(sb["sum_reward"])), (what, sa, sb)
    cols = [c for c in range(ra.shape[1]) if c != 5]
    assert np.array_equal(ra[:, cols], rb[:, cols]), what + ": per-arena counters"
    pa, pb = ra[:, 5].copy().view(np.float64), rb[:, 5].copy().view(np.float64)
    assert (np.abs(pa - pb) <= 1e-9 * np.maximum(1.0, np.abs(pb))).all(), (what, pa, pb)


# ---- 1. ca_nav_act ---------------------------------------------------------------------------------------------------------------------------
ROWS = ((6.3, 2.2, 0),      # an ordinary free cell, the door between it and its target
        (8.7, 2.3, 1),      # the source cell of target 1
        (7.5, 2.6, 1),      # beside it: a walk of 3 reaches STAY, a walk of 1 does not
        (2.5, 2.5, 0),      # inside the wall: a blocked cell, left by its escape pointer
        (7.5, 7.5, 0),      # the pen: NONE
        (-9.0, 12.0, 1),    # outside the grid's box: clamped into cell (0, 9)
        (5.5, 6.5, -1),     # class -1: steered towards its own goal
        (4.5, 3.5, 0))      # agent_done = 1 with a class: steered towards its own goal


@pytest.mark.parametrize("lookahead", [1, 3])
def test_nav_act_equals_the_definition_and_leaves_everything_else_alone(lookahead):
    A, N = 2, 8
    g = H.make_gpu(A, N, "doorway", H.scenario_params("doorway", N), polys=S.doorway_world(pen=True), agent_counts=[8, 7])
    grid = S.Grid(**S.DOORWAY_GRID)
    px = np.stack([np.asarray([r[0] for r in ROWS], F), np.asarray([r[0] for r in ROWS], F) + F(0.125)])
    py = np.stack([np.asarray([r[1] for r in ROWS], F), np.asarray([r[1] for r in ROWS], F) - F(0.125)])
    cls = np.stack([np.asarray([r[2] for r in ROWS], np.int32), np.asarray([1 - r[2] if r[2] >= 0 else -1 for r in ROWS], np.int32)])
    done = np.zeros((A, N), np.int32)
    done[0, 7] = 1                                                 # arena 1, row 7: absent under the counts (8, 7), and not done
    cls[1, 7] = 0
    g.set(_lib.FLD_POS_X, px); g.set(_lib.FLD_POS_Y, py); g.set(_lib.FLD_AGENT_DONE, done)
    _nav(g, S.DOORWAY_GRID, S.DOORWAY_CLEARANCE, S.DOORWAY_TARGETS, cls, lookahead=lookahead)
    edges = [S.edges_of_table(g.obstacle_table(0))]
    fields = S.all_fields(edges, grid, S.DOORWAY_CLEARANCE, S.DOORWAY_TARGETS)
    present = np.arange(N)[None, :] < np.asarray([8, 7])[:, None]
    actions = np.random.RandomState(7).uniform(-np.pi, np.pi, (A, N)).astype(F)
    actions[0, 0], actions[0, 1], actions[0, 2], actions[1, 0], actions[1, 3] = 0.0, np.pi, -np.pi, 0.0, np.pi
    gx_, gy_ = g.get(_lib.FLD_GOAL_X), g.get(_lib.FLD_GOAL_Y)
    for freeze, arena_done in ((False, (0, 0)), (False, (0, 1)), (True, (0, 1))):
        g.set(_lib.FLD_ARENA_DONE, np.asarray(arena_done, np.int32))
        old_x = np.random.RandomState(3).uniform(-1, 1, (A, N)).astype(F)
        old_y = np.random.RandomState(4).uniform(-1, 1, (A, N)).astype(F)
        g.set(_lib.FLD_PREF_X, old_x); g.set(_lib.FLD_PREF_Y, old_y)
        before = g.get_state()
        old_d, old_h = np.full((A, N), 123.0, F), np.full((2, A, N), -77.0, F)
        got = g.nav_act(actions, heading=old_h.copy(), dist=old_d.copy(), freeze=freeze)
        after = g.get_state()
        steered = present & ~(freeze & (np.asarray(arena_done) != 0))[:, None]
        w = NS.nav_act(grid, fields, cls, lookahead, px, py, gx_, gy_, done, actions, steered)
        what = "lookahead %d, freeze %s, arena_done %s" % (lookahead, freeze, arena_done)
        assert steered.sum() == (15 if not freeze else 8) and w["navigated"].sum() == (12 if not freeze else 6), (what, steered, w["navigated"])
        assert not w["navigated"][:, 6].any() and not w["navigated"][0, 7] and not steered[1, 7]
        H._eq(after["PREF_X"], np.where(steered, w["rot_x"], old_x), what + ": PREF_X")
        H._eq(after["PREF_Y"], np.where(steered, w["rot_y"], old_y), what + ": PREF_Y")
        H._eq(_np(got["heading"])[0], np.where(steered, w["dir_x"], old_h[0]), what + ": heading_out x")
        H._eq(_np(got["heading"])[1], np.where(steered, w["dir_y"], old_h[1]), what + ": heading_out y")
        H._eq(_np(got["dist"]), np.where(w["navigated"], w["dist"], old_d), what + ": dist_out")
        for k in before:
            if k not in ("PREF_X", "PREF_Y"):
                H._eq(after[k], before[k], what + ": " + k)
        # the kinds did occur (arena 0), and the restatement's heading of a navigated row is nav_pref's
        from oracle import oracle as o
        nx, ny, nd, m = S.nav_pref(grid, fields, cls, lookahead, px, py, gx_, gy_, o.pref_dir64, steered & (done == 0))
        H._eq(w["dir_x"][m], nx[m], what + ": the heading of navigated rows is nav_pref's"); H._eq(w["dir_y"][m], ny[m], what)
        own = lambda i: tuple(F(v) for v in o.pref_dir64(px[0, i], py[0, i], float(gx_[0, i]), float(gy_[0, i])))   # noqa: E731
        d0 = lambda i: (w["dir_x"][0, i], w["dir_y"][0, i])   # noqa: E731
        assert (w["rot_x"][0, 0], w["rot_y"][0, 0]) == d0(0)                                           # action 0: the heading's value
        assert w["dist"][0, 1] == 0.0 and d0(1) == own(1)                                               # the source: the own goal
        assert w["rot_x"][0, 1] * w["dir_x"][0, 1] + w["rot_y"][0, 1] * w["dir_y"][0, 1] < -0.999       # action pi turns round
        assert (d0(2) == own(2)) == (lookahead == 3)                                                    # STAY before the lookahead runs out
        assert np.isinf(w["dist"][0, 3]) and d0(3) != own(3)                                            # blocked: led out
        assert np.isinf(w["dist"][0, 4]) and d0(4) == own(4)                                            # the pen: the own goal
        assert np.isfinite(w["dist"][0, 5]) and w["dist"][0, 5] == fields[0][1][0][9, 0]                # clamped into cell (0, 9)
        assert d0(6) == own(6) and d0(7) == own(7)                                                      # class -1; done with a class
    assert g.nav_act(actions) is None
    g.close()


# ---- 2. ca_nav_step against the CPU loop -----------------------------------------------------------------------------------------------------
def test_step_nav_on_the_trap_equals_the_cpu_loop():
    A, N, T = 2, 8, 60
    actions = np.random.RandomState(21).uniform(-0.5, 0.5, (T, A, N)).astype(F)
    cpu = NS.trap_cpu_nav_run(A, T, actions, every=10)
    p = {k: v for k, v in S.trap_params().items() if k != "max_obst_neighbors"}
    g = H.make_gpu(A, N, "doorway", p, polys=S.trap_world(), max_obst_neighbors=16)
    S.trap_setup(g, _lib, A, N)
    _nav(g, S.TRAP_GRID, S.TRAP_CLEARANCE, [S.TRAP_TARGET], 0, lookahead=S.TRAP_LOOKAHEAD)
    H._eq(g.nav_field()[0], cpu["fields"][0][0][0], "the trap's field")
    for t in range(T):
        _, rew, _, _ = g.step_nav(actions[t], with_obs=False, stats=True)
        if (t + 1) % 10 == 0:
            rec = cpu["records"][(t + 1) // 10 - 1]
            for c, f in enumerate(("POS_X", "POS_Y", "VEL_X", "VEL_Y")):
                H._eq(g.get(getattr(_lib, "FLD_" + f)), rec[c], "after %d steps: %s" % (t + 1, f))
            H._eq(_np(rew), rec[4], "after %d steps: REWARD" % (t + 1))
    assert g.stats()["obst_collisions"] == 0 and (g.get(_lib.FLD_STEP_COUNT) == T).all()
    g.close()


# ---- 3. with no row navigated it is ca_step ---------------------------------------------------------------------------------------------------
def test_step_nav_with_no_row_navigated_is_step():
    A, N = 4, 16
    p = H.scenario_params("doorway", N, max_step=12)
    g, twin = (H.make_gpu(A, N, "doorway", p, seed=5) for _ in range(2))
    _nav(g, S.DOORWAY_GRID, S.DOORWAY_CLEARANCE, S.DOORWAY_TARGETS, -1)
    rs = np.random.RandomState(9)
    for t in range(30):
        a = rs.uniform(-np.pi / 4, np.pi / 4, (A, N)).astype(F)
        og, rg, dg, _ = g.step_nav(a, with_obs=True, stats=True, autoreset=True)
        ot, rt, dt, _ = twin.step(a, with_obs=True, stats=True, autoreset=True)
        what = "step %d" % t
        H._eq(_np(og), _np(ot), what + ": the observation"); H._eq(_np(rg), _np(rt), what + ": the reward returned")
        H._eq(_np(dg), _np(dt), what + ": dones")
        # PREF afterwards is goal_dir of the new position, ARRIVE_STEP is counted the ORCA-only way (include/ca_env.h): excluded
        _same_handles(g, twin, what, skip=("PREF_X", "PREF_Y", "ARRIVE_STEP"))
    assert (g.get(_lib.FLD_EPISODE) >= 2).all()                    # episodes did end inside: the step that ends one is rewarded like any other
    g.close(); twin.close()


# ---- 4. the action rollout is its loop ------------------------------------------------------------------------------------------------------
def _pair(A, N, scenario="doorway", polys=None, over=None, **kw):
    p = H.scenario_params(scenario, N, **(over or {}))
    return [H.make_gpu(A, N, scenario, p, seed=5, polys=polys, **kw) for _ in range(2)]


def _doorway_nav(envs, A, N, lookahead=2):
    cls = (np.arange(A * N).reshape(A, N) % 3 - 1).astype(np.int32)          # -1, 0, 1, ...
    for e in envs:
        _nav(e, S.DOORWAY_GRID, S.DOORWAY_CLEARANCE, S.DOORWAY_TARGETS, cls, lookahead=lookahead)


def _shape_pair(shape, over):
    if shape == "4x16_one_launch_handle":
        A, N = 4, 16
        g, twin = _pair(A, N, over=over)
        assert g.launch_info()["rollout_one_launch"] == 1                     # ca_rollout would be one launch here: the per-step form is taken
        _doorway_nav((g, twin), A, N)
    elif shape == "2x80_agent_params":
        A, N = 2, 80
        g, twin = _pair(A, N, over=over)
        rs = np.random.RandomState(2)
        ap = dict(radius=rs.uniform(0.3, 0.5, (A, N)).astype(F), max_speed=rs.uniform(0.8, 1.2, (A, N)).astype(F))
        for e in (g, twin):
            e.set_agent_params(**ap)
        assert g.launch_info()["agent_params"]
        _doorway_nav((g, twin), A, N, lookahead=3)
    elif shape == "2x20_counts":
        A, N = 2, 20
        g, twin = _pair(A, N, over=over, agent_counts=[12, 20])
        _doorway_nav((g, twin), A, N)
    else:
        A, N = 1, 200
        g, twin = _pair(A, N, scenario="crowd", polys=E.hall(200), over=over, tiled="grid", edge_grid=True, allow_obst_overflow=True)
        assert g.tiled_info()["tiled"] and g.edge_grid_info()["on"]
        cls = (np.arange(N)[None, :] % 2).astype(np.int32)
        for e in (g, twin):
            e.set_navigation([(2.75, 2.75), (8.75, 5.75)], cls, 0.5, lookahead=2)          # the grid: the table's bounding box
    return A, N, g, twin


def _loop_actions(twin, actions, hold, steps, weights, present, **kw):
    """the loop of step_nav on the twin; returns (returns, first_done) by numpy's fp32 ret + w * r over its per-step rewards"""
    A, N = twin.A, twin.N
    ret, fd = np.zeros((A, N), F), np.full(A, -1, np.int32)
    freeze = kw.get("freeze", False)
    for t in range(steps):
        advanced = ~((twin.get(_lib.FLD_ARENA_DONE) != 0) & freeze)
        _, r, d, _ = twin.step_nav(actions[t // hold], with_obs=False, **kw)
        wr = (F(1.0 if weights is None else weights[t]) * _np(r).astype(F)).astype(F)
        ret = np.where(advanced[:, None] & present, (ret + wr).astype(F), ret)
        fd = np.where((fd < 0) & advanced & (_np(d) != 0), t, fd).astype(np.int32)
    return ret, fd


@pytest.mark.parametrize("mode", ["autoreset", "freeze_max_step_7"])
@pytest.mark.parametrize("shape", ["4x16_one_launch_handle", "2x80_agent_params", "2x20_counts", "1x200_tiled_grid"])
def test_rollout_nav_actions_is_the_loop_of_step_nav(shape, mode):
    kw = dict(stats=True, autoreset=True) if mode == "autoreset" else dict(stats=True, freeze=True)
    A, N, g, twin = _shape_pair(shape, dict(max_step=7) if mode != "autoreset" else (dict(max_step=9) if shape != "1x200_tiled_grid" else None))
    present = g.agent_mask()
    steps, hold = 11, 3
    actions = np.random.RandomState(13).uniform(-0.6, 0.6, (4, A, N)).astype(F)
    weights = (F(0.9) ** np.arange(steps)).astype(F)
    res = g.rollout_nav_actions(actions, hold=hold, weights=weights, steps=steps, returns=True, first_done=True, **kw)
    ret, fd = _loop_actions(twin, actions, hold, steps, weights, present, **kw)
    what = "%s, %s" % (shape, mode)
    _same_handles(g, twin, what)
    H._eq(_np(res["returns"]), ret, what + ": returns"); H._eq(_np(res["first_done"]), fd, what + ": first_done")
    if mode != "autoreset":
        assert (fd == 6).all() and (g.get(_lib.FLD_STEP_COUNT) == 7).all() and (g.stats()["agent_steps"] == 7 * present.sum())
    elif shape != "1x200_tiled_grid":
        assert (fd == 8).all() and (g.get(_lib.FLD_EPISODE) >= 1).all()                   # an episode ended inside the call
    assert (ret[~present] == 0).all() and (ret[present] != 0).any()
    # the observation and the contact report behind the last step; no weights, no returns
    res = g.rollout_nav_actions(actions[:1], hold=3, returns=False, with_obs=True, contacts=True, **kw)
    for _ in range(2):
        twin.step_nav(actions[0], with_obs=False, **kw)
    obs, _, _, info = twin.step_nav(actions[0], with_obs=True, contacts=True, **kw)
    assert res["returns"] is None and res["first_done"] is None
    _same_handles(g, twin, what + ", obs and contacts")
    H._eq(_np(res["obs"]), _np(obs), what + ": the observation behind the last step")
    ca = g.last_contacts()
    for k in ca:
        H._eq(_np(ca[k]), _np(info["contacts"][k]), what + ": contact report, " + k)
    g.close(); twin.close()


# ---- 5. the policy rollout is its loop ------------------------------------------------------------------------------------------------------
def test_rollout_nav_policy_is_the_loop_of_observe_policy_actions_and_step_nav():
    A, N, steps, hold = 4, 16, 7, 2
    R = (steps + hold - 1) // hold
    g, twin = _pair(A, N)
    _doorway_nav((g, twin), A, N)
    rs = np.random.RandomState(31)
    layers = [((rs.standard_normal((2, o, i)) / np.sqrt(i)).astype(F), (0.3 * rs.standard_normal((2, o))).astype(F)) for i, o in ((64, 16), (16, 1))]
    sets = np.asarray([0, 1, 1, 0], np.int32)
    for e in (g, twin):
        e.set_policy(layers, sets=sets, out="clip", limit=1.0)
    noise = (0.3 * rs.standard_normal((R, A, N))).astype(F)
    res = g.rollout_nav_policy(steps, hold=hold, noise=noise, returns=True, first_done=True, stats=True)
    obs_r, act_r, rew_r, done_r = [], [], [], []
    ret = np.zeros((A, N), F)
    for t in range(steps):
        if t % hold == 0:
            obs_r.append(_np(twin.observe()).copy())
            act = _np(twin.policy_actions(noise[t // hold])).copy()
            act_r.append(act)
        _, r, d, _ = twin.step_nav(act, with_obs=False, stats=True)
        rew_r.append(_np(r).copy()); done_r.append(_np(d).astype(np.int32))
        ret = (ret + _np(r).astype(F)).astype(F)
    _same_handles(g, twin, "policy rollout")
    for name, want in (("obs", obs_r), ("actions", act_r), ("rewards", rew_r), ("dones", done_r)):
        H._eq(_np(res[name]), np.stack(want), "record: " + name)
    H._eq(_np(res["returns"]), ret, "returns")
    assert (_np(res["first_done"]) == -1).all() and (np.stack(act_r)[0] != np.stack(act_r)[1]).any() and (np.abs(np.stack(act_r)) <= 1.0).all()
    g.close(); twin.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def _code(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except RuntimeError as ex:
        return int(str(ex).split("(")[1].split(")")[0])
    return 0


def test_every_refusal_leaves_the_handle_working():
    A, N, steps, hold = 2, 8, 5, 2
    R = 3
    g, twin = _pair(A, N)
    act = np.random.RandomState(1).uniform(-0.5, 0.5, (R, A, N)).astype(F)
    layers = [((np.random.RandomState(2).standard_normal((o, i)) / np.sqrt(i)).astype(F), np.zeros(o, F)) for i, o in ((64, 16), (16, 1))]
    for e in (g, twin):
        e.set_policy(layers)
    err = lambda: g.L.ca_last_error(g.h).decode()   # noqa: E731

    def unchanged(before, what):
        g.sync()
        after = g.get_state()
        for k in before:
            H._eq(after[k], before[k], "%s advances nothing: %s" % (what, k))

    # no navigation, and a navigation cleared by set_obstacles
    for stage in ("never configured", "cleared by set_obstacles"):
        if stage != "never configured":
            _doorway_nav((g,), A, N)
            g.set_obstacles(S.doorway_world())
            assert not g.navigation_info()["configured"]
        before = g.get_state()
        for fn, args in ((g.step_nav, (act[0],)), (g.nav_act, (act[0],)), (g.rollout_nav_actions, (act,)), (g.rollout_nav_policy, (steps,))):
            assert _code(fn, *args) == EINVAL and "ca_nav_configure" in err(), (stage, fn, err())
        unchanged(before, stage)
    twin.set_obstacles(S.doorway_world())
    _doorway_nav((g, twin), A, N)
    before = g.get_state()
    # flags and null pointers, through the C ABI itself
    a_buf = g.host_array((R, A, N), np.float32)
    a_buf[...] = act
    ap = C.c_void_p(a_buf.ctypes.data)
    for flags in (_lib.F_NODONE, 64, _lib.F_NODONE | _lib.F_OBS):
        assert g.L.ca_nav_step(g.h, ap, flags) == EINVAL, flags
    assert g.L.ca_nav_step(g.h, None, 0) == EINVAL and "null" in err()
    assert g.L.ca_nav_act(g.h, None, None, None, 0) == EINVAL and g.L.ca_nav_act(g.h, ap, None, None, _lib.F_STATS) == EINVAL
    bufs = dict(weights=g.host_array((steps,), np.float32), returns=g.host_array((A, N), np.float32), first_done=g.host_array((A,), np.int32),
                noise=g.host_array((R, A, N), np.float32), obs_out=g.host_array((R, A, N, 64), np.float32), actions_out=g.host_array((R, A, N), np.float32),
                rewards_out=g.host_array((steps, A, N), np.float32), done_out=g.host_array((steps, A), np.int32))
    for b in bufs.values():
        b[...] = 0
    bufs["weights"][...] = 1.0
    full_a = dict(actions=a_buf.ctypes.data, actions_bytes=a_buf.nbytes, hold=hold)
    for n in ("weights", "returns", "first_done"):
        full_a[n], full_a[n + "_bytes"] = bufs[n].ctypes.data, bufs[n].nbytes
    full_p = dict(hold=hold)
    for n, b in bufs.items():
        full_p[n], full_p[n + "_bytes"] = b.ctypes.data, b.nbytes
    roll_a = lambda n, fl, kw: g.L.ca_rollout_nav_actions(g.h, n, fl, C.byref(_lib.ActionSeq(**kw)) if kw is not None else None)   # noqa: E731
    roll_p = lambda n, fl, kw: g.L.ca_rollout_nav_policy(g.h, n, fl, C.byref(_lib.PolicySeq(**kw)) if kw is not None else None)    # noqa: E731
    names = ("ca_rollout_nav_actions", "ca_rollout_nav_policy", "ca_rollout_actions", "ca_rollout_policy")
    for roll, full, own in ((roll_a, full_a, names[0]), (roll_p, full_p, names[1])):
        cases = [(steps, 0, None, EINVAL), (steps, 0, dict(full, hold=0), EINVAL), (-1, 0, full, EINVAL), (steps, _lib.F_NODONE, full, EINVAL),
                 (steps, 64, full, EINVAL)]
        cases += [(steps, 0, dict(full, **{n: v - 1}), ESIZE) for n, v in full.items() if n.endswith("_bytes")]      # every undersized buffer
        cases += [(steps + 2, 0, full, ESIZE)]
        for n_steps, flags, kw, code in cases:
            assert roll(n_steps, flags, kw) == code, (roll is roll_a, n_steps, flags, kw and {k: v for k, v in kw.items() if k.endswith("_bytes")}, err())
            # the refusal names the call that was made, and no other call that shares its checks
            assert (own + ":") in err() and not any((n + ":") in err() for n in names if n != own), (own, n_steps, flags, err())
    assert roll_a(steps, 0, dict(full_a, actions=None)) == EINVAL
    unchanged(before, "a refused call")
    assert not bufs["returns"].any() and not bufs["rewards_out"].any() and not bufs["first_done"].any()
    # steps == 0: zeros to returns, -1 to first_done, nothing else
    bufs["returns"][...] = 5.0
    assert roll_a(0, 0, full_a) == 0 and roll_p(0, 0, full_p) == 0, err()
    unchanged(before, "zero steps")
    assert not bufs["returns"].any() and (bufs["first_done"] == -1).all() and not bufs["rewards_out"].any()
    # the next valid calls are right
    for e in (g, twin):
        e.step_nav(act[0], with_obs=False, stats=True)
    _same_handles(g, twin, "a step after the refusals")
    res = g.rollout_nav_actions(act, hold=hold, steps=steps, stats=True)
    ret, _ = _loop_actions(twin, act, hold, steps, None, g.agent_mask(), stats=True)
    _same_handles(g, twin, "a rollout after the refusals")
    H._eq(_np(res["returns"]), ret, "returns after the refusals")
    assert (g.get(_lib.FLD_STEP_COUNT) == before["STEP_COUNT"] + 1 + steps).all()
    g.close(); twin.close()


# ---- 7. the adapters ------------------------------------------------------------------------------------------------------------------------
def test_adapters_with_navigate_step_through_step_nav():
    A, N = 2, 8
    g, twin = _pair(A, N, over=dict(max_step=6))
    with pytest.raises(ValueError):
        AgentVectorEnv(g, navigate=True)
    with pytest.raises(ValueError):
        MultiAgentVectorEnv(g, navigate=True)
    AgentVectorEnv(g)                                                         # the default asks for nothing
    _doorway_nav((g, twin), A, N)
    env = AgentVectorEnv(g, navigate=True)
    env.reset(); twin.reset()
    rs = np.random.RandomState(17)
    for t in range(8):                                                        # the episode ends at step 6: reset inside the call
        a = rs.uniform(-0.5, 0.5, (A, N)).astype(F)
        obs, rew, done, infos = env.step(a.reshape(A * N))
        ot, rt, dt, _ = twin.step_nav(a, with_obs=True, stats=True, autoreset=True)
        H._eq(_np(obs), _np(ot).reshape(A * N, 64), "AgentVectorEnv step %d: obs" % t)
        H._eq(_np(rew), _np(rt).reshape(A * N), "AgentVectorEnv step %d: rewards" % t)
        assert np.array_equal(_np(done), np.repeat(_np(dt) != 0, N)) and bool(_np(done).any()) == (t == 5)
    _same_handles(g, twin, "AgentVectorEnv")
    menv = MultiAgentVectorEnv(g, navigate=True)
    menv.vector_reset(); twin.reset()
    for t in range(3):
        a = rs.uniform(-0.5, 0.5, (A, N)).astype(F)
        ob, rb, db, _ = menv.vector_step([{"agent_%d" % i: a[e, i] for i in range(N)} for e in range(A)])
        ot, rt, dt, _ = twin.step_nav(a, with_obs=True, stats=True, autoreset=False)
        for e in range(A):
            assert len(ob[e]) >= 1
            for i in range(N):
                if "agent_%d" % i in ob[e]:                                   # (an agent reported done is left out from then on)
                    H._eq(ob[e]["agent_%d" % i], _np(ot)[e, i], "MultiAgentVectorEnv step %d: obs" % t)
                    assert rb[e]["agent_%d" % i] == float(_np(rt)[e, i])
            assert db[e]["__all__"] == bool(_np(dt)[e])
    _same_handles(g, twin, "MultiAgentVectorEnv")
    g.close(); twin.close()
