"""The definition of the navigated action step (ca_nav_act / ca_nav_step, include/ca_env.h), restated in numpy for the tests.  Built on
tests/nav_scenes.py -- its grid, its fields and the pointer walk of S.nav_pref -- and on the oracle's sincos64 / pref_dir64.  No device
and no library: tests/test_nav_step_cpu.py pins it to the oracle's reference-pinned step, tests/test_gpu_nav_step.py compares the
kernels with it bit for bit.

fp64 where the definition is fp64 (Python floats: one rounding per operation, never contracted), numpy float32 where it is fp32."""
import numpy as np

from tests import nav_scenes as S

F = np.float32


def nav_target(g, fields, k, lookahead, px, py, s=0):
    """the walk of S.nav_pref for one navigated row of class k: (the cell centre reached as (x, y) float32, or None when the walk never
    moved or ended on STAY -- the agent's own goal then --, the distance to go at the start cell)"""
    dist, nxt, _ = fields[s][k]
    cxs, cys = g.centres()
    cx, cy = g.cell_of(px, py)
    wx, wy, moved, p = int(cx), int(cy), False, S.NONE
    for _ in range(lookahead):
        p = int(nxt[wy, wx])
        if p >= 8:
            break
        wx, wy, moved = wx + S.OFFSETS[p][0], wy + S.OFFSETS[p][1], True
    d = dist[int(cy), int(cx)]
    if not moved or p == S.STAY:
        return None, d
    return (cxs[wx], cys[wy]), d


def action_pref(px, py, tx, ty, action):
    """csrc/ca_rules.h action_pref: pref_dir64, sincos64((double)action), the fp64 rotation; (dir, rot) rounded to fp32"""
    from oracle import oracle as o
    pf_x, pf_y = o.pref_dir64(F(px), F(py), float(tx), float(ty))
    sn, cs = o.sincos64(float(F(action)))
    rl_x = pf_x * cs - pf_y * sn
    rl_y = pf_x * sn + pf_y * cs
    return (F(pf_x), F(pf_y)), (F(rl_x), F(rl_y))


def nav_act(g, fields, cls, lookahead, pos_x, pos_y, goal_x, goal_y, agent_done, actions, steered, set_of_arena=None):
    """One ca_nav_act call.  cls int [A, N] (fields may be None when every class is -1); steered bool [A, N]: present and not frozen
    (the caller's).  Returns dict(dir_x, dir_y, rot_x, rot_y float32 [A, N], dist float32 [A, N], navigated bool [A, N] -- the rows
    whose dist is written); only the steered rows of the first four mean anything."""
    A, N = np.shape(pos_x)
    out = {k: np.zeros((A, N), F) for k in ("dir_x", "dir_y", "rot_x", "rot_y", "dist")}
    out["navigated"] = np.zeros((A, N), bool)
    n_goals = 0 if fields is None else len(fields[0])
    for a in range(A):
        s = 0 if set_of_arena is None else set_of_arena[a]
        for i in range(N):
            if not steered[a, i]:
                continue
            px, py = F(pos_x[a, i]), F(pos_y[a, i])
            tx, ty = float(goal_x[a, i]), float(goal_y[a, i])
            k = int(cls[a, i])
            if 0 <= k < n_goals and agent_done[a, i] == 0:
                t, d = nav_target(g, fields, k, lookahead, px, py, s)
                out["dist"][a, i], out["navigated"][a, i] = d, True
                if t is not None:
                    tx, ty = float(t[0]), float(t[1])
            (dx, dy), (rx, ry) = action_pref(px, py, tx, ty, actions[a, i])
            out["dir_x"][a, i], out["dir_y"][a, i], out["rot_x"][a, i], out["rot_y"][a, i] = dx, dy, rx, ry
    return out


def step_reward(reward_scale, vel_x, vel_y, dir_x, dir_y, rot_x, rot_y):
    """csrc/ca_rules.h step_reward in numpy float32: every product and sum rounded once"""
    vx, vy = np.asarray(vel_x, F), np.asarray(vel_y, F)
    scale = F(reward_scale)
    r_goal = (vx * np.asarray(dir_x, F)).astype(F) + (vy * np.asarray(dir_y, F)).astype(F)
    r_polite = (vx * np.asarray(rot_x, F)).astype(F) + (vy * np.asarray(rot_y, F)).astype(F)
    return ((scale * r_goal).astype(F) + ((F(1.0) - scale).astype(F) * r_polite).astype(F)).astype(F)


def cpu_nav_step(e, actions, g=None, fields=None, cls=None, lookahead=1, counts=None, freeze=False, flags=0, reward=None):
    """ca_nav_step on the CPU oracle `e`: restated nav_act -> set(PREF_X / PREF_Y) -> orca_step -> restated reward.  The oracle's
    REWARD field cannot be set, so the loop's reward field is the caller's: reward [A, N] (None: zeros) is what the field held, and
    the returned dict -- nav_act's -- carries reward [A, N], what it holds now (rows that were not steered keep theirs), and steered."""
    from oracle import oracle as o
    A, N = e.A, e.N
    cls = np.full((A, N), -1, np.int32) if cls is None else cls
    present = np.arange(N)[None, :] < (np.full(A, N) if counts is None else np.asarray(counts))[:, None]
    steered = present & ~((e.get(o.FLD_ARENA_DONE) != 0) & bool(freeze))[:, None]
    act = nav_act(g, fields, cls, lookahead, e.get(o.FLD_POS_X), e.get(o.FLD_POS_Y), e.get(o.FLD_GOAL_X), e.get(o.FLD_GOAL_Y),
                  e.get(o.FLD_AGENT_DONE), np.asarray(actions, F).reshape(A, N), steered)
    px, py = e.get(o.FLD_PREF_X), e.get(o.FLD_PREF_Y)
    px[steered], py[steered] = act["rot_x"][steered], act["rot_y"][steered]
    e.set(o.FLD_PREF_X, px); e.set(o.FLD_PREF_Y, py)
    e.orca_step(flags=flags | (o.F_FREEZE if freeze else 0))
    r = step_reward(e.cfg.reward_scale, e.get(o.FLD_VEL_X), e.get(o.FLD_VEL_Y), act["dir_x"], act["dir_y"], act["rot_x"], act["rot_y"])
    act["reward"] = np.where(steered, r, np.zeros((A, N), F) if reward is None else np.asarray(reward, F)).astype(F)
    act["steered"] = steered
    return act


def trap_oracle(A, n=8):
    """the trap of tests/nav_scenes.py on a fresh oracle environment, and its one field"""
    from oracle import oracle as o
    e = o.OracleEnv(o.make_config(n_arenas=A, n_agents=n, seed=0, **S.trap_params()))
    e.set_obstacles(S.trap_world())
    e.init_scenario(o.SCN_DOORWAY)
    S.trap_setup(e, o, A, n)
    g = S.Grid(**S.TRAP_GRID)
    fields = S.all_fields([S.edges_of_table(e.obstacle_table(cap=256))], g, S.TRAP_CLEARANCE, [S.TRAP_TARGET])
    return e, g, fields


def trap_cpu_nav_run(A, steps, actions, every=None, n=8, straight=False):
    """the CPU loop on the trap under actions [steps, A, n] (or None: zeros).  Returns dict(done, obst_collisions, records [(pos_x, pos_y,
    vel_x, vel_y, reward)] after every `every`-th step, sum_nav: the sum of the restated rewards, sum_straight (straight=True): the sum
    of the reward the same trajectory earns towards the agents' own goals, fields)."""
    from oracle import oracle as o
    e, g, fields = trap_oracle(A, n)
    cls, records = np.zeros((A, n), np.int32), []
    sum_nav = sum_straight = 0.0
    rew = np.zeros((A, n), F)
    zeros = np.zeros((A, n), F)
    for s in range(steps):
        a = zeros if actions is None else actions[s]
        if straight:
            own = nav_act(None, None, np.full((A, n), -1, np.int32), 1, e.get(o.FLD_POS_X), e.get(o.FLD_POS_Y), e.get(o.FLD_GOAL_X),
                          e.get(o.FLD_GOAL_Y), e.get(o.FLD_AGENT_DONE), a, np.ones((A, n), bool))
        rew = cpu_nav_step(e, a, g, fields, cls, S.TRAP_LOOKAHEAD, flags=o.F_STATS, reward=rew)["reward"]
        sum_nav += float(rew.astype(np.float64).sum())
        if straight:
            sum_straight += float(step_reward(e.cfg.reward_scale, e.get(o.FLD_VEL_X), e.get(o.FLD_VEL_Y), own["dir_x"], own["dir_y"],
                                              own["rot_x"], own["rot_y"]).astype(np.float64).sum())
        if every and (s + 1) % every == 0:
            records.append(tuple(e.get(f) for f in (o.FLD_POS_X, o.FLD_POS_Y, o.FLD_VEL_X, o.FLD_VEL_Y)) + (rew.copy(),))
    return dict(done=e.get(o.FLD_AGENT_DONE), obst_collisions=e.stats()["obst_collisions"], records=records, sum_nav=sum_nav,
                sum_straight=sum_straight, fields=fields)
