"""The oracle against the golden vectors the reference's own Python produced
(tests/golden/make_golden.py).  This is what pins the env loop and the laser observation."""
import os

import numpy as np
import pytest

from collision_avoidance_amd import scenarios
from oracle import oracle as o


def test_line_intersection_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "utils_vectors.npz"))
    for row, ref in zip(g["li_in"], g["li_out"]):
        d, p = o.line_intersection(((row[0], row[1]), (row[2], row[3])), ((row[4], row[5]), (row[6], row[7])))
        if np.isinf(ref[0]):
            assert np.isinf(d) and p == (0.0, 0.0)
        else:
            assert d == ref[0] and p[0] == ref[1] and p[1] == ref[2]  # same fp64 expressions


def _comp_laser_f64(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name))
    for segs, n, orient, ref in zip(g["cl_segs"], g["cl_counts"], g["cl_orient"], g["cl_out"]):
        out = o.comp_laser(g["rays"], segs[:n], orient, np.float64)
        np.testing.assert_allclose(out, ref, rtol=0, atol=1e-12)


def test_comp_laser_f64_matches_reference(golden_dir):
    _comp_laser_f64(golden_dir, "utils_vectors.npz")


def test_comp_laser_f32_close_to_reference(golden_dir):
    _comp_laser_f32(golden_dir, "utils_vectors.npz")


def _comp_laser_f32(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name))
    bad = tot = 0
    for segs, n, orient, ref in zip(g["cl_segs"], g["cl_counts"], g["cl_orient"], g["cl_out"]):
        out = o.comp_laser(g["rays"], segs[:n], orient, np.float32)
        err = np.abs(out.astype(np.float64) - ref).max(axis=1)
        bad += int((err > 2e-5).sum())
        tot += err.size
    # a ray grazing a segment end can flip hit/miss under fp32 rounding; it must stay rare
    assert bad <= max(1, tot // 200), (bad, tot)


def test_ray_and_octagon_tables(golden_dir):
    g = np.load(os.path.join(golden_dir, "utils_vectors.npz"))
    np.testing.assert_array_equal(o.ray_table(1.5), g["rays"])
    oct_ = o.octagon_table(0.5)
    assert oct_.shape == (8, 4)
    np.testing.assert_allclose(np.hypot(oct_[:, 0], oct_[:, 1]), 0.5, atol=1e-15)
    np.testing.assert_array_equal(oct_[1:, :2], oct_[:-1, 2:])   # closed chain
    np.testing.assert_array_equal(oct_[-1, 2:], oct_[0, :2])


# ---- the same at the range the bench runs at: utils_vectors_k10.npz (ray table at 5.0, ten octagons + walls per case) ----
def test_comp_laser_k10_f64_matches_reference(golden_dir):
    _comp_laser_f64(golden_dir, "utils_vectors_k10.npz")


def test_comp_laser_k10_f32_close_to_reference(golden_dir):
    _comp_laser_f32(golden_dir, "utils_vectors_k10.npz")


def test_comp_laser_k10_cases_are_what_they_are_for(golden_dir):
    """60-84 segments per case (ten octagons + 0-4 walls); a neighbour nearer than the octagon's inradius (the ray origin
    inside it: every ray hits it from within); two octagons at the same distance along a ray; a wall through the origin,
    reported as a miss on the rays along it (utils.py:103) although an octagon lies behind."""
    g = np.load(os.path.join(golden_dir, "utils_vectors_k10.npz"), allow_pickle=False)
    cnt, segs, out = g["cl_counts"], g["cl_segs"], g["cl_out"]
    assert float(g["neighbor_dist"]) == 5.0 and cnt.min() >= 60 and cnt.max() == 84 and len(cnt) >= 30
    assert set((cnt - 80).tolist()) == {0, 1, 2, 3, 4}
    inradius = 0.5 * np.cos(np.pi / 8)
    inside = tied = through = blinded = 0
    for c, sg, ot in zip(cnt, segs, out):
        ctr = sg[:80, :2].reshape(10, 8, 2).mean(axis=1)            # the octagons' centres
        dist = np.hypot(ctr[:, 0], ctr[:, 1])
        walls_through = [w for w in sg[80:c] if w[0] * w[3] - w[1] * w[2] == 0.0 and w[0] * w[2] + w[1] * w[3] < 0]
        through += len(walls_through)                                # cross(a, b) = 0 exactly, a . b < 0
        if walls_through:
            blinded += int((ot == 0).all(axis=1).sum())              # rays that end at the origin: reported as a miss
        elif dist.min() < inradius - 0.01:
            hit = np.hypot(ot[:, 0], ot[:, 1])
            assert (hit > 0).all() and (hit <= dist.min() + 0.5 + 1e-12).all()      # every ray ends on an octagon it starts in
        inside += int(dist.min() < inradius - 0.01)
        d = np.linalg.norm(ctr[:, None] - ctr[None], axis=2) + np.eye(10) * 9
        tied += int(d.min() < 1e-12 or np.any(np.abs(d - 1.0) < 1e-12))
    assert inside >= 10 and tied >= 8 and through >= 6 and blinded >= 3 * through, (inside, tied, through, blinded)


def test_ray_table_at_the_headline_range(golden_dir):
    g = np.load(os.path.join(golden_dir, "utils_vectors_k10.npz"))
    np.testing.assert_array_equal(o.ray_table(5.0), g["rays"])
    np.testing.assert_allclose(np.hypot(g["rays"][:, 0], g["rays"][:, 1]), 5.0, atol=1e-15)


FLIP_MARGIN = 1e-5   # a ray may differ between fp32 and the reference's fp64 only if it is this close to flipping


def count_bad(err, tol, margins, key, env, prec, n):
    """Rays whose error exceeds `tol`.  In the fp64 replay the flip margin of every ray is recorded (oracle field
    OBS_MARGIN: distance of the nearest segment's (s, t) from the edge of the accepted square [0,1]^2 of utils.py:21-31,
    or the relative gap between the two nearest hits); in an fp32 replay every such ray must then be a flip at a
    segment end / ray tip or between two equidistant hits -- anything else is a real error and fails."""
    bad = err.reshape(n, 16, 4).max(axis=2) > tol
    if margins is not None:
        if prec == o.PREC_F64:
            margins[key] = env.get(o.FLD_OBS_MARGIN)[0].copy()
        elif bad.any():
            m = margins[key]
            assert (m[bad] < FLIP_MARGIN).all(), "%s: rays %s differ by %s with flip margins %s" % (
                key, np.argwhere(bad).tolist(), err.reshape(n, 16, 4).max(axis=2)[bad], m[bad])
    return int(bad.sum())


def _replay(golden_dir, name, prec, margins=None):
    g = np.load(os.path.join(golden_dir, name))
    n = int(g["n_agents"])
    at = {}                                   # the range the run was recorded at (default: the env's own 1.5 / 5)
    if "neighbor_dist" in g.files:
        at = dict(neighbor_dist=float(g["neighbor_dist"]), max_neighbors=int(g["max_neighbors"]))
    cfg = o.make_config(n_arenas=1, n_agents=n, max_obst_neighbors=16, **at)
    env = o.OracleEnv(cfg)
    env.set_obstacles(scenarios.obstacles("doorway", n))
    env.set(o.FLD_POS_X, g["pos0"][:, 0]); env.set(o.FLD_POS_Y, g["pos0"][:, 1])
    env.set(o.FLD_VEL_X, g["vel0"][:, 0]); env.set(o.FLD_VEL_Y, g["vel0"][:, 1])
    env.set(o.FLD_PREF_X, g["pref0"][:, 0]); env.set(o.FLD_PREF_Y, g["pref0"][:, 1])
    env.set(o.FLD_GOAL_X, g["tgt0"][:, 0]); env.set(o.FLD_GOAL_Y, g["tgt0"][:, 1])
    env.set(o.FLD_GOAL2_X, np.full(n, -10.0)); env.set(o.FLD_GOAL2_Y, np.full(n, 5.0))
    obs_at = {int(s): k for k, s in enumerate(g["obs_steps"])}
    reset_at = {int(s): k for k, s in enumerate(g["reset_steps"])}
    obs_fld = o.FLD_OBS64 if prec == o.PREC_F64 else o.FLD_OBS
    rew_fld = o.FLD_REWARD64 if prec == o.PREC_F64 else o.FLD_REWARD
    tol = 1e-11 if prec == o.PREC_F64 else 3e-5
    obs_bad = obs_tot = 0
    if margins is not None and prec == o.PREC_F64:
        margins.clear()
    for s in range(len(g["kind"])):
        if s in reset_at:
            k = reset_at[s]
            env.reset(g["reset_pos"][k][:, 0], g["reset_pos"][k][:, 1], flags=o.F_OBS, prec=prec)
            err = np.abs(env.get(obs_fld)[0].astype(np.float64) - g["reset_obs"][k])
            obs_bad += count_bad(err, tol, margins, ("reset", k), env, prec, n); obs_tot += n * 16
        if g["kind"][s] == 1:
            env.orca_step(flags=o.F_OBS | o.F_NODONE, prec=prec)
        else:
            env.step(g["actions"][s], flags=o.F_OBS, prec=prec)
            np.testing.assert_allclose(env.get(rew_fld)[0], g["reward"][s], rtol=0,
                                       atol=1e-12 if prec == o.PREC_F64 else 1e-6, err_msg="reward step %d" % s)
            assert bool(env.get(o.FLD_ARENA_DONE)[0]) == bool(g["done_all"][s])
        st = env.state()
        # simulator state is fp32 on both sides and the ORCA underneath is the same code: exact
        np.testing.assert_array_equal(st["pos_x"][0], g["pos"][s][:, 0], err_msg="pos step %d" % s)
        np.testing.assert_array_equal(st["pos_y"][0], g["pos"][s][:, 1])
        np.testing.assert_array_equal(st["vel_x"][0], g["vel"][s][:, 0])
        np.testing.assert_array_equal(st["vel_y"][0], g["vel"][s][:, 1])
        np.testing.assert_array_equal(st["pref_x"][0], g["pref"][s][:, 0], err_msg="pref step %d" % s)
        np.testing.assert_array_equal(st["pref_y"][0], g["pref"][s][:, 1])
        np.testing.assert_array_equal(st["agent_done"][0], g["agents_done"][s])
        np.testing.assert_array_equal(st["goal_x"][0], g["tgt"][s][:, 0])
        np.testing.assert_array_equal(st["goal_y"][0], g["tgt"][s][:, 1])
        if "step_count" in g.files:          # the episode fixtures of round 5: the counter and its cap, step by step
            assert int(env.get(o.FLD_STEP_COUNT)[0]) == int(g["step_count"][s]), s
        if "nb_count" in g.files:            # the lists the reference's _get_obs walked (env.py:246-250, 283, 305)
            np.testing.assert_array_equal(env.get(o.FLD_NB_COUNT)[0], g["nb_count"][s], err_msg="nb_count step %d" % s)
            np.testing.assert_array_equal(env.get(o.FLD_OBST_COUNT)[0], g["obst_count"][s], err_msg="obst_count step %d" % s)
        if s in obs_at:
            err = np.abs(env.get(obs_fld)[0].astype(np.float64) - g["obs"][obs_at[s]])
            obs_bad += count_bad(err, tol, margins, ("step", s), env, prec, n); obs_tot += n * 16
    assert int(env.get(o.FLD_STEP_COUNT)[0]) == int(g["step_count_final"])
    return obs_bad, obs_tot


ENV_FIXTURES = ["env_doorway_n10.npz", "env_doorway_n6_dense.npz", "env_doorway_n6_episode.npz", "env_doorway_n4_all_done.npz"]


def test_episode_fixtures_reach_the_end_of_an_episode(golden_dir):
    """What the round-5 fixtures are FOR (env.py:352-365, 404-414, 461-488): an agent arrives and is retargeted to
    (-10, 5); '__all__' comes true by the step cap with agents still on their way, and by the last arrival before
    the cap; reset() zeroes the counter and the flags and keeps the swapped targets."""
    g = np.load(os.path.join(golden_dir, "env_doorway_n6_episode.npz"))
    r = int(g["reset_steps"][0])
    assert g["agents_done"][:r].max() == 1 and g["agents_done"][r - 1].min() == 0          # some arrived, not all
    assert bool(g["done_all"][r - 1]) and not g["done_all"][:r - 1].any() and int(g["step_count"][r - 1]) == 1000   # the cap
    arrived = g["agents_done"][r - 1] == 1
    assert (g["tgt"][r - 1][arrived] == (-10.0, 5.0)).all() and (g["tgt"][r - 1][~arrived] == (1.0, 5.0)).all()
    assert int(g["step_count"][r]) == 1 and (g["tgt"][r][arrived] == (-10.0, 5.0)).all()    # reset keeps the swapped targets
    assert len(g["kind"]) == r + 100 and not g["done_all"][r:].any()
    g = np.load(os.path.join(golden_dir, "env_doorway_n4_all_done.npz"))
    r = int(g["reset_steps"][0])
    assert g["agents_done"][r - 1].min() == 1 and bool(g["done_all"][r - 1]) and int(g["step_count"][r - 1]) < 1000
    assert (g["tgt"][r - 1] == (-10.0, 5.0)).all() and (g["tgt"][-1] == (-10.0, 5.0)).all()
    assert g["agents_done"][r].max() == 0                                                   # ... and clears the flags


@pytest.mark.parametrize("name", ENV_FIXTURES)
def test_env_loop_f64_matches_reference(golden_dir, name):
    bad, tot = _replay(golden_dir, name, o.PREC_F64)
    assert tot > 1000 and bad == 0, (bad, tot)


def flip_margins(golden_dir, name):
    """{("reset", k) | ("step", s): [n, 16] flip margins} from the fp64 replay of a golden run."""
    margins = {}
    bad, tot = _replay(golden_dir, name, o.PREC_F64, margins)
    assert bad == 0
    return margins


@pytest.mark.parametrize("name", ENV_FIXTURES)
def test_env_loop_f32_close_to_reference(golden_dir, name):
    """fp32 observation arithmetic against the reference's fp64: within 3e-5 except rays that graze a segment end
    (counted, bounded, and each one checked to BE such a ray)."""
    bad, tot = _replay(golden_dir, name, o.PREC_F32, flip_margins(golden_dir, name))
    assert bad <= max(2, tot // 500), (bad, tot)


# ---- the shape the bench times: 64 agents, neighborDist 5, maxNeighbors 10 (tests/golden/make_golden.py gen_headline) ----
HEADLINE = "env_n64_k10.npz"


def test_headline_fixture_is_what_it_is_for(golden_dir):
    """Conditions on the recording, not tolerances: it is there because no other fixture reaches this regime."""
    g = np.load(os.path.join(golden_dir, HEADLINE), allow_pickle=False)
    n = int(g["n_agents"])
    assert n == 64 and float(g["neighbor_dist"]) == 5.0 and int(g["max_neighbors"]) == 10
    steps = len(g["kind"])
    assert steps >= 240 and g["pos"].shape == g["vel"].shape == g["pref"].shape == (steps, n, 2)      # state at EVERY step
    snap = [int(s) for s in g["obs_steps"]]
    r = int(g["reset_steps"][0])
    assert len(snap) >= 24 and set(range(6)) <= set(snap) and {r - 1, r, r + 1, r + 2} <= set(snap)
    assert any(g["kind"][s] == 1 for s in snap) and len(g["reset_obs"]) == 1 and 0 < r < steps - 30
    nb, ob = g["nb_count"].astype(int), g["obst_count"].astype(int)
    assert (8 * nb + ob)[snap].max() >= 80                       # segments some agent's observation walks
    assert (nb == 10).mean() >= 0.9 and ob.max() <= 4            # full lists; the bench's template holds 4 obstacle neighbours
    d = np.linalg.norm(g["pos"][:, :, None].astype(np.float64) - g["pos"][:, None].astype(np.float64), axis=3)
    pairs = (d[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] < 1.0).sum(axis=1)
    assert pairs.max() >= 50, pairs.max()                        # overlapping pairs in one step
    rays = np.concatenate([g["obs"], g["reset_obs"]]).reshape(-1, 4)
    hit = (rays[:, 0] != 0) | (rays[:, 1] != 0)
    assert len(rays) >= 20000 and hit.mean() >= 0.8, (len(rays), hit.mean())
    assert np.hypot(rays[:, 0], rays[:, 1]).max() > 1.5          # ... and beyond the env's own 1.5 range
    assert not g["done_all"].any() and g["agents_done"].max() == 0


def test_headline_env_loop_f64_matches_reference(golden_dir):
    bad, tot = _replay(golden_dir, HEADLINE, o.PREC_F64)
    assert tot >= 20000 and bad == 0, (bad, tot)


def test_headline_env_loop_f32_close_to_reference(golden_dir):
    """The rules of test_env_loop_f32_close_to_reference at the bench's shape (observed: 0 of 25 600 rays beyond 3e-5)."""
    bad, tot = _replay(golden_dir, HEADLINE, o.PREC_F32, flip_margins(golden_dir, HEADLINE))
    assert bad <= max(2, tot // 500), (bad, tot)


def test_alan_scenarios_match_reference(golden_dir):
    """Start/goal layouts and obstacle polygons of every ALAN scenario against the reference's own
    generators (ALAN_true.py:175-457); random draws (crowd/congested positions, block obstacles) are
    checked for their boxes only."""
    g = np.load(os.path.join(golden_dir, "alan_scenarios.npz"))
    exact = (("circle", 8), ("circle", 100), ("incoming", 17), ("incoming", 26), ("blocks", 12),
             ("deadlock", 20), ("deadlock", 9))
    for scen, n in exact:
        key = "%s%d_" % (scen, n)
        p = scenarios.alan_params(n, scen)
        assert p["max_step"] == int(g[key + "max_step"])
        assert scenarios.envsize(scen, n) == float(g[key + "envsize"])
        env = o.OracleEnv(o.make_config(n_arenas=2, n_agents=n, **p))
        env.init_scenario(scenarios.SCENARIO_IDS[scen])
        for a in range(2):
            np.testing.assert_array_equal(env.get(o.FLD_POS_X)[a], g[key + "pos"][:, 0], err_msg=key)
            np.testing.assert_array_equal(env.get(o.FLD_POS_Y)[a], g[key + "pos"][:, 1], err_msg=key)
            for fx, fy, name in ((o.FLD_GOAL_X, o.FLD_GOAL_Y, "goal"), (o.FLD_GOAL2_X, o.FLD_GOAL2_Y, "goal2")):
                np.testing.assert_array_equal(env.get(fx)[a], g[key + name][:, 0], err_msg=key + name)   # fp64, exact
                np.testing.assert_array_equal(env.get(fy)[a], g[key + name][:, 1], err_msg=key + name)
        if scen != "blocks":
            polys = np.array(scenarios.obstacles(scen, n), np.float64).astype(np.float32)
            np.testing.assert_array_equal(polys, g[key + "obst"], err_msg=key + "obst")
    # random parts: same boxes as the reference's uniform() calls
    for scen, n in (("crowd", 16), ("congested", 24)):
        key = "%s%d_" % (scen, n)
        e = scenarios.envsize(scen, n)
        assert e == float(g[key + "envsize"])
        env = o.OracleEnv(o.make_config(n_arenas=3, n_agents=n, **scenarios.alan_params(n, scen)))
        env.init_scenario(scenarios.SCENARIO_IDS[scen])
        x, y = env.get(o.FLD_POS_X), env.get(o.FLD_POS_Y)
        x0 = 0.2 * e if scen == "congested" else 0.0
        assert x.min() >= x0 and x.max() <= e and y.min() >= 0 and y.max() <= e
        assert g[key + "pos"][:, 0].min() >= x0 - 1e-6
        np.testing.assert_array_equal(np.array(scenarios.obstacles(scen, n), np.float64).astype(np.float32), g[key + "obst"])
        if scen == "congested":
            np.testing.assert_array_equal(env.get(o.FLD_GOAL_X)[0], g[key + "goal"][:, 0])
            np.testing.assert_array_equal(env.get(o.FLD_GOAL2_X)[0], g[key + "goal2"][:, 0])
    blk = np.array(scenarios.obstacles("blocks", 12, seed=5), np.float64)
    e = scenarios.envsize("blocks", 12)
    np.testing.assert_array_equal(blk[0].astype(np.float32), g["blocks12_obst"][0])      # the border
    assert blk.shape == g["blocks12_obst"].shape and blk[1:].min() >= -e / 16 and blk[1:, :, 0].max() <= e
    np.testing.assert_allclose(blk[1:, 1, 0] - blk[1:, 0, 0], e / 8)                      # block size
