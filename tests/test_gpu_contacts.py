"""The per-agent contact report on the GPU (ca_contacts / CA_F_CONTACT, include/ca_env.h; csrc/ca_contact.h): all five planes bit for
bit against the numpy fp32 restatement of tests/contact_scenes.py, which tests/test_contacts_cpu.py ties to the CPU oracle's
per-arena totals.  Hand-made states go in through set(); the shapes are the smallest at which each path of the kernel can go wrong:
arenas packed into a workgroup with the last one partly filled, one arena per workgroup exactly (256), an arena over two workgroups
with one agent in the second (257), 1024, and every kind of handle."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from oracle import oracle as o
from tests import contact_scenes as CS
from tests import helpers as H

pytestmark = pytest.mark.gpu

BS = 256   # csrc/ca_contact.h CONTACT_BS
R = 0.5
DOORWAY = scenarios.obstacles("doorway", 10, R)
STATE = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "AGENT_DONE", "ARRIVE_STEP", "REGOAL_COUNT",
         "NB_COUNT", "NB_IDX", "OBST_COUNT", "OBST_IDX", "STEP_COUNT", "ARENA_DONE", "EPISODE", "REWARD", "OBS", "ARENA_STATS")


def _params(**over):
    p = scenarios.env_params()
    p.update(over)
    return p


def _handle(A, N, polys, **kw):
    return H.make_gpu(A, N, None, kw.pop("params", _params()), seed=kw.pop("seed", 5), polys=polys, **kw)


def _place(g, px, py):
    g.set(_lib.FLD_POS_X, px)
    g.set(_lib.FLD_POS_Y, py)


def _want(g, radius=R, counts=None):
    """the restatement of the handle's own positions and tables"""
    return CS.reference(g.get(_lib.FLD_POS_X), g.get(_lib.FLD_POS_Y), radius, CS.tables_of(g, g.A), counts)


def _report_of(g, px, py, what, radius=R, counts=None):
    _place(g, px, py)
    got = g.contacts()
    CS.assert_report(got, _want(g, radius, counts), what)
    return got


# ---- hand-made states --------------------------------------------------------------------------------------------------------
def test_boundary_pairs_and_coincident_agents():
    px, py = CS.boundary_pairs(R)
    g = _handle(1, px.shape[1], [])
    r = _report_of(g, px, py, "boundary pairs")
    assert r["agents"][0].tolist() == [0, 0, 1, 1, 0, 0, 2, 2, 2]       # d2 == sqr(cr): no; one ulp inside: yes; one ulp outside: no
    assert r["nearest"][0, 6:].tolist() == [7, 6, 6] and (r["nearest_d2"][0, 6:] == 0).all()   # coincident: both others counted
    assert (r["wall"] == 0).all() and np.isinf(r["wall_d2"]).all()      # a world without obstacles: 0, +inf
    g.close()


def test_nearest_tie_mixed_radii_and_a_lone_agent():
    px, py, rad = CS.nearest_cases()
    g = _handle(1, px.shape[1], [])
    g.set_agent_params(radius=rad)
    r = _report_of(g, px, py, "nearest", radius=rad)
    assert r["nearest"][0, 0] == 1                                      # agents 1 and 2 at the same d2: the smaller index
    assert r["nearest"][0, 3] == 4 and r["agents"][0].tolist() == [0, 0, 0, 1, 0, 1]   # 3 touches 5 (large), its nearest is 4
    g.clear_agent_params()                                              # back to ca_config.radius: 0.2 + 1.9 no longer applies
    r = _report_of(g, px, py, "nearest, uniform radius again")
    assert r["agents"][0].tolist() == [0] * 6
    g.close()
    one = _handle(3, 1, CS.WALL)
    r = _report_of(one, np.float32([[1.0], [2.0], [1.5]]), np.float32([[2.0], [0.25], [-9.0]]), "N = 1")
    assert (r["nearest"] == -1).all() and np.isinf(r["nearest_d2"]).all() and (r["agents"] == 0).all()
    assert r["wall"][:, 0].tolist() == [0, 1, 0]
    one.close()


def test_walls_one_ulp_inside_and_outside():
    px, py = CS.wall_cases(R)
    g = _handle(1, px.shape[1], CS.WALL)
    r = _report_of(g, px, py, "walls")
    assert r["wall"][0].tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0]         # at R | one ulp inside | one ulp outside, three places each
    assert r["wall_d2"][0, 0] == np.float32(0.25)
    g.close()


def test_per_arena_tables_of_different_sizes():
    worlds = [CS.WALL, [CS.WALL[0]], DOORWAY, [DOORWAY[1], DOORWAY[2]]]
    g = _handle(4, 12, dict(per_arena=worlds))
    sizes = [len(CS.table_edges(g.obstacle_table(a))) for a in range(4)]
    assert len(set(sizes)) == 4, sizes
    px, py = CS.random_state(4, 12, 21)
    r = _report_of(g, px, py, "a table per arena")
    assert r["wall"][2].sum() > 0 or r["wall"][3].sum() > 0
    g.close()


# ---- shapes and kinds of handle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N,kw", [
    (7, 10, {}), (27, 10, {}), (3, 64, {}), (1, BS, {}), (2, BS + 1, {}), (1, 1024, {}),
    (2, 1500, dict(tiled=True)),
    (1, 1500, dict(tiled="grid", edge_grid=True)),
    (1, 300, dict(tiled=True, tiled_params=True)),
    (1, 300, dict(tiled="grid", tiled_params=True)),
    (1, 300, dict(tiled=True, tiled_wide=True, max_obst_neighbors=40)),
    (1, 300, dict(tiled="grid", tiled_wide=True, max_obst_neighbors=40)),
    (2, 40, dict(max_obst_neighbors=40)),
], ids=["7x10", "27x10", "3x64", "1x256", "2x257", "1x1024", "tiled2x1500", "grid1x1500-edge-grid", "tiled-params300",
        "grid-params300", "tiled-wide300", "grid-wide300", "wide2x40"])
def test_shapes_and_handles(A, N, kw):
    g = _handle(A, N, DOORWAY, **kw)
    px, py = CS.random_state(A, N, 100 + N)
    rad = R
    if kw.get("tiled_params"):
        rad = np.random.RandomState(N).uniform(0.2, 0.8, (A, N)).astype(np.float32)
        g.set_agent_params(radius=rad)
    g.profile(1)
    g.profile_read()
    r = _report_of(g, px, py, "%d x %d %r" % (A, N, kw), radius=rad)
    prof = g.profile_read()
    print("%d x %d %r: %d touches, %d wall touches, kind-3 launches %d, mean %.4f ms" % (A, N, kw, int(r["agents"].sum()), int(r["wall"].sum()),
                                                                                prof["reset_kernels"][0], prof["reset_kernels"][1]))
    assert prof["reset_kernels"][0] == 1, prof
    assert r["agents"].sum() > 0 and r["wall"].sum() > 0 and (r["nearest_d2"][:, [0, N - 1]] == 0).all()
    if kw.get("tiled"):
        assert g.tiled_info()["tiled"]
    g.close()


def test_agent_counts_absent_rows_on_top_of_present_agents():
    counts = np.int32([1, 4, 10, 7, 2, 10, 9])
    A, N = len(counts), 10
    g = _handle(A, N, DOORWAY)
    g.set_agent_counts(counts)
    px, py = CS.random_state(A, N, 8)
    for a, n in enumerate(counts):
        px[a, n:], py[a, n:] = px[a, 0], py[a, 0]                       # absent rows sit on agent 0
    r = _report_of(g, px, py, "counts", counts=counts)
    absent = np.arange(N)[None, :] >= counts[:, None]
    assert (r["agents"][absent] == 0).all() and (r["wall"][absent] == 0).all() and (r["nearest"][absent] == -1).all()
    assert np.isinf(r["nearest_d2"][absent]).all() and np.isinf(r["wall_d2"][absent]).all()
    assert r["nearest"][0, 0] == -1 and r["agents"][0, 0] == 0          # the arena of one: its absent rows are nobody
    assert (r["nearest"][~absent] < np.broadcast_to(counts[:, None], (A, N))[~absent]).all()
    rad = np.random.RandomState(2).uniform(0.2, 0.9, (A, N)).astype(np.float32)
    g.set_agent_params(radius=rad)                                       # counts and radii together
    _report_of(g, px, py, "counts with radii", radius=rad, counts=counts)
    g.close()


def test_torch_views_of_the_device_buffer():
    torch = pytest.importorskip("torch")
    A, N = 5, 12
    g = _handle(A, N, DOORWAY, use_torch=True)
    px, py = CS.random_state(A, N, 3)
    _place(g, px, py)
    r = g.contacts()
    assert all(isinstance(r[k], torch.Tensor) and r[k].is_cuda and tuple(r[k].shape) == (A, N) for k in CS.PLANES)
    assert r["agents"].dtype == torch.int32 and r["nearest"].dtype == torch.int32 and r["wall_d2"].dtype == torch.float32
    g.sync()
    CS.assert_report(r, _want(g), "torch views")
    assert r["wall"].data_ptr() - r["agents"].data_ptr() == A * N * 4   # planes of the one [5, A, N] buffer
    _place(g, py, px)
    g.contacts()                                                         # the same views, rewritten in place
    g.sync()
    CS.assert_report(r, _want(g), "torch views after the next report")
    g.close()


# ---- the flag ----------------------------------------------------------------------------------------------------------------
def test_flag_on_the_doorway_run_equals_restatement_and_oracle_totals():
    A, N = 3, 64
    p = H.scenario_params("doorway", N)
    g = H.make_gpu(A, N, "doorway", p, seed=3)
    orc = H.make_oracle(A, N, "doorway", p, seed=3)
    tabs = CS.tables_of(g, A)
    prev = orc.get(o.FLD_ARENA_STATS).copy()
    touches = walls = 0
    for s, act in CS.doorway_actions(A, N, 3, 30):
        _, _, _, info = g.step(act, with_obs=False, stats=True, contacts=True)
        orc.step(act, flags=o.F_STATS)
        rep = info["contacts"]
        CS.assert_report(rep, CS.reference(g.get(_lib.FLD_POS_X), g.get(_lib.FLD_POS_Y), p["radius"], tabs), "step %d" % s)
        st = orc.get(o.FLD_ARENA_STATS).copy()
        np.testing.assert_array_equal(rep["agents"].sum(1), 2 * (st[:, 1] - prev[:, 1]).astype(np.int64), "step %d: pairs" % s)
        np.testing.assert_array_equal(rep["wall"].sum(1), (st[:, 2] - prev[:, 2]).astype(np.int64), "step %d: walls" % s)
        prev = st
        touches += int(rep["agents"].sum()); walls += int(rep["wall"].sum())
    print("doorway %d x %d on the device: %d touches, %d wall touches" % (A, N, touches, walls))
    assert touches >= 1000 and walls >= 100, (touches, walls)
    H.assert_stats_equal(g, orc, "doorway run")
    g.close()


def test_flag_on_the_other_calls():
    A, N = 6, 12
    p = H.scenario_params("crowd", N)
    g = H.make_gpu(A, N, "crowd", p, seed=9)
    rad = p["radius"]
    g.orca_step(contacts=True)
    CS.assert_report(g.last_contacts(), _want(g, rad), "orca_step")
    g.alan_configure([(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.7, -0.7)])
    g.alan_step(contacts=True)
    CS.assert_report(g.last_contacts(), _want(g, rad), "alan_step")
    g.alan_rollout(5, contacts=True)
    CS.assert_report(g.last_contacts(), _want(g, rad), "alan_rollout")
    before = g.last_contacts()
    g.orca_step()                                                        # no flag: the report stays the last one computed
    CS.assert_report(g.last_contacts(), before, "a step without the flag")
    g.reset(contacts=True)
    CS.assert_report(g.last_contacts(), _want(g, rad), "reset")
    mask = np.int32([1, 0, 0, 1, 0, 1])
    g.orca_step()
    g.reset_masked(mask, contacts=True)
    CS.assert_report(g.last_contacts(), _want(g, rad), "reset_masked")
    px, py = CS.random_state(A, N, 4, centre=(0.0, 0.0))
    g.reset(px, py, contacts=True)
    CS.assert_report(g.last_contacts(), CS.reference(px, py, rad, CS.tables_of(g, A)), "reset to given positions")
    tr = g.rollout(6, contacts=True, trace=dict(every=2))
    assert tuple(tr["agents"].shape)[0] == 3
    CS.assert_report(g.last_contacts(), _want(g, rad), "rollout with a trace")
    g.close()


def test_autoreset_reports_the_respawned_state():
    A, N = 4, 6
    p = H.scenario_params("doorway", N, max_step=3)
    g = H.make_gpu(A, N, "doorway", p, seed=2)
    for s in range(3):
        _, _, done, info = g.step(np.zeros((A, N), np.float32), with_obs=False, stats=True, autoreset=True, contacts=True)
    assert (g.get(_lib.FLD_STEP_COUNT) == 0).all() and (g.get(_lib.FLD_EPISODE) == 1).all()   # the cap ended every episode inside the call
    CS.assert_report(info["contacts"], _want(g, p["radius"]), "after the reset inside the call")
    g.close()


def test_rollout_is_one_more_launch_behind_the_last_step(monkeypatch):
    monkeypatch.setenv("CA_QUAD", "1")
    A, N, T = 37, 16, 40
    p = H.scenario_params("crowd", N, neighbor_dist=1.5, max_neighbors=5)
    a, b = (H.make_gpu(A, N, "crowd", p, seed=11) for _ in range(2))
    assert a.launch_info()["rollout_one_launch"] == 1
    a.profile(1)
    a.profile_read()
    a.rollout(T, stats=True, contacts=True)
    prof = a.profile_read()
    assert prof["step_kernel"][0] == 1 and prof["reset_kernels"][0] == 1, prof   # one launch for the T steps, one for the report
    assert a.launch_info()["rollout_one_launch"] == 1
    b.rollout(T, stats=True)
    want = b.contacts()
    CS.assert_report(a.last_contacts(), want, "rollout(T, contacts=True) against rollout(T) + contacts()")
    CS.assert_report(want, _want(b, p["radius"]), "the restatement")
    for n in STATE:
        H._eq(a.get(getattr(_lib, "FLD_" + n)), b.get(getattr(_lib, "FLD_" + n)), "rollout: " + n)
    a.close(); b.close()


@pytest.mark.parametrize("kw", [{}, dict(tiled=True)], ids=["ordinary", "tiled"])
def test_purity_and_one_more_small_launch_per_step(kw):
    A, N, steps = 5, 20, 4
    p = H.scenario_params("doorway", N)
    a, b = (H.make_gpu(A, N, "doorway", p, seed=6, **kw) for _ in range(2))
    rng = np.random.RandomState(6)
    for e in (a, b):
        e.profile(1)
        e.profile_read()
    for s in range(steps):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        a.step(act, stats=True, contacts=True)
        b.step(act, stats=True)
    pa, pb = a.profile_read(), b.profile_read()
    assert pa["reset_kernels"][0] == pb["reset_kernels"][0] + steps, (pa, pb)    # exactly one more kind-3 launch per step
    assert pa["step_kernel"][0] == pb["step_kernel"][0] and pa["obs_kernel"][0] == pb["obs_kernel"][0], (pa, pb)
    for n in STATE:
        H._eq(a.get(getattr(_lib, "FLD_" + n)), b.get(getattr(_lib, "FLD_" + n)), "purity: " + n)
    assert a.stats() == b.stats()
    assert a.tiled_info() == b.tiled_info() and a.launch_info() == b.launch_info()
    a.close(); b.close()


def test_step_packed_output_is_byte_identical():
    A, N = 3, 10
    p = H.scenario_params("doorway", N)
    a, b = (H.make_gpu(A, N, "doorway", p, seed=1) for _ in range(2))
    rng = np.random.RandomState(1)
    for s in range(3):
        act = rng.uniform(-1, 1, (A, N)).astype(np.float32)
        a.step_packed(act, stats=True, contacts=True)
        b.step_packed(act, stats=True)
        assert a._packed[0].tobytes() == b._packed[0].tobytes(), s
    CS.assert_report(a.last_contacts(), _want(a, p["radius"]), "step_packed")
    from collision_avoidance_amd import envs
    env = envs.Collision_Avoidance_Env(numAgents=8, contacts=True)
    _, _, _, infos = env.step({k: [0.3] for k in env._keys})
    want = _want(env.vec, env.radius)
    for i, k in enumerate(env._keys):
        assert infos[k] == dict(contact=bool(want["agents"][0, i] > 0 or want["wall"][0, i]), nearest_d2=float(want["nearest_d2"][0, i]))
    env.close(); a.close(); b.close()


def test_errors_leave_the_handle_working():
    A, N = 2, 9
    g = _handle(A, N, DOORWAY)
    L, vp = g.L, C.c_void_p
    buf = np.zeros((A, N), np.int32)
    ptr = buf.ctypes.data_as(vp)
    assert L.ca_get_contacts(g.h, ptr, None, None, None, None, buf.nbytes, 0) == -1          # CA_EINVAL: no report yet
    assert b"no contact report" in L.ca_last_error(g.h)
    with pytest.raises(RuntimeError):
        g.last_contacts()
    dev, nbytes = vp(), C.c_size_t()
    assert L.ca_contacts_ptr(g.h, C.byref(dev), C.byref(nbytes)) == 0 and dev.value and nbytes.value == 5 * A * N * 4
    assert L.ca_get_contacts(g.h, ptr, None, None, None, None, buf.nbytes, 0) == -1          # the buffer alone is no report
    px, py = CS.random_state(A, N, 1)
    _report_of(g, px, py, "after the refusals")
    assert L.ca_get_contacts(g.h, ptr, None, None, None, None, buf.nbytes - 4, 0) == -4      # CA_ESIZE
    assert L.ca_get_contacts(g.h, ptr, None, None, None, None, buf.nbytes, 0) == 0
    H._eq(buf, g.last_contacts()["agents"], "one plane alone")
    g.orca_step(contacts=True)
    CS.assert_report(g.last_contacts(), _want(g), "the handle works afterwards")
    g.close()
