"""Recording rollouts on the GPU (ca_rollout_trace / ca_alan_rollout_trace, include/ca_env.h): record r is what ca_get reads after
(r + 1) * every steps.  Every comparison is bit exact, against a twin handle advanced one orca_step / alan_step at a time and read
with get(), and against the CPU oracle.  The shapes are the smallest at which each mechanism can go wrong: a record index carried
over the 256-step launch boundary, arenas that share a wave, N that is no power of two, arenas that freeze or respawn inside a
launch, and one handle for every form in which a rollout is a sequence of launches per step (the record kernel)."""
import ctypes as C

import numpy as np
import pytest

from collision_avoidance_amd import _lib, alan, scenarios
from oracle import oracle as o
from tests import agent_count_scenes as CS
from tests import helpers as H
from tests import wide_worlds as W

pytestmark = pytest.mark.gpu

PLANES = ("POS_X", "POS_Y", "VEL_X", "VEL_Y")
WORDS = ("STEP_COUNT", "ARENA_DONE", "EPISODE")
STATE = PLANES + ("PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "AGENT_DONE", "ARRIVE_STEP", "REGOAL_COUNT", "NB_COUNT", "NB_IDX",
                  "OBST_COUNT", "OBST_IDX") + WORDS


def _snapshot(env, fld):
    """(planes [4, A, N] f32, words [3, A] i32) of a GPU handle (fld = _lib) or an oracle (fld = o), as get() reads them now"""
    return (np.stack([env.get(getattr(fld, "FLD_" + n)) for n in PLANES]),
            np.stack([env.get(getattr(fld, "FLD_" + n)) for n in WORDS]))


def _records(step, env, fld, steps, every, at=None):
    """step() `steps` times, a snapshot after every `every`-th; at: only the records r with at(r) (the others are None)"""
    out = []
    for s in range(1, steps + 1):
        step()
        if s % every == 0:
            r = s // every - 1
            out.append(_snapshot(env, fld) if at is None or at(r) else None)
    return out


def _host(trace):
    return trace["agents"].cpu().numpy(), (trace["arenas"].cpu().numpy() if trace["arenas"] is not None else None)


def _assert_records(trace, want, what, planes=(0, 1, 2, 3)):
    """the traced tensors against a list of snapshots (None entries are not compared)"""
    ag, ar = _host(trace)
    assert ag.shape[0] == len(want) and ag.shape[1] == len(planes), (what, ag.shape, len(want))
    for r, w in enumerate(want):
        if w is None:
            continue
        H._eq(ag[r], w[0][list(planes)], "%s: record %d, planes" % (what, r))
        if ar is not None:
            H._eq(ar[r], w[1], "%s: record %d, arena words" % (what, r))


def _assert_same_handles(a, b, what, fields=STATE):
    for n in fields:
        f = getattr(_lib, "FLD_" + n)
        H._eq(a.get(f), b.get(f), "%s: %s" % (what, n))
    sa, sb = a.stats(), b.stats()
    assert sa == sb, (what, sa, sb)
    assert np.array_equal(a.get(_lib.FLD_ARENA_STATS), b.get(_lib.FLD_ARENA_STATS)), what + ": per-arena counters"


def _is_one_launch(g):
    li = g.launch_info()
    assert li["rollout_one_launch"] == 1, li


# ---- the four-lanes kernel: records stored from registers inside the T-step launch ---------------------------------------------
def test_quad_records_continue_across_launches(monkeypatch):
    """300 steps are two launches (256 + 44) and 7 does not divide 256: record 36 is the first of the second launch, 4 steps in."""
    monkeypatch.setenv("CA_QUAD", "1")
    A, N, steps, every = 37, 16, 300, 7
    p = H.scenario_params("crowd", N, neighbor_dist=1.5, max_neighbors=5)
    traced, twin, plain = (H.make_gpu(A, N, "crowd", p, seed=11) for _ in range(3))
    orc = H.make_oracle(A, N, "crowd", p, seed=11)
    _is_one_launch(traced)
    tr = traced.rollout(steps, stats=True, trace=dict(every=every))
    assert tuple(tr["agents"].shape) == (42, 4, A, N) and tuple(tr["arenas"].shape) == (42, 3, A)
    _assert_records(tr, _records(lambda: twin.orca_step(stats=True), twin, _lib, steps, every), "twin")
    _assert_records(tr, _records(lambda: orc.orca_step(flags=o.F_STATS), orc, o, steps, every, at=lambda r: r % 10 == 0 or r == 41),
                    "oracle")
    plain.rollout(steps, stats=True)
    _assert_same_handles(traced, plain, "traced rollout against the same rollout without a trace")
    _assert_same_handles(traced, twin, "traced rollout against single steps", fields=PLANES + WORDS + ("PREF_X", "PREF_Y", "AGENT_DONE"))
    H.assert_state_equal(traced, orc, "final state")
    H.assert_stats_equal(traced, orc, "final stats")
    for e in (traced, twin, plain):
        e.close()


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("scenario,A,N", [("circle", 5, 12), ("doorway", 40, 10), ("crowd", 70, 1)],
                         ids=["circle5x12", "doorway40x10", "crowd70x1"])
def test_quad_arena_layouts(monkeypatch, scenario, A, N, every):
    """N no power of two with several arenas per wave; the dense 10-lane arenas of the doorway; one agent per arena."""
    monkeypatch.setenv("CA_QUAD", "1")
    p = H.scenario_params(scenario, N)
    traced, twin = (H.make_gpu(A, N, scenario, p, seed=4) for _ in range(2))
    orc = H.make_oracle(A, N, scenario, p, seed=4)
    _is_one_launch(traced)
    tr = traced.rollout(40, trace=dict(every=every))
    _assert_records(tr, _records(twin.orca_step, twin, _lib, 40, every), "twin")
    _assert_records(tr, _records(orc.orca_step, orc, o, 40, every), "oracle")
    H.assert_state_equal(traced, orc, "final state")
    traced.close(); twin.close()


def test_channels_and_no_record(monkeypatch):
    """POS alone, VEL alone and both: C = 2, 2, 4 and the planes in the stated order; every > steps touches no byte of the buffers."""
    import torch
    monkeypatch.setenv("CA_QUAD", "1")
    A, N = 6, 12
    p = H.scenario_params("crowd", N)
    twin = H.make_gpu(A, N, "crowd", p, seed=6)
    want = _records(twin.orca_step, twin, _lib, 12, 2)
    for channels, planes in ((("pos",), (0, 1)), (("vel",), (2, 3)), (("pos", "vel"), (0, 1, 2, 3)), (("vel", "pos"), (0, 1, 2, 3))):
        g = H.make_gpu(A, N, "crowd", p, seed=6)
        tr = g.rollout(12, trace=dict(every=2, channels=channels))
        assert tuple(tr["agents"].shape) == (6, len(planes), A, N)
        _assert_records(tr, want, "channels %s" % (channels,), planes=planes)
        g.close()
    g = H.make_gpu(A, N, "crowd", p, seed=6)
    ag = torch.full((2, 4, A, N), -7.5, dtype=torch.float32, device="cuda")
    ar = torch.full((2, 3, A), -7, dtype=torch.int32, device="cuda")
    t = _lib.Trace(agents=ag.data_ptr(), agents_bytes=ag.numel() * 4, arenas=ar.data_ptr(), arenas_bytes=ar.numel() * 4, every=13,
                   channels=3)
    g._call("ca_rollout_trace", g.h, 12, 0, C.byref(t))       # R = 0
    g.sync()
    assert (ag == -7.5).all().item() and (ar == -7).all().item()
    _assert_same_handles(g, twin, "12 unrecorded steps", fields=PLANES + WORDS)
    out = g.rollout(5, trace=dict(every=9, arenas=False))      # the front end: empty tensors, the steps advanced all the same
    assert tuple(out["agents"].shape) == (0, 4, A, N) and out["arenas"] is None
    assert (g.get(_lib.FLD_STEP_COUNT) == 17).all()
    g.close(); twin.close()


def test_frozen_arenas_repeat_their_final_state(monkeypatch):
    monkeypatch.setenv("CA_QUAD", "1")
    A, N, steps, every = 10, 12, 1200, 50
    p = H.scenario_params("circle", N)
    p.update(max_step=3000)
    traced, twin = (H.make_gpu(A, N, "circle", p, seed=2) for _ in range(2))
    orc = H.make_oracle(A, N, "circle", p, seed=2)
    px, py = traced.get(0), traced.get(1)      # the head starts of test_quad_freeze_rollout_equals_single_steps_and_oracle
    px[1::2] *= 1.0 + 0.01 * np.arange(px[1::2].shape[0])[:, None]
    for e in (traced, twin):
        e.set(0, px); e.set(1, py)
    orc.set(o.FLD_POS_X, px); orc.set(o.FLD_POS_Y, py)
    _is_one_launch(traced)
    tr = traced.rollout(steps, stats=True, freeze=True, trace=dict(every=every))
    want = _records(lambda: orc.orca_step(flags=o.F_STATS | o.F_FREEZE), orc, o, steps, every)
    _assert_records(tr, want, "oracle")
    _assert_records(tr, _records(lambda: twin.orca_step(stats=True, freeze=True), twin, _lib, steps, every), "twin")
    ag, ar = _host(tr)
    ended = np.flatnonzero(ar[-1, 1])                                       # the arenas whose episode ended within the rollout
    first = {a: int(np.argmax(ar[:, 1, a])) for a in ended}                 # ... and the record in which arena_done flips
    assert len(ended) >= 3 and len(set(ar[-1, 0, ended].tolist())) > 1 and len(set(first.values())) > 1, (ended, first)
    for a in ended:
        assert first[a] == int(np.argmax([w[1][1, a] for w in want])) and not ar[:first[a], 1, a].any()
        assert (first[a] * every if first[a] else 0) < ar[first[a], 0, a] <= (first[a] + 1) * every
        for r in range(first[a] + 1, ag.shape[0]):
            H._eq(ag[r, :, a], ag[first[a], :, a], "arena %d: record %d repeats the final state" % (a, r))
            H._eq(ar[r, :, a], ar[first[a], :, a], "arena %d: record %d repeats the final words" % (a, r))
    H.assert_stats_equal(traced, orc, "freeze")
    traced.close(); twin.close()


def test_autoreset_records_the_respawn(monkeypatch):
    monkeypatch.setenv("CA_QUAD", "1")
    A, N, steps = 12, 16, 130
    p = scenarios.bench_params(N, 3.0, 5)
    p.update(max_step=40, done_mode=1)
    traced, twin = (H.make_gpu(A, N, "crowd", p, seed=5) for _ in range(2))
    orc = H.make_oracle(A, N, "crowd", p, seed=5)
    _is_one_launch(traced)
    tr = traced.rollout(steps, stats=True, autoreset=True, trace=dict(every=1))
    want = _records(lambda: orc.orca_step(flags=o.F_STATS | o.F_AUTORESET), orc, o, steps, 1)
    _assert_records(tr, want, "oracle")
    _assert_records(tr, _records(lambda: twin.orca_step(stats=True, autoreset=True), twin, _lib, steps, 1), "twin")
    ag, ar = _host(tr)
    assert (ar[-1, 2] >= 3).all(), ar[-1, 2]                          # at least three episodes ended in every arena (the cap: 40 steps)
    for a in range(A):
        ends = np.flatnonzero(np.diff(ar[:, 2, a])) + 1               # the records taken at the steps that ended an episode
        assert len(ends) == ar[-1, 2, a] >= 3
        for r in ends:
            assert ar[r, 0, a] == 0 and ar[r, 2, a] == ar[r - 1, 2, a] + 1 and ar[r - 1, 0, a] > 0
            H._eq(ag[r, :2, a], want[r][0][:2, a], "arena %d: record %d holds the respawn the oracle draws" % (a, r))
    H.assert_stats_equal(traced, orc, "autoreset")
    traced.close(); twin.close()


# ---- ALAN ------------------------------------------------------------------------------------------------------------------------
def _alan_equal(g, e, fg, fe, what):
    for n in ("ALAN_WEIGHTS", "ALAN_TIMES"):
        gw, ew = g.get(getattr(fg, "FLD_" + n)), e.get(getattr(fe, "FLD_" + n))
        assert gw.shape == ew.shape and np.array_equal(gw.view(np.uint64), ew.view(np.uint64)), "%s: %s" % (what, n)
    H._eq(g.get(fg.FLD_ALAN_ACTION), e.get(fe.FLD_ALAN_ACTION), what + ": action")
    H._eq(g.get(fg.FLD_REWARD), e.get(fe.FLD_REWARD), what + ": reward")


def test_fused_alan_rollout_records(monkeypatch):
    """The bandit inside the four-lanes launch (test_gpu_alan.py's fused configuration, the eight default actions, the handle's own
    draws, CA_F_FREEZE): 300 steps = two launches, every = 7."""
    monkeypatch.setenv("CA_QUAD", "1")
    A, N, steps, every = 40, 12, 300, 7
    p = H.scenario_params("circle", N, max_step=90)
    traced, twin, plain = (H.make_gpu(A, N, "circle", p, seed=8) for _ in range(3))
    orc = H.make_oracle(A, N, "circle", p, seed=8)
    sc = (np.arange(A) % 31).astype(np.int32)                          # the arenas end at different steps
    for e in (traced, twin, plain):
        e.alan_configure(alan.DEFAULT_ACTIONS)
        e.set(_lib.FLD_STEP_COUNT, sc)
    orc.alan_configure(alan.DEFAULT_ACTIONS); orc.set(o.FLD_STEP_COUNT, sc)
    _is_one_launch(traced)
    tr = traced.alan_rollout(steps, stats=True, freeze=True, trace=dict(every=every))
    assert tuple(tr["agents"].shape) == (42, 4, A, N)
    _assert_records(tr, _records(lambda: twin.alan_step(stats=True, freeze=True), twin, _lib, steps, every), "twin")
    _assert_records(tr, _records(lambda: orc.alan_step(flags=o.F_STATS | o.F_FREEZE), orc, o, steps, every), "oracle")
    plain.alan_rollout(steps, stats=True, freeze=True)
    _assert_same_handles(traced, plain, "traced ALAN rollout against the same without a trace", fields=STATE + ("REWARD", "ALAN_ACTION"))
    _alan_equal(traced, plain, _lib, _lib, "without a trace")
    _alan_equal(traced, twin, _lib, _lib, "twin")
    _alan_equal(traced, orc, _lib, o, "oracle")
    H.assert_state_equal(traced, orc, "final state", reward=True)
    H.assert_stats_equal(traced, orc, "ALAN")
    ar = _host(tr)[1]
    first = np.argmax(ar[:, 1], axis=0)                                  # the record in which an arena's arena_done flips
    assert ar[-1, 1].all() and len(set(first.tolist())) > 3 and (ar[-1, 0] == 90).all(), (first, ar[-1, 0])
    for e in (traced, twin, plain):
        e.close()


def test_lone_last_step_behind_a_full_launch(monkeypatch):
    """257 = 256 + 1 steps: the second launch is a single step, which is a step and not a rollout -- the handle's step launch, with the
    record kernel behind it.  every = 1: record 256 is that step's; every = 257: it is the only record.  The ORCA-only rollout and the
    fused ALAN rollout (the handle's own draws) on a handle whose single step is the four-lanes kernel, with and without a trace,
    against a twin's 257 single steps.  (A handle with a one-launch rollout whose single step is another kernel exists at exactly 1024
    lane-waves only -- thousands of arenas: that branch of the lone step is not reached here.)"""
    monkeypatch.setenv("CA_QUAD", "1")
    A, N, steps = 3, 12, 257
    p = H.scenario_params("circle", N)
    moved = PLANES + WORDS + ("PREF_X", "PREF_Y", "AGENT_DONE")
    for bandit in (False, True):
        what = "ALAN" if bandit else "ORCA"

        def make():
            g = H.make_gpu(A, N, "circle", p, seed=5)
            if bandit:
                g.alan_configure(alan.DEFAULT_ACTIONS)
            return g

        def roll(g, **kw):
            return g.alan_rollout(steps, freeze=True, **kw) if bandit else g.rollout(steps, **kw)
        twin = make()
        li = twin.launch_info()
        assert li["rollout_one_launch"] == 1 and li["lanes_per_agent"] == 4, li
        want = _records((lambda: twin.alan_step(freeze=True)) if bandit else twin.orca_step, twin, _lib, steps, 1)
        for every in (1, steps):
            traced = make()
            tr = roll(traced, trace=dict(every=every))
            assert tr["agents"].shape[0] == steps // every
            _assert_records(tr, want[every - 1::every], "%s, every=%d" % (what, every))
            _assert_same_handles(traced, twin, "%s, every=%d: the final state" % (what, every), fields=moved)
            traced.close()
        plain = make()
        roll(plain)
        _assert_same_handles(plain, twin, "%s without a trace: the final state" % what, fields=moved)
        if bandit:
            _alan_equal(plain, twin, _lib, _lib, "ALAN without a trace")
        plain.close(); twin.close()


def test_alan_rollout_records_with_an_action_set_per_arena(monkeypatch):
    """Two arenas whose action sets differ in size (the per-step form: select / solve / update or the fused single step, then the
    record kernel); each arena against an oracle of its own."""
    monkeypatch.setenv("CA_QUAD", "1")
    A, N, steps, every = 2, 12, 40, 3
    sets = [list(alan.DEFAULT_ACTIONS), list(alan.DEFAULT_ACTIONS[:3])]
    p = H.scenario_params("circle", N)
    traced, twin = (H.make_gpu(A, N, "circle", p, seed=3) for _ in range(2))
    for e in (traced, twin):
        e.alan_configure_per_arena(sets)
    tr = traced.alan_rollout(steps, stats=True, freeze=True, trace=dict(every=every))
    _assert_records(tr, _records(lambda: twin.alan_step(stats=True, freeze=True), twin, _lib, steps, every), "twin")
    _alan_equal(traced, twin, _lib, _lib, "twin")
    ag, ar = _host(tr)
    for a in range(A):
        orc = H.make_oracle(1, N, "circle", p, seed=3, arena_offset=a)
        orc.alan_configure(sets[a])
        for r, w in enumerate(_records(lambda: orc.alan_step(flags=o.F_STATS | o.F_FREEZE), orc, o, steps, every)):
            H._eq(ag[r, :, a], w[0][:, 0], "arena %d record %d against its oracle" % (a, r))
            H._eq(ar[r, :, a], w[1][:, 0], "arena %d record %d words against its oracle" % (a, r))
        got = traced.get(_lib.FLD_ALAN_WEIGHTS)[a, :, :len(sets[a])]
        assert np.array_equal(got.view(np.uint64), orc.get(o.FLD_ALAN_WEIGHTS)[0].view(np.uint64)), "weights of arena %d" % a
    traced.close(); twin.close()


# ---- the record kernel: every form in which a rollout is a sequence of launches per step -----------------------------------------
def _per_step_case(traced, twin, orc, what, steps=20, every=3, one_launch=False, **roll):
    li = traced.launch_info()
    assert bool(li["rollout_one_launch"]) is one_launch, (what, li)
    traced.profile(1); traced.profile_read()
    tr = traced.rollout(steps, trace=dict(every=every), **roll)
    prof = traced.profile_read(); traced.profile(0)
    assert prof["reset_kernels"][0] == steps // every, (what, prof)          # one launch of the record kernel per record: kind 3
    _assert_records(tr, _records(lambda: twin.orca_step(**roll), twin, _lib, steps, every), what + ", twin")
    if orc is not None:
        flags = (o.F_OBS if roll.get("with_obs") else 0) | (o.F_STATS if roll.get("stats") else 0)
        _assert_records(tr, _records(lambda: orc.orca_step(flags=flags), orc, o, steps, every), what + ", oracle")
    return tr


def test_record_kernel_one_lane_per_agent(monkeypatch):
    monkeypatch.setenv("CA_QUAD", "0")
    A, N = 9, 64
    p = H.scenario_params("crowd", N, neighbor_dist=5.0, max_neighbors=10)
    traced, twin = (H.make_gpu(A, N, "crowd", p, seed=7) for _ in range(2))
    assert traced.launch_info()["lanes_per_agent"] == 1
    _per_step_case(traced, twin, H.make_oracle(A, N, "crowd", p, seed=7), "one lane per agent", stats=True)
    traced.close(); twin.close()


def test_record_kernel_behind_an_observation(monkeypatch):
    """CA_F_OBS takes the per-step form on a handle whose plain rollout is one launch"""
    monkeypatch.setenv("CA_QUAD", "1")
    A, N = 6, 12
    p = H.scenario_params("crowd", N)
    traced, twin = (H.make_gpu(A, N, "crowd", p, seed=6) for _ in range(2))
    orc = H.make_oracle(A, N, "crowd", p, seed=6)
    _per_step_case(traced, twin, orc, "with the observation", one_launch=True, with_obs=True)
    H._eq(traced.get(_lib.FLD_OBS), orc.get(o.FLD_OBS), "the observation of the last step")
    traced.close(); twin.close()


def test_record_kernel_two_lanes_per_agent():
    A, N = 2, 200
    p = H.scenario_params("crowd", N)
    traced, twin = (H.make_gpu(A, N, "crowd", p, seed=1) for _ in range(2))
    assert traced.launch_info()["lanes_per_agent"] == 2
    _per_step_case(traced, twin, H.make_oracle(A, N, "crowd", p, seed=1), "pair kernel", stats=True)
    traced.close(); twin.close()


def test_record_kernel_per_agent_parameters():
    """Mixed radii inside every arena.  (The oracle has no per-agent form: the twin's single steps are the reference here; they are
    pinned to the simulator by tests/test_gpu_agent_params.py.)"""
    A, N = 4, 20
    p = H.scenario_params("crowd", N)
    radius = np.random.RandomState(3).uniform(0.3, 0.6, (A, N)).astype(np.float32)
    traced, twin = (H.make_gpu(A, N, "crowd", p, seed=9, agent_params=dict(radius=radius)) for _ in range(2))
    assert traced.launch_info()["agent_params"]
    _per_step_case(traced, twin, None, "per-agent parameters", stats=True)
    traced.close(); twin.close()


def test_record_kernel_per_arena_counts():
    """counts [20, 7, 1, 13] of 20 rows: the records' absent rows hold what the test wrote into them"""
    N, counts = 20, (20, 7, 1, 13)
    A = len(counts)
    p, polys, sc = CS.doorway_scene(A, N, 33, max_step=50)
    decoys = CS.with_decoys(sc, counts)
    traced, twin = (H.make_gpu(A, N, None, p, seed=33, polys=polys, max_obst_neighbors=16) for _ in range(2))
    for e in (traced, twin):
        e.set_agent_counts(np.asarray(counts, np.int32))
        CS.set_state(e, _lib, decoys)
    assert traced.launch_info()["agent_counts"]
    rag = CS.RaggedOracleVec(N, counts, p, polys, 33, S_cap=traced.S)
    rag.set_scene(sc)
    tr = _per_step_case(traced, twin, None, "per-arena counts", stats=True)
    ag, ar = _host(tr)
    absent = ~traced.agent_mask()
    wrote = np.stack([decoys["pos"][..., 0], decoys["pos"][..., 1], decoys["vel"][..., 0], decoys["vel"][..., 1]])
    for r in range(ag.shape[0]):
        for _ in range(3):
            rag.orca_step(o.F_STATS)
        for a, (n, e) in enumerate(zip(counts, rag.orc)):
            got = _snapshot(e, o)
            H._eq(ag[r, :, a, :n], got[0][:, 0], "record %d arena %d against its oracle" % (r, a))
            H._eq(ar[r, :, a], got[1][:, 0], "record %d arena %d words against its oracle" % (r, a))
        H._eq(ag[r][:, absent], wrote[:, absent], "record %d: absent rows" % r)
    traced.close(); twin.close()


def test_record_kernel_wide_obstacle_lists():
    worlds = W.ragged_squares_worlds(10)
    traced, orc = W.make_pair(4, 10, worlds, 64)
    twin, _ = W.make_pair(4, 10, worlds, 64)
    assert traced.launch_info()["lanes_per_agent"] == 1 and traced.S == 64
    _per_step_case(traced, twin, orc, "wide lists", stats=True)
    traced.close(); twin.close()


@pytest.mark.parametrize("A,N,tiled", [(1, 1100, True), (2, 300, True), (1, 1100, "grid")], ids=["1x1100", "2x300", "grid1x1100"])
def test_record_kernel_tiled(A, N, tiled):
    """nine tiles, the last partial; two arenas of three tiles; the grid's six launches per step -- the record kernel behind the
    close launch"""
    p = H.scenario_params("crowd", N)
    traced, twin = (H.make_gpu(A, N, "crowd", p, seed=21, tiled=tiled) for _ in range(2))
    assert traced.tiled_info()["tiled"] and traced.tiled_info()["launches_per_step"] == (6 if tiled == "grid" else 3)
    _per_step_case(traced, twin, H.make_oracle(A, N, "crowd", p, seed=21), "tiled %s" % (tiled,), stats=True)
    traced.close(); twin.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_advance_nothing(monkeypatch):
    import torch
    monkeypatch.setenv("CA_QUAD", "1")
    A, N, steps = 6, 12, 10
    p = H.scenario_params("crowd", N)
    g = H.make_gpu(A, N, "crowd", p, seed=6)
    orc = H.make_oracle(A, N, "crowd", p, seed=6)
    g.alan_configure(alan.DEFAULT_ACTIONS)
    ag = torch.zeros((steps, 4, A, N), dtype=torch.float32, device="cuda")
    ar = torch.zeros((steps, 3, A), dtype=torch.int32, device="cuda")
    full = dict(agents=ag.data_ptr(), agents_bytes=ag.numel() * 4, arenas=ar.data_ptr(), arenas_bytes=ar.numel() * 4, every=1, channels=3)
    need_ag, need_ar = steps * 4 * A * N * 4, steps * 3 * A * 4
    cases = [(None, _lib_code("EINVAL"), "null"),
             (dict(full, agents=None), _lib_code("EINVAL"), "null"),
             (dict(full, every=0), _lib_code("EINVAL"), "every"),
             (dict(full, every=-1), _lib_code("EINVAL"), "every"),
             (dict(full, channels=0), _lib_code("EINVAL"), "channels"),
             (dict(full, channels=4), _lib_code("EINVAL"), "channels"),
             (dict(full, channels=7), _lib_code("EINVAL"), "channels"),
             (dict(full, agents_bytes=need_ag - 4), _lib_code("ESIZE"), str(need_ag)),
             (dict(full, arenas_bytes=need_ar - 4), _lib_code("ESIZE"), str(need_ar))]
    for name in ("ca_rollout_trace", "ca_alan_rollout_trace"):
        for kw, code, word in cases:
            t = _lib.Trace(**kw) if kw is not None else None
            rc = getattr(g.L, name)(g.h, steps, 0, C.byref(t) if t is not None else None)
            assert rc == code, (name, kw, rc)
            assert word in g.L.ca_last_error(g.h).decode(), (name, kw, g.L.ca_last_error(g.h))
            assert not g.get(_lib.FLD_STEP_COUNT).any(), (name, kw)
    assert not ag.any().item() and not ar.any().item()
    tr = g.rollout(steps, trace=dict(every=1))                      # the handle steps correctly afterwards
    _assert_records(tr, _records(orc.orca_step, orc, o, steps, 1), "after the refusals")
    H.assert_state_equal(g, orc, "after the refusals")
    g.close()


def _lib_code(name):
    return {"EINVAL": -1, "ESIZE": -4}[name]


# ---- run_sim(trace_every=) -------------------------------------------------------------------------------------------------------
def test_run_sim_keeps_a_trajectory():
    sim = alan.Collision_Avoidance_Sim(numAgents=8, scenario="circle", seed=2)
    twin = alan.Collision_Avoidance_Sim(numAgents=8, scenario="circle", seed=2)
    ok, total, _, _ = sim.run_sim(1, trace_every=10)
    last = sim.step_count
    assert ok and 10 <= last < sim.max_step and total == last * sim.timeStep
    assert sim.trajectory.shape == (last // 10, 8, 2) and sim.trajectory.dtype == np.float32
    assert sim.trajectory_records.tolist() == [last // 10]
    at = {}
    for s in range(1, last + 1):
        twin.vec.alan_step(freeze=True)
        if s % 10 == 0:
            at[s] = np.stack([twin.vec.get(_lib.FLD_POS_X)[0], twin.vec.get(_lib.FLD_POS_Y)[0]], -1)
    H._eq(sim.trajectory[-1], at[(last // 10) * 10], "the last record: at or before the arrival step")
    H._eq(sim.trajectory[2], at[30], "the record of step 30")
    assert twin.vec.get(_lib.FLD_ARENA_DONE).all() and int(twin.vec.get(_lib.FLD_STEP_COUNT)[0]) == last
    with pytest.raises(ValueError):
        sim.run_sim(1, trace_every=0)
    with pytest.raises(ValueError):
        sim.run_sim(1, trace_every=sim.POLL + 1)
