"""The policy kernels at the edges of fp32 and of their tiling (ca_policy_actions, ca_policy_evaluate, ca_rollout_policy_sample;
include/ca_env.h), bit for bit against the numpy restatement:
  * the scenes of tests/policy_edge_scenes.py -- subnormal operands and results, sums that overflow in the middle of a chain,
    cancelling products, constructed rounding ties, signed zeros, non-finite observations beside finite rows, every corner of the
    heads' epilogue -- written through ca_set(CA_FLD_OBS), through the kernel without heads and the kernel with them, noise off and
    on, both out modes.  tests/test_policy_edges_cpu.py shows that each scene reaches what it is named for;
  * a subnormal and a cancelling weight set beside an ordinary one through a sampling rollout of one step: the records of row 0;
  * shapes that reach tpa > 1 behind arena 0, tiles of 17, 8 and 1 rows, exactly full tiles, a single row, and the hidden widths 80,
    112-96, 128-128-128 and 16-16-16.
The header defines no payload or sign for a NaN, so the scenes in which the definition gives one are compared by _nan_eq: the same
places are NaN and every other element has the same bits.  Everything else is helpers._eq."""
import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from tests import helpers as H
from tests import policy_edge_scenes as E
from tests import policy_scenes as PS
from tests import ppo_scenes as PP
from tests import test_gpu_policy as TP
from tests import test_gpu_ppo as TQ

pytestmark = pytest.mark.gpu
f32 = np.float32
_np, OUTS = TP._np, TQ.OUTS


def _nan_eq(got, want, what):
    """the same elements are NaN; every other element has the same bits"""
    got, want = np.ascontiguousarray(_np(got)), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == f32, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN at %s on the card, at %s by the definition" % (what, np.argwhere(gn)[:8].tolist(), np.argwhere(wn)[:8].tolist())
    H._eq(np.where(gn, f32(0.0), got), np.where(wn, f32(0.0), want), what)


def _handle(A, N, seed=1):
    return H.make_gpu(A, N, "crowd", H.scenario_params("crowd", N), seed=seed)


def _compare(g, sc, eq, what, modes):
    """policy_actions() and policy_actions(noise) on the policy alone, then policy_evaluate() and policy_evaluate(eps), all five
    outputs, and policy_actions again with the heads installed; per out mode.  Returns what the card gave under the first mode."""
    Ws, bs = E.restated(sc)
    value, log_std = sc.heads
    first = None
    for out, limit in modes:
        got = {}
        g.set_policy(sc.layers, sets=sc.sets, out=out, limit=limit)
        for nz, tag in ((None, "no noise"), (sc.eps, "noise")):
            with np.errstate(all="ignore"):
                want = PS.actions_reference(sc.obs, Ws, bs, sc.sets, nz, out, limit)
            got["actions, " + tag] = _np(g.policy_actions(nz)).copy()
            eq(got["actions, " + tag], want, "%s: policy_actions, out=%s, %s" % (what, out, tag))
        g.set_policy_heads(value=value, log_std=log_std)
        for nz, tag in ((None, "no eps"), (sc.eps, "eps")):
            with np.errstate(all="ignore"):
                want = PP.evaluate_reference(sc.obs, Ws, bs, sc.sets, value, log_std, nz, out, limit)
            ev = g.policy_evaluate(nz)
            for n in OUTS:
                got["%s, %s" % (n, tag)] = _np(ev[n]).copy()
                eq(got["%s, %s" % (n, tag)], want[n], "%s: policy_evaluate %s, out=%s, %s" % (what, n, out, tag))
        eq(_np(g.policy_actions(sc.eps)), got["actions, noise"], "%s: policy_actions with the heads installed, out=%s" % (what, out))
        first = first or got
    return first


def _run_scene(name, modes=(("identity", np.pi),), obs=None):
    sc, reach = E.SCENES[name][0]()
    if obs is not None:
        sc = sc._replace(obs=obs)
    A, N = sc.obs.shape[:2]
    assert A <= 3 and N <= 40
    g = _handle(A, N)
    g.set(_lib.FLD_OBS, sc.obs)
    H._eq(g.get(_lib.FLD_OBS), sc.obs, name + ": the observation as written")
    got = _compare(g, sc, _nan_eq if E.SCENES[name][1] else H._eq, name, modes)
    g.close()
    return sc, reach, got


def test_subnormal_operands_and_results():
    _run_scene("subnormal", (("identity", np.pi), ("clip", 1e-39)))


def test_sums_that_overflow_in_the_middle_of_a_chain():
    _run_scene("overflow", (("identity", np.pi), ("clip", 3e38)))


def test_cancelling_products():
    _run_scene("cancellation")


def test_rounding_ties():
    _run_scene("ties")


def test_signed_zeros():
    _run_scene("zeros", (("identity", np.pi), ("clip", 0.05)))


def test_non_finite_rows_leave_their_neighbours_alone():
    sc, reach, got = _run_scene("isolation", (("identity", np.pi), ("clip", 0.5)))
    clean = E.isolation_scene(clean=True)[0]
    _, _, base = _run_scene("isolation", obs=clean.obs)
    keep = ~reach["poisoned"]
    assert keep.sum() == keep.size - len(E.POISON)
    for n in got:
        assert np.isfinite(got[n][keep]).all(), n
        H._eq(got[n][keep], base[n][keep], "the rows beside the poisoned ones against the card's own result without them: " + n)


def test_heads_epilogue_corners():
    sc, reach = E.SCENES["epilogue"][0]()
    _run_scene("epilogue", (("identity", np.pi), ("clip", reach["limit"])))


@pytest.mark.parametrize("name", ["subnormal", "cancellation"])
def test_edge_weight_sets_through_a_sampling_rollout(name):
    """the scene's weight set in arena 0 and an ordinary one in arena 1, one step of a doorway: the records of row 0 are the
    restatement's on the recorded observation"""
    sc, _ = E.SCENES[name][0]()
    layers, (value, log_std) = E.ordinary_set_beside(sc)
    A, N = 2, 10
    sets = np.asarray([0, 1], np.int32)
    g = H.make_gpu(A, N, "doorway", H.scenario_params("doorway", N), seed=3)
    act = np.random.RandomState(1).uniform(-np.pi, np.pi, (5, A, N)).astype(f32)
    for t in range(5):                                          # (the observation of a fresh handle is all zeros)
        g.step(act[t])
    g.set_policy(layers, sets=sets)
    g.set_policy_heads(value=value, log_std=log_std)
    eps = np.random.RandomState(4).standard_normal((1, A, N)).astype(f32)
    res = g.rollout_policy_sample(1, hold=1, noise=eps, record=("obs", "actions", "logp", "dist", "values"))
    res = {n: (None if v is None else _np(v)) for n, v in res.items()}
    obs = res["obs"][0]
    assert obs.shape == (A, N, 64) and np.abs(obs).max() > 0
    want = PP.evaluate_reference(obs, [W for W, _ in layers], [b for _, b in layers], sets, value, log_std, eps[0])
    H._eq(res["actions"][0], want["actions"], name + ": the action record")
    H._eq(res["logp"][0], want["logp"], name + ": the logp record")
    H._eq(res["dist"][0], np.stack([want["mean"], want["log_std"]]), name + ": the dist record")
    H._eq(res["values"][0], want["value"], name + ": the value record")
    if name == "subnormal":
        assert E.is_subnormal(want["mean"][0]).any() or E.is_subnormal(want["value"][0]).any(), (want["mean"][0], want["value"][0])
    else:
        assert (np.abs(want["mean"][0]) > 0).any()
    g.close()


# ---- the tiling -------------------------------------------------------------------------------------------------------------------------------
def _tiling_case(g, hidden, P, sets, what, seed):
    """random-normal observations through ca_set; policy_actions and policy_evaluate with both heads.  Returns the card's means."""
    A, N = g.A, g.N
    rs = np.random.RandomState(seed)
    obs = rs.standard_normal((A, N, 64)).astype(f32)
    g.set(_lib.FLD_OBS, obs)
    layers = TP._layers(hidden, P, seed=seed + 1)
    value, log_std = TQ._heads(hidden[-1], P, seed=seed + 2)
    sc = E.Scene([(W if W.ndim == 3 else W[None], b if b.ndim == 2 else b[None]) for W, b in layers], sets, obs, (value, log_std),
                 rs.standard_normal((A, N)).astype(f32))
    got = _compare(g, sc, H._eq, what, (("identity", np.pi),))
    return got["mean, no eps"]


@pytest.mark.parametrize("hidden", [(64, 64), (80,), (112, 96), (128, 128, 128), (16, 16, 16)], ids=lambda h: "-".join(map(str, h)))
def test_two_tiles_per_arena_behind_arena_zero(hidden):
    """3 x 40, two sets, sets [1, 0, 1]: tpa = 2, tiles of 32 and 8 rows, arenas 1 and 2 behind blockIdx.x / tpa.  Against a run with
    sets [0, 0, 0]: arenas 0 and 2 change and arena 1 does not -- the set is the arena's, not the tile's."""
    g = _handle(3, 40)
    what = "3 x 40, %s" % (hidden,)
    mean = _tiling_case(g, hidden, 2, np.asarray([1, 0, 1], np.int32), what, seed=len(hidden))
    base = _tiling_case(g, hidden, 2, np.asarray([0, 0, 0], np.int32), what + ", sets [0, 0, 0]", seed=len(hidden))
    H._eq(mean[1], base[1], what + ": arena 1 plays set 0 in both runs")
    assert (mean[0] != base[0]).all() and (mean[2] != base[2]).all(), what
    g.close()


@pytest.mark.parametrize("A,N,P,sets,why", [(1, 49, 2, [1], "a last tile of 17 rows"), (3, 11, None, None, "33 consecutive rows: a last tile of one row"),
                                            (2, 32, 2, [0, 1], "exactly full tiles")], ids=["1x49", "3x11", "2x32"])
def test_ragged_and_full_tiles(A, N, P, sets, why):
    g = _handle(A, N)
    _tiling_case(g, (64, 64), P, None if sets is None else np.asarray(sets, np.int32), "%d x %d, %s" % (A, N, why), seed=A + N)
    g.close()


def test_a_single_row():
    """one arena of one agent, the smallest handle the library creates"""
    g = H.make_gpu(1, 1, None, dict(scenarios.env_params(), max_step=0), polys=[[(0.0, 0.0), (0.0, 10.0), (10.0, 10.0), (10.0, 0.0)]])
    _tiling_case(g, (64, 64), None, None, "1 x 1", seed=11)
    g.close()
