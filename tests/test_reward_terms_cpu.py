"""The reward terms without a device: (a) the numpy fp32 restatement that the GPU tests compare the kernel with
(tests/reward_scenes.py) against the unchanged CPU oracle's per-arena collision totals and against exact rationals; (b) the
device-free helper's refusals; (c) the header, the ctypes binding and the Python interface; (d) the compiled kernels' resources."""
import ctypes as C
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from collision_avoidance_amd import _lib, adapters, build as B, vec_env as VE
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
from oracle import oracle as o
from tests import contact_scenes as CS
from tests import helpers as H
from tests import reward_scenes as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ca_env.h")
F = np.float32


# ---- (a) the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N,min_touch,min_wall", [(3, 64, 1000, 100), (7, 10, 100, 100)], ids=["doorway3x64", "doorway7x10"])
def test_counts_sum_to_the_oracles_per_arena_totals(A, N, min_touch, min_wall):
    """Every step of 30, every arena: c1 sums to twice the pairs and c2 to the wall hits the oracle counted for that state; with
    margin = 0, c3 == c1 and c4 == c2; with a margin the comfort counts include the touching ones."""
    p = H.scenario_params("doorway", N)
    orc = H.make_oracle(A, N, "doorway", p, seed=3)
    tabs = CS.tables_of(orc, A)
    prev = orc.get(o.FLD_ARENA_STATS).copy()
    touches = walls = crowd = 0
    for s, act in CS.doorway_actions(A, N, 3, 30):
        orc.step(act, flags=o.F_STATS)
        px, py = orc.get(o.FLD_POS_X), orc.get(o.FLD_POS_Y)
        st = orc.get(o.FLD_ARENA_STATS).copy()
        g0 = RS.geometry_counts(px, py, p["radius"], tabs, 0.0)
        np.testing.assert_array_equal(g0["collision"].sum(1), 2 * (st[:, 1] - prev[:, 1]).astype(np.int64), "step %d: pairs" % s)
        np.testing.assert_array_equal(g0["wall"].sum(1), (st[:, 2] - prev[:, 2]).astype(np.int64), "step %d: walls" % s)
        np.testing.assert_array_equal(g0["near"], g0["collision"])
        np.testing.assert_array_equal(g0["wall_near"], g0["wall"])
        g3 = RS.geometry_counts(px, py, p["radius"], tabs, 0.3)
        np.testing.assert_array_equal(g3["collision"], g0["collision"])
        assert (g3["near"] >= g0["collision"]).all() and (g3["wall_near"] >= g0["wall"]).all()
        touches += int(g0["collision"].sum()); walls += int(g0["wall"].sum()); crowd += int((g3["near"] - g0["collision"]).sum())
        prev = st
    print("doorway %d x %d: %d touches, %d wall touches, %d more within the margin" % (A, N, touches, walls, crowd))
    assert touches >= min_touch and walls >= min_wall and crowd > 0, (touches, walls, crowd)


def test_comfort_distance_on_hand_made_states():
    R, m = 0.5, 0.3
    px, py = RS.boundary_pairs(R, m)
    g = RS.geometry_counts(px, py, R, np.zeros((0, 4), F), m)
    assert g["near"][0].tolist() == [0, 0, 1, 1, 0, 0, 2, 2, 2]          # at: no; one ulp inside: yes; outside: no; coincident
    assert g["collision"][0].tolist() == [0, 0, 0, 0, 0, 0, 2, 2, 2]
    assert (g["wall"] == 0).all() and (g["wall_near"] == 0).all()        # no edges: the smallest distance is +inf
    px, py = RS.wall_cases(R, m)
    tab = CS.table_edges(dict(verts=F([[0, 0], [4, 0], [10, 0], [10, 4]]), next=[1, 0, 3, 2]))
    g = RS.geometry_counts(px, py, R, tab, m)
    assert g["wall_near"][0].tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0] and (g["wall"] == 0).all()
    px, py, rad = CS.nearest_cases()
    g = RS.geometry_counts(px, py, rad, np.zeros((0, 4), F), 0.0)
    assert g["collision"][0].tolist() == [0, 0, 0, 1, 0, 1] and g["near"][0].tolist() == [0, 0, 0, 1, 0, 1]
    g = RS.geometry_counts(px, py, rad, np.zeros((0, 4), F), 1.2)        # 3 - 4: 1.5 < 0.4 + 1.2
    assert g["near"][0].tolist() == [2, 1, 1, 2, 1, 1]
    g = RS.geometry_counts(np.zeros((1, 4), F), np.zeros((1, 4), F), R, tab, m, counts=[2])   # absent rows are nobody
    assert g["collision"][0].tolist() == [1, 1, 0, 0] and g["near"][0].tolist() == [1, 1, 0, 0] and g["wall_near"][0].tolist() == [1, 1, 0, 0]


def test_sum_order_against_exact_rationals():
    """r = w0 * r_ref, then r + w_k * c_k for k ascending where w_k != 0: every operation rounded once, against fractions.Fraction."""
    rng = np.random.RandomState(7)
    cases = [
        (F(0.1), [3, 1, 5, 1, 1, 1], F([0.7, -0.25, -0.3, -0.05, -0.01, 10.0, -0.001])),
        (F(-0.0), [0, 0, 0, 0, 0, 1], F([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])),          # identity keeps -0.0
        (F(-0.0), [2, 1, 0, 0, 0, 1], F([2.5, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0])),         # a skipped zero weight; w2 * 1 = -1
        (F(-0.0), [0, 0, 0, 0, 0, 0], F([1.0, -3.0, 0.0, 0.0, 0.0, 0.0, 0.0])),         # -0.0 + (-3 * 0 = -0.0) stays -0.0
        (F(0.0), [0, 0, 0, 0, 0, 0], F([1.0, -3.0, 0.0, 0.0, 0.0, 0.0, 0.0])),          # +0.0 + -0.0 = +0.0
        (F(1e-3), [7, 0, 9, 1, 0, 1], F([1.0, -1e-4, 5.0, -3e-5, -0.7, 0.0, -1e-7])),
        (F(16777216.0), [1, 0, 0, 0, 0, 1], F([1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0])),   # 2^24 + 1 rounds to even twice: not 2^24 + 2
    ]
    for _ in range(40):
        w = rng.uniform(-2, 2, 7).astype(F)
        w[rng.randint(1, 7)] = 0.0
        cases.append((F(rng.uniform(-1, 1)), rng.randint(0, 12, 6).tolist(), w))
    for r_ref, c, w in cases:
        got = RS.weighted_sum(F([[r_ref]]), [np.int32([[v]]) for v in c], w[None, :])[0, 0]
        want = RS.exact_weighted_sum(r_ref, c, w)
        assert got.tobytes() == F(want).tobytes(), (r_ref, c, w, got, want)
    # the skipped weight is skipped, not added as +0.0: -0.0 survives a zero weight on a zero count and on a non-zero count
    assert np.signbit(RS.weighted_sum(F([[-0.0]]), [np.int32([[5]])] * 6, F([[1, 0, 0, 0, 0, 0, 0]]))[0, 0])
    assert RS.weighted_sum(F([[16777216.0]]), [np.int32([[1]])] * 6, F([[1, 1, 0, 0, 0, 0, 1]]))[0, 0] == F(16777216.0)


def test_shaped_reference_rows_and_masks():
    A, N = 3, 4
    px = F(np.arange(A * N).reshape(A, N) * 10.0); py = np.zeros((A, N), F)
    px[0, 1] = px[0, 0] + F(0.5)                                              # one touching pair in arena 0
    r_ref = F(np.linspace(-1, 1, A * N).reshape(A, N))
    w = F([[1, -1, 0, 0, 0, 2, -0.5], [1, 0, 0, 0, 0, 0, 0], [0.5, -1, 0, 0, 0, 0, 0]])
    arr = np.zeros((A, N), np.int32); arr[2, 3] = 1
    out = RS.shaped_reference(px, py, 0.5, np.zeros((0, 4), F), r_ref, w, 0.0, arr, np.ones((A, N), np.int32), counts=[4, 4, 3],
                              advanced=[True, True, True])
    assert out["collision"][0].tolist() == [1, 1, 0, 0] and (out["near"] == 0).all()      # w3 == 0 everywhere: the plane reads 0
    assert out["written"][2].tolist() == [True, True, True, False] and out["arrival"][2, 3] == 0   # an absent row is not written
    assert out["reward"][2, 3] == r_ref[2, 3]
    H._eq(out["reward"][1], r_ref[1], "identity arena")
    assert out["reward"][0, 0] == F(F(r_ref[0, 0] + F(-1.0)) + F(-0.5))
    frozen = RS.shaped_reference(px, py, 0.5, np.zeros((0, 4), F), r_ref, w, 0.0, arr, np.ones((A, N), np.int32), advanced=[False, True, True])
    H._eq(frozen["reward"][0], r_ref[0], "a frozen arena keeps its reward")
    resp = RS.shaped_reference(px, py, 0.5, np.zeros((0, 4), F), r_ref, w, 0.0, arr, np.ones((A, N), np.int32), respawned=[True, False, False])
    assert (resp["collision"][0] == 0).all() and resp["step"][0].tolist() == [1, 1, 1, 1]
    # arrival: modes 0 / 1, a respawned arena reads the last-episode word; CA_DONE_REGOAL follows regoal_count
    saved = np.int32([[0, 1, 0], [0, 0, 1]]); after = np.int32([[1, 1, 0], [0, 0, 0]])
    c5, c6 = RS.arrival_counts(False, saved, after)
    assert c5.tolist() == [[1, 0, 0], [0, 0, 0]] and c6.tolist() == [[1, 0, 1], [1, 1, 0]]
    c5, _ = RS.arrival_counts(False, saved, after, respawned=[False, True], lastep_arrived=[0, 3])
    assert c5.tolist() == [[1, 0, 0], [1, 1, 0]]
    c5, _ = RS.arrival_counts(False, saved, after, respawned=[False, True], lastep_arrived=[0, 2])   # the cap ended it: nobody credited
    assert c5.tolist() == [[1, 0, 0], [0, 0, 0]]
    c5, c6 = RS.arrival_counts(True, np.int32([[3, 4]]), np.int32([[3, 5]]))
    assert c5.tolist() == [[0, 1]] and c6.tolist() == [[1, 1]]


# ---- (b) the helper ------------------------------------------------------------------------------------------------------------------
def test_helper_shapes_and_refusals():
    w, per_arena, m = VE.reward_terms(5)
    assert w.dtype == np.float32 and w.tolist() == [1, 0, 0, 0, 0, 0, 0] and per_arena == 0 and m == 0.0
    w, per_arena, m = VE.reward_terms(3, collision=-1.0, step=[-0.1, -0.2, -0.3], margin=0.25)
    assert w.shape == (3, 7) and per_arena == 1 and m == 0.25 and w.flags.c_contiguous
    assert w[:, 1].tolist() == [-1, -1, -1] and w[:, 6].tolist() == F([-0.1, -0.2, -0.3]).tolist() and w[:, 0].tolist() == [1, 1, 1]
    assert tuple(inspect.signature(VE.reward_terms).parameters)[1:8] == _lib.REWARD_TERMS
    for bad in (dict(collision=[1.0, 2.0]), dict(wall=np.zeros((3, 1))), dict(base=float("nan")), dict(step=[0.0, float("inf"), 0.0]),
                dict(near=1e39), dict(margin=-0.1), dict(margin=float("nan")), dict(margin=1001.0), dict(margin=float("inf"))):
        with pytest.raises(ValueError):
            VE.reward_terms(3, **bad)
    assert VE.reward_terms(3, margin=1000.0)[2] == 1000.0


# ---- (c) header, binding, interface -------------------------------------------------------------------------------------------------
PROTOTYPES = (
    "int ca_reward_configure(ca_env* env, const ca_reward_desc* desc);",
    "int ca_reward_clear(ca_env* env);",
    "int ca_reward_info(ca_env* env, int32_t* configured, int32_t* per_arena, float* margin);",
    "int ca_reward_get_weights(ca_env* env, float* weights, size_t bytes);",
    "int ca_reward_parts(ca_env* env);",
    "int ca_get_reward_parts(ca_env* env, float* ref, int32_t* counts /* [6, A, N] */, size_t ref_bytes, size_t counts_bytes, int32_t dst_is_device);",
    "int ca_reward_parts_ptr(ca_env* env, void** dev_ptr, size_t* bytes);",
)
NAMES = tuple(re.search(r"int (\w+)\(", p).group(1) for p in PROTOTYPES)


def test_header_and_binding_agree():
    text = open(HEADER).read()
    flat = " ".join(text.split())
    for p in PROTOTYPES:
        assert p in flat, p
    assert re.search(r"^#define CA_REWARD_N_TERMS 7\b", text, re.M) and _lib.REWARD_N_TERMS == 7
    for k, name in enumerate(_lib.REWARD_TERMS):
        assert re.search(r"^#define CA_REWARD_%s %d\b" % (name.upper(), k), text, re.M), name
        assert getattr(_lib, "REWARD_" + name.upper()) == k
    assert float(re.search(r"^#define CA_MAX_LENGTH (\S+?)f?$", text, re.M).group(1)) == _lib.MAX_LENGTH
    # the struct, member by member
    body = re.search(r"typedef struct ca_reward_desc \{(.*?)\} ca_reward_desc;", text, re.S).group(1)
    members = re.findall(r"^\s*(const float\*|size_t|int32_t|float)\s+(\w+);", body, re.M)
    ctype = {"const float*": C.c_void_p, "size_t": C.c_size_t, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in members] == list(_lib.RewardDesc._fields_)
    assert set(NAMES) <= set(_lib.EXPORTS)
    src = inspect.getsource(_lib.load)
    for name in NAMES:
        assert "L.%s.argtypes" % name in src, name
    assert os.path.join(os.path.dirname(B.LIB_PATH), "csrc", "ca_reward.h") in B.SOURCES      # the source hash covers the kernels
    hub = open(os.path.join(ROOT, "collision_avoidance_amd", "csrc", "ca_kernels.h")).read()
    assert '#include "ca_reward.h"' in hub
    block = text[text.index("enum ca_field {"):text.index("CA_FLD__COUNT")]
    assert len(re.findall(r"\bCA_FLD_\w+", block)) == 26                                          # the parts are no field
    for word in ("reward_begin_kernel", "reward_terms_kernel", "ONE CASE IS LEFT OUT", "NOT AFFECTED", "ca_solver_info does not change"):
        assert word in text, word


def test_library_exports_the_calls_and_a_null_handle_is_einval():
    L = _lib.load()
    for name in NAMES:
        assert getattr(L, name).restype is C.c_int
    d = _lib.RewardDesc()
    assert L.ca_reward_configure(None, C.byref(d)) == -1 and L.ca_reward_clear(None) == -1 and L.ca_reward_parts(None) == -1
    assert L.ca_reward_info(None, None, None, None) == -1 and L.ca_reward_get_weights(None, None, 0) == -1
    assert L.ca_get_reward_parts(None, None, None, 0, 0, 0) == -1 and L.ca_reward_parts_ptr(None, None, None) == -1


def test_interface():
    V = VecCollisionAvoidanceEnv
    par = inspect.signature(V.set_reward_terms).parameters
    assert tuple(par)[1:] == _lib.REWARD_TERMS + ("margin",)
    assert [par[k].default for k in tuple(par)[1:]] == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    for name in ("clear_reward_terms", "reward_terms_info", "reward_parts", "last_reward_parts"):
        assert callable(getattr(V, name)), name
    assert inspect.signature(V.__init__).parameters["reward_terms"].default is None
    assert not any("REWARD_PART" in n for n in V._STATE_FIELDS)                                     # the parts are not state
    from collision_avoidance_amd import envs, ppo
    for cls in (adapters.AgentVectorEnv, adapters.MultiAgentVectorEnv, envs.Collision_Avoidance_Env):
        assert inspect.signature(cls.__init__).parameters["reward_terms"].default is None, cls
    assert "set_reward_terms" in ppo.__doc__


class _TermsVec(H.OracleVec):
    def __init__(self, *a, **kw):
        H.OracleVec.__init__(self, *a, **kw)
        self.terms = None

    def set_reward_terms(self, **kw):
        self.terms = kw


def test_adapters_pass_the_terms_through():
    p = H.scenario_params("doorway", 3, max_step=40)
    terms = dict(collision=-1.0, margin=0.2)
    for make in (lambda v, **kw: adapters.AgentVectorEnv(v, **kw), lambda v, **kw: adapters.MultiAgentVectorEnv(v, **kw)):
        vec = _TermsVec(2, 3, "doorway", p, seed=1)
        make(vec, reward_terms=terms)
        assert vec.terms == terms
        vec = _TermsVec(2, 3, "doorway", p, seed=1)
        make(vec)
        assert vec.terms is None


# ---- (d) the compiled kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_reward_kernels_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    KR.ensure_asm()
    rows = {r["name"].split("(")[0].split("::")[-1]: r for r in KR.parse() if "reward_begin_kernel" in r["name"] or "reward_terms_kernel" in r["name"]}
    assert sorted(rows) == ["reward_begin_kernel", "reward_terms_kernel"], sorted(rows)    # one kernel text each, for all handles
    for name, r in rows.items():
        print("%s: %d VGPRs, %d SGPRs, %d B LDS, %d B code" % (name, r["vgpr"], r["sgpr"], r["lds"], r["code_bytes"]))
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert rows["reward_terms_kernel"]["lds"] == 3 * 256 * 4 and rows["reward_begin_kernel"]["lds"] == 0
