"""CPU-only checks of the host side of action-sequence rollouts (ca_rollout_actions, include/ca_env.h): the binding restates the
header's struct and prototype, the rule of the returns (tests/actseq_scenes.py) gives what the header says on hand-made reward tables,
the front end's shape checks refuse before any library call, and the compiler's metadata shows the ActionSeq instantiations of the
four-lanes kernel without scratch memory.  No compute call is made."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from collision_avoidance_amd import _lib, build, vec_env
from tests import actseq_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "ca_env.h")).read()


def test_header_struct_export_and_argtypes_agree():
    h = _header()
    assert re.search(r"^int ca_rollout_actions\(ca_env\* env, int32_t steps, uint32_t flags, const ca_action_seq\* seq\);", h, re.M)
    body = re.search(r"typedef struct ca_action_seq \{(.*?)\} ca_action_seq;", h, re.S).group(1)
    members = re.findall(r"^\s*(const float\*|float\*|int32_t\*|size_t|int32_t)\s+(\w+);", body, re.M)
    ctype = {"const float*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "size_t": C.c_size_t, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in members] == list(_lib.ActionSeq._fields_)
    assert [n for _, n in members] == ["actions", "actions_bytes", "hold", "weights", "weights_bytes", "returns", "returns_bytes",
                                       "first_done", "first_done_bytes"]
    assert "ca_rollout_actions" in _lib.EXPORTS
    L = _lib.load()
    f = L.ca_rollout_actions
    assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(_lib.ActionSeq)]
    doc = h[h.index("Action-sequence rollouts:"):h.index("typedef struct ca_action_seq")]
    for word in ("bit for bit", "RUNS ACROSS", "CA_F_NODONE", "CA_ESIZE", "CA_EINVAL", "frozen at", "steps == 0", "rollout_one_launch"):
        assert word in doc, word


def test_a_null_handle_is_refused():
    L = _lib.load()
    seq = _lib.ActionSeq(actions=None, actions_bytes=0, hold=1)
    assert L.ca_rollout_actions(None, 4, 0, C.byref(seq)) == -1
    assert L.ca_rollout_actions(None, 4, 0, None) == -1


def test_kernel_source_is_hashed():
    assert os.path.join(os.path.dirname(build.LIB_PATH), "csrc", "ca_actseq.h") in build.SOURCES


# ---- the rule of the returns on hand-made tables ----------------------------------------------------------------------------------
def _table(T, A, N, seed):
    return np.random.RandomState(seed).uniform(-1, 1, (T, A, N)).astype(f32)


def test_rows_of_steps():
    assert S.rows(7, 3) == (3, [0, 0, 0, 1, 1, 1, 2])          # steps no multiple of hold: the last row is held for one step
    assert S.rows(6, 3) == (2, [0, 0, 0, 1, 1, 1])
    assert S.rows(5, 1) == (5, [0, 1, 2, 3, 4])
    assert S.rows(2, 9) == (1, [0, 0])
    assert S.rows(0, 4) == (0, [])


def test_unweighted_sum_is_the_sequential_float32_sum():
    r = _table(9, 2, 3, 1)
    adv = S.advanced_reference(np.zeros(2, np.int32), np.zeros((9, 2), np.int32), freeze=False)
    got = S.returns_reference(r, adv)
    want = np.zeros((2, 3), f32)
    for t in range(9):
        want = want + r[t]
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_weights_are_a_product_and_a_sum_each_rounded_once():
    """one agent, two steps, chosen so that a fused multiply-add rounds differently: ret = 1, w * r = (1 + 2^-12)^2 * 2^-24 ..."""
    w = np.asarray([1.0, 1.0 + 2.0 ** -12], f32)
    r = np.asarray([1.0, (1.0 + 2.0 ** -12) * 2.0 ** -1], f32).reshape(2, 1, 1)
    got = S.returns_reference(r, np.ones((2, 1), bool), w)
    prod = f32(w[1]) * f32(r[1, 0, 0])                                   # rounded to float32: drops the 2^-25 term
    assert got[0, 0] == f32(f32(1.0) + prod)
    exact = 1.0 + float(w[1]) * float(r[1, 0, 0])
    assert float(prod) != float(w[1]) * float(r[1, 0, 0]) and got.dtype == f32 and abs(float(got[0, 0]) - exact) < 2.0 ** -23
    # discounts over a table, against a scalar loop
    r, wt = _table(12, 3, 2, 2), (f32(0.99) ** np.arange(12)).astype(f32)
    got = S.returns_reference(r, np.ones((12, 3), bool), wt)
    for a in range(3):
        for i in range(2):
            acc = f32(0.0)
            for t in range(12):
                acc = f32(acc + f32(wt[t] * r[t, a, i]))
            assert got[a, i] == acc


def test_a_frozen_tail_adds_nothing_and_first_done_is_the_step_that_froze():
    T, A, N = 8, 3, 2
    r = _table(T, A, N, 3)
    done = np.zeros((T, A), np.int32)
    done[4:, 1] = 1                                     # arena 1 ends at step 4 and stays done; arena 2 never; arena 0 at the last step
    done[7, 0] = 1
    adv = S.advanced_reference(np.zeros(A, np.int32), done, freeze=True)
    assert adv[:, 1].tolist() == [True] * 5 + [False] * 3 and adv[:, 0].all() and adv[:, 2].all()
    got = S.returns_reference(r, adv)
    assert np.array_equal(got[1], S.returns_reference(r[:5], np.ones((5, A), bool))[1])
    assert np.array_equal(got[0], S.returns_reference(r, np.ones((T, A), bool))[0])
    assert S.first_done_reference(done, adv).tolist() == [7, 4, -1]
    # without CA_F_FREEZE the same flags stop nothing
    adv = S.advanced_reference(np.zeros(A, np.int32), done, freeze=False)
    assert adv.all() and S.first_done_reference(done, adv).tolist() == [7, 4, -1]
    assert np.array_equal(S.returns_reference(r, adv), S.returns_reference(r, np.ones((T, A), bool)))


def test_all_frozen_at_entry():
    T, A, N = 5, 2, 3
    r = _table(T, A, N, 4)
    entry = np.ones(A, np.int32)
    done = np.ones((T, A), np.int32)
    adv = S.advanced_reference(entry, done, freeze=True)
    assert not adv.any()
    got = S.returns_reference(r, adv, (f32(0.9) ** np.arange(T)).astype(f32))
    assert np.array_equal(got.view(np.uint32), np.zeros((A, N), np.uint32))          # +0.0, bit for bit
    assert S.first_done_reference(done, adv).tolist() == [-1, -1]
    # one of two frozen at entry; the other runs and ends at step 2
    entry = np.asarray([1, 0], np.int32)
    done[:2, 1] = 0
    adv = S.advanced_reference(entry, done, freeze=True)
    assert S.first_done_reference(done, adv).tolist() == [-1, 2] and adv[:, 1].tolist() == [True, True, True, False, False]


def test_absent_rows_stay_zero_and_zero_steps():
    r = _table(4, 2, 3, 5)
    present = np.asarray([[True, True, False], [True, False, False]])
    got = S.returns_reference(r, np.ones((4, 2), bool), present=present)
    assert not got[~present].any() and got[present].all()
    got = S.returns_reference(np.zeros((0, 2, 3), f32), np.zeros((0, 2), bool))
    assert got.shape == (2, 3) and np.array_equal(got.view(np.uint32), np.zeros((2, 3), np.uint32))
    assert S.first_done_reference(np.zeros((0, 2), np.int32), np.zeros((0, 2), bool)).tolist() == [-1, -1]


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def test_signatures():
    V = vec_env.VecCollisionAvoidanceEnv
    p = inspect.signature(V.rollout_actions).parameters
    assert list(p)[1:11] == ["actions", "hold", "weights", "returns", "first_done", "with_obs", "stats", "autoreset", "freeze", "contacts"]
    assert (p["hold"].default, p["weights"].default, p["returns"].default, p["first_done"].default) == (1, None, True, False)
    assert not any(p[k].default for k in ("with_obs", "stats", "autoreset", "freeze", "contacts")) and p["steps"].default is None
    q = inspect.signature(V.step_repeat).parameters
    assert list(q)[1:] == ["actions", "k", "with_obs", "stats", "autoreset"] and q["with_obs"].default is True
    for f in (V.step, V.rollout):                              # as they were
        assert "hold" not in inspect.signature(f).parameters and "frame_skip" not in inspect.signature(f).parameters


@pytest.mark.parametrize("shape,hold,steps,wshape,want", [
    ((4, 3, 5), 1, None, None, (4, 4)),
    ((4, 3, 5), 3, None, (12,), (4, 12)),
    ((4, 3, 5), 3, 10, (10,), (4, 10)),                        # a shorter last row
    ((1, 3, 5), 7, None, None, (1, 7)),
    ((0, 3, 5), 2, None, None, (0, 0)),
    ((0, 3, 5), 2, 0, (0,), (0, 0)),
])
def test_shape_plan_accepts(shape, hold, steps, wshape, want):
    assert vec_env.action_seq_shape(shape, 3, 5, hold, steps, wshape) == want


@pytest.mark.parametrize("shape,hold,steps,wshape", [
    ((4, 3, 5), 0, None, None),                                # hold < 1
    ((4, 3, 5), -2, None, None),
    ((3, 5), 1, None, None),                                   # no row axis
    ((4, 5, 3), 1, None, None),                                # [R, N, A]
    ((4, 3, 6), 1, None, None),
    ((4, 3, 5), 3, 9, None),                                   # 9 steps need 3 rows
    ((4, 3, 5), 3, 13, None),                                  # 13 steps need 5
    ((4, 3, 5), 3, -1, None),
    ((4, 3, 5), 3, None, (4,)),                                # weights per row instead of per step
    ((4, 3, 5), 3, 10, (12,)),
    ((4, 3, 5), 1, None, (4, 1)),
])
def test_shape_plan_refuses(shape, hold, steps, wshape):
    with pytest.raises(ValueError, match="rollout_actions"):
        vec_env.action_seq_shape(shape, 3, 5, hold, steps, wshape)


def test_bad_shapes_raise_before_any_library_call():
    """an object with the attributes the front end reads and a library that fails the test if it is touched"""
    class NoLib(object):
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)
    V = vec_env.VecCollisionAvoidanceEnv
    e = V.__new__(V)
    e.A, e.N, e.use_torch, e.device, e.L, e.h = 3, 5, False, 0, NoLib(), None
    for kw in (dict(actions=np.zeros((4, 5, 3), f32)), dict(actions=np.zeros((3, 5), f32)), dict(actions=np.zeros((2, 3, 5), f32), hold=0),
               dict(actions=np.zeros((2, 3, 5), f32), hold=2, steps=5), dict(actions=np.zeros((2, 3, 5), f32), weights=np.ones(3, f32))):
        with pytest.raises(ValueError, match="rollout_actions"):
            e.rollout_actions(**kw)
    with pytest.raises(ValueError, match="step_repeat"):
        e.step_repeat(np.zeros((3, 5), f32), 0)
    with pytest.raises(ValueError):
        e.step_repeat(np.zeros((3, 4), f32), 2)


# ---- the compiler's metadata ----------------------------------------------------------------------------------------------------------
def test_action_seq_instantiations_use_no_scratch():
    """tools/kernel_resources.py: the four-lanes kernel under the ActionSeq tag for both K classes, the four workgroup sizes and both
    obstacle-list capacities, without the bandit; no scratch memory and no spilled register in any of them; nothing else carries the
    tag."""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    kr.ensure_asm()
    rows = {r["name"]: r for r in kr.parse()}
    want = ["quad_kernel<%d, %d, %d, false, ActionSeq>" % (k, bs, sq) for k in (5, 10) for bs in (64, 128, 256, 512) for sq in (4, 16)]
    for name in want:
        assert name in rows, name
        assert rows[name]["scratch"] == 0 and rows[name]["vgpr_spill"] == 0, (name, rows[name])
        plain = rows[name.replace(", ActionSeq", "")]
        assert rows[name]["lds"] == plain["lds"], (name, rows[name], plain)       # no static LDS of its own: the host's fit test holds
    assert sorted(n for n in rows if "ActionSeq" in n) == sorted(want)
    for small in ("actseq_begin_kernel", "actseq_accumulate_kernel", "actseq_setup_kernel"):
        assert any(small in n for n in rows), small
