"""CPU-only checks of PPO sample collection's host side (ca_policy_set_heads, ca_policy_evaluate, ca_rollout_policy_sample, ca_gae;
include/ca_env.h): the restatement (tests/ppo_scenes.py) against the oracle's exp64, exact rationals and float64 formulas, the
heads helper's refusals, the binding against the header, the compiler's metadata of the three new kernels.  No device."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from collision_avoidance_amd import _lib, vec_env
from tests import policy_scenes as PS
from tests import ppo_scenes as PP

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exp64_restatement_equals_the_oracle():
    """400 values in [-20, 2] -- the clamp's range --, its ends, zero and fp32 values as the kernel converts them"""
    from oracle import oracle as o
    rs = np.random.RandomState(3)
    x = np.concatenate([rs.uniform(-20.0, 2.0, 300), rs.uniform(-20.0, 2.0, 100).astype(f32).astype(f64), [-20.0, 2.0, 0.0, -0.0, 1e-30]])
    got = PP.exp64(x)
    want = np.asarray([o.exp64(v) for v in x], f64)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.flatnonzero(got != want)[:10]
    assert np.abs(got - np.exp(x)).max() <= 4e-16 * np.exp(2.0)


# ---- GAE ----------------------------------------------------------------------------------------------------------------------------
def _gae_exact(rewards, values, done, valid, gamma, lam):
    """ca_gae's definition with every operation rounded through exact rationals (fraction_to_f32)"""
    F = lambda v: Fraction(float(v))
    rnd = PS.fraction_to_f32
    R, A, N = rewards.shape
    g = f32(gamma)
    gl = rnd(F(g) * F(f32(lam)))
    adv, tgt = np.zeros((R, A, N), f32), np.zeros((R, A, N), f32)
    for a in range(A):
        for i in range(N):
            for r in range(R - 1, -1, -1):
                nd = done[r, a] == 0
                nv = values[r + 1, a, i] if nd else f32(0.0)
                delta = rnd(F(rnd(F(rewards[r, a, i]) + F(rnd(F(g) * F(nv))))) - F(values[r, a, i]))
                na = adv[r + 1, a, i] if nd and r < R - 1 else f32(0.0)
                x = rnd(F(delta) + F(rnd(F(gl) * F(na))))
                if valid is not None and valid[r, a] == 0:
                    x = f32(0.0)
                adv[r, a, i] = x
                tgt[r, a, i] = rnd(F(x) + F(values[r, a, i]))
    return adv, tgt


def _gae_case(R, A=2, N=3, seed=0):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((R, A, N)).astype(f32), rs.standard_normal((R + 1, A, N)).astype(f32)


@pytest.mark.parametrize("name,R,done,valid", [
    ("a done in the middle", 5, {(2, 0)}, None), ("a done at the last row", 4, {(3, 1)}, None),
    ("rows that are not valid", 5, {(1, 1)}, {(0, 0), (3, 1), (4, 1)}), ("one row", 1, set(), None), ("one row, done", 1, {(0, 0)}, None),
    ("no rows", 0, set(), None)])
def test_gae_reference_against_exact_rationals(name, R, done, valid):
    A, N = 2, 3
    rew, val = _gae_case(R, A, N, seed=R)
    d = np.zeros((R, A), np.int32)
    for r, a in done:
        d[r, a] = 1
    v = None
    if valid is not None:
        v = np.ones((R, A), np.int32)
        for r, a in valid:
            v[r, a] = 0
    for gamma, lam in ((0.95, 1.0), (0.99, 0.9)):
        got = PP.gae_reference(rew, val, d, v, gamma, lam)
        want = _gae_exact(rew, val, d, v, gamma, lam)
        for g, w, what in zip(got, want, ("advantages", "targets")):
            assert g.shape == (R, A, N) and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, what)
    if R and done:   # the done row bootstraps from nothing and passes nothing on
        r, a = sorted(done)[0]
        adv, _ = PP.gae_reference(rew, val, d, v, 0.95, 1.0)
        if v is None:
            assert np.array_equal(adv[r, a], (rew[r, a] - val[r, a]).astype(f32))
    if v is not None:
        adv, tgt = PP.gae_reference(rew, val, d, v, 0.95, 1.0)
        for r, a in valid:
            assert not adv[r, a].any() and np.array_equal(tgt[r, a], val[r, a])


def test_gae_telescopes_to_the_discounted_return():
    """lambda = 1, no done: adv[r] = sum_k gamma^k rew[r + k] + gamma^(R - r) values[R] - values[r].  Measured here against that
    formula in float64 at R = 64, gamma = 0.95, 2000 agents, rewards and values ~ N(0, 1): the largest deviation is 3.23e-6 =
    1.08 eps32 * scale, where scale = the largest sum over a row of the absolute values of the formula's terms (25.1): the fp32 chain
    rounds each of its four operations per row to half an ulp of a partial result no larger than scale, and the errors of the rows
    behind decay with gamma^k.  Asserted with a margin of 4 for the order of the summation: 4 * 1.1 eps32 * scale; the targets add
    one more rounding of a value below scale."""
    R, A, N, gamma = 64, 4, 500, 0.95
    rs = np.random.RandomState(11)
    rew, val = rs.standard_normal((R, A, N)).astype(f32), rs.standard_normal((R + 1, A, N)).astype(f32)
    adv, tgt = PP.gae_reference(rew, val, np.zeros((R, A), np.int32), None, gamma, 1.0)
    g = float(f32(gamma))
    ret = np.zeros((R + 1, A, N), f64)
    mag = np.zeros((R + 1, A, N), f64)
    ret[R], mag[R] = val[R], np.abs(val[R])
    for r in range(R - 1, -1, -1):
        ret[r] = rew[r].astype(f64) + g * ret[r + 1]
        mag[r] = np.abs(rew[r]).astype(f64) + g * mag[r + 1]
    want = ret[:R] - val[:R].astype(f64)
    scale = (mag[:R] + np.abs(val[:R])).max()
    err = np.abs(adv.astype(f64) - want).max()
    eps = float(np.finfo(f32).eps)
    print("gae telescoping: largest deviation %.3g = %.2f eps32 * scale (scale %.3g)" % (err, err / (eps * scale), scale))
    assert err <= 4 * 1.1 * eps * scale, (err, eps * scale)
    assert np.abs(tgt.astype(f64) - ret[:R]).max() <= 4 * 1.1 * eps * scale + 0.5 * eps * scale


def test_logp_against_the_float64_normal_log_density():
    """logp is the log-density of u under N(mean, std): -eps^2 / 2 - ls - log(2 pi) / 2, to a few ulps of its largest term"""
    rs = np.random.RandomState(5)
    n = 4000
    mean = rs.standard_normal(n).astype(f32)
    ls_raw = rs.uniform(-25.0, 4.0, n).astype(f32)
    eps = (3.0 * rs.standard_normal(n)).astype(f32)
    s = PP.sample_reference(mean, ls_raw, eps)
    ls = np.clip(ls_raw.astype(f64), -20.0, 2.0)
    assert np.array_equal(s["log_std"], ls.astype(f32)) and s["log_std"].min() == -20 and s["log_std"].max() == 2
    e = eps.astype(f64)
    want = -0.5 * e * e - ls - 0.5 * math.log(2 * math.pi)
    big = np.maximum(np.maximum(0.5 * e * e, np.abs(ls)), 0.92)
    assert (np.abs(s["logp"].astype(f64) - want) <= 4 * np.finfo(f32).eps * big).all()
    # u = mean + std * eps, and the density in terms of u: (u - mean) / std recovers eps to rounding where std * eps is not tiny beside mean
    std = np.exp(ls)
    assert (np.abs(s["u"].astype(f64) - (mean.astype(f64) + std * e)) <= 2 * np.finfo(f32).eps * (np.abs(mean) + std * np.abs(e))).all()
    none = PP.sample_reference(mean, ls_raw, None, has_log_std=False)
    assert np.array_equal(none["actions"], mean) and (none["logp"] == f32(-0.918938533)).all() and not none["log_std"].any()


def test_heads_reference_is_the_chain():
    """one set by hand: mean, log-std and value are three chains over the same hidden activations; a None log-std weight is the bias"""
    rs = np.random.RandomState(2)
    x = rs.standard_normal((1, 2, 64)).astype(f32)
    Ws = [rs.standard_normal((1, 16, 64)).astype(f32) / 8, rs.standard_normal((1, 1, 16)).astype(f32) / 4]
    bs = [rs.standard_normal((1, 16)).astype(f32), rs.standard_normal((1, 1)).astype(f32)]
    vw, vb = rs.standard_normal((1, 16)).astype(f32), rs.standard_normal(1).astype(f32)
    lb = np.asarray([-0.5], f32)
    mean, ls_raw, val = PP.heads_reference(x, Ws, bs, None, (vw, vb), (None, lb))
    assert np.array_equal(mean, PS.actions_reference(x, Ws, bs)) and (ls_raw == lb[0]).all()
    for i in range(2):
        h = []
        for j in range(16):
            acc = bs[0][0, j]
            for k in range(64):
                acc = PS.fma_exact(x[0, i, k], Ws[0][0, j, k], acc)
            h.append(acc if acc > 0 else f32(0.0))
        acc = vb[0]
        for k in range(16):
            acc = PS.fma_exact(h[k], vw[0, k], acc)
        assert val[0, i].view(np.uint32) == f32(acc).view(np.uint32)
    assert not PP.heads_reference(x, Ws, bs)[2].any()


def test_row_records_by_hand():
    rew = np.arange(1, 8, dtype=f32).reshape(7, 1, 1) * np.ones((7, 2, 1), f32)
    dones = np.zeros((7, 2), np.int32)
    dones[4:, 0] = 1
    rr, rd, rv = PP.row_records(np.zeros(2, np.int32), rew, dones, 3, True)
    assert rr[:, 0, 0].tolist() == [6.0, 9.0, 0.0] and rr[:, 1, 0].tolist() == [6.0, 15.0, 7.0]      # arena 0 froze behind step 4
    assert rd.tolist() == [[0, 0], [1, 0], [1, 0]] and rv.tolist() == [[1, 1], [1, 1], [0, 1]]
    rr, rd, rv = PP.row_records(np.zeros(2, np.int32), rew, dones, 3, False)
    assert rr[:, 0, 0].tolist() == [6.0, 15.0, 7.0] and rv.all()
    assert vec_env.policy_sample_shape(2, 1, 7, 3)["values"] == (4, 2, 1) and vec_env.policy_sample_shape(2, 1, 7, 3)["dist"] == (3, 2, 2, 1)


# ---- the heads helper -------------------------------------------------------------------------------------------------------------------
def test_policy_heads_forms():
    import torch
    h = vec_env.policy_heads(16, 2, value=(np.ones(16), 0.5), log_std=(None, [-1.0, -2.0]))
    assert h["value_w"].shape == (2, 16) and h["value_w"].dtype == f32 and h["value_w"].flags["C_CONTIGUOUS"]
    assert h["value_b"].tolist() == [0.5, 0.5] and h["logstd_w"] is None and h["logstd_b"].tolist() == [-1.0, -2.0]
    lin = torch.nn.Linear(16, 1)
    h = vec_env.policy_heads(16, 1, value=lin)
    assert np.array_equal(h["value_w"], lin.weight.detach().numpy()) and h["logstd_b"] is None and h["value_b"].shape == (1,)


@pytest.mark.parametrize("kw,word", [(dict(), "at least one"), (dict(value=(np.ones(8), 0.0)), "last hidden width"),
                                     (dict(value=(np.ones((3, 16)), 0.0)), "last hidden width"), (dict(value=(None, 0.0)), "no weights"),
                                     (dict(log_std=(np.ones(16), None)), "no bias"), (dict(log_std=(None, [0.0, 0.0, 0.0])), "one value per weight set"),
                                     (dict(value=(np.full(16, np.nan), 0.0)), "not finite"), (dict(log_std=(None, np.inf)), "not finite"),
                                     (dict(value=np.ones(16)), r"\(w, b\)")])
def test_policy_heads_refusals(kw, word):
    with pytest.raises(ValueError, match=word):
        vec_env.policy_heads(16, 2, **kw)


# ---- the binding against the header -------------------------------------------------------------------------------------------------
def _struct_fields(h, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*?\]", "", d).split()[-1].lstrip("*") for d in body.split(";") if d.strip()]


def test_binding_restates_the_header():
    h = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    for decl in (r"int ca_policy_set_heads\(ca_env\* env, const ca_policy_heads\* heads\);", r"int ca_policy_clear_heads\(ca_env\* env\);",
                 r"int ca_policy_heads_info\(ca_env\* env, int32_t\* has_value, int32_t\* has_logstd\);",
                 r"int ca_policy_evaluate\(ca_env\* env, const float\* noise, const ca_policy_eval\* out\);",
                 r"int ca_rollout_policy_sample\(ca_env\* env, int32_t steps, uint32_t flags, const ca_policy_sample_seq\* seq\);",
                 r"int ca_gae\(ca_env\* env, int32_t rows, const ca_gae_desc\* desc\);"):
        assert re.search("^" + decl, h, re.M), decl
    for struct, cls in (("ca_policy_heads", _lib.PolicyHeads), ("ca_policy_eval", _lib.PolicyEval), ("ca_policy_sample_seq", _lib.PolicySampleSeq),
                        ("ca_gae_desc", _lib.GaeDesc)):
        assert _struct_fields(h, struct) == [n for n, _ in cls._fields_], struct
    # the sampling sequence carries the members of ca_policy_seq, in their order and at their offsets
    seq = _struct_fields(h, "ca_policy_seq")
    assert _struct_fields(h, "ca_policy_sample_seq")[:len(seq)] == seq
    assert all(getattr(_lib.PolicySampleSeq, n).offset == getattr(_lib.PolicySeq, n).offset for n in seq)
    assert C.sizeof(_lib.PolicySeq) == 8 + 8 * 16                                         # (untouched)
    assert C.sizeof(_lib.PolicySampleSeq) == 8 + 8 * 16 + 8 * 16 + 8 and C.sizeof(_lib.GaeDesc) == 12 * 8 + 8
    assert C.sizeof(_lib.PolicyHeads) == 64 and C.sizeof(_lib.PolicyEval) == 40
    for name in ("ca_policy_set_heads", "ca_policy_clear_heads", "ca_policy_heads_info", "ca_policy_evaluate", "ca_rollout_policy_sample", "ca_gae"):
        assert name in _lib.EXPORTS
    for macro, val in (("CA_POLICY_LOGSTD_MIN", _lib.POLICY_LOGSTD_MIN), ("CA_POLICY_LOGSTD_MAX", _lib.POLICY_LOGSTD_MAX)):
        assert float(re.search(r"#define %s \(?(-?[\d.]+)f\)?" % macro, h).group(1)) == val
    L = _lib.load()
    assert L.ca_policy_set_heads(None, None) == -1 and L.ca_policy_clear_heads(None) == -1 and L.ca_policy_heads_info(None, None, None) == -1
    assert L.ca_policy_evaluate(None, None, None) == -1 and L.ca_rollout_policy_sample(None, 4, 0, None) == -1 and L.ca_gae(None, 1, None) == -1


# ---- the compiler's metadata ----------------------------------------------------------------------------------------------------------
def test_ppo_kernels_use_no_scratch():
    """tools/kernel_resources.py: the heads kernel (policy_kernel<true>) runs on the f32-input MFMA like policy_kernel<false> -- the same eight MFMAs, no fp32 FMA
    (the chains are the MFMA's, the output stage multiplies and adds) --, and none of the three new kernels uses scratch memory, a
    spilled register or static LDS"""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    kr.ensure_asm()
    rows = {r["name"]: r for r in kr.parse()}
    new = {k: [r for n, r in rows.items() if k in n] for k in ("policy_kernel<true>", "sample_record_kernel", "gae_kernel")}
    for k, found in new.items():
        assert len(found) == 1, (k, sorted(rows))
        r = found[0]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, r
    assert new["policy_kernel<true>"][0]["vgpr"] <= 128 and new["sample_record_kernel"][0]["vgpr"] <= 32 and new["gae_kernel"][0]["vgpr"] <= 64
    asm = open(kr.ASM).read()
    body = asm[asm.index(new["policy_kernel<true>"][0]["sym"] + ":"):]
    body = body[:body.index(".Lfunc_end")]
    assert body.count("v_mfma_f32_16x16x4_f32") == 8 and "v_fma_f32" not in body and "v_fmac_f32" not in body
