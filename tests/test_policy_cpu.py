"""CPU-only checks of the policy's host side (ca_policy_*, ca_rollout_policy; include/ca_env.h): the fp32 fmaf of the restatement
(tests/policy_scenes.py) against exact rationals, the shape helper, set_policy's normalisation of its three input forms, the binding
against the header.  No device."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from collision_avoidance_amd import _lib, build, vec_env
from tests import policy_scenes as PS

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulp_up(x):
    return np.nextafter(f32(x), f32(np.inf))


def test_fmaf_agrees_with_exact_rationals():
    """1.2e5 random triples over many magnitudes (results that cancel, results that are subnormal), constructed midpoint ties, and
    constructed double-rounding hazards: the float64 sum sits on an fp32 midpoint, the exact sum just beside it"""
    rs = np.random.RandomState(7)
    n = 120000
    a = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 20, n)).astype(f32)
    b = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 20, n)).astype(f32)
    c = (rs.standard_normal(n) * 2.0 ** rs.randint(-30, 30, n)).astype(f32)
    c[:20000] = -(a[:20000].astype(np.float64) * b[:20000]).astype(f32)                  # cancellation: the low bits of the product
    a[20000:30000] = (rs.standard_normal(10000) * 2.0 ** -70).astype(f32)                # subnormal results
    b[20000:30000] = (rs.standard_normal(10000) * 2.0 ** -65).astype(f32)
    c[20000:30000] = (rs.standard_normal(10000) * 2.0 ** -140).astype(f32)
    # exact ties: c = 1, a * b = 2^-24 (half an ulp of 1) -> even; c = 1 + ulp: the other parity
    ta, tb = np.full(4, 2.0 ** -12, f32), np.full(4, 2.0 ** -12, f32)
    tc = np.asarray([1.0, _ulp_up(1.0), -1.0, -_ulp_up(1.0)], f32)
    tb[2:] = -tb[2:]
    # hazards: a * b = 2^-24 (1 + 2^-23) (1 - 2^-23) = 2^-24 (1 - 2^-46) is a little less than half an ulp of 1; the float64 sum cannot
    # hold the deficit and lands on the tie, which ties-to-even then rounds UP from an odd c
    ha = np.full(4, 1 + 2.0 ** -23, f32)
    hb = np.full(4, 2.0 ** -24 * (1 - 2.0 ** -23), f32)
    hc = tc.copy()
    hb[2:] = -hb[2:]
    a, b, c = (np.concatenate(v) for v in ((a, ta, ha), (b, tb, hb), (c, tc, hc)))
    count = []
    got = PS.fmaf32(a, b, c, counter=count)
    want = np.asarray([PS.fma_exact(x, y, z) for x, y, z in zip(a, b, c)], f32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:10]
    assert count[0] >= 4                                                                  # the hazards took the exact path ...
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    assert (naive[-4:].view(np.uint32) != want[-4:].view(np.uint32)).any()                # ... and two roundings get them wrong
    sub = np.abs(want[20000:30000])
    assert ((sub > 0) & (sub < np.finfo(f32).tiny)).sum() > 1000                          # subnormal results were among the cases
    assert got[n] == f32(1.0) and got[n + 1] == _ulp_up(_ulp_up(1.0))                     # ties go to the even neighbour


def test_fraction_rounding_edges():
    tiny = Fraction(2) ** -149
    assert PS.fraction_to_f32(tiny / 2) == 0 and PS.fraction_to_f32(tiny * 3 / 2) == f32(2.0 ** -148)     # ties to even among subnormals
    assert PS.fraction_to_f32(tiny * 3 / 4) == f32(2.0 ** -149)
    big = Fraction(float(np.finfo(f32).max))
    assert PS.fraction_to_f32(big + Fraction(2) ** 102) == f32(np.finfo(f32).max)                          # below the midpoint to 2^128
    assert np.isinf(PS.fraction_to_f32(big + Fraction(2) ** 103)) and PS.fraction_to_f32(-big - Fraction(2) ** 103) == -np.inf
    assert PS.fraction_to_f32(Fraction(1, 3)) == f32(1.0 / 3.0)


def test_mlp_reference_is_the_chain():
    """one row, by hand: the chain starts from the bias, k ascending, ReLU gives +0 for a negative sum"""
    rs = np.random.RandomState(1)
    x = rs.standard_normal((3, 64)).astype(f32)
    W0, b0 = rs.standard_normal((16, 64)).astype(f32), rs.standard_normal(16).astype(f32)
    W1, b1 = rs.standard_normal((1, 16)).astype(f32), rs.standard_normal(1).astype(f32)
    got = PS.mlp_reference(x, [W0, W1], [b0, b1])
    for i in range(3):
        h = []
        for j in range(16):
            acc = b0[j]
            for k in range(64):
                acc = PS.fma_exact(x[i, k], W0[j, k], acc)
            h.append(acc if acc > 0 else f32(0.0))
        acc = b1[0]
        for k in range(16):
            acc = PS.fma_exact(h[k], W1[0, k], acc)
        assert got[i].view(np.uint32) == f32(acc).view(np.uint32)
    assert PS.out_reference(np.asarray([-5, 0.5, 5], f32), "clip", 1.0).tolist() == [-1.0, 0.5, 1.0]


# ---- the shape helper --------------------------------------------------------------------------------------------------------------
def test_policy_seq_shape_sizes():
    sh = vec_env.policy_seq_shape(3, 5, steps=7, hold=3, noise_shape=(3, 3, 5), weights_shape=(7,))
    assert sh == dict(R=3, noise=(3, 3, 5), weights=(7,), returns=(3, 5), first_done=(3,), obs=(3, 3, 5, 64), actions=(3, 3, 5),
                      rewards=(7, 3, 5), dones=(7, 3))
    assert vec_env.policy_seq_shape(3, 5, 0, 2)["R"] == 0 and vec_env.policy_seq_shape(3, 5, 6, 1)["R"] == 6
    assert PS.record_rows(7, 3) == (3, [0, 3, 6])


@pytest.mark.parametrize("kw", [dict(steps=7, hold=0), dict(steps=-1, hold=1), dict(steps=7, hold=3, noise_shape=(2, 3, 5)),
                                dict(steps=7, hold=3, noise_shape=(3, 5, 3)), dict(steps=7, hold=3, weights_shape=(6,))])
def test_policy_seq_shape_refusals(kw):
    with pytest.raises(ValueError, match="rollout_policy"):
        vec_env.policy_seq_shape(3, 5, **kw)


# ---- set_policy's three input forms ------------------------------------------------------------------------------------------------
def _layers(widths, P=None, seed=0):
    rs = np.random.RandomState(seed)
    lead = () if P is None else (P,)
    return [(rs.standard_normal(lead + (o, i)).astype(np.float64), rs.standard_normal(lead + (o,)).astype(np.float64))
            for i, o in zip(widths[:-1], widths[1:])]


def test_policy_layers_numpy_one_set_and_several():
    one = _layers((64, 32, 48, 1))
    widths, P, Ws, bs = vec_env.policy_layers(one)
    assert widths == [64, 32, 48, 1] and P == 1
    assert [W.shape for W in Ws] == [(1, 32, 64), (1, 48, 32), (1, 1, 48)] and [b.shape for b in bs] == [(1, 32), (1, 48), (1, 1)]
    assert all(W.dtype == f32 and W.flags["C_CONTIGUOUS"] for W in Ws + bs)
    assert np.array_equal(Ws[1][0], one[1][0].astype(f32))
    widths, P, Ws, bs = vec_env.policy_layers(_layers((64, 16, 1), P=3))
    assert widths == [64, 16, 1] and P == 3 and Ws[0].shape == (3, 16, 64) and bs[1].shape == (3, 1)


def test_policy_layers_torch_tensors_and_sequential():
    import torch
    tl = [(torch.as_tensor(W), torch.as_tensor(b)) for W, b in _layers((64, 64, 64, 1), seed=2)]
    widths, P, Ws, bs = vec_env.policy_layers(tl)
    assert widths == [64, 64, 64, 1] and P == 1 and np.array_equal(Ws[2][0], tl[2][0].numpy().astype(f32))
    net = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 1))
    widths, P, Ws, bs = vec_env.policy_layers(net)
    assert widths == [64, 64, 64, 1] and P == 1
    assert np.array_equal(Ws[0][0], net[0].weight.detach().numpy()) and np.array_equal(bs[2][0], net[4].bias.detach().numpy())
    with pytest.raises(ValueError, match="Sequential"):
        vec_env.policy_layers(torch.nn.Sequential(torch.nn.Linear(64, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1)))
    with pytest.raises(ValueError, match="Sequential"):
        vec_env.policy_layers(torch.nn.Sequential(torch.nn.Linear(64, 16), torch.nn.ReLU(), torch.nn.Linear(16, 1), torch.nn.ReLU()))


@pytest.mark.parametrize("widths,word", [((64, 20, 1), "multiple of 16"), ((64, 144, 1), "multiple of 16"), ((32, 16, 1), "observation"),
                                         ((64, 16, 2), "output layer"), ((64, 1), "layers"), ((64, 16, 16, 16, 16, 1), "layers")])
def test_policy_layers_refusals(widths, word):
    with pytest.raises(ValueError, match=word):
        vec_env.policy_layers(_layers(widths))


def test_policy_layers_refuses_what_does_not_chain_or_is_not_finite():
    bad = _layers((64, 16, 1))
    bad[1] = (np.zeros((1, 32)), np.zeros(1))
    with pytest.raises(ValueError, match="layer 1 reads 32"):
        vec_env.policy_layers(bad)
    nan = _layers((64, 16, 1))
    nan[0][0][3, 5] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        vec_env.policy_layers(nan)
    mixed = _layers((64, 16, 1), P=2)
    mixed[1] = _layers((64, 16, 1), P=3)[1]
    with pytest.raises(ValueError, match="sets"):
        vec_env.policy_layers(mixed)


# ---- the binding against the header ------------------------------------------------------------------------------------------------
def _struct_fields(h, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*?\]", "", d).split()[-1].lstrip("*") for d in body.split(";") if d.strip()]


def test_binding_restates_the_header():
    h = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    assert re.search(r"^int ca_rollout_policy\(ca_env\* env, int32_t steps, uint32_t flags, const ca_policy_seq\* seq\);", h, re.M)
    assert re.search(r"^int ca_policy_actions\(ca_env\* env, const float\* noise, float\* actions_out\);", h, re.M)
    assert _struct_fields(h, "ca_policy_seq") == [n for n, _ in _lib.PolicySeq._fields_]
    assert _struct_fields(h, "ca_policy_desc") == [n for n, _ in _lib.PolicyDesc._fields_]
    assert C.sizeof(_lib.PolicySeq) == 8 + 8 * 16 and C.sizeof(_lib.PolicyDesc) == 24 + 4 * 32 + 8 + 16 + 8
    for name in ("ca_policy_configure", "ca_policy_clear", "ca_policy_info", "ca_policy_actions", "ca_rollout_policy"):
        assert name in _lib.EXPORTS
    for macro, val in (("CA_POLICY_OUT_IDENTITY", _lib.POLICY_OUT_IDENTITY), ("CA_POLICY_OUT_CLIP", _lib.POLICY_OUT_CLIP),
                       ("CA_POLICY_MAX_LAYERS", _lib.POLICY_MAX_LAYERS), ("CA_POLICY_MAX_WIDTH", _lib.POLICY_MAX_WIDTH)):
        assert int(re.search(r"#define %s (\d+)" % macro, h).group(1)) == val
    assert os.path.join(os.path.dirname(build.LIB_PATH), "csrc", "ca_policy.h") in build.SOURCES   # the source hash covers the kernels
    L = _lib.load()
    assert L.ca_rollout_policy(None, 4, 0, None) == -1 and L.ca_policy_actions(None, None, None) == -1
    assert L.ca_policy_configure(None, None) == -1


# ---- the compiler's metadata ----------------------------------------------------------------------------------------------------------
def test_policy_kernels_use_no_scratch():
    """tools/kernel_resources.py: the policy kernel (the instance without heads of the one kernel template) runs on the f32-input
    MFMA with no scratch memory, no spilled register and no static LDS (its LDS is dynamic: two images of 32 rows); the record kernel is a small kernel"""
    import shutil
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    kr.ensure_asm()
    rows = {r["name"]: r for r in kr.parse()}
    pol = [r for n, r in rows.items() if "policy_kernel<false>" in n]
    rec = [r for n, r in rows.items() if "policy_record_kernel" in n]
    assert len(pol) == 1 and len(rec) == 1, sorted(n for n in rows if "policy" in n)
    for r in pol + rec:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, r
    assert pol[0]["vgpr"] <= 128 and rec[0]["vgpr"] <= 32, (pol, rec)
    asm = open(kr.ASM).read()
    body = asm[asm.index(pol[0]["sym"] + ":"):]
    body = body[:body.index(".Lfunc_end")]
    assert body.count("v_mfma_f32_16x16x4_f32") == 8 and "v_fma_f32" not in body and "v_fmac_f32" not in body
