"""CPU-only checks of the edge scenes (tests/policy_edge_scenes.py): every scene reaches the numbers it was built for -- conditions on
the restatement alone, so a scene that stopped reaching them fails here and not on the card --, the tracing twin is the restatement,
the fused multiply-add of the restatement follows IEEE 754 where an operand is inf or a sum overflows, and each of three wrong
multiply-adds (operands flushed, two roundings, the float64 double rounding) changes what its scene reads out: the scenes can tell.
No device."""
from fractions import Fraction

import numpy as np
import pytest

from tests import policy_edge_scenes as E
from tests import policy_scenes as PS
from tests import ppo_scenes as PP

f32 = np.float32
_built = {}


def _scene(name):
    if name not in _built:
        _built[name] = E.SCENES[name][0]()
    return _built[name]


# ---- reach ----------------------------------------------------------------------------------------------------------------------------------
def test_subnormal_scene_reaches_the_subnormals():
    sc, r = _scene("subnormal")
    assert r["subnormal_obs"] >= 1000 and r["subnormal_weights"] >= 1000 and r["subnormal_bias"] >= 16, r
    assert r["first_layer_subnormal_states"] >= 1000, r
    assert r["chains_through_and_into_subnormal"] >= 32, r
    assert r["subnormal_hidden"] >= 100, r
    assert r["subnormal_means"] >= 8 and r["subnormal_values"] >= 8 and r["rounded_subnormal_values"] >= 8, r
    assert np.isfinite(sc.obs).all() and all(np.isfinite(W).all() for W, _ in sc.layers)


def test_overflow_scene_reaches_inf_from_finite_operands():
    sc, r = _scene("overflow")
    assert np.isfinite(sc.obs).all() and all(np.isfinite(W).all() and np.isfinite(b).all() for W, b in sc.layers)
    assert r["of_them_with_a_finite_exact_sum"] >= 16 and r["chains_with_mid_inf"] > r["of_them_with_a_finite_exact_sum"], r
    assert r["chains_at_flt_max"] >= 8 and r["flt_max_read_outs"] >= 4, r
    assert r["nan_behind_inf_times_zero"] >= 16, r
    # an inf that is read out has passed fifteen units that were NaN in front of the ReLU: +0 behind it, or the read-out were NaN
    assert r["inf_means"] >= 4 and r["inf_values"] >= 4 and r["nan_read_outs"] >= 8 and r["finite_read_outs"] >= 16, r


def test_cancellation_scene_leaves_rounding_errors():
    sc, r = _scene("cancellation")
    assert r["pairs_small_and_nonzero"] >= 0.9 and min(r["groups_small_and_nonzero"]) >= 0.9, r
    assert r["positive_read_outs"] >= r["read_outs"] * 0.45, r
    assert E.CANCEL_INSIDE % 4 == 0 and E.CANCEL_ACROSS % 4 == 2


def test_ties_scene_takes_the_exact_path():
    sc, r = _scene("ties")
    assert r["exact_path_elements"] >= 32, r
    assert r["positive_read_outs"] == r["read_outs"], r
    assert r["normal_read_outs"] >= 32 and r["subnormal_read_outs"] >= 32, r
    # the constructor: x * c + b is the midpoint of two fp32 neighbours exactly (kinds 0, 2) or 2^-46 of a half ulp beside it (1, 3)
    c = [Fraction(float(v)) for v in sc.layers[1][0][0, 0]]
    kinds = {0: 0, 1: 0, 2: 0, 3: 0}
    for row in sc.obs.reshape(-1, 64):
        k = int(np.flatnonzero(row[1:5])[0]) + 1
        b, p = Fraction(float(row[0])), Fraction(float(row[k])) * c[k]
        ulp = Fraction(float(np.nextafter(row[0], f32(np.inf)))) - b
        for s in (b + p, b - p):
            off = (s / ulp) % 1 - Fraction(1, 2)
            assert (off == 0) if k in (1, 3) else (0 < abs(off) <= Fraction(1, 2 ** 46)), (k, row[0], row[k], off)
        kinds[k - 1] += 1
    assert min(kinds.values()) >= 16, kinds


def test_zeros_scene_reaches_negative_zero():
    sc, r = _scene("zeros")
    assert r["negative_zero_obs"] >= 64 and r["negative_zero_states"] >= 64 and r["negative_zero_into_relu"] >= 2, r
    assert r["negative_zero_means"] >= 4 and r["negative_zero_values"] >= 4 and r["positive_zero_means"] >= 4, r
    assert r["zero_row_is_the_bias_chain"], r
    assert (E.bits(sc.layers[0][1]) == 0x80000000).any() and (E.bits(sc.layers[1][1]) == 0x80000000).any()       # -0 biases in both layers


def test_isolation_scene_poisons_single_rows():
    sc, r = _scene("isolation")
    bad = ~np.isfinite(sc.obs)
    assert bad.sum() == len(E.POISON) and (bad.any(axis=2) == r["poisoned"]).all()
    assert sorted(i for a, i, _, _ in E.POISON if a == 0) == [0, 15, 16, 31]
    assert sc.sets[1] != sc.sets[0] and any(a == 1 for a, _, _, _ in E.POISON)
    # a NaN does not survive the ReLU (NaN > 0 is false: +0), so the NaN rows come out as the chain of the output biases over zero
    # activations -- the definition's clamp; the inf rows come out non-finite.  Either way they differ from the zeroed rows
    assert all(r["poisoned_rows_marked"]) and all(r["poisoned_rows_differ"]), r
    assert r["others_finite"] and r["others_equal_clean"], r


def test_epilogue_scene_reaches_every_corner():
    sc, r = _scene("epilogue")
    assert r["ls_raw_as_planned"] and r["limit"] > 0, r
    assert r["u_at_plus_limit"] and r["u_at_minus_limit"], r
    assert r["nan_u"] >= 7 and r["nan_u_clips_to_minus_limit"], r
    assert r["logp_minus_inf"] >= 3 * len(E.LS_CASES) and r["clamped_low"] >= 7 and r["clamped_high"] >= 7 and r["finite_means"] >= 40, r
    eps = sc.eps.reshape(-1)[:len(E.LS_CASES) * len(E.EPS_CASES)].reshape(len(E.LS_CASES), -1)
    assert all(E.same_bits(row, np.asarray(E.EPS_CASES, f32)) for row in eps)
    assert E.is_subnormal(f32(E.EPS_CASES[2]))


# ---- the trace is the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.SCENES))
def test_trace_equals_the_restatement(name):
    sc, _ = _scene(name)
    Ws, bs = E.restated(sc)
    t = E.scene_trace(sc)
    with np.errstate(all="ignore"):
        mean, ls_raw, value = PP.heads_reference(sc.obs, Ws, bs, sc.sets, *sc.heads)
        act = PS.actions_reference(sc.obs, Ws, bs, sc.sets)
    for got, want, what in ((t["mean"], mean, "mean"), (t["ls_raw"], ls_raw, "ls_raw"), (t["value"], value, "value"), (t["mean"], act, "actions")):
        assert E.same_bits(got, want), (name, what)
    for a, tr in enumerate(t["traces"]):                     # a trace ends in what the next layer reads
        Wa, ba = E.scene_sets(sc, a)
        h = PP.hidden_reference(sc.obs[a], Wa, ba)
        last = tr[len(Wa) - 2][-1]
        assert E.same_bits(np.where(last > 0, last, f32(0.0)), h), (name, a)


# ---- the judge: fmaf32 where an operand is inf or the sum overflows ----------------------------------------------------------------------------
def test_fmaf_follows_ieee_for_inf_nan_and_overflow():
    """compared as "NaN or equal bits" """
    inf, big, fmax = f32(np.inf), f32(3e38), E.FMAX
    cases = [  # (a, b, c, expected; None: NaN)
        (inf, 2.0, 1.0, inf), (inf, -2.0, 1.0, -inf), (-inf, 1e-45, -3e38, -inf), (3.0, inf, fmax, inf),
        (inf, 0.0, 1.0, None), (inf, -0.0, -inf, None), (0.0, -inf, 0.0, None),
        (big, 2.0, -inf, -inf), (big, big, -inf, -inf), (-big, 2.0, inf, inf),                  # a product past FLT_MAX is still finite: -inf wins
        (inf, 1.0, -inf, None), (-inf, 2.0, inf, None), (inf, -1.0, inf, None),
        (inf, 1.0, inf, inf), (np.nan, 0.0, 0.0, None), (1.0, 1.0, np.nan, None),
        (big, 2.0, -big, big), (2.0, big, 0.0, inf), (-2.0, big, 1.0, -inf),                    # overflow by the one rounding alone
        (fmax, 1.0, f32(2.0 ** 102), fmax), (fmax, 1.0, f32(2.0 ** 103), inf), (-fmax, 1.0, -f32(2.0 ** 103), -inf),
        # 2^-46 of half an ulp short of the midpoint between FLT_MAX and 2^128: the float64 sum sits on the midpoint, the sum does not
        (f32((1 + 2.0 ** -23) * 2.0 ** 51), f32((1 - 2.0 ** -23) * 2.0 ** 52), fmax, fmax),
        (f32((1 + 2.0 ** -23) * 2.0 ** 51), -f32((1 - 2.0 ** -23) * 2.0 ** 52), -fmax, -fmax)]
    a, b, c = (np.asarray([q[i] for q in cases], f32) for i in range(3))
    got = PS.fmaf32(a, b, c)
    for (x, y, z, want), g in zip(cases, got):
        if want is None:
            assert np.isnan(g), (x, y, z, g)
        else:
            assert E.same_bits(g, f32(want)), (x, y, z, g, want)
    fin = [q for q in cases if np.isfinite(np.asarray(q[:3], np.float64)).all()]
    for x, y, z, want in fin:                               # and the finite ones against exact rationals
        assert E.same_bits(PS.fma_exact(f32(x), f32(y), f32(z)), f32(want)), (x, y, z)


# ---- the scenes can tell ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fma,least", [("subnormal", E.fma_flushing, 0.1), ("cancellation", E.fma_unfused, 0.1), ("ties", E.fma_double_rounding, 32)],
                         ids=["subnormal_operands_flushed", "cancellation_unfused", "ties_double_rounding"])
def test_a_wrong_multiply_add_changes_the_read_outs(name, fma, least):
    sc, _ = _scene(name)
    right, wrong = E.read_outs(E.scene_trace(sc)), E.read_outs(E.scene_trace(sc, fma=fma))
    differ = int((E.bits(right) != E.bits(wrong)).sum())
    assert differ >= (least if least >= 1 else least * right.size), (name, differ, right.size)
