"""The observation kernel's chord selection without a device (collision_avoidance_amd/csrc/ca_obs_chord.h; CA_OBS_ENTRY_CHORD in
ca_obs.h): a (neighbour, ray) pair whose agent is outside the neighbour's circle (d^2 > 1.0404 R^2) and whose ray's line passes no
vertex of the octagon within the filter's tolerance is decided by the chord the ray ENTERS the octagon by.

tests/abi/obs_chord_main.cpp, a host program with its own main, sends every case the way a lane of phase A's pair loop goes,
through the header's own functions.  The expected winner is a numpy fp32 restatement, written for this test, of the reference's
accept test and distance (utils.py:14-38) over ALL eight chords of the octagon (env.py:335-350), first minimum.  Cases: random
pairs from 0.2 R to beyond the range, a vertex placed within 1e-9 .. 1e-2 of a ray's line on either side (corner cuts among them),
agents inside the octagon, agents between the octagon and its circle, rays that end inside the octagon."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from collision_avoidance_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
RANGE = 5.0
RADII = (0.5, 0.25, 0.3, 0.75, 1.0, 0.05)
N_RANDOM, N_ADVERSARIAL, N_EACH_SPECIAL = 1050000, 320000, 20000


def f32(x):
    return np.asarray(x, dtype=F)


def _octagon(R):
    """vertex e of the octagon of the fp32 radius R: fp64, then rounded once (env.py:335-350)"""
    ang = np.arange(8) * (2.0 * np.pi / 8)
    return f32(float(R) * np.cos(ang)), f32(-(float(R) * np.sin(ang)))


def _rays():
    ang = np.arange(16) * (2.0 * np.pi / 16)
    return f32(RANGE * np.cos(ang)), f32(-RANGE * np.sin(ang))   # env.py:321-332


def _frame_to_world(th, px, py):
    """the point (px, py) of the agent's frame, in world axes relative to the agent: the frame turns the world by th"""
    ct, st = np.cos(th), np.sin(th)
    return ct * px + st * py, -st * px + ct * py


def _cases():
    """(cos, sin, rx, ry, R, ray index) of every case and the slice of each family"""
    rng = np.random.RandomState(20)
    parts, names = [], []

    def add(name, th, wx, wy, R, ray):
        parts.append((f32(np.cos(th)), f32(np.sin(th)), f32(wx), f32(wy), f32(R), np.asarray(ray, np.int64)))
        names.append((name, len(th)))

    def draw(M):
        return rng.uniform(0, 2 * np.pi, M), rng.randint(0, 16, M), np.asarray(RADII)[rng.randint(0, len(RADII), M)]

    # random pairs: the neighbour 0.2 R .. 5.8 from the agent, mostly near the ray's direction (elsewhere no chord survives)
    M = N_RANDOM
    th, ray, R = draw(M)
    d = np.where(rng.rand(M) < 0.3, rng.uniform(0.2, 2.4, M) * R, rng.uniform(0.5, RANGE + 0.8, M))
    half = np.arcsin(np.minimum(1.0, R / d))
    off = np.where(rng.rand(M) < 0.85, rng.uniform(-1.3, 1.3, M) * half, rng.uniform(-np.pi, np.pi, M))
    a = -ray * (2 * np.pi / 16) + off                       # ray i points along (cos, -sin)(i 2 pi / 16)
    add("random", th, *_frame_to_world(th, d * np.cos(a), d * np.sin(a)), R, ray)

    # adversarial: vertex e at u along the ray and delta beside its line
    M = N_ADVERSARIAL
    th, ray, _ = draw(M)
    ri = rng.randint(0, len(RADII), M)
    R = np.asarray(RADII)[ri]
    e = rng.randint(0, 8, M)
    u = rng.uniform(0.05, RANGE + 0.3, M)
    delta = 10.0 ** rng.uniform(-9, -2, M) * rng.choice([-1.0, 1.0], M)
    dx, dy = np.cos(ray * 2 * np.pi / 16), -np.sin(ray * 2 * np.pi / 16)
    wx, wy = _frame_to_world(th, u * dx - delta * dy, u * dy + delta * dx)
    vx = np.stack([_octagon(F(r))[0] for r in RADII]).astype(np.float64)
    vy = np.stack([_octagon(F(r))[1] for r in RADII]).astype(np.float64)
    add("adversarial", th, wx - vx[ri, e], wy - vy[ri, e], R, ray)

    M = N_EACH_SPECIAL
    th, ray, R = draw(M)                                    # the agent inside the octagon (its inradius is 0.924 R)
    d, a = rng.uniform(0.0, 0.9, M) * R, rng.uniform(0, 2 * np.pi, M)
    add("inside", th, d * np.cos(a), d * np.sin(a), R, ray)
    th, ray, R = draw(M)                                    # between the octagon and its circle: off the middle of a chord
    d = rng.uniform(0.93, 1.0, M) * R
    a = (rng.randint(0, 8, M) + 0.5) * (np.pi / 4) + rng.uniform(-0.05, 0.05, M)
    add("between", th, d * np.cos(a), d * np.sin(a), R, ray)
    th, ray, R = draw(M)                                    # just outside the circle, either side of the pre-pass's 2 % bound
    d, a = rng.uniform(0.99, 1.06, M) * R, rng.uniform(0, 2 * np.pi, M)
    add("rim", th, d * np.cos(a), d * np.sin(a), R, ray)
    th, ray, R = draw(M)                                    # the ray ends inside the octagon
    d = RANGE + rng.uniform(-0.9, 0.9, M) * R
    a = -ray * (2 * np.pi / 16) + rng.uniform(-0.5, 0.5, M) * R / RANGE
    add("ray end", th, *_frame_to_world(th, d * np.cos(a), d * np.sin(a)), R, ray)

    cols = [np.concatenate([p[i] for p in parts]) for i in range(6)]
    edges = np.cumsum([0] + [n for _, n in names])
    return cols, {name: slice(edges[i], edges[i + 1]) for i, (name, _) in enumerate(names)}


def _brute_force(c, s, rx, ry, R, s10x, s10y):
    """the reference's test of all eight chords in the agent's frame, fp32, no fused operations: (winning chord or -1, accepted)"""
    n = len(c)
    vx, vy = np.zeros((8, n), F), np.zeros((8, n), F)
    for r in RADII:
        m = R == F(r)
        ox, oy = _octagon(F(r))
        vx[:, m], vy[:, m] = ox[:, None], oy[:, None]
    best, bm, oks = np.full(n, np.inf, F), np.full(n, -1), []
    for e in range(8):
        x1, y1, x2, y2 = vx[e] + rx, vy[e] + ry, vx[(e + 1) % 8] + rx, vy[(e + 1) % 8] + ry      # env.py:305-315
        r1x, r1y, r2x, r2y = c * x1 - s * y1, s * x1 + c * y1, c * x2 - s * y2, s * x2 + c * y2  # utils.py:59-60
        s32x, s32y, s02x, s02y = r2x - r1x, r2y - r1y, F(0) - r1x, F(0) - r1y
        tn = s32x * s02y - s32y * s02x                                                           # utils.py:26
        den = s10x * s32y - s32x * s10y                                                          # utils.py:14
        sn = s10x * s02y - s10y * s02x                                                           # utils.py:21
        dpos = den > 0
        ok = (den != 0) & ((sn < 0) != dpos) & ((tn < 0) != dpos) & ((sn > den) != dpos) & ((tn > den) != dpos)
        with np.errstate(all="ignore"):
            t = tn / den                                                                         # utils.py:34
        hx, hy = F(0) + t * s10x, F(0) + t * s10y
        dd = np.where(ok, np.sqrt(hx * hx + hy * hy), np.inf).astype(F)                          # utils.py:38
        upd = dd < best                                                                          # strict: the first minimum
        best, bm = np.where(upd, dd, best), np.where(upd, e, bm)
        oks.append(ok)
    return bm, np.array(oks)


def _cross(c, s, rx, ry, R, s10x, s10y):
    """cr[v] = ray x vertex v and the tolerance, as the filter forms them (ca_obs_chord.h)"""
    wx, wy = c * s10x + s * s10y, c * s10y - s * s10x
    wb = wx * ry - wy * rx
    Rh = F(0.70710678) * R
    c0, c2, c1, c3 = R * wy, R * wx, Rh * (wx + wy), Rh * (wy - wx)
    tol = F(2e-5) * F(RANGE) * (F(RANGE) + F(2.0) * R + F(1.0))
    return np.stack([wb - c0, wb - c1, wb - c2, wb + c3, wb + c0, wb + c1, wb + c2, wb - c3]), tol


def _compiler():
    for name in ("g++", "c++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    return os.path.join(os.path.dirname(os.path.realpath(B.hipcc())), "..", "lib", "llvm", "bin", "clang++")


def _compile(exe, extra=()):
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(B.hipcc()))), "include")   # ca_math.h includes hip_runtime.h
    cmd = [_compiler(), "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", inc,
           "-I", os.path.join(ROOT, "collision_avoidance_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "abi", "obs_chord_main.cpp")]
    return cmd + list(extra)


def _run(exe, rec, tmp, tag, env=None):
    src, dst = os.path.join(tmp, tag + ".f32"), os.path.join(tmp, tag + ".i8")
    np.ascontiguousarray(rec, F).tofile(src)
    r = subprocess.run([exe, src, dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "OBS_CHORD_OK" in r.stdout, r.stdout[-4000:]
    out = np.fromfile(dst, np.int8).reshape(-1, 4)
    os.remove(src)
    return out, r.stdout


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("obs_chord"))
    exe = os.path.join(tmp, "obs_chord_main")
    r = subprocess.run(_compile(exe, ["-O2"]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    (c, s, rx, ry, R, ray), fam = _cases()
    rayx, rayy = _rays()
    s10x, s10y = rayx[ray], rayy[ray]
    rec = np.stack([c, s, rx, ry, R, s10x, s10y, np.full(len(c), RANGE, F)], axis=1)
    out, log = _run(exe, rec, tmp, "all")
    assert len(out) == len(rec)
    bm, ok = _brute_force(c, s, rx, ry, R, s10x, s10y)
    cr, tol = _cross(c, s, rx, ry, R, s10x, s10y)
    d2 = rx * rx + ry * ry
    return dict(tmp=tmp, exe=exe, rec=rec, fam=fam, fast=out[:, 0] == 1, chord=out[:, 1].astype(np.int64), acc=out[:, 2].view(np.uint8),
                first=out[:, 3].astype(np.int64), bm=bm, ok=ok, cr=cr, tol=tol, outside=d2 > F(1.0404) * R * R, log=log)


def test_the_families_are_what_they_claim(world):
    w, fam = world, world["fam"]
    assert fam["random"].stop - fam["random"].start >= 1000000 and fam["adversarial"].stop - fam["adversarial"].start >= 300000
    nsurv = np.unpackbits(w["acc"][:, None], axis=1).sum(axis=1)
    adv = fam["adversarial"]
    hmin = np.abs(w["cr"][:, adv]).min(axis=0)
    assert (hmin < 1e-6).sum() > 20000 and (hmin > 1e-3).sum() > 20000, "vertex offsets from 1e-9 to 1e-2 of a ray's line"
    # corner cuts: the two crossings on the two chords that meet in one vertex, both accepted by the reference
    both = w["ok"][:, adv].sum(axis=0) == 2
    adjacent = (w["ok"][:, adv] & np.roll(w["ok"][:, adv], -1, axis=0)).any(axis=0)
    assert (both & adjacent).sum() > 20000 and (both & adjacent & w["fast"][adv]).sum() > 1000, "corner cuts, on the fast path too"
    assert not w["outside"][fam["inside"]].any() and not w["outside"][fam["between"]].any()
    assert w["outside"][fam["rim"]].any() and not w["outside"][fam["rim"]].all()
    assert not w["fast"][fam["inside"]].any() and not w["fast"][fam["between"]].any()
    assert (w["bm"][fam["inside"]] >= 0).mean() > 0.9, "from inside the octagon nearly every ray leaves through a chord"
    end = fam["ray end"]                                     # the ray enters and ends inside: one chord accepted, the exit chord is not
    assert ((w["ok"][:, end].sum(axis=0) == 1) & (nsurv[end] >= 2) & w["fast"][end]).sum() > 1000
    assert (nsurv >= 3).sum() > 1000, "grazed vertices: three survivors"


def test_fast_path_winner_is_the_brute_force_winner(world):
    w = world
    fast, two = w["fast"], w["fast"] & (w["acc"] != 0)
    print(w["log"].strip(), "| fast with two survivors:", int(two.sum()), "| both chords accepted by the reference:",
          int((two & (w["ok"].sum(axis=0) == 2)).sum()))
    bad = fast & (w["chord"] != w["bm"])
    assert bad.sum() == 0, "%d fast cases differ, first records: %s" % (bad.sum(), w["rec"][bad][:5])
    assert fast.sum() > 1000 and (~fast).sum() > 1000 and two.sum() > 1000, (fast.sum(), (~fast).sum(), two.sum())
    assert (two & (w["ok"].sum(axis=0) == 2)).sum() > 1000, "pairs in which the reference accepts the exit chord as well"
    assert (two & (w["bm"] < 0)).sum() > 1000, "pairs whose entry chord is rejected: no hit"


def test_slow_path_winner_is_the_brute_force_winner(world):
    w = world
    bad = ~w["fast"] & (w["chord"] != w["bm"])
    assert bad.sum() == 0, "%d slow cases differ, first records: %s" % (bad.sum(), w["rec"][bad][:5])


def test_every_qualifying_case_takes_the_fast_path_and_no_other(world):
    w = world
    strict = (np.abs(w["cr"]) > w["tol"]).all(axis=0)
    qualifies = w["outside"] & strict
    assert (w["fast"] == qualifies).all(), (int((w["fast"] & ~qualifies).sum()), int((~w["fast"] & qualifies).sum()))
    assert (qualifies & ~w["outside"]).sum() == 0 and (strict & ~w["outside"]).sum() > 1000 and (~strict & w["outside"]).sum() > 1000


def test_the_entry_chord_is_the_survivor_the_line_crosses_upwards(world):
    """fast: none or two survivors, and the chord tested first is the one with cr[e + 1] - cr[e] > 0"""
    w = world
    cr, tol = w["cr"], w["tol"]
    surv = np.stack([~(((cr[e] > tol) & (cr[(e + 1) % 8] > tol)) | ((cr[e] < -tol) & (cr[(e + 1) % 8] < -tol))) for e in range(8)])
    acc = (surv * (1 << np.arange(8))[:, None]).sum(axis=0)
    assert (acc == w["acc"]).all()
    n = surv.sum(axis=0)
    fast = w["fast"]
    assert set(np.unique(n[fast])) == {0, 2}
    two = fast & (n == 2)
    up = surv & (np.roll(cr, -1, axis=0) - cr > 0)
    assert (up[:, two].sum(axis=0) == 1).all()
    assert (w["first"][two] == up[:, two].argmax(axis=0)).all()
    slow = ~fast & (n > 0)
    assert (w["first"][slow] == surv[:, slow].argmax(axis=0)).all() and (w["first"][n == 0] == -1).all()


def test_program_under_address_and_undefined_sanitizers(world):
    """the stand-alone program, once, on a sample of every family: clean, and the answers of the plain build"""
    exe = os.path.join(world["tmp"], "obs_chord_main_san")
    cmd = _compile(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cmd[0]) else ["-static-libsan"]
    r = subprocess.run(cmd + static, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|libclang_rt", r.stdout):
        pytest.skip("the host compiler lacks the sanitizer runtime: " + r.stdout[-300:])
    assert r.returncode == 0, r.stdout[-4000:]
    pick = np.concatenate([np.arange(sl.start, sl.stop)[::max(1, (sl.stop - sl.start) // 4000)] for sl in world["fam"].values()])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out, log = _run(exe, world["rec"][pick], world["tmp"], "san", env=env)
    assert "AddressSanitizer" not in log and "runtime error:" not in log, log[-4000:]
    assert (out[:, 0] == world["fast"][pick]).all() and (out[:, 1] == world["chord"][pick]).all()
