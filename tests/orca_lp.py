"""LP1 / LP2 / LP3 in the operation order of SURVEY App. A.5, restated in numpy fp64 (test infrastructure, beside
tests/orca_geometry.py, which states the same programme from the geometry), and what fp32 can do to that order.

Run on the fp32 half-planes the oracle captured, this is the reference for "is an answer off the speed disc the
algorithm's or the arithmetic's": the same operations without fp32 rounding.

fp32_limits(far, z): LP1 cuts line (point, dir) with the disc through disc = dp^2 + r^2 - |point|^2 and returns
point + t dir, t = -dp +- sqrt(disc) (or a t between the two).  With |dir| = 1 and exact arithmetic,
|point + t dir|^2 = r^2 + (disc used - disc true) at both ends, and less between them.  In fp32, with U = 2^-24 and
far = the largest |point| among the lines LP1 is given, to first order:
    dp = fl(fl(px dx) + fl(py dy))      is off by at most (sqrt 2 + 1) U far   (two products of total size <= sqrt 2 far, one sum)
    sqr(dp)                              by 2 |dp| times that + its own rounding:  <= 5.83 U far^2
    absSq(point)                         two products and a sum:                   <= 2 U far^2
    sqr(dp) + sqr(r)                     one sum of that size:                     <= 1 U far^2   (the last subtraction is exact enough)
    |dir|^2 - 1                          dir = normalize(..) in fp32: <= 5 U, times t^2 <= far^2:  <= 5 U far^2
so |v|^2 <= r^2 + delta, delta = 14 U far^2, plus the roundings of point + t dir itself (4 U far).  Lines of overlapping
agents lie 30 / s from the origin (delta = 8e-4); LP3's projected lines -- the intersection of two of them -- lie anywhere:
at far = 2 000 the limit is 2.1 maxSpeed, at 7e4 it is 65.  It passes 1 % at far = 155.
The largest penetration is 1-Lipschitz in the velocity and no point of the disc does better than the optimum z, so an answer
`over` outside the disc penetrates at least z - over.  Above the optimum there is no such one-sided argument: sqrt(disc) moves
by up to sqrt(delta) along the line when the true disc is near zero, so where delta lets the speed limit pass 1 % the
penetration may exceed the optimum by sqrt(delta); below that the by-value limit of the other families (5e-5 relative above
1) holds unchanged."""
import numpy as np

EPS = 1e-5                       # RVO_EPSILON
U32 = 2.0 ** -24                 # fp32 unit roundoff


def _det(a, b):
    return a[0] * b[1] - a[1] * b[0]


def lp1_f64(lines, k, radius, opt, dir_opt, slack=None):
    """App. A.5 LP1 on lines[k] = (point, dir) against lines[:k]; the new point, or None.  slack: a list that receives how far the
    outcome was from the other one -- the length of the interval left on the line, or by how much it came out empty."""
    note = (lambda x: slack.append(abs(float(x)))) if slack is not None else (lambda x: None)
    p, d = lines[k]
    dp = p @ d
    disc = dp * dp + radius * radius - p @ p
    if disc < 0.0:
        note(disc)
        return None
    sq = np.sqrt(disc)
    t_left, t_right = -dp - sq, -dp + sq
    for pj, dj in lines[:k]:
        den, num = _det(d, dj), _det(dj, p - pj)
        if abs(den) <= EPS:
            if num < 0.0:
                note(num)
                return None
            continue
        t = num / den
        if den >= 0.0:
            t_right = min(t_right, t)
        else:
            t_left = max(t_left, t)
        if t_left > t_right:
            note(t_left - t_right)
            return None
    note(t_right - t_left)
    if dir_opt:
        return p + (t_right if opt @ d > 0.0 else t_left) * d
    return p + min(max((opt - p) @ d, t_left), t_right) * d


def lp2_f64(lines, radius, opt, dir_opt, slack=None):
    """App. A.5 LP2: (index of the line it failed at, or len(lines); the point).  slack: a list that receives, for every line
    visited, the distance of its decision from the other outcome: how far the point lay inside the half-plane, or LP1's slack."""
    if dir_opt:
        res = opt * radius
    elif opt @ opt > radius * radius:
        res = opt / np.sqrt(opt @ opt) * radius
    else:
        res = opt.copy()
    for i, (p, d) in enumerate(lines):
        if _det(d, p - res) > 0.0:
            new = lp1_f64(lines, i, radius, opt, dir_opt, slack)
            if new is None:
                return i, res
            res = new
        elif slack is not None:
            slack.append(abs(float(_det(d, p - res))))
    return len(lines), res


def lp3_f64(lines, n_obst, begin, radius, res, slack=None):
    """App. A.5 LP3: (the point, the largest |point| among the projected lines it built).  slack: as in lp2_f64, for every decision
    of this call and of the LP2 calls it makes."""
    distance, far = 0.0, 0.0
    for i in range(begin, len(lines)):
        pi, di = lines[i]
        if slack is not None:
            slack.append(abs(float(_det(di, pi - res) - distance)))
        if _det(di, pi - res) > distance:
            proj = list(lines[:n_obst])
            for pj, dj in lines[n_obst:i]:
                d = _det(di, dj)
                if abs(d) <= EPS:
                    if di @ dj > 0.0:
                        continue
                    pt = 0.5 * (pi + pj)
                else:
                    pt = pi + (_det(dj, pi - pj) / d) * di
                nd = dj - di
                proj.append((pt, nd / np.sqrt(nd @ nd)))
                far = max(far, float(np.sqrt(pt @ pt)))
            fail, new = lp2_f64(proj, radius, np.array([-di[1], di[0]]), True, slack)
            if fail == len(proj):
                res = new
            distance = _det(di, pi - res)
    return res, far


def solve_published_f64(captured, n_obst, pref, vmax):
    """The call sequence of App. A.5 on captured lines [n, 4] = point, dir: (new velocity, infeasible?, far)."""
    lines = [(np.array(l[:2], np.float64), np.array(l[2:], np.float64)) for l in captured]
    fail, res = lp2_f64(lines, vmax, np.asarray(pref, np.float64), False)
    if fail == len(lines):
        return res, False, 0.0
    res, far = lp3_f64(lines, n_obst, fail, vmax, res)
    return res, True, far


def fp32_limits(far, z, vmax=1.0):
    """(speed above vmax, penetration below the optimum, penetration above it; the last two relative above 1) that fp32
    rounding of the published order can account for, given the largest |point| among the lines LP1 saw."""
    delta = 14 * U32 * far * far
    over = float(np.sqrt(vmax * vmax + delta)) - vmax + 4 * U32 * far + 1e-4
    rel = max(1.0, abs(z))
    above = 5e-5 + (float(np.sqrt(delta)) / rel if over > 0.01 * vmax + 1e-4 else 0.0)
    return over, 5e-5 + over / rel, above
