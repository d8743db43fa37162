// ca_obs_chord.h -- which chords of a neighbour's octagon phase A of obs_kernel (ca_obs.h) sends through the reference's arithmetic
// Part of the HIP kernels of libcaenv.so.  Host and device forms are the same fixed sequences of single IEEE operations, so a host
// program (tests/abi/obs_chord_main.cpp) calls exactly what the kernel calls.
#pragma once
#include "ca_math.h"

namespace ca {

// The filter's tolerance, in the units of cr (|ray| x distance): 100x the rounding error of the cross products below.
// range = rays[0] = neighbor_dist (env.py:321-332), R the radius of the SOURCE's octagon.
CA_HD float obs_chord_tol(float range, float R) { return 2e-5f * range * (range + 2.0f * R + 1.0f); }

// cr[v] = ray x vertex v of the octagon of radius R centred at (rx, ry) from the agent, v = 0 .. 7, in the WORLD frame, where the
// octagon's vertices are constants: ray_w x (oct_v + rel) with ray_w the ray (s10x, s10y) turned back by the agent's frame
// (fc, fs) = (cos, sin) -- no vertex is rotated.  Vertex v is R (cos v pi/4, -sin v pi/4) (env.py:335-350) and vertex v + 4 its mirror
// image, so the eight cross products are four, each added to and subtracted from the ray x centre term.  (= -s_numer of chord v,
// utils.py:21, up to rounding: a filter's value, never a result.)
CA_HD void obs_chord_cross(float fc, float fs, float rx, float ry, float s10x, float s10y, float R, float (&cr)[8]) {
    const float wx = fc * s10x + fs * s10y, wy = fc * s10y - fs * s10x;
    const float wb = wx * ry - wy * rx;
    const float Rh = 0.70710678f * R;
    const float c0 = R * wy, c2 = R * wx, c1 = Rh * (wx + wy), c3 = Rh * (wy - wx);
    cr[0] = wb - c0; cr[1] = wb - c1; cr[2] = wb - c2; cr[3] = wb + c3;
    cr[4] = wb + c0; cr[5] = wb + c1; cr[6] = wb + c2; cr[7] = wb - c3;
}

struct ChordSel {
    unsigned acc;   // the surviving chords, bit e = chord e (vertex e to vertex e + 1)
    unsigned rest;  // what is left to test behind `first`: acc without `first`, and nothing at all on the fast path
    int first;      // the chord to test first: the entry chord on the fast path, else the lowest survivor (-1: none)
    bool fast;      // the entry chord decides the pair
};

// The selection rule of a (neighbour, ray) pair.
//
// Survivors.  The exact test needs the crossing parameter along the chord, s_numer / denom (utils.py:21-31), inside [0, 1], i.e. the
// ray's LINE must separate the chord's end points: a chord whose two end points lie on the same side of the line by more than `tol`
// cannot be accepted.  The others survive -- the chord the line enters the octagon by and the one it leaves by, a third one when
// the line grazes a vertex.
//
// The fast path.  A pair qualifies iff
//   (a) the agent lies outside the neighbour's circle by the pre-pass's bound, d2 > 1.0404 R^2 (so outside the octagon), and
//   (b) no vertex has |cr[v]| <= tol: each of the eight is strictly on one side of the ray's line.
// Going round a convex polygon the side changes twice or never (the rounding of cr, ~1e-6 R |ray|, is 1/100 of tol and cannot fake
// a third change between vertices that are more than tol off the line), so exactly two chords survive, or none.  Both crossings
// are on the same ray, and the agent is outside: the exit crossing lies FURTHER along the ray by the length of the path through the
// octagon, and every condition of the accept test that fails for the entry chord (the crossing behind the origin or beyond the
// ray's end; its place ALONG the chord is settled by (b)) fails for the exit chord too.  So the entry chord is the pair's
// first minimum if it is accepted, and otherwise the pair has no hit: the exit chord need not be built at all.
//   The margin: a line that passes a vertex (interior angle 135 degrees) at distance h cuts a corner on a path of at least
// 2 h tan 67.5 = 4.8 h, and any other path through the octagon is longer; 0.83 h is what is relied on.  With (b), h > tol / |ray|
// = 1.4e-4 at range 5 and R = 0.5, a path of more than 1.2e-4, while t = t_numer / denom, the two products and the square root of
// utils.py:34-38 round a distance of at most range + R by a few ulp, ~2e-6: a factor of 50.  (A ray at a small angle th to its entry
// chord has a crossing that is th times less certain, and a path of at least h / th: the factor stays.)  The rounded distances
// of the two chords can therefore neither tie nor change order, which is all that a first-minimum scan could tell them apart by.
//
// The entry chord is the survivor e with cr[e + 1] - cr[e] > 0, the one the line crosses from the negative side to the positive:
// cr[e] < -tol and cr[e + 1] > tol.  Vertex 0 is never strictly between the two survivors lo < hi (the vertices lo + 1 .. hi are),
// so it has the sign of vertex lo: lo is the entry chord iff cr[0] < -tol, else hi is.  One comparison that the masks already hold.
CA_HD ChordSel obs_chord_select(const float (&cr)[8], float tol, float d2, float R) {
    unsigned acc = 0;
    bool strict = true;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float ca = cr[e], cb = cr[(e + 1) & 7];
        const bool same_side = (ca > tol && cb > tol) || (ca < -tol && cb < -tol);
        acc |= same_side ? 0u : (1u << e);
        strict = strict && (ca > tol || ca < -tol);
    }
    ChordSel cs;
    cs.acc = acc;
    cs.fast = strict && d2 > 1.0404f * R * R;
    const unsigned above = acc & (acc - 1u);                      // the survivors above the lowest
    const int lo = __builtin_ffs((int)acc) - 1, hi = __builtin_ffs((int)above) - 1;
    cs.first = (cs.fast && !(cr[0] < -tol)) ? hi : lo;
    cs.rest = cs.fast ? 0u : above;
    return cs;
}

}  // namespace ca
