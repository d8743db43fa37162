// ca_nav_host.h -- the host side of the navigation fields (ca_nav_configure, ca_nav_mask_build): the grid's one cell expression, the
// cell centres and the blocked mask.  Plain C++, no HIP: libcaenv.so includes it, and so may a stand-alone program
// (tests/abi/nav_mask_main.cpp builds it under the address and undefined-behaviour sanitizers).
//
// The grid is the caller's: origin (x0, y0), cell size `cell`, gx x gy cells, ics = 1.0f / cell divided once on the host.
//     cell(v) = (int)fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1))            (fp32, every operation rounded once)
// is the edge grid's expression (ca_edge_grid_host.h, include/ca_env.h): a coordinate outside the box is clamped into the outermost
// cell.  The centre of column cx is x0 + ((float)cx + 0.5f) * cell, rows alike.
//
// Blocked mask: cell c is blocked iff some edge (p, q) has distSqPointSegment(p, q, centre(c)) < clearance * clearance, strictly,
// like touches_wall (ca_rules.h).  dist_sq_point_segment below is ca_math.h's function with the host's IEEE division, which is
// what div_ir returns on the device: the same bits.  Edges only, no inside test.
//
// The builder walks, per edge, only the cells of the edge's bounding box inflated by clearance + m and one cell more per side; every
// other cell fails the test for that edge.  Why: the function returns absSq(fl(c - z)) for a point z within 5 u M per axis of the true
// segment (the argument of ca_edge_grid_host.h, u = 2^-24, M the largest absolute coordinate involved), absSq and the square of the
// clearance carry relative errors of 4 u and u, and an fp32 centre lies within 2 u M of x0 + (cx + 0.5) cell.  So a centre that passes
// lies within clearance (1 + 3 u) + 7 u M of the edge's box per axis; m = 32 u (M + clearance) covers that, the rectangle is computed in
// double, and the extra cell per side covers the rounding of that computation.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace ca_nav {

enum { MAX_SIDE = 256,         // cells per axis
       MAX_CELLS = 32768,      // cells per grid: 128 KiB of fp32 distances + 4 KiB of mask bits in one workgroup's LDS
       MAX_GOALS = 16,
       MAX_LOOKAHEAD = 8,
       STAY = 8,               // `next` of the source cell
       NONE = 9 };             // `next` of a cell nothing leads out of

// the one cell expression (see above)
inline int cell(float v, float x0, float ics, int g) { return (int)fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1)); }
inline float centre(float x0, int c, float cs) { return x0 + ((float)c + 0.5f) * cs; }

// ca_math.h distSqPointSegment(a, b, c), operation for operation
inline float dist_sq_point_segment(float ax, float ay, float bx, float by, float cx, float cy) {
    const float ex = bx - ax, ey = by - ay, fx = cx - ax, fy = cy - ay;
    const float r = (fx * ex + fy * ey) / (ex * ex + ey * ey);
    if (r < 0.0f) return fx * fx + fy * fy;
    if (r > 1.0f) { const float gx = cx - bx, gy = cy - by; return gx * gx + gy * gy; }
    const float hx = cx - (ax + r * ex), hy = cy - (ay + r * ey);
    return hx * hx + hy * hy;
}

inline bool grid_ok(int gx, int gy) { return gx >= 1 && gy >= 1 && gx <= MAX_SIDE && gy <= MAX_SIDE && gx * gy <= MAX_CELLS; }

// blocked[gx * gy] (one byte per cell, 0 / 1) for the n edges pq[n][4] = (px, py, qx, qy)
inline void mask_build(const float* pq, int n, float x0, float y0, float cs, int gx, int gy, float clearance, uint8_t* blocked) {
    memset(blocked, 0, (size_t)gx * (size_t)gy);
    const float c2 = clearance * clearance;
    if (!(c2 > 0.0f)) return;   // (a squared distance is never below zero)
    double M = fmax(fabs((double)x0) + (double)gx * (double)cs, fabs((double)y0) + (double)gy * (double)cs);
    for (int k = 0; k < 4 * n; ++k) M = fmax(M, fabs((double)pq[k]));
    const double reach = (double)clearance + 32.0 * (M + (double)clearance) / 16777216.0;
    for (int e = 0; e < n; ++e) {
        const float* s = pq + 4 * e;
        int lo[2], hi[2];
        for (int ax = 0; ax < 2; ++ax) {   // centre index c passes only if o + (c + 0.5) cs lies in [lo - reach, hi + reach]
            const double o = (double)(ax ? y0 : x0), g = (double)(ax ? gy : gx);
            const double a = (fmin((double)s[ax], (double)s[2 + ax]) - reach - o) / (double)cs - 0.5;
            const double b = (fmax((double)s[ax], (double)s[2 + ax]) + reach - o) / (double)cs - 0.5;
            const double fa = floor(a) - 1.0, cb = ceil(b) + 1.0;
            lo[ax] = !(fa > 0.0) ? 0 : (fa > g ? (int)g : (int)fa);      // (a NaN takes the whole axis)
            hi[ax] = !(cb < g - 1.0) ? (int)g - 1 : (cb < -1.0 ? -1 : (int)cb);
        }
        for (int cy = lo[1]; cy <= hi[1]; ++cy) {
            const float py = centre(y0, cy, cs);
            for (int cx = lo[0]; cx <= hi[0]; ++cx)
                if (dist_sq_point_segment(s[0], s[1], s[2], s[3], centre(x0, cx, cs), py) < c2) blocked[(size_t)cy * gx + cx] = 1;
        }
    }
}

}  // namespace ca_nav
