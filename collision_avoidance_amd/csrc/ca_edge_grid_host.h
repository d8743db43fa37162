// ca_edge_grid_host.h -- the static uniform grid over the obstacle edges of one table (ca_tiled_edge_grid, ca_edge_grid_build):
// the host-side builder.  Plain C++, no HIP: libcaenv.so includes it, and so may a stand-alone program (tests/abi/edge_grid_main.cpp
// builds it under the address and undefined-behaviour sanitizers).
//
// Edges do not move, so the index is built once when a table is installed.  The table is UNWRAPPED and bounded: it covers the
// bounding box of the edges, and a coordinate outside it (or a NaN) is clamped into the outermost cell --
//     cell(v) = (int)fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1))            (fp32, every operation rounded once)
// which is the expression of include/ca_env.h and of ca_tiled.h's edge_cell: all three are this one line.  It is monotone in v
// (a subtraction of a constant, a product with a positive constant, floor, clamp), and monotone is all the argument needs.
//
// An edge is registered in every cell of the rectangle cell(fl_down(lo - m)) .. cell(fl_up(hi + m)) per axis, lo / hi its smaller /
// larger end coordinate and m the margin below.  An agent at x with obstacle range R walks cell(fl(x - R)) .. cell(fl(x + R)).
//
// No miss (DESIGN.md 7g has the long form).  u = 2^-24.  Let an edge pass ca_math.h's distSqPointSegment(a, b, p) < fl(R * R)
// in fp32.  Whatever branch the function took, it returned absSq(fl(p - q)) for a point q that is a, b or fl(a + fl(r * fl(b - a)))
// with 0 <= r <= 1.  (i) absSq and the square of R carry relative errors of at most 4 u and u, so |p - q| < R (1 + 3 u).  (ii) q
// differs per axis from the point q* = a + r (b - a) of the true segment by at most 2 u |b - a| + u |q| <= 5 u M, M the largest
// absolute end coordinate of the table.  So per axis |p - q*| < R (1 + 3 u) + 5 u M, and q* lies inside the edge's box: lo <= q* <= hi.
// (iii) fl(x -+ R) differs from x -+ R by at most u (|x| + R) <= u (M + 3 R).  Together: fl(x - R) <= hi + s and fl(x + R) >= lo - s
// with s = u (6 M + 7 R), and with m >= s the monotone cell function puts the agent's lowest cell at or below the edge's highest
// and the other way round: the two rectangles intersect.  The margin is 16 u (M + R), computed in double and rounded outwards.
//
// No duplicate: an entry carries the low corner of its edge's rectangle, and the walk takes an edge only in the cell
// (max(edge_lo_col, agent_lo_col), max(edge_lo_row, agent_lo_row)) -- the low corner of the intersection of the two rectangles.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace ca_edge_grid {

enum { MAX_SIDE = 256,            // cells per axis: a cell coordinate fits 8 bits
       MAX_EDGES = 65535,         // edges per table: an edge id fits 16 bits and 0xFFFF stays free
       MAX_ENTRIES = 1 << 22 };   // entries per table (16 MiB): long diagonal walls inflate the table -- subdivide them

struct Desc {   // (the layout of ca_edge_grid_desc, include/ca_env.h)
    float x0, y0, ics_x, ics_y;
    int32_t gx, gy, n_entries;
    float margin;
};

enum Result { OK = 0, BAD_RANGE = 1, TOO_MANY_EDGES = 2, TOO_MANY_ENTRIES = 3 };

// the one cell expression (see above)
inline int cell(float v, float x0, float ics, int g) { return (int)fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1)); }

inline float round_down(double v) { const float f = (float)v; return (double)f <= v ? f : nextafterf(f, -INFINITY); }
inline float round_up(double v) { const float f = (float)v; return (double)f >= v ? f : nextafterf(f, INFINITY); }

struct Rect { int c0, c1, r0, r1; };

inline double margin_of(const float* pq, int n, float range) {
    double M = 0.0;
    for (int k = 0; k < 4 * n; ++k) M = fmax(M, fabs((double)pq[k]));
    return 16.0 * (M + (double)range) / 16777216.0;
}

// one axis of the table: origin, reciprocal cell size, side
inline void axis_of(double lo, double hi, float range, float* x0, float* ics, int32_t* g) {
    *x0 = round_down(lo);
    const double extent = (double)round_up(hi) - (double)*x0;
    const double cs = fmax((double)range, extent / MAX_SIDE);
    *ics = (float)(1.0 / cs);
    const double side = ceil(extent / cs);
    *g = side < 1.0 ? 1 : (side > MAX_SIDE ? MAX_SIDE : (int32_t)side);
}

inline Rect rect_of(const float* e, const Desc& d, double m) {
    Rect r;
    r.c0 = cell(round_down(fmin((double)e[0], (double)e[2]) - m), d.x0, d.ics_x, d.gx);
    r.c1 = cell(round_up(fmax((double)e[0], (double)e[2]) + m), d.x0, d.ics_x, d.gx);
    r.r0 = cell(round_down(fmin((double)e[1], (double)e[3]) - m), d.y0, d.ics_y, d.gy);
    r.r1 = cell(round_up(fmax((double)e[1], (double)e[3]) + m), d.y0, d.ics_y, d.gy);
    return r;
}

// The table of n edges pq[n][4] = (px, py, qx, qy) for obstacle range `range`.  Fills d; with cell_start != nullptr also
// cell_start[gx * gy + 1] and entries[d.n_entries] (CSR; an entry = edge id | lowest column << 16 | lowest row << 24).  A refusal
// leaves the vectors alone; d then says what was refused (n_entries: the count that broke the cap).
inline Result build(const float* pq, int n, float range, Desc& d, std::vector<uint32_t>* cell_start, std::vector<uint32_t>* entries) {
    d = Desc{0.0f, 0.0f, 1.0f, 1.0f, 1, 1, 0, 0.0f};
    if (!(range > 0.0f) || !(range <= 3.0e38f)) return BAD_RANGE;
    if (n > MAX_EDGES) return TOO_MANY_EDGES;
    const double m = margin_of(pq, n, range);
    d.margin = round_up(m);
    d.ics_x = d.ics_y = (float)(1.0 / (double)range);
    if (n > 0) {
        double lo[2] = {(double)pq[0], (double)pq[1]}, hi[2] = {lo[0], lo[1]};
        for (int k = 0; k < 4 * n; ++k) {   // (pq[k]: x of an end point for even k, y for odd k)
            lo[k & 1] = fmin(lo[k & 1], (double)pq[k]);
            hi[k & 1] = fmax(hi[k & 1], (double)pq[k]);
        }
        axis_of(lo[0] - m, hi[0] + m, range, &d.x0, &d.ics_x, &d.gx);
        axis_of(lo[1] - m, hi[1] + m, range, &d.y0, &d.ics_y, &d.gy);
    }
    const size_t cells = (size_t)d.gx * d.gy;
    uint64_t total = 0;
    for (int e = 0; e < n; ++e) {
        const Rect r = rect_of(pq + 4 * e, d, m);
        total += (uint64_t)(r.c1 - r.c0 + 1) * (uint64_t)(r.r1 - r.r0 + 1);
    }
    d.n_entries = total > 0x7FFFFFFFull ? 0x7FFFFFFF : (int32_t)total;
    if (total > (uint64_t)MAX_ENTRIES) return TOO_MANY_ENTRIES;
    if (!cell_start || !entries) return OK;
    std::vector<uint32_t> start(cells + 1, 0u), ent((size_t)total);
    for (int e = 0; e < n; ++e) {
        const Rect r = rect_of(pq + 4 * e, d, m);
        for (int y = r.r0; y <= r.r1; ++y)
            for (int x = r.c0; x <= r.c1; ++x) ++start[(size_t)y * d.gx + x + 1];
    }
    for (size_t c = 0; c < cells; ++c) start[c + 1] += start[c];
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (int e = 0; e < n; ++e) {   // (edges in id order: a cell's run is sorted by id)
        const Rect r = rect_of(pq + 4 * e, d, m);
        const uint32_t w = (uint32_t)e | ((uint32_t)r.c0 << 16) | ((uint32_t)r.r0 << 24);
        for (int y = r.r0; y <= r.r1; ++y)
            for (int x = r.c0; x <= r.c1; ++x) ent[fill[(size_t)y * d.gx + x]++] = w;
    }
    cell_start->swap(start);
    entries->swap(ent);
    return OK;
}

}  // namespace ca_edge_grid
