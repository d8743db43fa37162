// ca_contact.h -- the per-agent contact report (ca_contacts, CA_F_CONTACT): who touches whom, nearest neighbour, walls
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview and the numerics contract).
//
// For every agent i of every arena, from the state a call leaves (include/ca_env.h ca_get_contacts has the table):
//   agents     the other present agents j of its arena with absSq(p_i - p_j) < sqr(r_i + r_j)
//   wall       1 if distSqPointSegment(edge, p_i) < sqr(r_i) for any edge of the arena's processed table
//   nearest    the j != i with the smallest key (absSq(p_i - p_j), j), or -1;  nearest_d2 that distance, or +inf
//   wall_d2    the smallest distSqPointSegment over the arena's edges, or +inf
// in the operations and the order of the oracle's arena_collisions, so that over an arena `agents` sums to twice the pairs a solve
// kernel counts under CA_F_STATS and `wall` to its wall hits.  A pure function of positions, radii, per-arena counts and the obstacle
// tables: a kernel of its own, enqueued behind the launches of a step like the observation and the record kernel -- the solve
// kernels are not touched.
//
// One kernel text for every handle.  One lane per agent, CONTACT_BS lanes per workgroup:
//   * an arena of more than CONTACT_BS agents spans ceil(N / CONTACT_BS) workgroups;
//   * arenas of at most CONTACT_BS agents are packed floor(CONTACT_BS / N) to a workgroup, back to back (the reference's own shape
//     is 16384 arenas of 10 agents: a workgroup per arena would idle five lanes in six).
// The candidates go through LDS in chunks of CONTACT_BS agents -- x, y, and the radius only when radii are per agent --, and every
// lane runs over the chunk: the lanes of an arena read the same candidate in the same trip, an LDS broadcast.  A packed workgroup
// has one chunk (its arenas); a large arena ceil(N / CONTACT_BS) of them, so that a 16384-agent arena needs 3 KiB of LDS, not the
// 196 KB of its (x, y, r).  (x - y)^2 = (y - x)^2 bit for bit and the minimum over keys does not depend on the order, so any chunk
// order gives the same bits.  j = i is left out by index, not by d2 > 0: agents that a reset drops onto one spot do touch.
// The walls are a full scan of the arena's table whatever the handle (wall_d2 may lie beyond any obstacle range, so no grid bounds
// it); all lanes of an arena read the same edge, and with one table for every arena the loads are scalar.
#pragma once
#include "ca_common.h"

namespace ca {

constexpr int CONTACT_BS = 256;   // four waves: 3 KiB of LDS and few registers, so a CU holds eight such workgroups; a chunk of 256
                                  // candidates amortises the two barriers around it

struct ContactArgs {
    const float *pos_x, *pos_y;
    const float* ap_radius;   // StepCold::ap_radius: [A*N], or null: `radius` for every agent
    const int* agent_counts;  // StepCold::agent_counts: [A], or null: N agents in every arena
    const ObstDev* obst;      // the processed edge table(s), as in StepArgs
    const int* tab_off;       // null: one table of n_obst edges; else [A + 1] offsets
    int* out;                 // [5][A*N] words: agents | wall | nearest (i32), nearest_d2 | wall_d2 (f32)
    unsigned an;              // A * N: the stride of a plane
    int n_obst, A, N;
    int apb;                  // N <= CONTACT_BS: arenas per workgroup (CONTACT_BS / N); else 0
    int tiles;                // N >  CONTACT_BS: workgroups per arena (ceil(N / CONTACT_BS)); else 0
    float radius;
};

__global__ __launch_bounds__(CONTACT_BS) void contact_kernel(const ContactArgs p) {
    __shared__ float sx[CONTACT_BS], sy[CONTACT_BS], sr[CONTACT_BS];
    const int t = (int)threadIdx.x;
    const bool packed = p.apb > 0;
    const bool per_agent = p.ap_radius != nullptr;
    // lane -> (arena, agent); lbase: where the lane's arena begins in a staged chunk
    int a, i, lbase;
    bool have;
    if (packed) {
        const int la = t / p.N;
        i = t - la * p.N;
        a = (int)blockIdx.x * p.apb + la;
        lbase = la * p.N;
        have = la < p.apb && a < p.A;
    } else {
        a = (int)blockIdx.x / p.tiles;
        i = ((int)blockIdx.x - a * p.tiles) * CONTACT_BS + t;
        lbase = 0;
        have = i < p.N;   // (the grid is A * tiles workgroups: a < A)
    }
    const size_t q = (size_t)a * p.N + i;
    const int cnt = have ? (p.agent_counts != nullptr ? p.agent_counts[a] : p.N) : 0;
    const bool present = i < cnt;
    V2 pos = mk(0.0f, 0.0f);
    float ri = p.radius;
    if (present) {
        pos = mk(p.pos_x[q], p.pos_y[q]);
        if (per_agent) ri = p.ap_radius[q];
    }

    int touching = 0, nearest = -1;
    float nearest_d2 = __builtin_inff();
    // a packed workgroup stages its arenas' rows once; a large arena its N rows in chunks (a trip count of the whole workgroup)
    const int span = packed ? 1 : p.N;
    for (int c0 = 0; c0 < span; c0 += CONTACT_BS) {
        if (c0 > 0) __syncthreads();   // the chunk before is read
        {
            const size_t g = packed ? (size_t)blockIdx.x * p.apb * p.N + t : (size_t)a * p.N + c0 + t;
            const bool in = packed ? (t < p.apb * p.N && g < (size_t)p.an) : (c0 + t < p.N);
            if (in) {
                sx[t] = p.pos_x[g];
                sy[t] = p.pos_y[g];
                if (per_agent) sr[t] = p.ap_radius[g];
            }
        }
        __syncthreads();
        if (present) {
            const int jn = min(cnt - c0, CONTACT_BS);   // candidates of this chunk that are agents of the arena
            // (unrolled by four: a large arena is one wave per SIMD, and a trip that waits for its own LDS reads is all latency;
            //  the loads of four candidates are in flight together, the updates stay in candidate order)
#pragma unroll 4
            for (int jj = 0; jj < jn; ++jj) {
                const int j = c0 + jj;
                const float d2 = absSq(pos - mk(sx[lbase + jj], sy[lbase + jj]));
                const float cr = ri + (per_agent ? sr[lbase + jj] : p.radius);
                if (j != i) {
                    if (d2 < sqr(cr)) ++touching;
                    if (d2 < nearest_d2 || (d2 == nearest_d2 && j < nearest)) { nearest_d2 = d2; nearest = j; }
                }
            }
        }
    }

    int wall = 0;
    float wall_d2 = __builtin_inff();
    if (present) {
        const int off = p.tab_off != nullptr ? p.tab_off[a] : 0;
        const int ne = p.tab_off != nullptr ? p.tab_off[a + 1] - off : p.n_obst;
        const ObstDev* tab = p.obst + off;
        const float rr = sqr(ri);
        for (int e = 0; e < ne; ++e) {
            const ObstDev o1 = load_obst(tab, e);
            const float d2 = distSqPointSegment(mk(o1.px, o1.py), mk(o1.qx, o1.qy), pos);
            if (d2 < rr) wall = 1;
            if (d2 < wall_d2) wall_d2 = d2;
        }
    }

    // an absent row reports 0, 0, -1, +inf, +inf: the initial values
    if (have) {
        p.out[q] = touching;
        p.out[(size_t)p.an + q] = wall;
        p.out[2 * (size_t)p.an + q] = nearest;
        p.out[3 * (size_t)p.an + q] = __float_as_int(nearest_d2);
        p.out[4 * (size_t)p.an + q] = __float_as_int(wall_d2);
    }
}

}  // namespace ca
