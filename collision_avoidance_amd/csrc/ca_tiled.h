// ca_tiled.h -- the tiled solve path: arenas of up to 16384 agents, an arena spread over several workgroups (ca_create_ex, CA_CREATE_TILED)
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview and the numerics contract).
#pragma once
#include "ca_lp.h"
#include "ca_lines.h"
#include "ca_nbr.h"
#include "ca_rules.h"

namespace ca {

// One lane per agent; a workgroup owns one TILE of consecutive agents of one arena, the grid is ceil(N / TILE) x A (flat: workgroup
// b = arena b / tiles, tile b % tiles).  Every other solve kernel keeps an arena inside one workgroup and orders its phases with
// __syncthreads; here the arena's workgroups cannot wait for each other (no grid-wide barrier, no flag to spin on: a barrier that
// does not complete hangs the machine), so the phases are three launches on the handle's stream and the kernel boundary is the
// barrier:
//   tiled_solve_kernel   reads the arena's PRE-step positions and velocities (every tile reads all of them), writes the lists and
//                        the new velocity into nv_x / nv_y -- never vel or pos, which the other workgroups are still reading;
//   tiled_advance_kernel vel <- nv, pos += vel dt, reward, wall / goal tests, per-agent stores; the arena's partial results go into
//                        the per-arena scratch by integer atomics; a copy of the post-step position goes into nv_x / nv_y;
//   tiled_close_kernel   the pair count on that COPY (a neighbouring workgroup may already have respawned pos), the end of the
//                        episode, the arena's words, the in-kernel reset.
// The values a later phase needs of the arena's words (step count, episode, frozen or not) are latched into the scratch by the first
// launch, because the one lane that rewrites those words in the last launch runs beside workgroups that have not read them yet.
// Results are the one-workgroup kernels' (and the oracle's) bit for bit: the same device functions in the same order; only the sum
// of rewards is added in another order.
struct TiledArgs {
    StepArgs s;
    float *nv_x, *nv_y;   // [A*N] new velocity (solve -> advance), then the copy of the post-step position (advance -> close)
    unsigned* scr;        // [A][TS_STRIDE] per-arena scratch, see below
    int tiles;            // workgroups per arena = ceil(N / TILE)
};
// the per-arena scratch: written by lane 0 of tile 0 of the solve launch (zeros and latches), added to by the advance launch, read by
// the close launch
enum { TS_NOTDONE = 0,   // agents still on the way after this step
       TS_VMAX2 = 1,     // the arena's largest squared speed of this step, as float bits (the pair count's bound)
       TS_LIVE = 2,      // 1: the arena is advanced by this step (0: frozen, CA_F_FREEZE)
       TS_STEPS0 = 3,    // step_count[a] before this step
       TS_EPI = 4,       // episode[a] before this step
       TS_STRIDE = 8 };

// the overflow word of a tiled handle: the agent index takes 16 bits (bits 8 .. 23; the other handles' word has 11 at bits 8 .. 18
// and is written by note_overflow as before), the global arena the 36 bits above; the host decodes by the handle's kind
__device__ __forceinline__ void note_overflow_tiled(const StepCold* cold, int a, int i, int oin) {
    const unsigned long long g = (unsigned long long)(cold->arena_offset + (int64_t)a) & 0xFFFFFFFFFull;
    const unsigned long long v = (1ull << 63) | (g << 24) | ((unsigned long long)(i & 0xFFFF) << 8) | (unsigned long long)(oin > 255 ? 255 : oin);
    __hip_atomic_store(cold->ovf_word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// LDS of the solve launch (bytes): lines [K + S][TILE] | the staged candidate tile px py [TILE]
__host__ __device__ inline size_t tiled_lds_bytes(int TILE, int K, int S) { return (size_t)TILE * ((size_t)(K + S) * 16 + 8); }

// the step count an agent that arrives in this step records, and the one the arena holds after it (step_kernel's two increments)
__device__ __forceinline__ int tiled_steps_arrive(int steps0, bool actions, bool nodone) { return steps0 + ((!actions && !nodone) ? 1 : 0); }
__device__ __forceinline__ int tiled_steps_after(int steps0, bool actions, bool nodone) { return steps0 + ((actions || !nodone) ? 1 : 0); }

// ---- the uniform grid of a handle made with CA_CREATE_TILED_GRID ----------------------------------------------------------------
// The solve launch above tests every agent of the arena against every other.  A grid handle sorts the arena's agents by cell first
// -- a counting sort that crosses workgroups, so its phases are launches too -- and the solve launch tests only the cells an agent's
// range touches.  A step is then
//   tiled_bin_kernel      one lane per agent: its bucket, and its rank in the bucket by an integer atomic on the arena's cell counts
//                         (zero when the launch starts);
//   tiled_scan_kernel     one workgroup per arena: the exclusive prefix sum of the counts into cell_start[cells + 1], and the counts
//                         back to zero -- this workgroup is their only reader after the bin launch, and the next bin launch is a
//                         kernel boundary away;
//   tiled_scatter_kernel  one lane per agent: its PRE-step position and its id into slot cell_start[bucket] + rank of sx / sy / sidx;
//   tiled_solve_kernel<KMAX, TILE, SEARCH_GRID>, tiled_advance_kernel, tiled_close_kernel.
// The table is fixed and wrapped: cell c(v) = floor(v * ics) of a coordinate, bucket (c(y) & (GY - 1)) * GX + (c(x) & (GX - 1)), GX and
// GY powers of two.  No bounding box (it would be one more arena-wide reduction, one more launch): wrapping only aliases far cells
// into near ones, and an aliased stranger fails the distance test.  The mask keeps every index inside the table whatever the
// position arrays hold.  The order inside a cell comes from the atomics and differs from run to run; the lists do not depend on it
// (tiled_solve_kernel).  Frozen arenas (CA_F_FREEZE) are skipped by all three: arena_done was last written by the close launch of
// the step before, which is complete.
struct TiledGridArgs : TiledArgs {
    unsigned* cell_count;        // [A][cells]: zero between steps
    unsigned* cell_start;        // [A][cells + 1]
    unsigned* key;               // [A*N] bucket << 16 | rank in the bucket (both below 2^14)
    float *sx, *sy;              // [A*N] the arena's pre-step positions in cell order
    unsigned short* sidx;        // [A*N] ... and whose they are
    int gx, gy;                  // the table's sides: powers of two, 8 .. 128
    float ics;                   // 1 / cell size, computed once by the host
};

// the unwrapped cell coordinate: monotone in v (a product with a positive constant, floor, and a clamp that also gives NaN a value),
// which is all the choice of cells below needs
__device__ __forceinline__ int grid_cell(float v, float ics) {
    return (int)fminf(fmaxf(floorf(v * ics), -1073741824.0f), 1073741824.0f);
}

// ---- the static grid over the obstacle edges of a grid handle (ca_tiled_edge_grid; built by the host: ca_edge_grid_host.h) ----------
// The solve launch above tests every edge of the arena's table for every agent, and so does the wall test of the advance launch.
// Edges do not move: the host builds, once per installed table, a CSR table over the bounding box of the edges -- cell_start[cells + 1]
// and entries (edge id | the lowest column of the edge's cell rectangle << 16 | its lowest row << 24) -- and the edge-grid forms of the solve
// and advance kernels (SEARCH_GRID_EDGES, EDGES) walk the few cells an agent's range touches.  No launch, no sort, no barrier per step.  The table is unwrapped and clamped
// (edge_cell): an agent outside the box, or a NaN, stands in an outermost cell.  Every index is clamped -- the run's end by the
// table's entry count, the edge id by the arena's edge count -- so positions of any value stay inside the arrays.
struct EdgeGridDev {   // one table's grid: a table per arena (indexed like tab_off), or one for all
    float x0, y0, ics_x, ics_y;          // origin and reciprocal cell sizes
    int gx, gy;                          // sides, 1 .. 256
    unsigned n_entries;                  // entries of this table
    unsigned cells_off, entries_off;     // where this table's cell_start / entries begin
    unsigned pad;
};
struct TiledEdgeArgs : TiledGridArgs {
    const EdgeGridDev* eg;
    const unsigned* eg_cells;
    const unsigned* eg_entries;
};
// ca_edge_grid_host.h's cell expression, operation for operation (fp32, no contraction): monotone in v
__device__ __forceinline__ int edge_cell(float v, float x0, float ics, int g) {
    return (int)fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1));
}

__global__ __launch_bounds__(256) void tiled_bin_kernel(const TiledGridArgs t) {
    const StepArgs& p = t.s;
    const int a = (int)blockIdx.x / t.tiles, tile = (int)blockIdx.x - a * t.tiles;
    const int i = tile * (int)blockDim.x + (int)threadIdx.x;
    if (i >= p.N || arena_frozen(p, a)) return;
    const size_t q = (size_t)a * p.N + i;
    const int bucket = (grid_cell(p.pos_y[q], t.ics) & (t.gy - 1)) * t.gx + (grid_cell(p.pos_x[q], t.ics) & (t.gx - 1));
    const unsigned rank = atomicAdd(&t.cell_count[(size_t)a * (t.gx * t.gy) + bucket], 1u);
    t.key[q] = ((unsigned)bucket << 16) | (rank & 0xFFFFu);
}

// (1024 lanes, one workgroup per arena: at most 128 x 128 cells, 16 consecutive cells per lane)
__global__ __launch_bounds__(1024) void tiled_scan_kernel(const TiledGridArgs t) {
    const StepArgs& p = t.s;
    __shared__ unsigned s_wave[16];
    const int a = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (arena_frozen(p, a)) return;   // (the whole workgroup)
    const int cells = t.gx * t.gy;
    const int cpl = (cells + 1023) >> 10;
    unsigned* cnt = t.cell_count + (size_t)a * cells;
    unsigned* start = t.cell_start + (size_t)a * (cells + 1);
    const int c0 = tid * cpl;
    unsigned sum = 0u;
    for (int k = 0; k < cpl; ++k) sum += (c0 + k < cells) ? cnt[c0 + k] : 0u;
    unsigned incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_up(incl, off, 64);
        if ((tid & 63) >= off) incl += v;
    }
    if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    unsigned b = incl - sum;
    for (int w = 0; w < (tid >> 6); ++w) b += s_wave[w];
    for (int k = 0; k < cpl; ++k) {
        if (c0 + k < cells) {
            const unsigned c = cnt[c0 + k];
            start[c0 + k] = b;
            b += c;
            cnt[c0 + k] = 0u;
        }
    }
    if (tid == 1023) start[cells] = b;
}

__global__ __launch_bounds__(256) void tiled_scatter_kernel(const TiledGridArgs t) {
    const StepArgs& p = t.s;
    const int a = (int)blockIdx.x / t.tiles, tile = (int)blockIdx.x - a * t.tiles;
    const int i = tile * (int)blockDim.x + (int)threadIdx.x;
    if (i >= p.N || arena_frozen(p, a)) return;
    const size_t abase = (size_t)a * p.N;
    const unsigned k = t.key[abase + i];
    const unsigned bucket = min(k >> 16, (unsigned)(t.gx * t.gy - 1));
    const unsigned dst = t.cell_start[(size_t)a * (t.gx * t.gy + 1) + bucket] + (k & 0xFFFFu);
    if (dst < (unsigned)p.N) {   // (always, on consistent counts: the guard keeps a step that follows a failed launch inside the arrays)
        t.sx[abase + dst] = p.pos_x[abase + i];
        t.sy[abase + dst] = p.pos_y[abase + i];
        t.sidx[abase + dst] = (unsigned short)i;
    }
}

// ---- the three launches of the step: one kernel template each -------------------------------------------------------------------
// A variant is a template parameter, read with `if constexpr` inside the kernel (not a shared __device__ function: through one the
// plain kernel's instruction text moved).
// SEARCH of the solve launch: how an agent finds its neighbours and its obstacle edges.
enum TiledSearch { SEARCH_ALL = 0,          // every agent of the arena, a tile at a time through LDS; every edge of the arena's table
                   SEARCH_GRID = 1,         // the uniform grid of a handle made with CA_CREATE_TILED_GRID; every edge
                   SEARCH_GRID_EDGES = 2 }; // ... and the edges through the static edge grid (ca_tiled_edge_grid)
// AgentParams in PER (a handle made with CA_CREATE_TILED_PARAMS, while ca_set_agent_params is in force): radius, maximum speed and the
// two time horizons of agent i come from the per-agent arrays (StepCold::ap_*), a neighbour's radius is gathered beside its position
// and velocity, and each enters where DESIGN.md 7b says -- the obstacle range sqr(tho_i * ms_i + r_i) and the edge-grid walk over
// cell(x +- (tho_i * ms_i + r_i)), the obstacle lines and their covered test (r_i, 1 / tho_i), the agent lines (r_i, r_j, 1 / th_i),
// LP2 / LP3 (ms_i), the wall and goal tests (r_i), the pair count (sqr(r_i + r_j)).  The sort launches are the uniform handle's:
// the cells stay half the handle's neighbor_dist wide.  AgentSensing in PER (ca_set_agent_sensing; the tag includes AgentParams): neighbor_dist and
// max_neighbors per agent -- the solve launch's three searches take the lane's own range and list length, the close launch's list
// shortcut likewise; the advance launch does not see them.  The edge grid is built for the LARGEST range of the handle (ca_env.hip
// edge_grid_range); the corner rule of the walk does not depend on the cell size, so an agent of a smaller range simply walks fewer
// cells.
// WideObstLists in PER (a handle made with CA_CREATE_TILED_WIDE whose max_obst_neighbors exceeds SMAX; never beside AgentParams): the
// solve launch keeps up to SWIDE obstacle neighbours.  The sorted list is built in LDS, in the lane's column at the head of the line
// table (ca_nbr.h WideInsert), goes to obst_idx before the agent scan, and a barrier stands between the columns' last use and the first
// line; up to K + S lines per lane go into the table, LP3 projects KMAX + SWIDE.  The advance and close launches do not depend on S.
// The host sizes the tile so that tiled_lds_bytes fits a CU (ca_env.hip ca_create_ex: 64 unless CA_TILE says otherwise).
struct TiledCloseParamsArgs : TiledArgs {
    float r_max;   // the largest radius of the handle: R of lists_bound_pairs / list_misses_pairs (r_i + r_j <= 2 r_max)
};
// LDS of the close launch (bytes): the staged candidate tile px py [TILE], and with per-agent parameters its radii
__host__ __device__ inline size_t tiled_close_lds_bytes(int TILE, bool params) { return (size_t)TILE * (params ? 12 : 8); }

// the argument block of each launch follows from its variant (traits of our own, so that an instantiation's name stays short)
template <int SEARCH> struct TiledSolveArgs { using type = std::conditional_t<SEARCH == SEARCH_GRID_EDGES, TiledEdgeArgs, std::conditional_t<SEARCH == SEARCH_GRID, TiledGridArgs, TiledArgs>>; };
template <bool EDGES> struct TiledAdvanceArgs { using type = std::conditional_t<EDGES, TiledEdgeArgs, TiledArgs>; };
template <class... PER> struct TiledCloseArgs { using type = std::conditional_t<has_tag<AgentParams, PER...> || has_tag<AgentSensing, PER...>, TiledCloseParamsArgs, TiledArgs>; };

// ---- launch 1: neighbour search, ORCA lines, LP2 / LP3 ------------------------------------------------------------------------
// On a grid handle lane tile * TILE + tid works for SORTED POSITION s of the arena, its agent is i = sidx[s] -- the lanes of a wave then
// stand in the same few cells and walk the same runs -- and everything else addresses by i as before.
template <int KMAX, int TILE, int SEARCH, class... PER>
__global__ __launch_bounds__(TILE) void tiled_solve_kernel(const typename TiledSolveArgs<SEARCH>::type t) {
    constexpr bool AS = has_tag<AgentSensing, PER...>;
    constexpr bool AP = has_tag<AgentParams, PER...> || AS;   // (AgentSensing includes AgentParams: ca_common.h)
    constexpr bool WIDE = has_tag<WideObstLists, PER...>;
    static_assert(!(WIDE && AP), "per-agent parameters go with obstacle lists of up to 16");
    const StepArgs& p = t.s;
    extern __shared__ float4 smem4[];
    const int tid = threadIdx.x;
    const int a = (int)blockIdx.x / t.tiles, tile = (int)blockIdx.x - a * t.tiles;
    const int N = p.N, K = p.K, S = p.S;
    int i = tile * TILE + tid;
    if constexpr (SEARCH != SEARCH_ALL) {
        if (i < N && !arena_frozen(p, a)) i = min((int)t.sidx[(size_t)a * N + i], N - 1);   // (an inactive lane keeps i >= N)
    }
    const bool frozen = arena_frozen(p, a);   // (the whole workgroup: one arena)
    if (tile == 0 && tid == 0) {
        unsigned* sc = t.scr + (size_t)a * TS_STRIDE;
        sc[TS_NOTDONE] = 0u; sc[TS_VMAX2] = 0u; sc[TS_LIVE] = frozen ? 0u : 1u;
        sc[TS_STEPS0] = (unsigned)p.cold->step_count[a]; sc[TS_EPI] = (unsigned)p.cold->episode[a];
        if (frozen) p.arena_stats[(size_t)a * ST_STRIDE + ST_FROZEN] += 1;
    }
    if (frozen) return;
    const bool active = i < N;
    const size_t abase = (size_t)a * N;
    const size_t q = abase + (active ? i : 0);

    float4* s_lines = smem4;                                                   // [(K + S)][TILE]
    float* s_px = reinterpret_cast<float*>(smem4 + (size_t)(K + S) * TILE);    // the candidate tile
    float* s_py = s_px + TILE;
    LdsLines ls; ls.base = s_lines + tid; ls.stride = TILE;

    // ---- own state, preferred velocity (step_kernel's prologue) ----
    V2 pos = mk(0.0f, 0.0f), vel = mk(0.0f, 0.0f), pref = mk(0.0f, 0.0f);
    if (active) {
        pos = mk(p.pos_x[q], p.pos_y[q]);
        vel = mk(p.vel_x[q], p.vel_y[q]);
        if (p.actions) {
            V2 pf32;
            action_pref(pos, p.goal_x[q], p.goal_y[q], p.actions[q], pf32, pref);
        } else {
            pref = mk(p.pref_x[q], p.pref_y[q]);
        }
    }
    // the handle's four constants, or the agent's own four values (an inactive lane keeps the handle's: it computes nothing that is
    // stored); a neighbour's radius is gathered next to its position and velocity, where its line is built
    float radius = p.radius, max_speed = p.max_speed, horizon = p.time_horizon, horizon_obst = p.time_horizon_obst;
    const ColdK& ck = *(ColdK*)p.cold;
    if constexpr (AP) {
        if (active) { radius = ck.ap_radius[q]; max_speed = ck.ap_max_speed[q]; horizon = ck.ap_time_horizon[q]; horizon_obst = ck.ap_time_horizon_obst[q]; }
    }

    // ---- obstacle neighbours (App. A.2; ca_nbr.h's keys; its edge_in_range and ca_common.h arena_edges written out: through them this kernel's text moved) ----
    const ObstDev* tab = p.obst + ((p.tab_off != nullptr) ? p.tab_off[a] : 0);          // this arena's edge table
    const int n_edges = p.tab_off != nullptr ? p.tab_off[a + 1] - p.tab_off[a] : p.n_obst;
    int oin = 0;
    {
        // WideObstLists in PER (lists of 17 .. SWIDE edges, a handle made with CA_CREATE_TILED_WIDE): 2 S registers for the keys do not
        // exist, so the sorted list is built in the lane's column at the head of the line table, which is idle until the lines are built
        // (ca_nbr.h WideInsert: key slot k of lane t is the 64-bit word [k][t], consecutive lanes' words consecutive in LDS).  All
        // three searches feed it; it keeps the S smallest keys in whatever order they arrive.
        constexpr int SR = WIDE ? 1 : SMAX;   // register slots of the list (wide: none)
        const int sofs = SR - S;   // the S-entry list is right-aligned in the register array
        double okey[SR];
#pragma unroll
        for (int k = 0; k < SR; ++k) okey[k] = (k < sofs) ? key_dummy() : key_empty();
        unsigned long long* wkey = nullptr;
        int wcnt = 0;
        if constexpr (WIDE) wkey = reinterpret_cast<unsigned long long*>(smem4) + tid;
        const WideInsert<TILE> wide_insert{wkey, wcnt, S};
        const float rangeSq = sqr(horizon_obst * max_speed + radius);
        if constexpr (SEARCH == SEARCH_GRID_EDGES) {
            // The static edge grid (ca_edge_grid_host.h): the cells of the columns cell(fl(x - range)) .. cell(fl(x + range)) and the rows
            // likewise, 3 x 3 but for a rounding of ics; an edge registered in several of them is taken in the low corner of the intersection of its
            // rectangle with this one, so no edge enters twice; an accepted edge passes the test of the scan below, on tab[e].  The list
            // is the S smallest distinct keys of the accepted set: the order of the walk is immaterial.  Per-lane walks: the lanes of a
            // wave stand in the same few cells (sorted positions), so their loads of a run and of its records fall into the same lines.
            if (active) {
                const EdgeGridDev g = t.eg[p.tab_off != nullptr ? a : 0];
                const unsigned* cs = t.eg_cells + g.cells_off;
                const unsigned* en = t.eg_entries + g.entries_off;
                const float range = horizon_obst * max_speed + radius;   // (per agent: a smaller range walks fewer cells)
                const int cxlo = edge_cell(pos.x - range, g.x0, g.ics_x, g.gx), cxhi = edge_cell(pos.x + range, g.x0, g.ics_x, g.gx);
                const int cylo = edge_cell(pos.y - range, g.y0, g.ics_y, g.gy), cyhi = edge_cell(pos.y + range, g.y0, g.ics_y, g.gy);
                for (int r = cylo; r <= cyhi; ++r) {
                    for (int c = cxlo; c <= cxhi; ++c) {
                        const unsigned* run = cs + (r * g.gx + c);
                        const unsigned hi = min(run[1], g.n_entries);   // (every index clamped: EdgeGridDev above)
                        for (unsigned u = run[0]; u < hi; ++u) {
                            const unsigned w = en[u];
                            const int e = (int)(w & 0xFFFFu);
                            if (e >= n_edges || max((int)((w >> 16) & 0xFFu), cxlo) != c || max((int)(w >> 24), cylo) != r) continue;
                            const ObstDev& o1 = tab[e];
                            const V2 a1 = mk(o1.px, o1.py), a2 = mk(o1.qx, o1.qy);
                            const float alol = leftOf(a1, a2, pos);
                            const float dsl = div_ir(sqr(alol), absSq(a2 - a1));
                            if (dsl < rangeSq && alol < 0.0f) {
                                const float dsq = distSqPointSegment(a1, a2, pos);
                                if (dsq < rangeSq) {
                                    ++oin;
                                    if constexpr (WIDE) wide_insert(wide_key(dsq, e));
                                    else sorted_insert<SR>(okey, make_key(dsq, e));
                                }
                            }
                        }
                    }
                }
            }
        } else {
            for (int e = 0; e < n_edges; ++e) {   // (uniform: scalar loads of the edge records)
                const ObstDev& o1 = tab[e];
                const V2 a1 = mk(o1.px, o1.py), a2 = mk(o1.qx, o1.qy);
                const float alol = leftOf(a1, a2, pos);
                const float dsl = div_ir(sqr(alol), absSq(a2 - a1));
                if (active && dsl < rangeSq && alol < 0.0f) {
                    const float dsq = distSqPointSegment(a1, a2, pos);
                    if (dsq < rangeSq) {
                        ++oin;
                        if constexpr (WIDE) wide_insert(wide_key(dsq, e));
                        else sorted_insert<SR>(okey, make_key(dsq, e));
                    }
                }
            }
        }
        if constexpr (WIDE) {   // the LDS list goes to memory before the agent scan (an empty slot reads -1, as in the register form)
            if (active) {
                for (int k = 0; k < S; ++k) p.obst_idx[((size_t)a * S + k) * N + i] = wide_id<TILE>(wkey, wcnt, k);
            }
            // a lane's line slot overlaps OTHER lanes' key words (16 B lines over 8 B keys): every column has been read before the
            // first line is written, whatever the search -- the grid forms have no other barrier, the scan below none at K = 0
            __syncthreads();
        } else if (active) {
#pragma unroll
            for (int k = 0; k < SR; ++k)
                if (k >= sofs) p.obst_idx[((size_t)a * S + (k - sofs)) * N + i] = (unsigned short)key_index(okey[k]);
        }
    }
    const int ocnt = oin < S ? oin : S;

    // ---- agent neighbours: the K smallest (distance, index) keys below neighbor_dist^2 ----
    const int kofs = KMAX - K;
    double nkey[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) nkey[k] = (k < kofs) ? key_dummy() : key_empty();
    int ncnt = 0;
    // AgentSensing in PER: the lane's own range nd_i and list length K_i (ca_nbr.h states the rule: the list is the head of the K-list
    // taken with range nd_i, so the searches keep K slots and the cut to K_i is made once, at the store).  An idle lane keeps nothing.
    [[maybe_unused]] float nd_own = p.neighbor_dist;
    [[maybe_unused]] int K_own = 0;
    if constexpr (AS) {
        if (active) { nd_own = ck.as_neighbor_dist[q]; K_own = (int)ck.as_max_neighbors[q]; }
    }
    if constexpr (SEARCH != SEARCH_ALL) {
        // The cells of the columns c(fl(x - B)) .. c(fl(x + B)) and the rows likewise, B = nd * 1.0001 + 1e-4 (ca_nbr.h: a candidate
        // that passes the distance test has |xi - xj| < B, so xj lies between the two floats, and c is monotone) -- not a fixed
        // block around the own cell.  At most GX columns and GY rows, so no bucket is visited twice; a row's columns are one run of
        // the sorted arrays, or two where they wrap.  Cells arrive in no index order: a candidate enters on `distance <= the current
        // K-th distance` and the 64-bit keys settle ties, which also makes the order inside a cell immaterial.
        if (K > 0 && active) {
            const size_t cbase = (size_t)a * (t.gx * t.gy + 1);
            // (AS: the lane's fl(nd_i^2), and the block of its own B_i -- the derivation above holds for any range, the cell size stays the
            // handle's, so a short-sighted agent walks fewer cells)
            const float rangeSq0 = AS ? sqr(nd_own) : sqr(p.neighbor_dist);
            float rangeK = rangeSq0;
            const float B = (AS ? nd_own : p.neighbor_dist) * 1.0001f + 1e-4f;
            const int cxlo = grid_cell(pos.x - B, t.ics), cxhi = grid_cell(pos.x + B, t.ics);
            const int cylo = grid_cell(pos.y - B, t.ics), cyhi = grid_cell(pos.y + B, t.ics);
            const int ncol = (int)min((unsigned)cxhi - (unsigned)cxlo, (unsigned)(t.gx - 1)) + 1;   // (lo <= hi: c is monotone; NaN gives 1)
            const int nrow = (int)min((unsigned)cyhi - (unsigned)cylo, (unsigned)(t.gy - 1)) + 1;
            const int c0 = cxlo & (t.gx - 1);
            const int n1 = min(ncol, t.gx - c0), n2 = ncol - n1;   // columns c0 .. c0 + n1 - 1, then 0 .. n2 - 1
            auto scan_run = [&](unsigned lo, unsigned hi) {
                hi = min(hi, (unsigned)N);   // (prefix sums of at most N agents: already so on consistent counts)
                for (unsigned u = lo; u < hi; ++u) {
                    const int j = (int)t.sidx[abase + u];
                    const float dsq = absSq(pos - mk(t.sx[abase + u], t.sy[abase + u]));
                    if (j != i && dsq < rangeSq0 && dsq <= rangeK) {
                        sorted_insert<KMAX>(nkey, make_key(dsq, j));
                        if (ncnt < K) ++ncnt;
                        if (ncnt == K) rangeK = key_dist(nkey[KMAX - 1]);
                    }
                }
            };
            for (int r = 0; r < nrow; ++r) {
                const unsigned* rs = t.cell_start + cbase + (size_t)((cylo + r) & (t.gy - 1)) * t.gx;
                scan_run(rs[c0], rs[c0 + n1]);
                if (n2 > 0) scan_run(rs[0], rs[n2]);
            }
        }
    } else {
        // candidates in index order, a tile at a time through LDS -- the oracle's scan, so the shrinking range is its strict one
        if (K > 0) {
            float rangeSq = AS ? sqr(nd_own) : sqr(p.neighbor_dist);
            for (int ct = 0; ct < t.tiles; ++ct) {
                const int j0 = ct * TILE;
                const int nj = min(TILE, N - j0);
                __syncthreads();   // (the previous tile has been read by every lane)
                if (tid < nj) { s_px[tid] = p.pos_x[abase + j0 + tid]; s_py[tid] = p.pos_y[abase + j0 + tid]; }
                __syncthreads();
                V2 o_next = mk(s_px[0], s_py[0]);
                for (int jj = 0; jj < nj; ++jj) {
                    const V2 o = o_next;   // the next candidate's position is in flight while this one is inserted
                    if (jj + 1 < nj) o_next = mk(s_px[jj + 1], s_py[jj + 1]);
                    const int j = j0 + jj;
                    const float dsq = absSq(pos - o);
                    if (active && j != i && dsq < rangeSq) {
                        sorted_insert<KMAX>(nkey, make_key(dsq, j));
                        if (ncnt < K) ++ncnt;
                        if (ncnt == K) rangeSq = key_dist(nkey[KMAX - 1]);
                    }
                }
            }
        }
    }
    if (active) {
        if (__builtin_expect(oin > S, 0)) {
            atomicAdd(reinterpret_cast<int*>(&p.arena_stats[(size_t)a * ST_STRIDE + ST_OVERFLOW]), 1);
            note_overflow_tiled(p.cold, a, i, oin);
        }
        if constexpr (AS) ncnt = ncnt < K_own ? ncnt : K_own;   // the head of the K-list: its K_i nearest (the lines below take ncnt entries)
        p.counts[q] = (unsigned short)(ncnt | (ocnt << 8));
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k >= kofs) st_idx_t<true>(p.nb_idx, ((size_t)a * K + (k - kofs)) * N + i, (AS && k - kofs >= K_own) ? -1 : key_index(nkey[k]));
    }

    // ---- ORCA lines into the LDS table (step_kernel's LDS-table path; the neighbours' state gathered from global memory) ----
    int nl = 0;
    {
        const float invTO = 1.0f / horizon_obst;
        const float R = radius;
        for (int s = 0; s < ocnt; ++s) {
            const int e = ld_idx_t<true>(p.obst_idx, ((size_t)a * S + s) * N + i);   // (this lane wrote it)
            Line line;
            auto covered = [&](V2 c1, V2 c2) {
                return table_covers(ls, nl, c1, c2, invTO, R);
            };
            if (obst_orca_line(tab, e, pos, vel, R, invTO, covered, line)) {
                ls.put(nl, line);
                ++nl;
            }
        }
    }
    const int numObstLines = nl;
    {
        const float invT = 1.0f / horizon;
        const float invDt = 1.0f / p.time_step;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k >= kofs && k - kofs < ncnt) {
                const size_t j = abase + (size_t)key_index(nkey[k]);
                if constexpr (AP)
                    ls.put(nl, agent_orca_line(pos, vel, mk(p.pos_x[j], p.pos_y[j]), mk(p.vel_x[j], p.vel_y[j]), radius, ck.ap_radius[j], invT, invDt));
                else
                    ls.put(nl, agent_orca_line(pos, vel, mk(p.pos_x[j], p.pos_y[j]), mk(p.vel_x[j], p.vel_y[j]), radius, invT, invDt));
                ++nl;
            }
        }
    }
    // ---- 2-D linear program (App. A.5), LP3 where it is infeasible ----
    V2 nv = mk(0.0f, 0.0f);
    int fail = nl;
    if (active) fail = lp2(ls, nl, max_speed, pref, false, nv);
    if (active && fail < nl) lp3<KMAX + (WIDE ? SWIDE : SMAX)>((__attribute__((address_space(3))) char*)ls.base, ls.stride, nl, numObstLines, fail, max_speed, nv);
    if (active) { t.nv_x[q] = nv.x; t.nv_y[q] = nv.y; }
}

// ---- launch 2: integrate, reward, wall / goal tests, the arena's partial results ---------------------------------------------------
// (any workgroup size: a workgroup is one tile of one arena, blockDim.x = TILE.  EDGES: the wall test walks the static edge grid.
// AgentParams in PER: the wall and goal tests take the agent's own radius.)
template <bool EDGES, class... PER>
__global__ __launch_bounds__(256) void tiled_advance_kernel(const typename TiledAdvanceArgs<EDGES>::type t) {
    constexpr bool AP = has_tag<AgentParams, PER...>;
    const StepArgs& p = t.s;
    const ColdK& c = *(ColdK*)p.cold;
    __shared__ int s_red[4];   // [0] not-done agents, [1] wall hits, [2] goals, [3] largest squared speed (float bits)
    const int tid = threadIdx.x, TILE = blockDim.x;
    const int a = (int)blockIdx.x / t.tiles, tile = (int)blockIdx.x - a * t.tiles;
    if (arena_frozen(p, a)) return;   // (nobody writes arena_done in this launch)
    const int N = p.N;
    const int i = tile * TILE + tid;
    const bool active = i < N;
    const size_t q = (size_t)a * N + (active ? i : 0);
    if (tid < 4) s_red[tid] = 0;
    __syncthreads();
    const bool nodone = (p.flags & 8u) != 0;  // CA_F_NODONE
    const int steps0 = c.step_count[a];
    float rew = 0.0f;
    if (active) {
        const V2 pos0 = mk(p.pos_x[q], p.pos_y[q]);
        float radius = p.radius;
        if constexpr (AP) radius = c.ap_radius[q];
        const V2 vel = mk(t.nv_x[q], t.nv_y[q]);
        const V2 pos = pos0 + vel * p.time_step;   // (App. A.1)
        double gx = c.goal_x[q], gy = c.goal_y[q];
        V2 pref;
        if (p.actions) {   // the directions of the prologue again, from the agent's own pre-step position: the same inputs, the same bits
            V2 pf32;
            action_pref(pos0, gx, gy, p.actions[q], pf32, pref);
            rew = step_reward(c.reward_scale, vel, pf32, pref);
            c.reward[q] = rew;
        } else {
            pref = goal_dir(pos, gx, gy);
        }
        if (p.flags & 2u) {  // CA_F_STATS
            const ObstDev* tab = p.obst + (p.tab_off != nullptr ? p.tab_off[a] : 0);
            const int ne = p.tab_off != nullptr ? p.tab_off[a + 1] - p.tab_off[a] : p.n_obst;
            if constexpr (EDGES) {
                // ca_rules.h touches_wall over the cells cell(fl(x - R)) .. cell(fl(x + R)) of the post-step position (R <= the range the
                // table was built for): an OR over edges, so an edge met in two cells is harmless and nothing is deduplicated
                const EdgeGridDev g = t.eg[p.tab_off != nullptr ? a : 0];
                const unsigned* cs = t.eg_cells + g.cells_off;
                const unsigned* en = t.eg_entries + g.entries_off;
                const float R = radius;
                const int cxlo = edge_cell(pos.x - R, g.x0, g.ics_x, g.gx), cxhi = edge_cell(pos.x + R, g.x0, g.ics_x, g.gx);
                const int cylo = edge_cell(pos.y - R, g.y0, g.ics_y, g.gy), cyhi = edge_cell(pos.y + R, g.y0, g.ics_y, g.gy);
                bool wall = false;
                for (int r = cylo; r <= cyhi; ++r) {
                    for (int cc = cxlo; cc <= cxhi; ++cc) {
                        const unsigned* run = cs + (r * g.gx + cc);
                        const unsigned hi = min(run[1], g.n_entries);
                        for (unsigned u = run[0]; u < hi; ++u) {
                            const int e = (int)(en[u] & 0xFFFFu);
                            if (e >= ne) continue;
                            const ObstDev o1 = load_obst(tab, e);
                            if (distSqPointSegment(mk(o1.px, o1.py), mk(o1.qx, o1.qy), pos) < sqr(R)) wall = true;
                        }
                    }
                }
                if (wall) atomicAdd(&s_red[1], 1);
            } else {
                if (touches_wall(tab, ne, pos, radius)) atomicAdd(&s_red[1], 1);
            }
        }
        bool goal_changed = false;
        int done = c.agent_done[q];
        if (!nodone && goal_hit(c, pos, gx, gy, radius, done)) {
            if (c.done_mode == 2) {
                const int rc = c.regoal_count[q];
                regoal_draw(c, a, i, rc, &gx, &gy);
                c.regoal_count[q] = rc + 1;
            } else {
                done = 1;
                c.arrive_step[q] = tiled_steps_arrive(steps0, p.actions != nullptr, nodone);
                arrival_goal(c, (int)q, &gx, &gy);
                c.agent_done[q] = 1;
            }
            c.goal_x[q] = gx; c.goal_y[q] = gy;
            goal_changed = true;
            atomicAdd(&s_red[2], 1);
        }
        if (done == 0) atomicAdd(&s_red[0], 1);
        atomicMax(reinterpret_cast<unsigned*>(&s_red[3]), __float_as_uint(absSq(vel)));
        const V2 o = obs_frame(pref, p.actions != nullptr || goal_changed, pos, gx, gy);
        c.orient_x[q] = o.x; c.orient_y[q] = o.y;
        c.pos_x[q] = pos.x; c.pos_y[q] = pos.y;
        c.vel_x[q] = vel.x; c.vel_y[q] = vel.y;
        c.pref_x[q] = pref.x; c.pref_y[q] = pref.y;
        t.nv_x[q] = pos.x; t.nv_y[q] = pos.y;   // the copy the pair count reads
    }
    if (p.actions && (p.flags & 2u)) {   // sum of rewards: a tree inside the wave, one f64 atomic per wave
        double r = active ? (double)rew : 0.0;
        for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
        if ((tid & 63) == 0 && tile * TILE + tid < N)
            atomicAdd(reinterpret_cast<double*>(&c.arena_stats[(size_t)a * ST_STRIDE + ST_SUMREW]), r);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned* sc = t.scr + (size_t)a * TS_STRIDE;
        if (s_red[0]) atomicAdd(&sc[TS_NOTDONE], (unsigned)s_red[0]);
        atomicMax(&sc[TS_VMAX2], (unsigned)s_red[3]);
        unsigned long long* st = c.arena_stats + (size_t)a * ST_STRIDE;
        if (s_red[1]) atomicAdd(&st[ST_OBST_COLL], (unsigned long long)s_red[1]);
        if (s_red[2]) atomicAdd(&st[ST_GOALS], (unsigned long long)s_red[2]);
    }
}

// ---- launch 3: pair count on the copy, end of the episode, the arena's words, the in-kernel reset ---------------------------------
// dynamic LDS: the staged candidate tile px py [TILE] (8 B per lane).  AgentParams in PER: the pair count takes every agent's own
// radius -- a pair overlaps within sqr(r_i + r_j), the tile's radii staged beside its positions (12 B per lane) -- and its shortcut
// through the neighbour lists is bounded by t.r_max, the handle-wide largest radius.
template <class... PER>
__global__ __launch_bounds__(256) void tiled_close_kernel(const typename TiledCloseArgs<PER...>::type t) {
    constexpr bool AS = has_tag<AgentSensing, PER...>;
    constexpr bool AP = has_tag<AgentParams, PER...> || AS;   // (AgentSensing includes AgentParams: ca_common.h)
    const StepArgs& p = t.s;
    const ColdK& c = *(ColdK*)p.cold;
    extern __shared__ float4 smem4[];
    __shared__ int s_pairs;
    const int tid = threadIdx.x, TILE = blockDim.x;
    const int a = (int)blockIdx.x / t.tiles, tile = (int)blockIdx.x - a * t.tiles;
    const unsigned* sc = t.scr + (size_t)a * TS_STRIDE;
    if (sc[TS_LIVE] == 0u) return;   // frozen when the step began (arena_done itself is rewritten in this launch)
    const int N = p.N, K = p.K;
    const int i = tile * TILE + tid;
    const bool active = i < N;
    const size_t abase = (size_t)a * N;
    const size_t q = abase + (active ? i : 0);
    float* s_px = reinterpret_cast<float*>(smem4);
    float* s_py = s_px + TILE;
    float* s_pr = s_py + TILE;   // (AP) the candidate tile's radii, beside its positions
    if (tid == 0) s_pairs = 0;

    if (p.flags & 2u) {  // CA_F_STATS: overlapping pairs (i < j) after the step -- step_kernel's shortcut through the neighbour lists
        // with the arena-wide largest speed of this step, and for the lanes that cannot conclude from their list a scan of the copy
        int pairs = 0;
        // (AP: an overlapping pair is closer than r_i + r_j <= 2 r_max: with r_max for R the two tests of ca_rules.h stay conservative)
        float R = p.radius;
        if constexpr (AP) R = t.r_max;
        const float ri = (AP && active) ? c.ap_radius[q] : 0.0f;
        float crSq = 0.0f;   // one radius: a pair overlaps within sqr(R + R) (formed here in that form only: where it stands moves the text)
        if constexpr (!AP) crSq = sqr(R + R);
        const float m2 = pair_reach(sc[TS_VMAX2], p.time_step);
        V2 pos = mk(0.0f, 0.0f);
        if (active) pos = mk(t.nv_x[q], t.nv_y[q]);
        // (AS: the shortcut reasons "my list holds every agent that can overlap me" -- from the lane's OWN range and list length: its list
        // reaches nd_i, and is full at K_i entries.  K_i = 0 is a list both full and empty (far2 = 0): such a lane scans.  Lane i counts
        // the pairs (i, j > i) from its own list alone, so the asymmetry of the lists does not enter.)
        [[maybe_unused]] float nd_own = p.neighbor_dist;
        [[maybe_unused]] int K_own = K;
        if constexpr (AS) {
            if (active) { nd_own = c.as_neighbor_dist[q]; K_own = (int)c.as_max_neighbors[q]; }
        }
        bool scan_all = active && !lists_bound_pairs(AS ? nd_own : p.neighbor_dist, R, m2);
        if (active && !scan_all) {
            float far2 = 0.0f;
            const int ncnt = (int)(p.counts[q] & 0xFFu);
            for (int k = 0; k < ncnt; ++k) {
                const int j = ld_idx_t<true>(p.nb_idx, ((size_t)a * K + k) * N + i);
                const float d2 = absSq(pos - mk(t.nv_x[abase + j], t.nv_y[abase + j]));
                far2 = d2 > far2 ? d2 : far2;
                if (j > i && (AP ? d2 < sqr(ri + c.ap_radius[abase + j]) : d2 < crSq)) ++pairs;
            }
            scan_all = list_misses_pairs(ncnt, AS ? K_own : K, far2, R, m2);
        }
        if (__syncthreads_or(scan_all ? 1 : 0)) {   // (workgroup-uniform: the barriers below are met by every lane)
            if (scan_all) pairs = 0;
            for (int ct = tile; ct < t.tiles; ++ct) {   // candidates j > i: this tile and the ones behind it
                const int j0 = ct * TILE;
                const int nj = min(TILE, N - j0);
                __syncthreads();
                if (tid < nj) {
                    s_px[tid] = t.nv_x[abase + j0 + tid]; s_py[tid] = t.nv_y[abase + j0 + tid];
                    if constexpr (AP) s_pr[tid] = c.ap_radius[abase + j0 + tid];
                }
                __syncthreads();
                if (scan_all) {
                    for (int jj = (ct == tile ? tid + 1 : 0); jj < nj; ++jj) {
                        const float d2 = absSq(pos - mk(s_px[jj], s_py[jj]));
                        if (AP ? d2 < sqr(ri + s_pr[jj]) : d2 < crSq) ++pairs;
                    }
                }
            }
        }
        if (pairs) atomicAdd(&s_pairs, pairs);
        __syncthreads();
        if (tid == 0 && s_pairs) atomicAdd(&c.arena_stats[(size_t)a * ST_STRIDE + ST_COLL], (unsigned long long)s_pairs);
    }

    const bool nodone = (p.flags & 8u) != 0;  // CA_F_NODONE
    const int steps = tiled_steps_after((int)sc[TS_STEPS0], p.actions != nullptr, nodone);
    const int not_done = (int)sc[TS_NOTDONE];
    const bool all_done = episode_over(c, nodone, not_done, steps);
    const bool do_reset = all_done && (p.flags & 4u);  // CA_F_AUTORESET
    const int epi = (int)sc[TS_EPI];
    if (active && do_reset) {  // env.py:461-488 for this arena
        const V2 pos = spawn_draw(c, a, i, epi);
        const V2 pref = goal_dir(pos, c.goal_x[q], c.goal_y[q]);
        c.agent_done[q] = 0;
        c.pos_x[q] = pos.x; c.pos_y[q] = pos.y;
        c.pref_x[q] = pref.x; c.pref_y[q] = pref.y;
        c.orient_x[q] = pref.x; c.orient_y[q] = pref.y;
    }
    if (tile == 0 && tid == 0) {   // the arena's words (the other workgroups add to ST_COLL only)
        unsigned long long* st = c.arena_stats + (size_t)a * ST_STRIDE;
        if (all_done) { atomicAdd(&st[ST_EPISODES], 1ull); st[ST_LASTEP] = lastep_word(steps, N, not_done); }
        c.arena_done[a] = all_done ? 1 : 0;
        c.step_count[a] = do_reset ? 0 : steps;
        atomicAdd(&c.arena_steps[a], 1ull);
        if (do_reset) c.episode[a] = epi + 1;
    }
}

}  // namespace ca

