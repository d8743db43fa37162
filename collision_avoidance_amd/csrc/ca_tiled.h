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
//   tiled_grid_solve_kernel<KMAX, TILE>, tiled_advance_kernel, tiled_close_kernel.
// The table is fixed and wrapped: cell c(v) = floor(v * ics) of a coordinate, bucket (c(y) & (GY - 1)) * GX + (c(x) & (GX - 1)), GX and
// GY powers of two.  No bounding box (it would be one more arena-wide reduction, one more launch): wrapping only aliases far cells
// into near ones, and an aliased stranger fails the distance test.  The mask keeps every index inside the table whatever the
// position arrays hold.  The order inside a cell comes from the atomics and differs from run to run; the lists do not depend on it
// (tiled_solve_body).  Frozen arenas (CA_F_FREEZE) are skipped by all three: arena_done was last written by the close launch of
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
// and entries (edge id | the lowest column of the edge's cell rectangle << 16 | its lowest row << 24) -- and the twins of the two
// kernels walk the few cells an agent's range touches.  No launch, no sort, no barrier per step.  The table is unwrapped and clamped
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

// ---- launch 1: neighbour search, ORCA lines, LP2 / LP3 ------------------------------------------------------------------------
// The solve launch has three kernels with one body (ca_tiled_solve.inl; CA_TILED_PARAMS 0: the handle's four constants).
// Grid (tiled_grid_solve_kernel, a handle made with CA_CREATE_TILED_GRID): lane tile * TILE + tid works for SORTED POSITION s of the
// arena, its agent is i = sidx[s] -- the lanes of a wave then stand in the same few cells and walk the same runs -- and everything
// else addresses by i as before.
#define CA_TILED_PARAMS 0
template <int KMAX, int TILE>
__global__ __launch_bounds__(TILE) void tiled_solve_kernel(const TiledArgs t) {
#define CA_TILED_SOLVE_GRID 0
#include "ca_tiled_solve.inl"
#undef CA_TILED_SOLVE_GRID
}
template <int KMAX, int TILE>
__global__ __launch_bounds__(TILE) void tiled_grid_solve_kernel(const TiledGridArgs t) {
#define CA_TILED_SOLVE_GRID 1
#include "ca_tiled_solve.inl"
#undef CA_TILED_SOLVE_GRID
}
// ... and the grid kernel whose obstacle block walks the static edge grid (ca_tiled_edge_grid): everything else is the same text
template <int KMAX, int TILE>
__global__ __launch_bounds__(TILE) void tiled_grid_edges_solve_kernel(const TiledEdgeArgs t) {
#define CA_TILED_SOLVE_GRID 2
#include "ca_tiled_solve.inl"
#undef CA_TILED_SOLVE_GRID
}

// ---- launch 2: integrate, reward, wall / goal tests, the arena's partial results ---------------------------------------------------
// (any workgroup size: a workgroup is one tile of one arena, blockDim.x = TILE; two kernels with one body, ca_tiled_advance.inl)
__global__ __launch_bounds__(256) void tiled_advance_kernel(const TiledArgs t) {
#define CA_TILED_ADVANCE_EDGES 0
#include "ca_tiled_advance.inl"
#undef CA_TILED_ADVANCE_EDGES
}
__global__ __launch_bounds__(256) void tiled_grid_edges_advance_kernel(const TiledEdgeArgs t) {
#define CA_TILED_ADVANCE_EDGES 1
#include "ca_tiled_advance.inl"
#undef CA_TILED_ADVANCE_EDGES
}
#undef CA_TILED_PARAMS

// ---- launch 3: pair count on the copy, end of the episode, the arena's words, the in-kernel reset ---------------------------------
// dynamic LDS: the staged candidate tile px py [TILE] (8 B per lane); the statements are ca_tiled_close.inl's
__global__ __launch_bounds__(256) void tiled_close_kernel(const TiledArgs t) {
#define CA_TILED_PARAMS 0
#include "ca_tiled_close.inl"
#undef CA_TILED_PARAMS
}

// ---- the twins for per-agent ORCA parameters (a handle made with CA_CREATE_TILED_PARAMS, while ca_set_agent_params is in force) ------
// The same three texts with CA_TILED_PARAMS 1: radius, maximum speed and the two time horizons of agent i come from the per-agent arrays
// (StepCold::ap_*), a neighbour's radius is gathered beside its position and velocity, and each enters where DESIGN.md 7b says --
// the obstacle range sqr(tho_i * ms_i + r_i) and the edge-grid walk over cell(x +- (tho_i * ms_i + r_i)), the obstacle lines and their
// covered test (r_i, 1 / tho_i), the agent lines (r_i, r_j, 1 / th_i), LP2 / LP3 (ms_i), the wall and goal tests (r_i), the pair count
// (sqr(r_i + r_j)).  The sort launches are the uniform handle's: neighbor_dist and max_neighbors stay per handle.  The edge grid is
// built for the LARGEST range of the handle (ca_env.hip edge_grid_range); the corner rule of the walk does not depend on the cell
// size, so an agent of a smaller range simply walks fewer cells.
struct TiledCloseParamsArgs : TiledArgs {
    float r_max;   // the largest radius of the handle: R of lists_bound_pairs / list_misses_pairs (r_i + r_j <= 2 r_max)
};
// LDS of the close launch (bytes): the staged candidate tile px py [TILE], and with per-agent parameters its radii
__host__ __device__ inline size_t tiled_close_lds_bytes(int TILE, bool params) { return (size_t)TILE * (params ? 12 : 8); }

#define CA_TILED_PARAMS 1
template <int KMAX, int TILE>
__global__ __launch_bounds__(TILE) void tiled_params_solve_kernel(const TiledArgs t) {
#define CA_TILED_SOLVE_GRID 0
#include "ca_tiled_solve.inl"
#undef CA_TILED_SOLVE_GRID
}
template <int KMAX, int TILE>
__global__ __launch_bounds__(TILE) void tiled_params_grid_solve_kernel(const TiledGridArgs t) {
#define CA_TILED_SOLVE_GRID 1
#include "ca_tiled_solve.inl"
#undef CA_TILED_SOLVE_GRID
}
template <int KMAX, int TILE>
__global__ __launch_bounds__(TILE) void tiled_params_grid_edges_solve_kernel(const TiledEdgeArgs t) {
#define CA_TILED_SOLVE_GRID 2
#include "ca_tiled_solve.inl"
#undef CA_TILED_SOLVE_GRID
}
__global__ __launch_bounds__(256) void tiled_params_advance_kernel(const TiledArgs t) {
#define CA_TILED_ADVANCE_EDGES 0
#include "ca_tiled_advance.inl"
#undef CA_TILED_ADVANCE_EDGES
}
__global__ __launch_bounds__(256) void tiled_params_grid_edges_advance_kernel(const TiledEdgeArgs t) {
#define CA_TILED_ADVANCE_EDGES 1
#include "ca_tiled_advance.inl"
#undef CA_TILED_ADVANCE_EDGES
}
// dynamic LDS: the staged candidate tile px py r [TILE] (12 B per lane)
__global__ __launch_bounds__(256) void tiled_params_close_kernel(const TiledCloseParamsArgs t) {
#include "ca_tiled_close.inl"
}
#undef CA_TILED_PARAMS

}  // namespace ca
