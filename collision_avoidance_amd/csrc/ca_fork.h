// ca_fork.h -- the one kernel behind ca_arena_gather and ca_snapshot_save / ca_snapshot_load
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview).
//
// Moving an arena is pure data movement: every plane of the state (ca_env.hip state_planes) is [A][rows][n] elements of 1, 2, 4
// or 8 bytes, so "arena a := arena src[a]" is, per plane, a copy of rows * n * esize contiguous bytes from one set of buffers to
// another.  The host describes the planes in a small table that travels in the kernel arguments; one launch walks all of them:
//   * blockIdx.y is the plane, so a workgroup reads one descriptor through scalar loads and never searches the table;
//   * the work item is (arena, 16-byte chunk) where both bases and the arena's byte stride are multiples of 16 -- one 128-bit load
//     and one 128-bit store per lane, consecutive lanes on consecutive chunks --, and (arena, element) where they are not (the
//     reference's own shape has 50-byte rows of 8-bit ids) or where single elements have to be left out (per-arena agent counts);
//   * a grid-stride loop over the plane's items: 4096 arenas of 64 agents and one arena of 16384 both spread over the whole chip;
//   * no LDS, no scratch, nothing read twice: the roof is the HBM rate over bytes read + bytes written.
// A save has no index (arena a of the handle -> arena a of the set); a load has one, or none for "every arena", and skips the arenas
// it is told to keep, which are then not written at all.  The in-place gather is a save into the handle's scratch set followed by a
// load from it, so no lane ever reads what another may already have overwritten.
#pragma once
#include "ca_common.h"

namespace ca {

enum { FORK_BS = 256, FORK_MAX_PLANES = 24 };

struct ForkPlane {
    const unsigned char* src;   // arena 0 of the plane in the set that is read
    unsigned char* dst;         // ... and in the set that is written
    unsigned esize;             // bytes per element: 1, 2, 4 or 8
    unsigned n;                 // elements per row
    unsigned rows;              // rows per arena: 1 for an [A,N] plane, K or S for a list, n_actions for the bandit; an [A] word: n = rows = 1
    unsigned items;             // work items per arena: 16-byte chunks (vec) or elements
    unsigned vec;               // 1: bases and arena stride are multiples of 16 and every element moves
    unsigned per_agent;         // n is the agent axis: under per-arena counts only elements i < counts[a] of a row are written
    unsigned keep;              // AND mask over every 32 bits moved (all ones but for the packed list counts under a clearing rule)
};

struct ForkArgs {
    ForkPlane p[FORK_MAX_PLANES];
    const int* idx;      // INDEXED: [A] the arena of the source set that arena a takes; negative: arena a is kept
    const int* counts;   // COUNTS: [A] agents per arena (ca_set_agent_counts)
    int A;
    int keep_self;       // INDEXED: idx[a] == a keeps arena a as well (the gather: source and destination are the same arena)
};

template <class T>
__device__ __forceinline__ void fork_elem(const unsigned char* s, unsigned char* d, unsigned e, unsigned keep) {
    T v = reinterpret_cast<const T*>(s)[e];
    if constexpr (sizeof(T) == 8) v &= ((unsigned long long)keep << 32) | keep;
    else v = (T)(v & (T)keep);
    reinterpret_cast<T*>(d)[e] = v;
}

template <bool INDEXED, bool COUNTS>
__global__ __launch_bounds__(FORK_BS) void fork_kernel(const ForkArgs f) {
    const ForkPlane& pl = f.p[blockIdx.y];
    const unsigned items = pl.items;
    const unsigned long long total = (unsigned long long)(unsigned)f.A * items;
    const unsigned long long stride = (unsigned long long)gridDim.x * FORK_BS;
    const size_t arena_bytes = (size_t)pl.esize * pl.n * pl.rows;
    for (unsigned long long w = (unsigned long long)blockIdx.x * FORK_BS + threadIdx.x; w < total; w += stride) {
        unsigned a, c;
        if (w >> 32) { a = (unsigned)(w / items); c = (unsigned)(w - (unsigned long long)a * items); }
        else { a = (unsigned)w / items; c = (unsigned)w - a * items; }
        unsigned s = a;
        if constexpr (INDEXED) {
            const int si = f.idx[a];
            if (si < 0 || (f.keep_self && (unsigned)si == a)) continue;
            s = (unsigned)si;
        }
        const unsigned char* sp = pl.src + (size_t)s * arena_bytes;
        unsigned char* dp = pl.dst + (size_t)a * arena_bytes;
        if (pl.vec) {
            uint4 v = reinterpret_cast<const uint4*>(sp)[c];
            v.x &= pl.keep; v.y &= pl.keep; v.z &= pl.keep; v.w &= pl.keep;
            reinterpret_cast<uint4*>(dp)[c] = v;
        } else {
            if constexpr (COUNTS) {
                if (pl.per_agent && (int)(c % pl.n) >= f.counts[a]) continue;   // an absent row keeps what the caller put there
            }
            if (pl.esize == 4) fork_elem<unsigned>(sp, dp, c, pl.keep);
            else if (pl.esize == 8) fork_elem<unsigned long long>(sp, dp, c, pl.keep);
            else if (pl.esize == 2) fork_elem<unsigned short>(sp, dp, c, pl.keep);
            else fork_elem<unsigned char>(sp, dp, c, pl.keep);
        }
    }
}

}  // namespace ca
