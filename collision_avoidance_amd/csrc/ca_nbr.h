// ca_nbr.h -- neighbour search (App. A.2): sorted key lists, brute-force and uniform-grid scans
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview and the numerics contract).
#pragma once
#include "ca_common.h"

namespace ca {

// Sorted insertion into a register-resident list kept ascending, the last entry falling off.
// An entry is the 64-bit key (distance bits << 32 | index) held in a double register pair: for
// non-negative floats the bit pattern is monotone, so key order IS the (distance, index) order of the
// contract (App. A.2: ascending distance, ties to the lower index), and as positive, never-NaN doubles
// the keys are ordered by v_min_f64 / v_max_f64.  Insertion is then, for every slot independently and
// in place,   new[k] = max(old[k-1], min(old[k], x))   -- two VALU instructions per slot, no compare
// masks, no register copies.  (Inline asm because the compiler would add a canonicalising
// v_max_f64 v,v,v per operand; keys are never NaN so nothing needs quieting.)
// A list shorter than the array is stored RIGHT-ALIGNED behind dummy -inf slots (which never move):
// its largest key is then always the last element, a compile-time index.
__device__ __forceinline__ double key_min(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double key_max(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double make_key(float d, int idx) {
    return __longlong_as_double((long long)(((unsigned long long)__float_as_uint(d) << 32) | (unsigned)idx));
}
// the two keys that are no candidate: an empty slot (+inf, -1) sorts behind every candidate; a dummy slot (-inf) never moves
__device__ __forceinline__ double key_empty() { return __longlong_as_double(0x7F800000FFFFFFFFll); }
__device__ __forceinline__ double key_dummy() { return __longlong_as_double((long long)0xFFF0000000000000ull); }
__device__ __forceinline__ float key_dist(double k) { return __uint_as_float((unsigned)((unsigned long long)__double_as_longlong(k) >> 32)); }
__device__ __forceinline__ int key_index(double k) { return (int)(unsigned)(unsigned long long)__double_as_longlong(k); }
__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
template <int MAXN>
__device__ __forceinline__ void sorted_insert(double (&key)[MAXN], double x) {
#pragma unroll
    for (int k = MAXN - 1; k >= 1; --k) key[k] = key_max(key[k - 1], key_min(key[k], x));
    key[0] = key_min(key[0], x);
}

// A sorted list too long for registers (the wide obstacle lists, up to SWIDE keys): the lane's column of 64-bit words in LDS, slot k
// at col[k * STRIDE], ascending in slots [0, cnt).  The key is `distance bits << 32 | index`, sorted_insert's order as an integer.  A
// newcomer shifts the larger keys up by one slot; on a full list (cnt == cap) the largest key falls off -- the newcomer itself, if it
// is that -- so the list is the cap smallest keys whatever order they arrive in.  Stated once for the one-workgroup kernel (nbr_body)
// and the tiled solve launch (ca_tiled.h).  (A closure written out -- references to the caller's three variables -- and not a function
// with parameters: through one the instruction text of the wide step_kernel instantiations moved.)
template <int STRIDE>
struct WideInsert {
    unsigned long long*& col;   // the lane's column, its fill and its capacity
    int& cnt;
    const int& cap;
    __device__ __forceinline__ void operator()(unsigned long long x) const {
        int k = cnt;
        if (cnt == cap) {
            if (col[(cap - 1) * STRIDE] < x) return;
            k = cap - 1;
        } else {
            ++cnt;
        }
        while (k > 0) {
            const unsigned long long y = col[(k - 1) * STRIDE];
            if (y < x) break;
            col[k * STRIDE] = y;
            --k;
        }
        col[k * STRIDE] = x;
    }
};
// the index of slot k as the lists store it: an empty slot reads -1, as in the register form
template <int STRIDE>
__device__ __forceinline__ unsigned short wide_id(const unsigned long long* col, int cnt, int k) {
    return k < cnt ? (unsigned short)(unsigned)col[k * STRIDE] : (unsigned short)0xFFFFu;
}
__device__ __forceinline__ unsigned long long wide_key(float d, int idx) { return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)idx; }

// App. A.2, the range test of the obstacle-neighbour list: the agent at pos is on the outer side of edge o1, within range of its line and -- only then
// computed, into dsq -- of the segment.  `mine`: this lane really has such an edge (inside, and the statements in this order: the kernels' text depends on it).
__device__ __forceinline__ bool edge_in_range(const ObstDev& o1, V2 pos, float rangeSq, bool mine, float& dsq) {
    const V2 a1 = mk(o1.px, o1.py), a2 = mk(o1.qx, o1.qy);
    const float alol = leftOf(a1, a2, pos);
    const float dsl = div_ir(sqr(alol), absSq(a2 - a1));   // (an edge has a length; the quotient is only compared with the range)
    if (mine && dsl < rangeSq && alol < 0.0f) {
        dsq = distSqPointSegment(a1, a2, pos);
        if (dsq < rangeSq) return true;
    }
    return false;
}

// ============================================================================================
// Neighbour search for every agent (App. A.2): the obstacle edges within range and
// the K nearest agents, written as the lists [A,S,N] / [A,K,N] that the solve kernel and the
// observation read.  It runs at the head of the solve kernel (ca_step.h step_kernel).
// ============================================================================================
// SM: capacity of the register list of obstacle neighbours (S <= SM): 4 for the register-line solve, SMAX for the LDS table.
// SM > SMAX (the wide LDS-table kernels, lists of up to SWIDE edges): 2 SM registers for the keys do not exist, so the sorted list
// is built in LDS instead -- in the line table, which is idle until the lines are built after the search: key slot k of lane t
// is the 64-bit word [k][t] at the head of the kernel's dynamic LDS (S x 8 B per lane, always less than the table's (K + S) x 16 B;
// the 64-bit words of consecutive lanes are consecutive in LDS, the conflict-free pattern of a ds_read_b64 / ds_write_b64).  Only
// the lane itself touches its column, and the solve kernel has a barrier between the search and its first line.  The order is
// sorted_insert's: ascending (distance, index) key.  Cost: a data-dependent shift loop per accepted edge -- edges arrive in index
// order, not by distance, so an insert is up to S LDS round trips on the slowest lane of the wave.
// AP (the AgentParams instantiation of the solve kernel): the range of the obstacle search is the agent's own,
// sqr(time_horizon_obst_i * max_speed_i + radius_i), from the per-agent arrays of the cold block.
// AC (the ArenaCounts instantiation): arena a holds n_a = agent_counts[a] agents.  A lane is active for i < n_a, and a candidate j
// counts for j < n_a: the loops over candidates keep their wave-uniform trip count N (several arenas of different counts may share
// a wave) and the count joins the accept test, so the staged position of an absent lane is never taken, whatever it holds.  The
// grid scan sorts the present agents only.
// AS (the AgentSensing instantiations): agent i's list is the K_i = as_max_neighbors[i] smallest (dsq, j) keys with dsq < fl(nd_i * nd_i),
// nd_i = as_neighbor_dist[i] -- the oracle's compute_neighbors with the agent's own two values.  K_i <= K and nd_i <= neighbor_dist
// (checked by the host), so that list is the head of the K-list taken with range nd_i: the three searches below test against the
// lane's fl(nd_i^2) and keep K slots as before, and the cut to K_i entries is made once, where the list is stored (slots at or beyond
// the count read -1).  What is wave-uniform stays the handle's: K and its right-aligned register list, the composite-key image
// (top / u0 from neighbor_dist^2: a passing dsq lies below fl(nd_i^2) <= fl(neighbor_dist^2), so the image is exact over the same
// binades), the grid's cell size and the block of cells walked (B from neighbor_dist covers every smaller range).  Lists are
// asymmetric -- i may hold j while j does not hold i -- and nothing below relies on symmetry: a lane reads positions, never lists.
#ifndef CA_CK_MAXN
#define CA_CK_MAXN 64    // the largest arena that first tries the composite keys (see below: larger arenas measured slower)
#endif
// SD (the SeededScan instantiations of the solve kernel; CA_NBR_SEED, build switch: 0 = there are none): the composite-key scan of
// arenas of at most 64 agents starts from the lane's list of the LAST step and skips, wave-wide, every candidate that no lane can
// take (see the scan itself, below).  One-wave workgroups only -- an arena of at most 64 agents has no other (ca_create: BS =
// max(64, P)) -- and never with AgentSensing: those kernels store K_i < K entries, so their seed never fills the K slots and most
// candidates in range would run the network anyway.  Without the tag the scan starts every list empty and runs the insertion
// network for every candidate, as it always did: those instantiations keep their instruction text.
#ifndef CA_NBR_SEED
#define CA_NBR_SEED 1
#endif
template <int KMAX, int BS, int SM, bool AP = false, bool AC = false, bool AS = false, bool SD = false>
__device__ __forceinline__ void nbr_body(const StepArgs& p) {
    static_assert(!SD || (CA_NBR_SEED && !AS && BS == 64), "the seeded scan: one wave, not with AgentSensing");
#ifndef CA_NBR_NO_VGPR_PAD
    // Claim 128 VGPRs (the kernel needs 56): at most 4 waves then fit on a SIMD, so a launch that brings one
    // wave per SIMD slot (4096 x 64 lanes on 256 CUs) is spread evenly.  Without it the dispatcher puts
    // anything from 1 to 7 of these light waves on a SIMD and the kernel waits for the fullest one.
    asm volatile("" ::: "v127");
#endif
    __shared__ float s_px[BS];
    __shared__ float s_py[BS];
    const int tid = threadIdx.x;
    const int P = p.P;
    int la, i;
    lane_slot(p, tid, la, i);
    const int apb = p.apb;
    const int a = p.a0 + work_block(p) * apb + la;
    int n_a = p.N;   // agents of this lane's arena
    if constexpr (AC) n_a = ((a < p.a1) && (la < apb)) ? p.cold->agent_counts[a] : 0;
    const bool active = (a < p.a1) && (i < n_a) && (la < apb) && !arena_frozen(p, a);
    const int N = p.N, K = p.K, S = p.S;
    const int q = active ? a * N + i : 0;
    const int lbase = tid - i;
    CA_STAMP(12);
    V2 pos = mk(0.0f, 0.0f);
    if (active) pos = mk(p.pos_x[q], p.pos_y[q]);
    s_px[tid] = pos.x; s_py[tid] = pos.y;
#if CA_NBR_SEED
    // (seeded scan) the lane's list of the last step -- count and K ids, whatever they hold: the scan below takes nothing from
    // them unchecked -- loaded here, so that the obstacle-edge loop hides the latency
    constexpr bool SEED = SD;
    [[maybe_unused]] int seed_n = 0;
    [[maybe_unused]] int seed_id[KMAX];
    if constexpr (SEED) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) seed_id[k] = 0;
        if (active && K > 0 && N <= CA_CK_MAXN) {
            seed_n = (int)p.counts[q] & 0xFF;
            // (one 64-bit index per lane and a scalar stride, not a 64-bit product per slot; slots at or beyond K read slot K - 1
            // again and are not looked at: no branch between the loads)
            size_t at = (size_t)a * K * N + i;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                seed_id[k] = ld_idx_t<CA_NBW16(BS)>(p.nb_idx, at);
                if (k + 1 < K) at += (unsigned)N;
            }
        }
    }
#endif
    __syncthreads();

    const float INF = __int_as_float(0x7f800000);
    // ---- obstacle neighbours (App. A.2): brute force over the edge table ----
    constexpr bool WIDE = SM > SMAX;
    constexpr int SR = WIDE ? 1 : SM;   // register slots of the list (wide: none, the list is in LDS)
    const int sofs = SR - S;  // the S-entry list is right-aligned in the register array
    double okey[SR];
#pragma unroll
    for (int k = 0; k < SR; ++k) okey[k] = (k < sofs) ? key_dummy() : key_empty();
    int oin = 0;
    // (wide) the lane's column of the LDS list (WideList above)
    unsigned long long* wkey = nullptr;
    int wcnt = 0;
    if constexpr (WIDE) {
        extern __shared__ float4 smem4[];
        wkey = reinterpret_cast<unsigned long long*>(smem4) + tid;
    }
    const WideInsert<BS> wide_insert{wkey, wcnt, S};
    {
        float rangeSq = sqr(p.time_horizon_obst * p.max_speed + p.radius);
        if constexpr (AP) {
            const StepCold* cp = p.cold;
            rangeSq = active ? sqr(cp->ap_time_horizon_obst[q] * cp->ap_max_speed[q] + cp->ap_radius[q]) : 0.0f;
        }
        auto visit = [&](const ObstDev& o1, int e, bool mine) __attribute__((always_inline)) {
            float dsq;
            if (edge_in_range(o1, pos, rangeSq, mine, dsq)) {
                ++oin;
                if constexpr (WIDE) wide_insert(wide_key(dsq, e));
                else sorted_insert<SR>(okey, make_key(dsq, e));
            }
        };
        if (p.tab_off == nullptr) {  // one table for every arena: uniform loop, scalar loads of the edge records
            for (int e = 0; e < p.n_obst; ++e) visit(p.obst[e], e, active);
        } else {                     // a table per arena (several arenas may share this wave): ids are local to it
            const ArenaEdges E = arena_edges(p, a, active);
            for (int e = 0; __ballot(e < E.n) != 0ull; ++e) {
                const bool mine = e < E.n;
                visit(load_obst(p.obst, mine ? E.off + e : 0), e, mine);
            }
        }
    }
    const int ocnt = oin < S ? oin : S;
    if constexpr (WIDE) {     // the LDS list goes to memory before the agent scan (an empty slot reads -1, as in the register form)
        if (active) {
            for (int k = 0; k < S; ++k) p.obst_idx[((size_t)a * S + k) * N + i] = wide_id<BS>(wkey, wcnt, k);
        }
    } else if constexpr (SM > 4) {   // a list of 16 keys is 32 registers: it goes to memory now, not after the agent scan
        if (active) {
#pragma unroll
            for (int k = 0; k < SM; ++k)
                if (k >= sofs) p.obst_idx[((size_t)a * S + (k - sofs)) * N + i] = (unsigned short)key_index(okey[k]);
        }
    }
    CA_STAMP(13);

    // ---- agent neighbours (App. A.2): K nearest within neighbor_dist, ties -> lower index ----
    const int kofs = KMAX - K;  // the K-entry list is right-aligned in the register array
    double nkey[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) nkey[k] = (k < kofs) ? key_dummy() : key_empty();
    int ncnt = 0;
    bool scanned = false;
    [[maybe_unused]] float ndSq_own = 0.0f;   // (AS) the lane's fl(nd_i^2): one fp32 product, as the oracle forms it
    [[maybe_unused]] int K_own = 0;           // (AS) the lane's K_i; an idle lane keeps nothing
    if constexpr (AS) {
        const StepCold* cp = p.cold;
        if (active) { ndSq_own = sqr(cp->as_neighbor_dist[q]); K_own = (int)cp->as_max_neighbors[q]; }
    }
    if constexpr (BS >= 256) {
        // Large arenas (one arena per workgroup, >= 192 agents): a uniform grid with cells at least neighbor_dist
        // wide, rebuilt in LDS every step (counting sort of the agent indices by cell), so that an agent scans
        // the block of cells around it -- one contiguous run of the sorted list per cell row -- instead of the whole arena.
        // The cells are visited in no particular index order, so a candidate enters on `distance <= current
        // K-th distance` and the 64-bit (distance, index) keys settle ties; the list is the same K smallest
        // keys within neighbor_dist that the index-order scan keeps.
        if (P == BS && N >= 192 && K > 0) {
            constexpr int GMAX = BS >= 1024 ? 16 : 32;  // at most GMAX x GMAX cells (the 1024-lane shape has no LDS to spare)
            __shared__ unsigned s_box[4];          // ordered-uint images of min x, min y, max x, max y
            __shared__ int s_ccnt[GMAX * GMAX];    // agents per cell
            __shared__ int s_cstart[GMAX * GMAX + 1];  // first position of a cell in s_sorted
            __shared__ unsigned short s_sorted[BS];
            auto ord = [](float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
            auto unord = [](unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); };
            if (tid < 2) s_box[tid] = 0xFFFFFFFFu;
            if (tid >= 2 && tid < 4) s_box[tid] = 0u;
            for (int cidx = tid; cidx < GMAX * GMAX; cidx += BS) s_ccnt[cidx] = 0;
            __syncthreads();
            const bool in_arena = (a < p.a1) && (i < n_a);  // frozen arenas skip the scan but keep the barriers
            {  // the arena's bounding box: a reduction per wave, then one atomic per wave and corner
                const unsigned ox = ord(pos.x), oy = ord(pos.y);
                const unsigned bx0 = wave_min_u32(in_arena ? ox : 0xFFFFFFFFu), by0 = wave_min_u32(in_arena ? oy : 0xFFFFFFFFu);
                const unsigned bx1 = wave_max_u32(in_arena ? ox : 0u), by1 = wave_max_u32(in_arena ? oy : 0u);
                if ((tid & 63) == 63) {
                    atomicMin(&s_box[0], bx0); atomicMin(&s_box[1], by0);
                    atomicMax(&s_box[2], bx1); atomicMax(&s_box[3], by1);
                }
            }
            __syncthreads();
            // Cells half a neighbour range wide (the 5 x 5 block around an agent's cell covers its range with 156 / 225 of
            // the area of 3 x 3 cells a full range wide: a third fewer candidates), or wider when the arena is so large that
            // 32 x 32 of them would not cover it.
            const float x0 = unord(s_box[0]), y0 = unord(s_box[1]);
            const float ex = unord(s_box[2]) - x0, ey = unord(s_box[3]) - y0;
            const float cs = fmaxf((GMAX >= 32 ? 0.5f : 1.0f) * p.neighbor_dist, fmaxf(ex, ey) * (1.0f / (GMAX - 0.5f)));
            const float ics = 1.0f / cs;
            const int Gx = min(GMAX, (int)(ex * ics) + 1), Gy = min(GMAX, (int)(ey * ics) + 1);
            const int cx = min(Gx - 1, max(0, (int)((pos.x - x0) * ics))), cy = min(Gy - 1, max(0, (int)((pos.y - y0) * ics)));
            int rank = 0;
            if (in_arena) rank = atomicAdd(&s_ccnt[cy * Gx + cx], 1);
            __syncthreads();
            if (tid < 64) {  // exclusive prefix sum over the cells: GMAX^2 / 64 cells per lane of the first wave
                constexpr int CPL = GMAX * GMAX / 64;
                int cnt[CPL];
                int sum = 0;
#pragma unroll
                for (int k = 0; k < CPL; ++k) { cnt[k] = s_ccnt[CPL * tid + k]; sum += cnt[k]; }
                int incl = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int t = __shfl_up(incl, off);
                    if (tid >= off) incl += t;
                }
                int b = incl - sum;
#pragma unroll
                for (int k = 0; k < CPL; ++k) { s_cstart[CPL * tid + k] = b; b += cnt[k]; }
                if (tid == 63) s_cstart[GMAX * GMAX] = incl;
            }
            __syncthreads();
            // (up to 512 lanes the positions are sorted along with the indices: a candidate then is one LDS address, known
            // an iteration ahead, instead of an index and a dependent gather; the 1024-lane shape has no LDS for that)
            constexpr bool SXY = BS <= 512;
            __shared__ float2 s_sxy[SXY ? BS : 1];
            if (in_arena) {
                const int dst = s_cstart[cy * Gx + cx] + rank;
                s_sorted[dst] = (unsigned short)i;
                if constexpr (SXY) s_sxy[dst] = make_float2(pos.x, pos.y);
            }
            __syncthreads();
            const float rangeSq0 = AS ? ndSq_own : sqr(p.neighbor_dist);
            float rangeK = rangeSq0;  // distance of the current K-th entry once the list is full
            // WHICH CELLS.  Not a fixed block cx +- RC: pos - x0 and its product with ics are rounded, so a candidate a few
            // ulps inside the range can land one cell beyond such a block (a pair at |dx| = nd - 1 ulp, 3 cells apart at
            // cs = nd / 2).  A candidate that passes fl(fl(dx^2) + fl(dy^2)) < fl(nd^2) has fl(dx^2) < fl(nd^2), hence
            // |xi - xj| < nd (1 + 2^-21) < B = nd * 1.0001 + 1e-4 (and so in y): xj >= xi - B exactly, and as xj is a float,
            // fl(xi - B) <= xj.  The cell index (the same expression as below) is monotone in the coordinate, so the cell of
            // xj lies between the cells of fl(xi - B) and fl(xi + B) -- the bounds the pair kernel takes (ca_pair.h).
            const float B = p.neighbor_dist * 1.0001f + 1e-4f;
            // (both ends clamped to the grid, as cx / cy are: every LDS index below stays in bounds whatever the positions hold)
            auto cell_of = [&](float v, float v0, int G) { return min(G - 1, max(0, (int)((v - v0) * ics))); };
            const int cxlo = cell_of(pos.x - B, x0, Gx), cxhi = cell_of(pos.x + B, x0, Gx);
            const int cylo = cell_of(pos.y - B, y0, Gy), cyhi = cell_of(pos.y + B, y0, Gy);
            const int rowend = active ? cyhi : cylo - 1;
            auto row_range = [&](int row, int& lo, int& hi) {
                lo = s_cstart[row * Gx + cxlo];
                hi = s_cstart[row * Gx + cxhi + 1];
            };
            auto visit = [&](int j, const V2& o) {
                const float dsq = absSq(pos - o);
                if (j != i && dsq < rangeSq0 && dsq <= rangeK) {
                    sorted_insert<KMAX>(nkey, make_key(dsq, j));
                    if (ncnt < K) ++ncnt;
                    if (ncnt == K) rangeK = key_dist(nkey[KMAX - 1]);
                }
            };
            int lo_n = 0, hi_n = 0;
            if (cylo <= rowend) row_range(cylo, lo_n, hi_n);
            for (int row = cylo; row <= rowend; ++row) {
                const int lo = lo_n, hi = hi_n;
                if (row < rowend) row_range(row + 1, lo_n, hi_n);  // the next row's bounds are in flight during this row
                int t = lo;
                if constexpr (SXY) {
                    int jn = 0;
                    float2 on = make_float2(0.0f, 0.0f);
                    if (t < hi) { jn = s_sorted[t]; on = s_sxy[t]; }
                    while (t < hi) {
                        const int j = jn;
                        const V2 o = mk(on.x, on.y);
                        ++t;
                        if (t < hi) { jn = s_sorted[t]; on = s_sxy[t]; }  // the next candidate is in flight during this one
                        visit(j, o);
                    }
                } else {
                    for (; t < hi; ++t) {
                        const int j = s_sorted[t];
                        visit(j, mk(s_px[j], s_py[j]));
                    }
                }
            }
            scanned = true;
        }
    }
    if (K > 0 && !scanned && N <= CA_CK_MAXN) {
        // Arenas of at most 64 agents: 32-bit composite keys = (distance image << logP) | candidate index and
        // one v_med3_u32 per list slot and candidate -- new[k] = med3(old[k-1], old[k], x) IS the sorted insert,
        // at half the instructions of the 64-bit network (in so small an arena some lane accepts nearly every
        // candidate, so the shrinking range of the contract never lets a wave skip the network anyway -- as long as
        // every list starts empty: the seeded scan below, CA_NBR_SEED, starts from last step's list and does skip).
        // The image is the fp32 BIT PATTERN of the squared distance, counted down from that of neighbor_dist^2
        // (round 5): 32 - logP bits hold every float of the top 2^(9 - logP) binades below the range -- for 64 agents and a range
        // of 5 every d2 in [0.125, 25) -- at full resolution, so there the composite order IS the contract's exact (distance, index)
        // order (equal images = equal distances = index order), and everything nearer than that is clamped to image 0.  Only a
        // lane with two or more such candidates (agents within 0.35 of each other at radius 0.5: deep overlaps) cannot order
        // them; a wave in which some lane has them falls through to the exact 64-bit scan below.  (Rounds 2-4 used a fixed-point
        // image floor(d2 * 2^26 / 25): a settled crowd packs at exactly the contact distance, the neighbours of an agent in a
        // dense core differ by a few ulps of d2 = 1 -- less than that image resolves -- and every fifth wave scanned twice:
        // profiles/r05_c_exact_composite_keys.txt.)
        const float rangeSq0 = sqr(p.neighbor_dist);
        const unsigned lowmask = (unsigned)(P - 1);
        const unsigned top = __float_as_uint(rangeSq0);                  // a passing candidate's bits lie below it
        const unsigned span = 0xFFFFFFFFu >> p.logP;                     // images 0 .. span - 2 (the composite never is ~0)
        // bit patterns up to u0 share image 0 (arenas of at most four lanes with a range below 1: every pattern fits, u0 = 0)
        const unsigned u0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(top >= span ? top - span + 1u : 0u));
        unsigned ck[KMAX + 1];
#pragma unroll
        for (int k = 0; k <= KMAX; ++k) ck[k] = (k < kofs) ? 0u : 0xFFFFFFFFu;
        auto visit = [&](int j, V2 o) __attribute__((always_inline)) {
            const float dsq = absSq(pos - o);
            const bool pass = active && j != i && (!AC || j < n_a) && dsq < (AS ? ndSq_own : rangeSq0);
            const unsigned u = __float_as_uint(dsq);
            unsigned key = (((u > u0 ? u : u0) - u0) << p.logP) | (unsigned)j;
            asm volatile("" : "+v"(key));   // (computed for every lane: left to itself the compiler branches around these three
            const unsigned c = pass ? key : 0xFFFFFFFFu;   // instructions, twice per candidate; now one v_cndmask)
#pragma unroll
            for (int k = KMAX; k >= 1; --k) ck[k] = umed3(ck[k - 1], ck[k], c);
            ck[0] = ck[0] < c ? ck[0] : c;
        };
#if CA_NBR_SEED
        if constexpr (SEED) {
            // THE SEEDED SCAN.  An agent moves at most max_speed * time_step per step, a sixtieth of its radius or so: the K nearest
            // of this step are, but for one or two, those of the last.  So the list starts from them -- the lane's K ids of the last
            // step, inserted first with their CURRENT distances through the same pass test, key and network -- and the scan in
            // index order then runs the network only for a candidate that some lane of the wave can still take: one whose squared
            // distance is at most the lane's threshold, the distance of its current K-th key (the range, while the list is short),
            // and that the lane has not inserted already.  Everything else is five instructions of distance and three of test.
            // WHY THE LISTS ARE THE SAME BITS.  A key c >= ck[KMAX - 1], the lane's K-th smallest so far, leaves slots 0 .. KMAX - 1
            // as they are: slot k becomes med3(ck[k - 1], ck[k], c) = ck[k].  It can only enter slot KMAX, which is read once, by
            // clamped_pair when K = 1 (the second smallest key): there the threshold is that of ck[KMAX].  The K-th smallest only
            // shrinks, so a skipped candidate is none of the final K smallest, and the K smallest of a set of distinct keys (the index
            // sits in the low bits) do not depend on the order of insertion.  Each candidate is inserted at most once: `vis` holds,
            // per lane, a bit for itself, for every absent row (AC: j >= n_a; an idle lane: all 64) and for every seed member taken.
            // Two clamped candidates carry the smallest keys there are, never above a threshold: clamped_pair sees what it saw.
            // The threshold is the K-th key's image taken back to fp32 bits, u0 + (key >> logP), capped at the bits of the range
            // (top): key_c < key_K implies image_c <= image_K, that is max(u_c, u0) <= u0 + image_K, and a passing u_c lies below top.
            // Squared distances are non-negative, so their order as floats is their order as unsigned bit patterns (a NaN lies
            // above top either way and never passes, here as in the exact test).
            // THE SEED IS NOT TRUSTED: the lists are settable (ca_set), stale after a reset or set_state, zero in a fresh handle.
            // The count is clamped to K; a member is taken only if it is a present row other than the lane's own and not yet
            // taken (the vis bit), and only then is its position read from the staged arena.
            unsigned long long vis = ~0ull;
            if (active) vis = (n_a < 64 ? ~0ull << n_a : 0ull) | (1ull << i);
            auto insert = [&](unsigned jj, float dsq, bool take) __attribute__((always_inline)) {
                const bool pass = take && dsq < rangeSq0;
                const unsigned u = __float_as_uint(dsq);
                unsigned key = (((u > u0 ? u : u0) - u0) << p.logP) | jj;
                asm volatile("" : "+v"(key));   // (as in visit above)
                const unsigned c = pass ? key : 0xFFFFFFFFu;
#pragma unroll
                for (int k = KMAX; k >= 1; --k) ck[k] = umed3(ck[k - 1], ck[k], c);
                ck[0] = ck[0] < c ? ck[0] : c;
            };
            unsigned thr = 0u;
            auto refresh = [&]() __attribute__((always_inline)) {
                const unsigned kth = (K >= 2) ? ck[KMAX - 1] : ck[KMAX];
                const unsigned t = u0 + (kth >> p.logP);   // (no overflow: at most top + 1, or u0 = 0)
                thr = t < top ? t : top;
            };
            const int sn = seed_n < K ? seed_n : K;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                if (k < K) {   // wave-uniform
                    // (a slot that holds no member stands for the lane itself: its bit is set, so it is never taken, and its
                    // staged position is the lane's own slot -- no test of its own, no index that was not checked)
                    const unsigned m = (unsigned)seed_id[k];
                    const unsigned mm = (k < sn && m < (unsigned)n_a) ? m : (unsigned)i;
                    const unsigned long long bit = 1ull << mm;
                    const bool ok = (vis & bit) == 0ull;
                    if (__builtin_amdgcn_ballot_w64(ok) != 0ull) {   // wave-uniform
                        vis |= bit;
                        const int src = lbase + (int)mm;
                        insert(mm, absSq(pos - mk(s_px[src], s_py[src])), ok);
                    }
                }
            }
            refresh();
#ifdef CA_STAMPS
            unsigned long long dbg_trips = 0ull, dbg_ran = 0ull;
#endif
            // a candidate this lane can still take: not taken yet, at or below the threshold (ties pass: the exact test follows)
            auto want = [&](unsigned visw, unsigned bit, float dsq) __attribute__((always_inline)) {
                return __float_as_uint(dsq) <= thr && (visw & bit) == 0u;
            };
            auto take = [&](int jj, unsigned visw, unsigned bit, float dsq, bool w) __attribute__((always_inline)) {
                if (__builtin_amdgcn_ballot_w64(w) != 0ull) {   // wave-uniform: some lane can take candidate jj
                    insert((unsigned)jj, dsq, (visw & bit) == 0u);
                    refresh();
#ifdef CA_STAMPS
                    ++dbg_ran;
#endif
                }
            };
            int j = 0;
            for (; j + 4 <= N; j += 4) {   // (four per trip, positions read at the head of the trip: as in the unseeded scan below)
                const V2 o0 = mk(s_px[lbase + j], s_py[lbase + j]), o1 = mk(s_px[lbase + j + 1], s_py[lbase + j + 1]);
                const V2 o2 = mk(s_px[lbase + j + 2], s_py[lbase + j + 2]), o3 = mk(s_px[lbase + j + 3], s_py[lbase + j + 3]);
                const unsigned visw = (j & 32) ? (unsigned)(vis >> 32) : (unsigned)vis;   // (j is a multiple of four: one word for the trip)
                const unsigned b0 = 1u << (j & 31);
                const float d0 = absSq(pos - o0), d1 = absSq(pos - o1), d2 = absSq(pos - o2), d3 = absSq(pos - o3);
                const bool w0 = want(visw, b0, d0), w1 = want(visw, b0 << 1, d1), w2 = want(visw, b0 << 2, d2), w3 = want(visw, b0 << 3, d3);
#ifdef CA_STAMPS
                dbg_trips += 4;
#endif
                if (__builtin_amdgcn_ballot_w64(w0 || w1 || w2 || w3) != 0ull) {   // wave-uniform
                    take(j, visw, b0, d0, w0); take(j + 1, visw, b0 << 1, d1, w1);
                    take(j + 2, visw, b0 << 2, d2, w2); take(j + 3, visw, b0 << 3, d3, w3);
                }
            }
            for (; j < N; ++j) {
                const unsigned visw = (j & 32) ? (unsigned)(vis >> 32) : (unsigned)vis;
                const unsigned b = 1u << (j & 31);
                const float d = absSq(pos - mk(s_px[lbase + j], s_py[lbase + j]));
#ifdef CA_STAMPS
                ++dbg_trips;
#endif
                take(j, visw, b, d, want(visw, b, d));
            }
#ifdef CA_STAMPS   // (diagnostic build) this wave's candidate trips and how many of them ran the network: the row behind the launch's time stamps
            // (rows [0, ceil(A / apb)) are the time stamps of a launch over all arenas, one per wave, indexed by blockIdx.x as CA_STAMP
            // does; the counts go behind them whatever this launch's own grid is -- a chunked launch (a0 > 0) overwrites rows from 0,
            // like its stamps, and a block order (work_block) changes which arenas a row stands for, not the row)
            if (CA_STAMPS < 3 && (tid & 63) == 0 && p.dbg) {
                unsigned long long* r = p.dbg + ((size_t)((p.A + apb - 1) / apb + blockIdx.x) * (BS / 64) + (tid >> 6)) * 16;
                r[0] = dbg_trips; r[1] = dbg_ran;
            }
#endif
        } else
#endif
        {
        // four candidates per trip, their positions read at the head of the trip (immediate LDS offsets, no register rotation
        // between trips: the rolled loop with a one-ahead prefetch spent 5 of its 28 vector instructions per candidate on moves
        // and address increments)
        int j = 0;
        for (; j + 4 <= N; j += 4) {
            const V2 o0 = mk(s_px[lbase + j], s_py[lbase + j]), o1 = mk(s_px[lbase + j + 1], s_py[lbase + j + 1]);
            const V2 o2 = mk(s_px[lbase + j + 2], s_py[lbase + j + 2]), o3 = mk(s_px[lbase + j + 3], s_py[lbase + j + 3]);
            visit(j, o0); visit(j + 1, o1); visit(j + 2, o2); visit(j + 3, o3);
        }
        for (; j < N; ++j) visit(j, mk(s_px[lbase + j], s_py[lbase + j]));
        }
        int cnt = 0;
        bool clamped_pair = false;   // (the list is ascending: two clamped candidates, if there are any, are its first two entries)
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k >= kofs && ck[k] != 0xFFFFFFFFu) ++cnt;
            if (k == kofs) clamped_pair = ck[k + 1] <= lowmask;
        }
        if (__builtin_amdgcn_ballot_w64(clamped_pair) == 0ull) {  // wave-uniform
            ncnt = cnt;
#pragma unroll
            for (int k = 0; k < KMAX; ++k)  // hand the indices over in the key array the store below reads
                nkey[k] = (k < kofs) ? key_dummy() : make_key(0.0f, (ck[k] == 0xFFFFFFFFu) ? -1 : (int)(ck[k] & lowmask));
            scanned = true;
        }
    }
    if (K > 0 && !scanned) {
        float rangeSq = AS ? ndSq_own : sqr(p.neighbor_dist);
        V2 o_next = mk(s_px[lbase], s_py[lbase]);
        for (int j = 0; j < N; ++j) {
            const V2 o = o_next;  // the next candidate's position is in flight while this one is inserted
            if (j + 1 < N) o_next = mk(s_px[lbase + j + 1], s_py[lbase + j + 1]);
            const float dsq = absSq(pos - o);
            if (active && j != i && (!AC || j < n_a) && dsq < rangeSq) {
                sorted_insert<KMAX>(nkey, make_key(dsq, j));
                if (ncnt < K) ++ncnt;
                if (ncnt == K) rangeSq = key_dist(nkey[KMAX - 1]);
            }
        }
    }

    CA_STAMP(14);
    if (active) {
        if (__builtin_expect(oin > S, 0)) {
            atomicAdd(reinterpret_cast<int*>(&p.arena_stats[(size_t)a * ST_STRIDE + ST_OVERFLOW]), 1);
            note_overflow(p.cold, a, i, oin);
        }
        if constexpr (AS) ncnt = ncnt < K_own ? ncnt : K_own;   // the head of the K-list: its K_i nearest
        p.counts[q] = (unsigned short)(ncnt | (ocnt << 8));
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k >= kofs) st_idx_t<CA_NBW16(BS)>(p.nb_idx, ((size_t)a * K + (k - kofs)) * N + i, (AS && k - kofs >= K_own) ? -1 : key_index(nkey[k]));  // ids of <= 256 agents fit a byte
        if constexpr (SM <= 4) {
#pragma unroll
            for (int k = 0; k < SM; ++k)
                if (k >= sofs) p.obst_idx[((size_t)a * S + (k - sofs)) * N + i] = (unsigned short)key_index(okey[k]);
        }
    }
    CA_STAMP(15);
}

}  // namespace ca
