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

// ---- launch 1: neighbour search, ORCA lines, LP2 / LP3 ------------------------------------------------------------------------
template <int KMAX, int TILE>
__global__ __launch_bounds__(TILE) void tiled_solve_kernel(const TiledArgs t) {
    const StepArgs& p = t.s;
    extern __shared__ float4 smem4[];
    const int tid = threadIdx.x;
    const int a = (int)blockIdx.x / t.tiles, tile = (int)blockIdx.x - a * t.tiles;
    const int N = p.N, K = p.K, S = p.S;
    const int i = tile * TILE + tid;
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

    // ---- obstacle neighbours (App. A.2; ca_nbr.h's keys; its edge_in_range and ca_common.h arena_edges written out: through them this kernel's text moved) ----
    const ObstDev* tab = p.obst + ((p.tab_off != nullptr) ? p.tab_off[a] : 0);          // this arena's edge table
    const int n_edges = p.tab_off != nullptr ? p.tab_off[a + 1] - p.tab_off[a] : p.n_obst;
    int oin = 0;
    {
        const int sofs = SMAX - S;   // the S-entry list is right-aligned in the register array
        double okey[SMAX];
#pragma unroll
        for (int k = 0; k < SMAX; ++k) okey[k] = (k < sofs) ? key_dummy() : key_empty();
        const float rangeSq = sqr(p.time_horizon_obst * p.max_speed + p.radius);
        for (int e = 0; e < n_edges; ++e) {   // (uniform: scalar loads of the edge records)
            const ObstDev& o1 = tab[e];
            const V2 a1 = mk(o1.px, o1.py), a2 = mk(o1.qx, o1.qy);
            const float alol = leftOf(a1, a2, pos);
            const float dsl = div_ir(sqr(alol), absSq(a2 - a1));
            if (active && dsl < rangeSq && alol < 0.0f) {
                const float dsq = distSqPointSegment(a1, a2, pos);
                if (dsq < rangeSq) {
                    ++oin;
                    sorted_insert<SMAX>(okey, make_key(dsq, e));
                }
            }
        }
        if (active) {
#pragma unroll
            for (int k = 0; k < SMAX; ++k)
                if (k >= sofs) p.obst_idx[((size_t)a * S + (k - sofs)) * N + i] = (unsigned short)key_index(okey[k]);
        }
    }
    const int ocnt = oin < S ? oin : S;

    // ---- agent neighbours: the K smallest (distance, index) keys below neighbor_dist^2, candidates in index order, a tile at a time
    // through LDS -- the oracle's scan, so the shrinking range is its strict one ----
    const int kofs = KMAX - K;
    double nkey[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) nkey[k] = (k < kofs) ? key_dummy() : key_empty();
    int ncnt = 0;
    if (K > 0) {
        float rangeSq = sqr(p.neighbor_dist);
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
    if (active) {
        if (__builtin_expect(oin > S, 0)) {
            atomicAdd(reinterpret_cast<int*>(&p.arena_stats[(size_t)a * ST_STRIDE + ST_OVERFLOW]), 1);
            note_overflow_tiled(p.cold, a, i, oin);
        }
        p.counts[q] = (unsigned short)(ncnt | (ocnt << 8));
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k >= kofs) st_idx_t<true>(p.nb_idx, ((size_t)a * K + (k - kofs)) * N + i, key_index(nkey[k]));
    }

    // ---- ORCA lines into the LDS table (step_kernel's LDS-table path; the neighbours' state gathered from global memory) ----
    int nl = 0;
    {
        const float invTO = 1.0f / p.time_horizon_obst;
        const float R = p.radius;
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
        const float invT = 1.0f / p.time_horizon;
        const float invDt = 1.0f / p.time_step;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k >= kofs && k - kofs < ncnt) {
                const size_t j = abase + (size_t)key_index(nkey[k]);
                ls.put(nl, agent_orca_line(pos, vel, mk(p.pos_x[j], p.pos_y[j]), mk(p.vel_x[j], p.vel_y[j]), p.radius, invT, invDt));
                ++nl;
            }
        }
    }
    // ---- 2-D linear program (App. A.5), LP3 where it is infeasible ----
    V2 nv = mk(0.0f, 0.0f);
    int fail = nl;
    if (active) fail = lp2(ls, nl, p.max_speed, pref, false, nv);
    if (active && fail < nl) lp3<KMAX + SMAX>((__attribute__((address_space(3))) char*)ls.base, ls.stride, nl, numObstLines, fail, p.max_speed, nv);
    if (active) { t.nv_x[q] = nv.x; t.nv_y[q] = nv.y; }
}

// ---- launch 2: integrate, reward, wall / goal tests, the arena's partial results ---------------------------------------------------
// (any workgroup size: a workgroup is one tile of one arena, blockDim.x = TILE)
__global__ __launch_bounds__(256) void tiled_advance_kernel(const TiledArgs t) {
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
            if (touches_wall(tab, ne, pos, p.radius)) atomicAdd(&s_red[1], 1);
        }
        bool goal_changed = false;
        int done = c.agent_done[q];
        if (!nodone && goal_hit(c, pos, gx, gy, p.radius, done)) {
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
// dynamic LDS: the staged candidate tile px py [TILE] (8 B per lane)
__global__ __launch_bounds__(256) void tiled_close_kernel(const TiledArgs t) {
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
    if (tid == 0) s_pairs = 0;

    if (p.flags & 2u) {  // CA_F_STATS: overlapping pairs (i < j) after the step -- step_kernel's shortcut through the neighbour lists
        // with the arena-wide largest speed of this step, and for the lanes that cannot conclude from their list a scan of the copy
        int pairs = 0;
        const float R = p.radius;
        const float crSq = sqr(R + R);
        const float m2 = pair_reach(sc[TS_VMAX2], p.time_step);
        V2 pos = mk(0.0f, 0.0f);
        if (active) pos = mk(t.nv_x[q], t.nv_y[q]);
        bool scan_all = active && !lists_bound_pairs(p.neighbor_dist, R, m2);
        if (active && !scan_all) {
            float far2 = 0.0f;
            const int ncnt = (int)(p.counts[q] & 0xFFu);
            for (int k = 0; k < ncnt; ++k) {
                const int j = ld_idx_t<true>(p.nb_idx, ((size_t)a * K + k) * N + i);
                const float d2 = absSq(pos - mk(t.nv_x[abase + j], t.nv_y[abase + j]));
                far2 = d2 > far2 ? d2 : far2;
                if (j > i && d2 < crSq) ++pairs;
            }
            scan_all = list_misses_pairs(ncnt, K, far2, R, m2);
        }
        if (__syncthreads_or(scan_all ? 1 : 0)) {   // (workgroup-uniform: the barriers below are met by every lane)
            if (scan_all) pairs = 0;
            for (int ct = tile; ct < t.tiles; ++ct) {   // candidates j > i: this tile and the ones behind it
                const int j0 = ct * TILE;
                const int nj = min(TILE, N - j0);
                __syncthreads();
                if (tid < nj) { s_px[tid] = t.nv_x[abase + j0 + tid]; s_py[tid] = t.nv_y[abase + j0 + tid]; }
                __syncthreads();
                if (scan_all) {
                    for (int jj = (ct == tile ? tid + 1 : 0); jj < nj; ++jj)
                        if (absSq(pos - mk(s_px[jj], s_py[jj])) < crSq) ++pairs;
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
