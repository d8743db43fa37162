// ca_reward.h -- the reward terms (ca_reward_configure, ca_reward_parts): collisions, walls, crowding, arrival, time
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview and the numerics contract).
//
// While terms are configured, a step that writes the reference's reward from actions runs two small kernels round its launches:
//   * reward_begin_kernel, in front: one lane per agent row saves the word the arrival test compares with -- agent_done, or
//     regoal_count under CA_DONE_REGOAL --, and the lane of agent 0 notes whether the step advances the arena at all (CA_F_FREEZE), as
//     nav_act_kernel's `advance` word does;
//   * reward_terms_kernel, behind: for every present row of an advanced arena, from the state the step left (include/ca_env.h
//     ca_reward_desc has the table),
//         r = w0 * r_ref;   for k = 1 .. 6 ascending, where w_k != 0:   r = r + w_k * (float)c_k          (fp32, every operation rounded)
//     into CA_FLD_REWARD, r_ref and c_1 .. c_6 into the handle's [7][A*N] parts buffer, and under CA_F_STATS (double)r - (double)r_ref
//     into the arena's sum_reward (a segmented sum inside the wave, one atomic per arena and wave, as nav_reward_kernel's).
// Every kernel that reads CA_FLD_REWARD afterwards -- the accumulate and record kernels, the packed copy -- sees the shaped value.
//
// reward_terms_kernel has contact_kernel's geometry (ca_contact.h) and is a kernel of its own: one lane per agent, REWARD_BS lanes per
// workgroup; arenas of at most REWARD_BS agents packed floor(REWARD_BS / N) to a workgroup, larger ones in chunks of REWARD_BS
// candidates through LDS, every lane of an arena reading the same candidate in the same trip (an LDS broadcast); the walls are a scan
// of the arena's table, with scalar loads where every arena has the one table.  One pass over the candidates gives c1 and c3, one pass
// over the edges c2 and c4.  A scan that no arena has a weight for is not made (need_pairs / need_walls), and a count that no arena has
// a weight for is stored as 0 (need_mask).  A step that respawned its arena (CA_F_AUTORESET and arena_done != 0 behind it) holds the
// next episode's positions: its lanes make no scan, c1 .. c4 are 0.
#pragma once
#include "ca_common.h"

namespace ca {

constexpr int REWARD_BS = 256;   // as CONTACT_BS: four waves, 3 KiB of LDS
constexpr int REWARD_N_TERMS = 7;   // CA_REWARD_N_TERMS

struct RewardBeginArgs {
    const int* word;         // [A*N] agent_done, or regoal_count under CA_DONE_REGOAL
    const int* arena_done;   // [A]
    int* saved;              // [A*N]
    int* advance;            // [A] 1: the step behind this launch advances the arena, 0: frozen
    unsigned an;
    int N, freeze;
};

__global__ __launch_bounds__(256) void reward_begin_kernel(const RewardBeginArgs p) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= p.an) return;
    const int a = (int)(g / (unsigned)p.N), i = (int)(g - (unsigned)a * (unsigned)p.N);
    p.saved[g] = p.word[g];
    if (i == 0) p.advance[a] = (p.freeze && p.arena_done[a] != 0) ? 0 : 1;
}

struct RewardTermsArgs {
    // contact_kernel's view of the state (ContactArgs)
    const float *pos_x, *pos_y;
    const float* ap_radius;    // [A*N], or null: `radius` for every agent
    const int* agent_counts;   // [A], or null: N agents in every arena
    const ObstDev* obst;
    const int* tab_off;        // null: one table of n_obst edges; else [A + 1] offsets
    unsigned an;
    int n_obst, A, N;
    int apb;                   // N <= REWARD_BS: arenas per workgroup; else 0
    int tiles;                 // N >  REWARD_BS: workgroups per arena; else 0
    float radius;
    // the terms
    const float* weights;      // [A][REWARD_N_TERMS]
    float margin;
    float* reward;             // [A*N] CA_FLD_REWARD
    int* parts;                // [REWARD_N_TERMS][A*N] words: r_ref (f32) | c_1 .. c_6 (i32)
    const int* saved;          // [A*N] what reward_begin_kernel saved
    const int* advance;        // [A]
    const int* agent_done;     // [A*N]
    const int* regoal_count;   // [A*N]
    const int* arena_done;     // [A]
    unsigned long long* arena_stats;   // [A][ST_STRIDE]: ST_LASTEP is read at a respawn, ST_SUMREW added to when `stats`
    int regoal;                // done_mode == CA_DONE_REGOAL
    int autoreset, stats;      // the step's CA_F_AUTORESET / CA_F_STATS
    int need_pairs, need_walls;
    int need_mask;             // bit k: some arena has w_k != 0
    int parts_only;            // ca_reward_parts: every present row, arrival 0, step = agent_done == 0, the reward is not written
};

__global__ __launch_bounds__(REWARD_BS) void reward_terms_kernel(const RewardTermsArgs p) {
    __shared__ float sx[REWARD_BS], sy[REWARD_BS], sr[REWARD_BS];
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
        i = ((int)blockIdx.x - a * p.tiles) * REWARD_BS + t;
        lbase = 0;
        have = i < p.N;   // (the grid is A * tiles workgroups: a < A)
    }
    const size_t q = (size_t)a * p.N + i;
    const int cnt = have ? (p.agent_counts != nullptr ? p.agent_counts[a] : p.N) : 0;
    const bool present = i < cnt;
    // the rows this launch writes, and among them those whose positions are the state the counts are about
    const bool shaped = present && (p.parts_only || p.advance[a] == 1);
    const int adone = shaped ? p.arena_done[a] : 0;
    const bool respawned = !p.parts_only && p.autoreset && adone != 0;
    const bool scan = shaped && !respawned;
    float w[REWARD_N_TERMS];
#pragma unroll
    for (int k = 0; k < REWARD_N_TERMS; ++k) w[k] = shaped ? p.weights[(size_t)a * REWARD_N_TERMS + k] : 0.0f;
    V2 pos = mk(0.0f, 0.0f);
    float ri = p.radius;
    if (scan) {
        pos = mk(p.pos_x[q], p.pos_y[q]);
        if (per_agent) ri = p.ap_radius[q];
    }

    int touching = 0, near = 0;
    if (p.need_pairs) {
        // a packed workgroup stages its arenas' rows once; a large arena its N rows in chunks (a trip count of the whole workgroup)
        const int span = packed ? 1 : p.N;
        for (int c0 = 0; c0 < span; c0 += REWARD_BS) {
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
            if (scan) {
                const int jn = min(cnt - c0, REWARD_BS);   // candidates of this chunk that are agents of the arena
#pragma unroll 4
                for (int jj = 0; jj < jn; ++jj) {
                    const int j = c0 + jj;
                    const float d2 = absSq(pos - mk(sx[lbase + jj], sy[lbase + jj]));
                    const float cr = ri + (per_agent ? sr[lbase + jj] : p.radius);
                    if (j != i) {
                        if (d2 < sqr(cr)) ++touching;
                        if (d2 < sqr(cr + p.margin)) ++near;
                    }
                }
            }
        }
    }

    int wall = 0, wall_near = 0;
    if (p.need_walls && scan) {
        const int off = p.tab_off != nullptr ? p.tab_off[a] : 0;
        const int ne = p.tab_off != nullptr ? p.tab_off[a + 1] - off : p.n_obst;
        const ObstDev* tab = p.obst + off;
        const float rr = sqr(ri);
        float wall_d2 = __builtin_inff();
        for (int e = 0; e < ne; ++e) {
            const ObstDev o1 = load_obst(tab, e);
            const float d2 = distSqPointSegment(mk(o1.px, o1.py), mk(o1.qx, o1.qy), pos);
            if (d2 < rr) wall = 1;
            if (d2 < wall_d2) wall_d2 = d2;
        }
        if (wall_d2 < sqr(ri + p.margin)) wall_near = 1;
    }

    float r = 0.0f, r_ref = 0.0f;
    if (shaped) {
        const int saved = p.parts_only ? 0 : p.saved[q];
        int arrived = 0, stepping;
        if (p.parts_only) {
            stepping = p.agent_done[q] == 0 ? 1 : 0;
        } else if (p.regoal) {
            arrived = saved != p.regoal_count[q] ? 1 : 0;
            stepping = 1;
        } else {
            stepping = saved == 0 ? 1 : 0;
            if (saved == 0) {
                if (respawned) {   // the flags are the next episode's: the last-episode word says whether every agent arrived
                    const unsigned long long le = p.arena_stats[(size_t)a * ST_STRIDE + ST_LASTEP];
                    arrived = (unsigned)(le & 0xFFFFFFFFull) == (unsigned)cnt ? 1 : 0;
                } else {
                    arrived = p.agent_done[q] != 0 ? 1 : 0;
                }
            }
        }
        int c[REWARD_N_TERMS] = {0, touching, wall, near, wall_near, arrived, stepping};
        r_ref = p.reward[q];
        r = __fmul_rn(w[0], r_ref);
#pragma unroll
        for (int k = 1; k < REWARD_N_TERMS; ++k) {
            if (((p.need_mask >> k) & 1) == 0) c[k] = 0;
            if (w[k] != 0.0f) r = __fadd_rn(r, __fmul_rn(w[k], (float)c[k]));
        }
        p.parts[q] = __float_as_int(r_ref);
#pragma unroll
        for (int k = 1; k < REWARD_N_TERMS; ++k) p.parts[(size_t)k * p.an + q] = c[k];
        if (!p.parts_only) p.reward[q] = r;
    }
    if (p.stats) {
        // the rows of an arena are consecutive lanes: a suffix sum that stops at the arena's last lane, its first lane of this wave adds
        const int sa = have ? a : -1;
        double sum = shaped ? (double)r - (double)r_ref : 0.0;
        const int lane = t & 63;
        for (int off = 1; off < 64; off <<= 1) {
            const double ts = __shfl_down(sum, off, 64);
            const int ta = __shfl_down(sa, off, 64);
            if (lane + off < 64 && ta == sa) sum += ts;
        }
        const int pa = __shfl_up(sa, 1, 64);
        if (have && (lane == 0 || pa != sa) && sum != 0.0)
            atomicAdd(reinterpret_cast<double*>(&p.arena_stats[(size_t)a * ST_STRIDE + ST_SUMREW]), sum);
    }
}

}  // namespace ca
