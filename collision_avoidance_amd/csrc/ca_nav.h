// ca_nav.h -- the kernels of the navigation fields (ca_nav_configure, ca_nav_pref, ca_rollout_nav)
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview and the numerics contract).
//
// A navigation field is, per (field set, target), the shortest 8-connected grid distance to the target's cell over the unblocked cells
// of a caller-given grid (ca_nav_host.h: the cell expression, the centres, the blocked mask), and per cell the neighbour to walk to.
// Neighbours k = 0 .. 7 are offset by (1,0) (0,1) (-1,0) (0,-1) (1,1) (-1,1) (-1,-1) (1,-1); an axis move weighs w = cell, a diagonal
// one w = cell * 1.41421354f (rounded once, on the host), and a diagonal move is allowed only when both axis cells it passes between
// are in the grid and unblocked.  The field is THE solution of
//     d[source] = 0,   d[c] = min over allowed neighbours u_k of fl(d[u_k] + w_k)   (+inf: blocked, or nothing to take the minimum of)
// which is unique: fp32 addition is monotone and d + w > d for every finite d of a grid (w >= 2^-10, d < 2^19), so values settle in
// increasing order exactly as in a label-setting pass, and relaxing downwards from +inf in ANY order -- Jacobi, raster, or lanes racing
// in place -- ends in that solution (a value is only ever lowered, to the sum of a neighbour's current value, which is never below
// the neighbour's final one).  nav_field_kernel relies on it:
//   * one workgroup per (set, target); the mask bits and the distance image live in LDS (32768 cells: 128 KiB + 4 KiB);
//   * a sweep relaxes every unblocked cell in place, lanes reading whatever their neighbours hold at that moment; one
//     __syncthreads_or per sweep carries "some lane lowered a value".  A sweep that lowers nothing has read final values only;
//   * it leaves then, and in any case after cells + 1 sweeps: an in-place sweep does at least what a Jacobi sweep does and Jacobi settles
//     one more cell of the label-setting order per sweep, so the bound is never what ends the loop -- it makes the loop finite by construction;
//   * a last pass writes dist, and next: the smallest k with fl(d[u_k] + w_k) == d[c]; STAY in the source; NONE in an unblocked cell of
//     infinite distance; in a blocked cell the escape pointer, the smallest (d[u_k], k) over ALL in-grid neighbours of finite distance
//     (no corner rule), NONE without one.
// nav_pref_kernel: one lane per agent row; the row's cell, `lookahead` pointer steps through next, and goal_dir (ca_rules.h) towards the
// centre of the cell reached -- or towards the agent's own goal when the walk never moved or ended on STAY.  It writes PREF_X / PREF_Y
// (and dist_out) of navigated rows and nothing else.
// The navigated action step (ca_nav_act, ca_nav_step, ca_rollout_nav_actions / _policy) is two more small kernels round the
// launches of an ORCA-only step, which reads PREF as its input and leaves VEL alone across a respawn:
//   * nav_act_kernel, in front: one lane per agent row; the point T the row heads for -- nav_pref_kernel's for a row it would navigate
//     (the same walk, nav_walk below), the agent's own goal for every other present row --, then action_pref (ca_rules.h: the function of
//     the solve kernels) towards T.  PREF = the rotated direction; the direction and the rotated direction are kept in a buffer of the
//     handle's for the kernel behind the step, and the lane of agent 0 notes whether the arena is advanced at all (CA_F_FREEZE);
//   * nav_reward_kernel, behind: REWARD = step_reward (ca_rules.h) of the velocity the step left and the two kept directions, for
//     the present rows of the arenas that were advanced; under CA_F_STATS the arena's sum in f64 (a segmented sum inside the wave, one
//     atomic per arena and wave); and, for the rollouts, the return, first_done and the reward / done records by the rule of
//     actseq_accumulate_kernel / policy_record_kernel word for word, so that no second launch follows.
#pragma once
#include "ca_common.h"
#include "ca_rules.h"
#include "ca_actseq.h"

namespace ca {

enum { NAV_STAY = 8, NAV_NONE = 9 };

// the offsets of neighbour k: two bits each of (dx + 1) / (dy + 1), k = 0 in the lowest
__device__ __forceinline__ int nav_dx(int k) { return (int)((0x8246u >> (2 * k)) & 3u) - 1; }
__device__ __forceinline__ int nav_dy(int k) { return (int)((0x0A19u >> (2 * k)) & 3u) - 1; }

struct NavFieldArgs {
    const unsigned* mask;    // [sets][mw] blocked bits, cell c = bit c & 31 of word c >> 5
    const int* source;       // [sets * G] the target's cell
    float* dist;             // [sets * G][cells]
    unsigned char* next;     // [sets * G][cells]
    int* sweeps;             // [sets * G] sweeps made (the last, which lowered nothing, included)
    int gx, gy, cells, mw, G;
    float w_axis, w_diag;
};

// the eight candidates fl(d[u_k] + w_k) of cell (cx, cy): +inf where the neighbour is outside the grid or the move is not allowed.
// (A blocked neighbour holds +inf, so only the corner rule needs the mask.)
__device__ __forceinline__ void nav_candidates(const float* d, const unsigned* mb, int c, int cx, int cy, int gx, int gy, float wa, float wd,
                                               float (&cand)[8]) {
    const float inf = __int_as_float(0x7F800000);
    const bool xp = cx + 1 < gx, xm = cx > 0, yp = cy + 1 < gy, ym = cy > 0;
    auto open = [&](int q) { return ((mb[q >> 5] >> (q & 31)) & 1u) == 0u; };
    const bool f0 = xp && open(c + 1), f1 = yp && open(c + gx), f2 = xm && open(c - 1), f3 = ym && open(c - gx);
    cand[0] = xp ? __fadd_rn(d[c + 1], wa) : inf;
    cand[1] = yp ? __fadd_rn(d[c + gx], wa) : inf;
    cand[2] = xm ? __fadd_rn(d[c - 1], wa) : inf;
    cand[3] = ym ? __fadd_rn(d[c - gx], wa) : inf;
    cand[4] = (f0 && f1) ? __fadd_rn(d[c + gx + 1], wd) : inf;
    cand[5] = (f2 && f1) ? __fadd_rn(d[c + gx - 1], wd) : inf;
    cand[6] = (f2 && f3) ? __fadd_rn(d[c - gx - 1], wd) : inf;
    cand[7] = (f0 && f3) ? __fadd_rn(d[c - gx + 1], wd) : inf;
}

template <int BS>
__global__ __launch_bounds__(BS) void nav_field_kernel(const NavFieldArgs p) {
    extern __shared__ __attribute__((aligned(16))) float nav_lds[];   // [cells] distances | [mw] mask words
    float* d = nav_lds;
    unsigned* mb = (unsigned*)(nav_lds + p.cells);
    const int tid = (int)threadIdx.x, f = (int)blockIdx.x, set = f / p.G;
    const int gx = p.gx, gy = p.gy, cells = p.cells, src = p.source[f];
    const float inf = __int_as_float(0x7F800000);
    for (int w = tid; w < p.mw; w += BS) mb[w] = p.mask[(size_t)set * p.mw + w];
    for (int c = tid; c < cells; c += BS) d[c] = c == src ? 0.0f : inf;
    __syncthreads();
    const int sx = BS % gx, sy = BS / gx;   // a lane's cells: tid, tid + BS, ... with (cx, cy) carried along
    int sweeps = 0;
    for (;;) {
        int changed = 0;
        int cx = tid % gx, cy = tid / gx;
        for (int c = tid; c < cells; c += BS) {
            if (c != src && ((mb[c >> 5] >> (c & 31)) & 1u) == 0u) {
                float cand[8];
                nav_candidates(d, mb, c, cx, cy, gx, gy, p.w_axis, p.w_diag, cand);
                float best = cand[0];
#pragma unroll
                for (int k = 1; k < 8; ++k) best = cand[k] < best ? cand[k] : best;
                if (best < d[c]) { d[c] = best; changed = 1; }
            }
            cx += sx; cy += sy;
            if (cx >= gx) { cx -= gx; cy += 1; }
        }
        ++sweeps;
        if (__syncthreads_or(changed) == 0 || sweeps > cells) break;
    }
    float* dist = p.dist + (size_t)f * cells;
    unsigned char* next = p.next + (size_t)f * cells;
    int cx = tid % gx, cy = tid / gx;
    for (int c = tid; c < cells; c += BS) {
        const float dc = d[c];
        int k_out = NAV_NONE;
        if (c == src) {
            k_out = NAV_STAY;
        } else if (((mb[c >> 5] >> (c & 31)) & 1u) == 0u) {
            if (dc < inf) {
                float cand[8];
                nav_candidates(d, mb, c, cx, cy, gx, gy, p.w_axis, p.w_diag, cand);
#pragma unroll
                for (int k = 7; k >= 0; --k) k_out = cand[k] == dc ? k : k_out;
            }
        } else {   // the escape pointer of a blocked cell
            float best = inf;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int ux = cx + nav_dx(k), uy = cy + nav_dy(k);
                if (ux >= 0 && ux < gx && uy >= 0 && uy < gy) {
                    const float du = d[uy * gx + ux];
                    if (du < best) { best = du; k_out = k; }
                }
            }
        }
        dist[c] = dc;
        next[c] = (unsigned char)k_out;
        cx += sx; cy += sy;
        if (cx >= gx) { cx -= gx; cy += 1; }
    }
    if (tid == 0) p.sweeps[f] = sweeps;
}

struct NavPrefArgs {
    const float *pos_x, *pos_y;
    const double *goal_x, *goal_y;
    const int* agent_done;
    const int* arena_done;
    const int* agent_counts;     // [A] (ca_set_agent_counts), or null
    const int* cls;              // [A*N] the row's target, or -1: not navigated
    const float* dist;           // [sets * G][cells]
    const unsigned char* next;   // [sets * G][cells]
    float *pref_x, *pref_y;
    float* dist_out;             // [A*N], or null
    unsigned an;
    int N, G, gx, gy, cells, per_arena, lookahead, freeze;
    float x0, y0, cell, ics;
};

// the grid's cell expression (ca_nav_host.h; the edge grid's)
__device__ __forceinline__ int nav_cell(float v, float x0, float ics, int g) { return (int)fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1)); }

// the pointer walk from cell (wx, wy): `lookahead` steps through next, (ox, oy) the cell reached.  True: the walk never moved or ended on
// STAY -- the row heads for the agent's own goal; false: for the centre of (ox, oy).  (The cell by value, the order of the locals and
// the sense of the result are what leaves nav_pref_kernel's instruction text as it was with the loop written out in it:
// profiles/nav_step_kernel_resources.txt.)
__device__ __forceinline__ bool nav_walk(int wx, int wy, const NavPrefArgs& p, const unsigned char* next, int& ox, int& oy) {
    int k = NAV_NONE;
    bool moved = false;
    for (int l = 0; l < p.lookahead; ++l) {
        k = (int)next[wy * p.gx + wx];
        if (k >= 8) break;
        const int ux = wx + nav_dx(k), uy = wy + nav_dy(k);
        if (ux < 0 || ux >= p.gx || uy < 0 || uy >= p.gy) break;   // (a pointer never leaves the grid; this keeps the read in bounds whatever the table holds)
        wx = ux; wy = uy; moved = true;
    }
    ox = wx; oy = wy;
    return !moved || k == NAV_STAY;
}

__global__ __launch_bounds__(256) void nav_pref_kernel(const NavPrefArgs p) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= p.an) return;
    const int a = (int)(g / (unsigned)p.N), i = (int)(g - (unsigned)a * (unsigned)p.N);
    const int cls = p.cls[g];
    const int count = p.agent_counts != nullptr ? p.agent_counts[a] : p.N;
    if (i >= count || cls < 0 || cls >= p.G || p.agent_done[g] != 0) return;
    if (p.freeze && p.arena_done[a] != 0) return;
    const V2 pos = mk(p.pos_x[g], p.pos_y[g]);
    const int wx = nav_cell(pos.x, p.x0, p.ics, p.gx), wy = nav_cell(pos.y, p.y0, p.ics, p.gy);
    const size_t f = ((size_t)(p.per_arena ? a : 0) * (size_t)p.G + (size_t)cls) * (size_t)p.cells;
    const unsigned char* next = p.next + f;
    if (p.dist_out != nullptr) p.dist_out[g] = p.dist[f + (size_t)(wy * p.gx + wx)];
    int ox, oy;
    V2 dir;
    if (nav_walk(wx, wy, p, next, ox, oy)) {
        dir = goal_dir(pos, p.goal_x[g], p.goal_y[g]);
    } else {
        const float tx = p.x0 + ((float)ox + 0.5f) * p.cell, ty = p.y0 + ((float)oy + 0.5f) * p.cell;
        dir = goal_dir(pos, (double)tx, (double)ty);
    }
    p.pref_x[g] = dir.x;
    p.pref_y[g] = dir.y;
}

struct NavActArgs {
    NavPrefArgs n;           // the state, the navigation, pref_x / pref_y, dist_out (or null), freeze
    const float* actions;    // [A*N]
    float* keep;             // [4][A*N] the handle's: dir.x | dir.y | rot.x | rot.y for nav_reward_kernel
    float* heading_out;      // [2][A*N] dir, or null
    int* advance;            // [A] 1: the step behind this launch advances the arena, 0: frozen
};

__global__ __launch_bounds__(256) void nav_act_kernel(const NavActArgs q) {
    const NavPrefArgs& p = q.n;
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g >= p.an) return;
    const int a = (int)(g / (unsigned)p.N), i = (int)(g - (unsigned)a * (unsigned)p.N);
    const bool frozen = p.freeze && p.arena_done[a] != 0;
    if (i == 0) q.advance[a] = frozen ? 0 : 1;
    const int count = p.agent_counts != nullptr ? p.agent_counts[a] : p.N;
    if (i >= count || frozen) return;
    const V2 pos = mk(p.pos_x[g], p.pos_y[g]);
    double tx = p.goal_x[g], ty = p.goal_y[g];
    const int cls = p.cls[g];
    if (cls >= 0 && cls < p.G && p.agent_done[g] == 0) {   // a row nav_pref_kernel navigates: its cell, its walk, its centre
        const int wx = nav_cell(pos.x, p.x0, p.ics, p.gx), wy = nav_cell(pos.y, p.y0, p.ics, p.gy);
        const size_t f = ((size_t)(p.per_arena ? a : 0) * (size_t)p.G + (size_t)cls) * (size_t)p.cells;
        if (p.dist_out != nullptr) p.dist_out[g] = p.dist[f + (size_t)(wy * p.gx + wx)];
        int ox, oy;
        if (!nav_walk(wx, wy, p, p.next + f, ox, oy)) {
            const float cx = p.x0 + ((float)ox + 0.5f) * p.cell, cy = p.y0 + ((float)oy + 0.5f) * p.cell;
            tx = (double)cx; ty = (double)cy;
        }
    }
    V2 dir, rot;
    action_pref(pos, tx, ty, q.actions[g], dir, rot);
    p.pref_x[g] = rot.x;
    p.pref_y[g] = rot.y;
    const size_t an = (size_t)p.an;
    q.keep[g] = dir.x; q.keep[an + g] = dir.y; q.keep[2 * an + g] = rot.x; q.keep[3 * an + g] = rot.y;
    if (q.heading_out != nullptr) { q.heading_out[g] = dir.x; q.heading_out[an + g] = dir.y; }
}

struct NavRewardArgs {
    const float *vel_x, *vel_y;
    const float* keep;             // [4][A*N] what nav_act_kernel kept
    const int* advance;            // [A]
    const int* agent_counts;       // [A] (ca_set_agent_counts), or null
    float* reward;                 // [A*N] CA_FLD_REWARD
    unsigned long long* arena_stats;   // CA_F_STATS: the per-arena rows (ST_SUMREW), else null
    double reward_scale;
    // a rollout's step t (first_done != null), as ActSeqAccArgs / PolicyRecArgs
    const int* arena_done;
    const int* entry_frozen;
    const float* weight;           // &weights[t], or null
    float* returns;                // or null
    int* first_done;               // the caller's or the handle's own; null: a single ca_nav_step
    float* rewards_rec;            // [A*N] row t of the reward record, or null
    int* done_rec;                 // [A] row t of the done record, or null
    unsigned an;
    int N, t, freeze;
};

__global__ __launch_bounds__(256) void nav_reward_kernel(const NavRewardArgs s) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    const bool row = g < s.an;   // (no lane leaves before the wave's sum)
    const int a = row ? (int)(g / (unsigned)s.N) : -1, i = row ? (int)(g - (unsigned)a * (unsigned)s.N) : 0;
    const int count = row ? (s.agent_counts != nullptr ? s.agent_counts[a] : s.N) : 0;
    const bool stepped = row && s.advance[a] == 1 && i < count;
    float r = 0.0f;
    if (stepped) {
        const size_t an = (size_t)s.an;
        r = step_reward(s.reward_scale, mk(s.vel_x[g], s.vel_y[g]), mk(s.keep[g], s.keep[an + g]), mk(s.keep[2 * an + g], s.keep[3 * an + g]));
        s.reward[g] = r;
    } else if (row) {
        r = s.reward[g];
    }
    if (s.arena_stats != nullptr) {
        // the rows of an arena are consecutive lanes: a suffix sum that stops at the arena's last lane, its first lane of this wave adds
        double sum = stepped ? (double)r : 0.0;
        const int lane = (int)(threadIdx.x & 63u);
        for (int off = 1; off < 64; off <<= 1) {
            const double ts = __shfl_down(sum, off, 64);
            const int ta = __shfl_down(a, off, 64);
            if (lane + off < 64 && ta == a) sum += ts;
        }
        const int pa = __shfl_up(a, 1, 64);
        if (row && (lane == 0 || pa != a) && s.advance[a] == 1)
            atomicAdd(reinterpret_cast<double*>(&s.arena_stats[(size_t)a * ST_STRIDE + ST_SUMREW]), sum);
    }
    if (!row || s.first_done == nullptr) return;
    // (r: what CA_FLD_REWARD holds behind this step; the count is in a register already)
    actseq_account(g, a, i, r, nullptr, count, s.arena_done, s.entry_frozen, s.weight, s.returns, s.first_done, s.rewards_rec, s.done_rec, s.t, s.freeze);
}

}  // namespace ca
