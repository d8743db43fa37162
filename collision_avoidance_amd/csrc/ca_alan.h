// ca_alan.h -- ALAN online action selection kernels
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview and the numerics contract).
#pragma once
#include "ca_rules.h"

namespace ca {

// ============================================================================================
// ALAN online action selection (ALAN_true.py:569-628), one lane per agent, around the ORCA step:
//   alan_select_kernel : softmax over the agent's action weights, one draw, preferred velocity =
//                        goal direction rotated by the chosen action (ALAN:578-598);
//   [step_kernel in ORCA mode: sim.doStep(), step counter, goal test (ALAN:601, 118-121)]
//   alan_update_kernel : reward of the executed action, sliding-window bandit update (ALAN:603-628).
// Weights, times and the reward that feeds them are fp64 like the reference's Python floats.
// ============================================================================================
enum { ALAN_MAX_ACTIONS = 32, ALAN_BS = 128 };
struct AlanArgs {
    const float *pos_x, *pos_y, *vel_x, *vel_y;
    const double *goal_x, *goal_y;
    float *pref_x, *pref_y, *reward;
    double *w, *t;        // [A][nA][N] action weights / time since the action's weight was set
    int* action;          // [A*N] the action of the current step (complemented while its arena sits out a step)
    double* dirs;         // [4][A*N] goal direction and rotated direction of the current step
    const double* u;      // [A*N] caller-supplied uniforms in [0,1), or null: Philox (RNG_ALAN, episode, step)
    const int *step_count, *arena_done, *episode;
    unsigned long long* arena_stats;
    double act_c[ALAN_MAX_ACTIONS], act_s[ALAN_MAX_ACTIONS];  // (cos, sin) of every action's angle
    const double2* tab;   // per-arena sets: [A][ALAN_MAX_ACTIONS] (cos, sin) and [A] counts (ca_common.h alan_count / alan_cs)
    const int* tab_n;
    double temp, window, dt, reward_scale;
    uint64_t seed;
    int64_t arena_offset;
    int A, N, nA;         // nA: the stride of w / t (per-arena sets: the largest)
    uint32_t flags;
};

// ALAN = 1: one action set for the handle; 2: a set per arena (the loops run over the arena's own count, stride nA)
template <int ALAN>
__global__ __launch_bounds__(ALAN_BS) void alan_select_kernel(const AlanArgs p) {
    extern __shared__ double s_ps[];  // [n_actions][lane]: sized by the launch (8 B x n_actions x ALAN_BS)
    const int q = blockIdx.x * ALAN_BS + threadIdx.x;
    if (q >= p.A * p.N) return;
    const int a = q / p.N, i = q - a * p.N, nA = p.nA, nk = alan_count<ALAN>(p, a);
    if ((p.flags & 16u) && p.arena_done[a] != 0) {  // CA_F_FREEZE: tell the update kernel, keep the last action
        p.action[q] = ~p.action[q];
        return;
    }
    double* ps = s_ps + threadIdx.x;
    // weights and times are stored [A][n_actions][N]: the lanes of a wave read consecutive doubles
    const double* w = p.w + (size_t)a * nA * p.N + i;
    auto psk = [&](int k) -> double& { return ps[k * ALAN_BS]; };
    alan_terms(nk, 0, 1, psk, [&](int k) { return w[(size_t)k * p.N]; }, p.temp);
    const int id = alan_draw(nk, psk, [&] { return alan_uniform(p.u, q, p.seed, p.arena_offset, a, i, p.episode[a], p.step_count[a]); });
    p.action[q] = id;
    double gx, gy, lx, ly;
    alan_dirs<ALAN>(p, a, id, mk(p.pos_x[q], p.pos_y[q]), p.goal_x[q], p.goal_y[q], &gx, &gy, &lx, &ly);
    const size_t an = (size_t)p.A * p.N;  // dirs: [4][A*N]
    p.dirs[q] = gx; p.dirs[an + q] = gy; p.dirs[2 * an + q] = lx; p.dirs[3 * an + q] = ly;
    p.pref_x[q] = (float)lx; p.pref_y[q] = (float)ly;                               // ALAN:598
}

template <int ALAN>
__global__ __launch_bounds__(ALAN_BS) void alan_update_kernel(const AlanArgs p) {
    const int q = blockIdx.x * ALAN_BS + threadIdx.x;
    if (q >= p.A * p.N) return;
    const int id = p.action[q];
    if (id < 0) {  // the arena was frozen when this step began
        p.action[q] = ~id;
        return;
    }
    const int a = q / p.N, nA = p.nA, nk = alan_count<ALAN>(p, a);
    const size_t an = (size_t)p.A * p.N;
    const double d[4] = {p.dirs[q], p.dirs[an + q], p.dirs[2 * an + q], p.dirs[3 * an + q]};
    const float vxf = p.vel_x[q], vyf = p.vel_y[q];
    {
        const float rew = step_reward(p.reward_scale, mk(vxf, vyf), mk((float)d[0], (float)d[1]), mk((float)d[2], (float)d[3]));
        p.reward[q] = rew;
        if (p.flags & 2u) {
            double* sum = reinterpret_cast<double*>(&p.arena_stats[(size_t)a * ST_STRIDE + ST_SUMREW]);
            if ((p.N & 63) == 0) {  // a wave lies inside one arena (and leaves the kernel as a whole): one atomic per wave
                double r = (double)rew;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
                if ((threadIdx.x & 63) == 0) atomicAdd(sum, r);
            } else {
                atomicAdd(sum, (double)rew);
            }
        }
    }
    const int i = q - a * p.N;
    double* w = p.w + (size_t)a * nA * p.N + i;
    double* t = p.t + (size_t)a * nA * p.N + i;
    alan_update(p, mk(vxf, vyf), d[0], d[1], d[2], d[3], id, nk, 0, 1, [&](int k) -> double& { return w[(size_t)k * p.N]; },
                [&](int k) -> double& { return t[(size_t)k * p.N]; });
    // the solve kernel left the goal direction in pref (its ORCA-mode epilogue); the reference's agent
    // still holds the velocity it was given at ALAN:598
    p.pref_x[q] = (float)d[2]; p.pref_y[q] = (float)d[3];
}

}  // namespace ca
