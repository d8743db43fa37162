// ca_rules.h -- the reference environment's per-agent rules, stated once for every kernel that applies them
// Part of the HIP kernels of libcaenv.so (see ca_kernels.h for the overview and the numerics contract).
//
// Callers: the solve kernels -- ca_step.h (one lane per agent), ca_pair.h (two lanes), ca_quad.h (four lanes), ca_tiled.h (the tiled
// path's three launches) --, the reset kernels (ca_step.h) and the three-launch ALAN kernels (ca_alan.h).  The rules work on values:
// what lane writes, barriers, LDS staging and the reward sums stay in the kernels, and storage that differs by kernel (the softmax
// terms, the ALAN weights and times, the lists of the pair count) is reached through an accessor or stays in the kernel's loop.
// Every fp32 / fp64 operation is in the order the oracle uses.  (The solve's geometry: ca_lines.h, ca_nbr.h, ca_common.h arena_edges.)
#pragma once
#include "ca_common.h"

namespace ca {

typedef const __attribute__((address_space(4))) StepCold ColdK;  // the cold block through the constant address space
typedef const __attribute__((address_space(4))) AlanCold AlanK;
typedef const __attribute__((address_space(4))) TraceDev TraceK;
typedef const __attribute__((address_space(4))) ActSeqDev ActSeqK;

// the unit vector pos -> goal of env.py:236 / 449 (pref_dir64), rounded to fp32
__device__ __forceinline__ V2 goal_dir(V2 pos, double gx, double gy) {
    double dx, dy;
    pref_dir64(pos.x, pos.y, gx, gy, &dx, &dy);
    return mk((float)dx, (float)dy);
}

// env.py:371-383: the goal direction and the preferred velocity = that direction rotated by the action, both rounded to fp32
// as the reward uses them (env.py:394-399 on the simulator's floats)
__device__ __forceinline__ void action_pref(V2 pos, double gx, double gy, float action, V2& dir, V2& pref) {
    double pf_x, pf_y, sn, cs;
    pref_dir64(pos.x, pos.y, gx, gy, &pf_x, &pf_y);
    sincos64((double)action, &sn, &cs);
    const double rl_x = pf_x * cs - pf_y * sn;
    const double rl_y = pf_x * sn + pf_y * cs;
    dir = mk((float)pf_x, (float)pf_y);
    pref = mk((float)rl_x, (float)rl_y);
}

// env.py:389-400 in fp32: progress along the goal direction and along the rotated direction, mixed by reward_scale
__device__ __forceinline__ float step_reward(double reward_scale, V2 vel, V2 dir, V2 rot) {
    const float scale = (float)reward_scale;
    const float r_goal = vel.x * dir.x + vel.y * dir.y;
    const float r_polite = vel.x * rot.x + vel.y * rot.y;
    return scale * r_goal + (1.0f - scale) * r_polite;
}

// The done test (env.py:352-365, 404-410; ALAN:118-121): done_mode 0 -- past the x threshold, once; 1 -- within 2 R of the
// goal, once; 2 -- within 2 R of the goal, every time (the caller draws a new goal)
__device__ __forceinline__ bool goal_hit(const ColdK& c, V2 pos, double gx, double gy, float radius, int done) {
    if (c.done_mode == 0) return (done == 0) && (pos.x < c.done_x_thresh);
    const double dx = (double)pos.x - gx, dy = (double)pos.y - gy;
    const double lim = 2.0 * (double)radius;
    bool hit = (dx * dx + dy * dy) < lim * lim;
    if (c.done_mode == 1) hit = hit && (done == 0);
    return hit;
}

// done_mode 2: the agent's rc-th new goal, uniform in the goal box (stream RNG_REGOAL, counter rc)
__device__ __forceinline__ void regoal_draw(const ColdK& c, int a, int i, int rc, double* gx, double* gy) {
    double u0, u1;
    rng2(c.seed, c.arena_offset + a, i, RNG_REGOAL, (uint32_t)rc, &u0, &u1);
    *gx = uniform64((double)c.goal_x0, (double)c.goal_x1, u0);
    *gy = uniform64((double)c.goal_y0, (double)c.goal_y1, u1);
}

// done_mode 0 / 1: an agent that arrives heads on to its second goal
__device__ __forceinline__ void arrival_goal(const ColdK& c, int q, double* gx, double* gy) {
    *gx = c.goal2_x[q];
    *gy = c.goal2_y[q];
}

// the end of an arena's episode: nobody left on the way (unless the done test is off), or the step cap reached
__device__ __forceinline__ bool episode_over(const ColdK& c, bool nodone, int not_done, int steps) {
    bool over = !nodone && (not_done == 0);
    if (c.max_step > 0 && steps >= c.max_step) over = true;
    return over;
}

// env.py:461-488: agent i's spawn point of episode epi, uniform in the spawn box (stream RNG_RESET, counter epi)
__device__ __forceinline__ V2 spawn_draw(const ColdK& c, int a, int i, int epi) {
    double u0, u1;
    rng2(c.seed, c.arena_offset + a, i, RNG_RESET, (uint32_t)epi, &u0, &u1);
    return mk((float)uniform64((double)c.spawn_x0, (double)c.spawn_x1, u0), (float)uniform64((double)c.spawn_y0, (double)c.spawn_y1, u1));
}

// Orientation of the observation frame (env.py:236): the direction to the goal from the final state.  After an ORCA-only
// step or a reset `pref` already is that vector (fresh = false); otherwise it is derived here, once per agent, instead of
// in each of the 16 ray lanes of the observation kernel.
__device__ __forceinline__ V2 obs_frame(V2 pref, bool fresh, V2 pos, double gx, double gy) {
    return fresh ? goal_dir(pos, gx, gy) : pref;
}

// does the agent touch a wall -- lie within R of one of the ne edges of its arena's table (edges e0, e0 + de,
// ...: the quad kernel deals them over its lanes)?
__device__ __forceinline__ bool touches_wall(const ObstDev* tab, int ne, V2 pos, float R, int e0 = 0, int de = 1) {
    bool wall = false;
    for (int e = e0; e < ne; e += de) {
        const ObstDev o1 = load_obst(tab, e);
        if (distSqPointSegment(mk(o1.px, o1.py), mk(o1.qx, o1.qy), pos) < sqr(R)) wall = true;
    }
    return wall;
}

// SURVEY A20, the overlapping pairs (i < j, distance < 2 R after the step) counted through the neighbour lists instead of a scan of
// the arena.  Nobody moves farther than m = the arena's largest speed of this step x dt (measured, not assumed: two agents that a
// reset drops onto the same spot can leave the linear programs at hundreds of times max_speed -- the oracle does the same -- and a
// bound of 1.01 max_speed dt then misses a pair: one in 2.8e7 agent-steps of the soak with auto-reset,
// profiles/r04_soak_parity.txt), so an agent that overlaps this one now was within 2R + 2m of it when the neighbour list was built:
// if the list is not full it holds every agent within neighbor_dist (>= 2R + 2m required), and if it is full and its farthest
// member is still beyond 2R + 4m now, its K-th distance then was beyond 2R + 2m -- either way every candidate is in the list and K
// distances replace the scan.  The kernels (ca_step.h above 64 agents, ca_pair.h, ca_tiled.h's close launch) keep their own loops
// over their own storage: they measure far2, the largest squared distance to a list member now, and scan for the lanes that cannot
// conclude.  One radius for all: the AgentParams instantiations scan.  m2 = 2 m, a hair wide for the rounding of the update
// (vmax2: the largest squared speed as float bits; NaN / infinite speeds fail every test below: full scan)
__device__ __forceinline__ float pair_reach(unsigned vmax2, float dt) { return 2.0002f * __builtin_sqrtf(__uint_as_float(vmax2)) * dt; }
// the lists can bound the pairs at all: they reach as far as an agent that overlaps now was when they were built
__device__ __forceinline__ bool lists_bound_pairs(float neighbor_dist, float R, float m2) { return neighbor_dist >= R + R + m2; }
// this agent's list of ncnt members (capacity K) did not: it is full and its farthest member is not beyond 2R + 4m
__device__ __forceinline__ bool list_misses_pairs(int ncnt, int K, float far2, float R, float m2) {
    return (ncnt == K) && !(far2 > sqr(R + R + 2.0f * m2));
}

// the ST_LASTEP word of an ended episode: its steps, and how many agents reached their goal
__device__ __forceinline__ unsigned long long lastep_word(int steps, int N, int not_done) {
    return ((unsigned long long)(unsigned)steps << 32) | (unsigned)(N - not_done);
}

// the per-arena statistics of a launch, added to the arena's row (lastep: the last ended episode's word, when have_lastep)
__device__ __forceinline__ void flush_stats(unsigned long long* st, unsigned coll, unsigned wall, unsigned goals, unsigned epis,
                                            bool have_lastep, unsigned long long lastep) {
    if (coll) st[ST_COLL] += coll;
    if (wall) st[ST_OBST_COLL] += wall;
    if (goals) st[ST_GOALS] += goals;
    if (epis) st[ST_EPISODES] += epis;
    if (have_lastep) st[ST_LASTEP] = lastep;
}

// ---- ALAN online action selection (ALAN_true.py:569-628) ----

// numpy's float64 add.reduce for n < 128: < 8 sequential, otherwise eight accumulators combined as a
// fixed tree plus a sequential tail -- the value np.sum(ps) has at ALAN_true.py:582
template <class Get>
__device__ __forceinline__ double np_sum(int n, Get get) {
    if (n < 8) {
        double res = 0.0;
        for (int k = 0; k < n; ++k) res += get(k);
        return res;
    }
    double r0 = get(0), r1 = get(1), r2 = get(2), r3 = get(3), r4 = get(4), r5 = get(5), r6 = get(6), r7 = get(7);
    int k = 8;
    for (; k < n - (n % 8); k += 8) {
        r0 += get(k); r1 += get(k + 1); r2 += get(k + 2); r3 += get(k + 3);
        r4 += get(k + 4); r5 += get(k + 5); r6 += get(k + 6); r7 += get(k + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; k < n; ++k) res += get(k);
    return res;
}

// ALAN:580-581: the softmax terms exp(w_k / temp) of actions k = k0, k0 + dk, ... < nk (ps, w: accessors of action k)
template <class PS, class W>
__device__ __forceinline__ void alan_terms(int nk, int k0, int dk, PS ps, W w, double temp) {
    for (int k = k0; k < nk; k += dk) ps(k) = exp64(w(k) / temp);
}

// the step's uniform of ALAN:585: the caller's (u != null), or the stream (seed, global arena, agent, RNG_ALAN + 256 x
// episode, step) -- a new stream every episode of the arena
__device__ __forceinline__ double alan_uniform(const double* u, int q, uint64_t seed, int64_t arena_offset, int a, int i, int episode, int step) {
    if (u) return u[q];
    double ui, u1;
    rng2(seed, arena_offset + a, i, RNG_ALAN + (episode << 8), (uint32_t)step, &ui, &u1);
    return ui;
}

// ALAN:582-585: the terms normalised in place by their numpy sum, then np.random.choice(nk, 1, p=ps): cdf = cumsum(p) /
// cdf[-1], the first action whose cdf exceeds u = uniform() (searchsorted 'right')
template <class PS, class U>
__device__ __forceinline__ int alan_draw(int nk, PS ps, U uniform) {
    const double sum = np_sum(nk, [&](int k) { return ps(k); });
    double acc = 0.0;
    for (int k = 0; k < nk; ++k) {
        const double v = ps(k) / sum;
        ps(k) = v;
        acc += v;
    }
    const double ui = uniform();
    int id = nk - 1;
    double run = 0.0;
    bool found = false;
    for (int k = 0; k < nk - 1; ++k) {
        run += ps(k);
        if (!found && run / acc > ui) { id = k; found = true; }
    }
    return id;
}

// ALAN:588-598: the goal direction (dg) and the direction the agent is sent in (dl) = dg rotated by action id
template <int AM, class AL>
__device__ __forceinline__ void alan_dirs(const AL& al, int a, int id, V2 pos, double gx, double gy, double* dgx, double* dgy, double* dlx, double* dly) {
    pref_dir64(pos.x, pos.y, gx, gy, dgx, dgy);
    double cs, sn;
    alan_cs<AM>(al, a, id, &cs, &sn);
    *dlx = *dgx * cs - *dgy * sn;
    *dly = *dgx * sn + *dgy * cs;
}

// ALAN:606-628: the fp64 reward of the executed action id, then the sliding window over actions k = k0, k0 + dk, ... < nk
// (w, t: accessors of action k's weight and time): a weight older than the window is forgotten, the executed action's is
// the reward
template <class AL, class W, class T>
__device__ __forceinline__ void alan_update(const AL& al, V2 vel, double dgx, double dgy, double dlx, double dly, int id,
                                            int nk, int k0, int dk, W w, T t) {
    const double vx = (double)vel.x, vy = (double)vel.y;
    const double Rw = al.reward_scale * (vx * dgx + vy * dgy) + (1.0 - al.reward_scale) * (vx * dlx + vy * dly);
    for (int k = k0; k < nk; k += dk) {
        double tk = t(k) + al.dt;
        double wk = w(k);
        if (tk >= al.window) { tk = 0.0; wk = 0.0; }
        if (k == id) wk = Rw;
        t(k) = tk; w(k) = wk;
    }
}

}  // namespace ca
