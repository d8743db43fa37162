// ca_tiled_advance.inl -- the statements of the tiled path's advance launch, included by ca_tiled.h into each of its two kernels
// (CA_TILED_ADVANCE_EDGES 0: tiled_advance_kernel, 1: tiled_grid_edges_advance_kernel, whose wall test walks the static edge grid; `t`
// is the kernel's argument block; CA_TILED_PARAMS 1: the tiled_params_* twin of each, whose wall and goal tests take the agent's own radius).
// Textual inclusion for the reason ca_tiled_solve.inl gives.
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
#if CA_TILED_PARAMS
        const float ap_r = c.ap_radius[q];
#define CA_T_RADIUS ap_r
#else
#define CA_T_RADIUS p.radius
#endif
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
#if CA_TILED_ADVANCE_EDGES
            // ca_rules.h touches_wall over the cells cell(fl(x - R)) .. cell(fl(x + R)) of the post-step position (R <= the range the
            // table was built for): an OR over edges, so an edge met in two cells is harmless and nothing is deduplicated
            const EdgeGridDev g = t.eg[p.tab_off != nullptr ? a : 0];
            const unsigned* cs = t.eg_cells + g.cells_off;
            const unsigned* en = t.eg_entries + g.entries_off;
            const float R = CA_T_RADIUS;
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
#else
            if (touches_wall(tab, ne, pos, CA_T_RADIUS)) atomicAdd(&s_red[1], 1);
#endif
        }
        bool goal_changed = false;
        int done = c.agent_done[q];
        if (!nodone && goal_hit(c, pos, gx, gy, CA_T_RADIUS, done)) {
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
#undef CA_T_RADIUS
