// ca_tiled_close.inl -- the statements of the tiled path's close launch, included by ca_tiled.h into each of its two kernels
// (CA_TILED_PARAMS 0: tiled_close_kernel; 1: tiled_params_close_kernel, whose pair count takes every agent's own radius -- a pair
// overlaps within sqr(r_i + r_j) -- and whose shortcut through the neighbour lists is bounded by t.r_max, the handle-wide largest
// radius; `t` is the kernel's argument block).  Textual inclusion for the reason ca_tiled_solve.inl gives.
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
#if CA_TILED_PARAMS
    float* s_pr = s_py + TILE;   // the candidate tile's radii, beside its positions
#endif
    if (tid == 0) s_pairs = 0;

    if (p.flags & 2u) {  // CA_F_STATS: overlapping pairs (i < j) after the step -- step_kernel's shortcut through the neighbour lists
        // with the arena-wide largest speed of this step, and for the lanes that cannot conclude from their list a scan of the copy
        int pairs = 0;
#if CA_TILED_PARAMS
        // (an overlapping pair is closer than r_i + r_j <= 2 r_max: with r_max for R the two tests of ca_rules.h stay conservative)
        const float R = t.r_max;
        const float ri = active ? c.ap_radius[q] : 0.0f;
#define CA_T_OVERLAPS(d2, rj) ((d2) < sqr(ri + (rj)))
#else
        const float R = p.radius;
        const float crSq = sqr(R + R);
#define CA_T_OVERLAPS(d2, rj) ((d2) < crSq)
#endif
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
                if (j > i && CA_T_OVERLAPS(d2, c.ap_radius[abase + j])) ++pairs;
            }
            scan_all = list_misses_pairs(ncnt, K, far2, R, m2);
        }
        if (__syncthreads_or(scan_all ? 1 : 0)) {   // (workgroup-uniform: the barriers below are met by every lane)
            if (scan_all) pairs = 0;
            for (int ct = tile; ct < t.tiles; ++ct) {   // candidates j > i: this tile and the ones behind it
                const int j0 = ct * TILE;
                const int nj = min(TILE, N - j0);
                __syncthreads();
#if CA_TILED_PARAMS
                if (tid < nj) { s_px[tid] = t.nv_x[abase + j0 + tid]; s_py[tid] = t.nv_y[abase + j0 + tid]; s_pr[tid] = c.ap_radius[abase + j0 + tid]; }
#else
                if (tid < nj) { s_px[tid] = t.nv_x[abase + j0 + tid]; s_py[tid] = t.nv_y[abase + j0 + tid]; }
#endif
                __syncthreads();
                if (scan_all) {
                    for (int jj = (ct == tile ? tid + 1 : 0); jj < nj; ++jj)
                        if (CA_T_OVERLAPS(absSq(pos - mk(s_px[jj], s_py[jj])), s_pr[jj])) ++pairs;
                }
            }
        }
#undef CA_T_OVERLAPS
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
