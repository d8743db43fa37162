// ca_tiled_solve.inl -- the statements of the tiled path's solve launch, included by ca_tiled.h into each of its three kernels
// (CA_TILED_SOLVE_GRID 0: tiled_solve_kernel, 1: tiled_grid_solve_kernel, 2: tiled_grid_edges_solve_kernel -- the grid kernel with the
// obstacle edges found through the static edge grid; `t` is the kernel's argument block, KMAX and TILE its template parameters;
// CA_TILED_PARAMS 1: the tiled_params_* twin of each, which takes radius, maximum speed and the two time horizons of agent i from the
// per-agent arrays of ca_set_agent_params -- p.cold->ap_*, DESIGN.md 7h -- where the others take the handle's four constants).  Textual inclusion and not a shared __device__ function: through a function -- by reference or by value --
// the plain kernel's instruction text moved, and that kernel is to stay what it was before the grid existed.
    const StepArgs& p = t.s;
    extern __shared__ float4 smem4[];
    const int tid = threadIdx.x;
    const int a = (int)blockIdx.x / t.tiles, tile = (int)blockIdx.x - a * t.tiles;
    const int N = p.N, K = p.K, S = p.S;
#if CA_TILED_SOLVE_GRID
    int i = tile * TILE + tid;
    if (i < N && !arena_frozen(p, a)) i = min((int)t.sidx[(size_t)a * N + i], N - 1);   // (an inactive lane keeps i >= N)
#else
    const int i = tile * TILE + tid;
#endif
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
#if CA_TILED_PARAMS
    // the agent's own four values (an inactive lane keeps the handle's: it computes nothing that is stored); a neighbour's radius is
    // gathered next to its position and velocity, where its line is built
    float ap_r = p.radius, ap_ms = p.max_speed, ap_th = p.time_horizon, ap_tho = p.time_horizon_obst;
    const ColdK& ck = *(ColdK*)p.cold;
    if (active) { ap_r = ck.ap_radius[q]; ap_ms = ck.ap_max_speed[q]; ap_th = ck.ap_time_horizon[q]; ap_tho = ck.ap_time_horizon_obst[q]; }
#define CA_T_RADIUS ap_r
#define CA_T_MAX_SPEED ap_ms
#define CA_T_HORIZON ap_th
#define CA_T_HORIZON_OBST ap_tho
#else
#define CA_T_RADIUS p.radius
#define CA_T_MAX_SPEED p.max_speed
#define CA_T_HORIZON p.time_horizon
#define CA_T_HORIZON_OBST p.time_horizon_obst
#endif

    // ---- obstacle neighbours (App. A.2; ca_nbr.h's keys; its edge_in_range and ca_common.h arena_edges written out: through them this kernel's text moved) ----
    const ObstDev* tab = p.obst + ((p.tab_off != nullptr) ? p.tab_off[a] : 0);          // this arena's edge table
    const int n_edges = p.tab_off != nullptr ? p.tab_off[a + 1] - p.tab_off[a] : p.n_obst;
    int oin = 0;
    {
        const int sofs = SMAX - S;   // the S-entry list is right-aligned in the register array
        double okey[SMAX];
#pragma unroll
        for (int k = 0; k < SMAX; ++k) okey[k] = (k < sofs) ? key_dummy() : key_empty();
        const float rangeSq = sqr(CA_T_HORIZON_OBST * CA_T_MAX_SPEED + CA_T_RADIUS);
#if CA_TILED_SOLVE_GRID == 2
        // The static edge grid (ca_edge_grid_host.h): the cells of the columns cell(fl(x - range)) .. cell(fl(x + range)) and the rows
        // likewise, 3 x 3 but for a rounding of ics; an edge registered in several of them is taken in the low corner of the intersection of its
        // rectangle with this one, so no edge enters twice; an accepted edge passes the test of the scan below, on tab[e].  The list
        // is the S smallest distinct keys of the accepted set: the order of the walk is immaterial.  Per-lane walks: the lanes of a
        // wave stand in the same few cells (sorted positions), so their loads of a run and of its records fall into the same lines.
        if (active) {
            const EdgeGridDev g = t.eg[p.tab_off != nullptr ? a : 0];
            const unsigned* cs = t.eg_cells + g.cells_off;
            const unsigned* en = t.eg_entries + g.entries_off;
            const float range = CA_T_HORIZON_OBST * CA_T_MAX_SPEED + CA_T_RADIUS;   // (per agent: a smaller range walks fewer cells)
            const int cxlo = edge_cell(pos.x - range, g.x0, g.ics_x, g.gx), cxhi = edge_cell(pos.x + range, g.x0, g.ics_x, g.gx);
            const int cylo = edge_cell(pos.y - range, g.y0, g.ics_y, g.gy), cyhi = edge_cell(pos.y + range, g.y0, g.ics_y, g.gy);
            for (int r = cylo; r <= cyhi; ++r) {
                for (int c = cxlo; c <= cxhi; ++c) {
                    const unsigned* run = cs + (r * g.gx + c);
                    const unsigned hi = min(run[1], g.n_entries);   // (every index clamped: ca_tiled.h EdgeGridDev)
                    for (unsigned u = run[0]; u < hi; ++u) {
                        const unsigned w = en[u];
                        const int e = (int)(w & 0xFFFFu);
                        if (e >= n_edges || max((int)((w >> 16) & 0xFFu), cxlo) != c || max((int)(w >> 24), cylo) != r) continue;
                        const ObstDev& o1 = tab[e];
                        const V2 a1 = mk(o1.px, o1.py), a2 = mk(o1.qx, o1.qy);
                        const float alol = leftOf(a1, a2, pos);
                        const float dsl = div_ir(sqr(alol), absSq(a2 - a1));
                        if (dsl < rangeSq && alol < 0.0f) {
                            const float dsq = distSqPointSegment(a1, a2, pos);
                            if (dsq < rangeSq) {
                                ++oin;
                                sorted_insert<SMAX>(okey, make_key(dsq, e));
                            }
                        }
                    }
                }
            }
        }
#else
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
#endif
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
#if CA_TILED_SOLVE_GRID
    {
        // The cells of the columns c(fl(x - B)) .. c(fl(x + B)) and the rows likewise, B = nd * 1.0001 + 1e-4 (ca_nbr.h: a candidate
        // that passes the distance test has |xi - xj| < B, so xj lies between the two floats, and c is monotone) -- not a fixed
        // block around the own cell.  At most GX columns and GY rows, so no bucket is visited twice; a row's columns are one run of
        // the sorted arrays, or two where they wrap.  Cells arrive in no index order: a candidate enters on `distance <= the current
        // K-th distance` and the 64-bit keys settle ties, which also makes the order inside a cell immaterial.
        if (K > 0 && active) {
            const size_t cbase = (size_t)a * (t.gx * t.gy + 1);
            const float rangeSq0 = sqr(p.neighbor_dist);
            float rangeK = rangeSq0;
            const float B = p.neighbor_dist * 1.0001f + 1e-4f;
            const int cxlo = grid_cell(pos.x - B, t.ics), cxhi = grid_cell(pos.x + B, t.ics);
            const int cylo = grid_cell(pos.y - B, t.ics), cyhi = grid_cell(pos.y + B, t.ics);
            const int ncol = (int)min((unsigned)cxhi - (unsigned)cxlo, (unsigned)(t.gx - 1)) + 1;   // (lo <= hi: c is monotone; NaN gives 1)
            const int nrow = (int)min((unsigned)cyhi - (unsigned)cylo, (unsigned)(t.gy - 1)) + 1;
            const int c0 = cxlo & (t.gx - 1);
            const int n1 = min(ncol, t.gx - c0), n2 = ncol - n1;   // columns c0 .. c0 + n1 - 1, then 0 .. n2 - 1
            auto scan_run = [&](unsigned lo, unsigned hi) {
                hi = min(hi, (unsigned)N);   // (prefix sums of at most N agents: already so on consistent counts)
                for (unsigned u = lo; u < hi; ++u) {
                    const int j = (int)t.sidx[abase + u];
                    const float dsq = absSq(pos - mk(t.sx[abase + u], t.sy[abase + u]));
                    if (j != i && dsq < rangeSq0 && dsq <= rangeK) {
                        sorted_insert<KMAX>(nkey, make_key(dsq, j));
                        if (ncnt < K) ++ncnt;
                        if (ncnt == K) rangeK = key_dist(nkey[KMAX - 1]);
                    }
                }
            };
            for (int r = 0; r < nrow; ++r) {
                const unsigned* rs = t.cell_start + cbase + (size_t)((cylo + r) & (t.gy - 1)) * t.gx;
                scan_run(rs[c0], rs[c0 + n1]);
                if (n2 > 0) scan_run(rs[0], rs[n2]);
            }
        }
    }
#else
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
#endif
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
        const float invTO = 1.0f / CA_T_HORIZON_OBST;
        const float R = CA_T_RADIUS;
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
        const float invT = 1.0f / CA_T_HORIZON;
        const float invDt = 1.0f / p.time_step;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k >= kofs && k - kofs < ncnt) {
                const size_t j = abase + (size_t)key_index(nkey[k]);
#if CA_TILED_PARAMS
                ls.put(nl, agent_orca_line(pos, vel, mk(p.pos_x[j], p.pos_y[j]), mk(p.vel_x[j], p.vel_y[j]), ap_r, ck.ap_radius[j], invT, invDt));
#else
                ls.put(nl, agent_orca_line(pos, vel, mk(p.pos_x[j], p.pos_y[j]), mk(p.vel_x[j], p.vel_y[j]), p.radius, invT, invDt));
#endif
                ++nl;
            }
        }
    }
    // ---- 2-D linear program (App. A.5), LP3 where it is infeasible ----
    V2 nv = mk(0.0f, 0.0f);
    int fail = nl;
    if (active) fail = lp2(ls, nl, CA_T_MAX_SPEED, pref, false, nv);
    if (active && fail < nl) lp3<KMAX + SMAX>((__attribute__((address_space(3))) char*)ls.base, ls.stride, nl, numObstLines, fail, CA_T_MAX_SPEED, nv);
    if (active) { t.nv_x[q] = nv.x; t.nv_y[q] = nv.y; }
#undef CA_T_RADIUS
#undef CA_T_MAX_SPEED
#undef CA_T_HORIZON
#undef CA_T_HORIZON_OBST
