// ca_env.hip -- host side of libcaenv.so: the C ABI declared in include/ca_env.h.
// Owns the device buffers (struct-of-arrays, fp32/int32), the obstacle table and the launch
// geometry; every entry point enqueues work on the handle's stream.  No CPU fallback exists.
#include "../../include/ca_env.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ca_kernels.h"
#include "ca_edge_grid_host.h"
#include "ca_nav_host.h"

using namespace ca;

// a second set of the state buffers (state_planes below): one allocation for the planes every handle has, one for the bandit's,
// which exist after ca_alan_configure* only and change shape with n_actions
struct StateSet {
    unsigned char* base = nullptr;
    unsigned char* alan = nullptr;
    int alan_nA = 0;   // n_actions the bandit's allocation was made for
};
struct ca_env;
struct ca_snapshot {
    ca_env* owner = nullptr;
    StateSet set;
    bool saved = false;
    int n_actions = 0;         // the ALAN shape at the save
    std::vector<int> counts;   // the per-arena agent counts at the save (empty: none were set)
};

struct ca_env {
    ca_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // [A*N] fp32
    float *pos_x = nullptr, *pos_y = nullptr, *vel_x = nullptr, *vel_y = nullptr, *pref_x = nullptr,
          *pref_y = nullptr, *reward = nullptr, *orient_x = nullptr, *orient_y = nullptr;
    bool orient_valid = false;  // orient_x/y match pos/goal (false after the caller edits them)
    double *goal_x = nullptr, *goal_y = nullptr, *goal2_x = nullptr, *goal2_y = nullptr;  // fp64 targets
    int *agent_done = nullptr, *arrive_step = nullptr, *regoal_count = nullptr;
    // neighbour lists, packed (ca_common.h StepArgs): counts u16 [A,N]; indices u8 or u16 [A,K,N] / [A,S,N]
    unsigned short* counts = nullptr;
    void* nb_idx = nullptr;
    unsigned short* obst_idx = nullptr;
    int nidx16 = 0;
    int* cvt_buf = nullptr;  // staging of the i32 image the ABI shows for the packed fields (ca_get / ca_set)
    size_t cvt_cap = 0;
    int *step_count = nullptr, *arena_done = nullptr, *episode = nullptr;
    unsigned long long* arena_stats = nullptr;
    unsigned long long* arena_steps = nullptr;  // [A] steps each arena was advanced, counted by the solve kernels
    float* obs = nullptr;
    bool obs_external = false;
    // the per-agent contact report (ca_contacts, CA_F_CONTACT; ca_contact.h): [5][A*N] words, allocated on first use; no field and no
    // part of the state.  contact_valid: a report has been computed on this handle (ca_get_contacts refuses before)
    int* contact = nullptr;
    bool contact_valid = false;
    // what a step hands back -- observation | reward | arena_done | step_count -- lies in ONE device allocation in this order, so
    // that the host-array form of a step (ca_step_packed) fetches all of it with one copy (obs points elsewhere after ca_bind_obs)
    float* slab = nullptr;
    unsigned long long* dbg = nullptr;  // CA_STAMPS diagnostic build only
    unsigned long long* dbg_obs = nullptr;
    float *tmp_x = nullptr, *tmp_y = nullptr;  // staging for explicit reset positions / host actions
    // ALAN online learning (ca_alan_configure): [A*N][n_actions] fp64 weights / times, [A*N] action,
    // [A*N][4] fp64 directions of the step in flight
    double *alan_w = nullptr, *alan_t = nullptr, *alan_dirs = nullptr, *alan_u = nullptr;
    int* alan_action = nullptr;
    AlanCold* d_alan = nullptr;
    bool alan_fused = false;      // ca_alan_step / ca_alan_rollout run as ONE launch of the four-lanes kernel
    bool alan_lane = false;       // ca_alan_step runs as ONE launch of the register-line lane kernel (its ALAN instantiation)   // the bandit's arguments for the four-lanes kernel (ca_common.h)
    int* mask_buf = nullptr;  // staging for ca_reset_masked's host mask
    std::vector<std::pair<void*, size_t>> host_allocs;   // page-locked host buffers handed out by ca_host_alloc (freed by ca_host_free / ca_destroy)
    int n_actions = 0;   // one set: its size; per-arena sets: the largest (the stride of alan_w / alan_t)
    double act_c[CA_ALAN_MAX_ACTIONS], act_s[CA_ALAN_MAX_ACTIONS];
    // per-arena sets (ca_alan_configure_per_arena): [A][CA_ALAN_MAX_ACTIONS] (cos, sin) and [A] counts, on the device and a
    // host copy for ca_alan_actions_arena; alan_per selects the kernels' ALAN = 2 instantiations
    bool alan_per = false;
    double2* d_act_tab = nullptr;
    int* d_act_n = nullptr;
    std::vector<double> h_act_tab;
    std::vector<int> h_act_n;
    double alan_temp = 0.2, alan_window = 2.0, alan_dt = 1.0 / 60.0;
    ObstDev* d_obst = nullptr;
    std::vector<ObstDev> h_obst;     // every table, concatenated
    std::vector<int> h_tab_off;      // empty: one table for all arenas; else [A + 1] offsets into h_obst
    int* d_tab_off = nullptr;
    StepCold* d_cold = nullptr;      // the epilogue's arguments (ca_common.h)
    TraceDev* d_trace = nullptr;     // the trace block behind StepCold::trace, rewritten in front of every Trace launch of the four-lanes kernel
    bool trace_on = false;           // ca_rollout_trace / ca_alan_rollout_trace: the T-step launch in flight is a Trace instantiation
    ActSeqDev* d_actseq = nullptr;   // the action-sequence block behind StepCold::actseq, rewritten in front of every ActionSeq launch of the four-lanes kernel
    bool actseq_on = false;          // ca_rollout_actions: the launch in flight is an ActionSeq instantiation
    int* actseq_words = nullptr;     // [2][A] first_done of a caller that gave none | frozen at entry (the per-step form); allocated on first use
    // the policy (ca_policy_configure; ca_policy.h): configuration, like the ALAN action sets.  d_wp / d_bp hold the P sets' weights in
    // the order the kernel's B operand reads them and their biases, d_set the arenas' set indices (P > 1), act the [A*N] actions a
    // policy rollout steps under
    struct Policy {
        bool on = false;
        int L = 0, P = 0, out_mode = 0, maxw = 0;
        int width[CA_POLICY_MAX_LAYERS + 1] = {0, 0, 0, 0, 0};
        float limit = 0.0f;
        unsigned wp_off[CA_POLICY_MAX_LAYERS] = {0, 0, 0, 0}, bp_off[CA_POLICY_MAX_LAYERS] = {0, 0, 0, 0}, wset = 0, bset = 0;
        float *d_wp = nullptr, *d_bp = nullptr, *act = nullptr;
        int* d_set = nullptr;
    } pol;
    // the heads of the policy (ca_policy_set_heads; ca_policy.h): d_wp / d_bp are copies of the policy's whose output tile also holds the
    // log-std row (column 1) and the value row (column 2); rr / words: the row records of a sampling rollout that wants its GAE
    // but gave no buffers for them ([cap_rows][A*N] floats, [2][cap_rows][A] words)
    struct Heads {
        bool on = false, has_value = false, has_logstd = false;
        float *d_wp = nullptr, *d_bp = nullptr;
        float* rr = nullptr;
        int* words = nullptr;
        size_t rr_rows = 0, words_rows = 0;
    } heads;
    // the navigation fields (ca_nav_configure; ca_nav.h, ca_nav_host.h): configuration, like the policy.  d_dist / d_next hold the
    // fields of `sets` x G targets over gx x gy cells, d_class the agents' targets, h_blocked the sets' masks (a byte per cell)
    struct Nav {
        bool on = false;
        float x0 = 0.0f, y0 = 0.0f, cell = 0.0f, ics = 0.0f, clearance = 0.0f;
        int gx = 0, gy = 0, G = 0, sets = 0, per_arena = 0, lookahead = 0, sweeps_max = 0, block = 0;
        float* d_dist = nullptr;
        unsigned char* d_next = nullptr;
        int* d_class = nullptr;
        std::vector<unsigned char> h_blocked;
    } nav;
    // the navigated action step (ca_nav_act, ca_nav_step; ca_nav.h): [4][A*N] the direction and the rotated direction nav_act_kernel
    // keeps for nav_reward_kernel, [A] whether the step between them advances the arena.  Allocated on first use; no field and no state
    float* nav_keep = nullptr;
    int* nav_advance = nullptr;
    // the reward terms (ca_reward_configure; ca_reward.h): configuration, like the policy and the navigation.  d_w / h_w hold the [A][7]
    // weights as the kernel uses them (one row repeated when they were given once), need_mask bit k: some arena has w_k != 0.  saved /
    // advance: [A*N] / [A] what reward_begin_kernel keeps for reward_terms_kernel; parts: [7][A*N] r_ref and the counts.  The three are
    // allocated on first use; no field and no state.  parts_valid: parts have been computed on this handle (ca_get_reward_parts refuses before)
    struct Reward {
        bool on = false, parts_valid = false;
        int per_arena = 0, need_mask = 0;
        float margin = 0.0f;
        float* d_w = nullptr;
        std::vector<float> h_w;
        int *saved = nullptr, *advance = nullptr, *parts = nullptr;
    } rew;
    // obstacle-neighbour overflow made loud: a page-locked host word the kernels write (ca_common.h note_overflow); unless the
    // caller opted in (ca_allow_obstacle_overflow) it is the handle's sticky CA_ERANGE status (overflow_status below)
    unsigned long long* ovf_host = nullptr;
    bool allow_overflow = false;
    int* d_order = nullptr;          // [grid] block order of the solve kernel (null: identity)
    int P = 1, logP = 0, BS = 64, grid = 1, K = 0, S = 1;
    bool obs_dense_on = false;
    bool lists_trusted = true;   // the neighbour lists in memory were written by the kernels (not by the caller through ca_set)
    int LS = 1, apb = 1, linv = 65536, dense = 0;   // lanes per arena, arenas per workgroup, ceil(2^16 / LS), packed back to back (ca_common.h StepArgs)
    // diagnostic environment switches, read ONCE by ca_create (a handle never changes behaviour because the environment did):
    // -1 = unset, else the first character's digit
    struct { int reg_lines = -1, pair = -1, alan_fused = -1, nbr_seed = -1, lp3_pairs = -1, nav_block = 0; } sw;
    int ST = 0, KT = 16;  // solve-kernel variant: ST > 0 = register lines with ST obstacle slots; KT = KMAX
    int SMX = 4;          // ... and the capacity of its obstacle-neighbour list (4, or 16: agents with more than ST are solved apart;
                          // SWIDE = 64 with ST = 0: the wide LDS-table kernel of a handle with max_obst_neighbors > 16)
    int max_edges = 0;    // edges of the largest installed obstacle table (the variant depends on it: pick_variant)
    int n_cus = 256;      // compute units of the device (pick_variant: is the batch resident with the LDS line table?)
    bool pair = false;     // large arenas: two lanes per agent for the whole step (ca_pair.h)
    size_t lds_p = 0;
    bool quad = false;     // four lanes per agent (ca_quad.h): small batches / small arenas
    bool quad_roll = false;  // ... for ca_rollout's one-launch-for-T-steps form (pays a little longer than for single steps)
    int BSq = 64, grid_q = 1, SQ = 4;   // SQ: obstacle-neighbour capacity of the quad variant (4 or 16)
    size_t lds_q = 0;
    size_t lds = 0;
    // per-agent ORCA parameters (ca_set_agent_params): configuration, like the obstacle tables.  ap = the handle runs the
    // AgentParams instantiations (one lane per agent on the LDS line table, the observation with an octagon per neighbour);
    // quad_cfg / quad_roll_cfg keep what ca_create chose for uniform parameters, to return to when the parameters are cleared.
    bool ap = false, quad_cfg = false, quad_roll_cfg = false;
    float* d_ap[4] = {nullptr, nullptr, nullptr, nullptr};   // [A*N] radius | max_speed | time_horizon | time_horizon_obst
    float* d_ap_oct = nullptr;                               // [A*N][8] float2: every agent's octagon (ca_obs.h ObsArgs::ap_oct)
    std::vector<float> h_ap[4];                              // host copies (ca_get_agent_params)
    // per-arena agent counts (ca_set_agent_counts): configuration too.  ac = the handle runs the ArenaCounts instantiations, which
    // are AgentParams kernels: ap = ap_user || ac, and without parameters of the caller's (ap_user) the per-agent arrays hold the
    // ca_config values.
    bool ac = false, ap_user = false;
    int* d_counts = nullptr;                                 // [A]
    std::vector<int> h_counts;                               // host copy (ca_get_agent_counts, ca_get_stats); empty while !ac
    // per-agent sensing (ca_set_agent_sensing): configuration too.  sens = the handle runs the AgentSensing instantiations, which
    // exist beside AgentParams / ArenaCounts only: ap = ap_user || ac || sens, the per-agent arrays holding the ca_config values
    // unless the caller set them, as under counts.  cfg.neighbor_dist and cfg.max_neighbors stay the capacities everything is sized by.
    bool sens = false;
    float* d_as_nd = nullptr;                                // [A*N] neighbor_dist_i
    unsigned char* d_as_k = nullptr;                         // [A*N] max_neighbors_i (0 .. CA_MAX_NEIGHBORS fits a byte)
    std::vector<float> h_as_nd;                              // host copies (ca_get_agent_sensing); empty while !sens
    std::vector<int> h_as_k;
    // the tiled solve path (ca_create_ex, CA_CREATE_TILED; ca_tiled.h): an arena spans `tiles` workgroups of TILE lanes, a step is
    // three launches (solve, advance, close)
    bool tiled = false;
    int TILE = 128, tiles = 1;
    float *nv_x = nullptr, *nv_y = nullptr;   // [A*N] new velocity, then the copy of the post-step position (ca_tiled.h TiledArgs)
    unsigned* tscr = nullptr;                 // [A][TS_STRIDE] per-arena scratch of the three launches
    // ... with the uniform grid (CA_CREATE_TILED_GRID; ca_tiled.h TiledGridArgs): three launches of a counting sort in front of them
    bool tgrid = false;
    int tgx = 0, tgy = 0;                     // the wrapped cell table's sides: powers of two, 8 .. 128
    float tcs = 0.0f, tics = 0.0f;            // cell size = neighbor_dist / 2, and its reciprocal
    unsigned *tg_count = nullptr, *tg_start = nullptr, *tg_key = nullptr;   // [A][cells] | [A][cells + 1] | [A*N]
    float *tg_sx = nullptr, *tg_sy = nullptr; // [A*N] positions in cell order
    unsigned short* tg_sidx = nullptr;        // [A*N] agent ids in cell order
    // ... and the static grid over the obstacle edges (ca_tiled_edge_grid; ca_tiled.h EdgeGridDev): configuration, like the tables it
    // indexes; rebuilt by install_tables while on
    struct EdgeGrids {
        std::vector<EdgeGridDev> desc;            // one per table: [A] with tables per arena, else [1]
        EdgeGridDev* d_desc = nullptr;
        unsigned *d_cells = nullptr, *d_entries = nullptr;
    };
    bool egrid = false;
    EdgeGrids eg;
    // ... and per-agent ORCA parameters on it (CA_CREATE_TILED_PARAMS; ca_tiled.h's AgentParams instantiations): tparams = the handle accepts
    // ca_set_agent_params; while parameters are set, ap = ap_user = true as on an ordinary handle, and ap_rmax is their largest radius
    bool tparams = false;
    float ap_rmax = 0.0f;
    // ... or obstacle lists of up to 64 on it (CA_CREATE_TILED_WIDE; ca_tiled.h's WideObstLists instantiations, run when S > 16)
    bool twide = false;
    // forking and rewinding arenas (ca_arena_gather, ca_snapshot_*; ca_fork.h): fork_scratch is the second set of the state buffers the
    // in-place gather copies through, allocated on first use; fork_idx the [A] index array on the device; snapshots the sets handed out
    // and still alive (ca_destroy frees them)
    StateSet fork_scratch;
    int* fork_idx = nullptr;
    std::vector<ca_snapshot*> snapshots;
    uint64_t agent_steps_base = 0;   // agent-steps of the arena steps counted before the counts last changed (ca_get_stats)
    uint64_t steps_done = 0;  // env steps enqueued (profiling cadence only: ca_stats.agent_steps is counted in the kernels)
    float rays[32], oct[32];
    // opt-in per-kernel timing (ca_profile): event pairs recorded around launches, drained on read
    bool profiling = false;   // events are recorded for the current step
    int prof_period = 0;      // 0 = off, k = every k-th step
    struct Span { hipEvent_t t0, t1; int kind; int steps; };  // steps: env steps advanced by the timed launch (ca_rollout: T)
    std::vector<Span> spans;
    std::vector<hipEvent_t> free_events;
    std::string err;
};

static thread_local std::string g_create_err;

static int fail(ca_env* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->err = buf;
    else g_create_err = buf;
    return code;
}
#define HIPCHK(e, call)                                                                         \
    do {                                                                                        \
        hipError_t _r = (call);                                                                 \
        if (_r != hipSuccess) return fail(e, CA_EHIP, "%s failed: %s", #call, hipGetErrorString(_r)); \
    } while (0)

// RVO2 keeps EVERY obstacle edge in range of an agent (env.py:249, 301-318 iterate them all); the lists here hold
// max_obst_neighbors (<= CA_MAX_OBST_NEIGHBORS) and drop the farthest beyond that -- a deviation that must not pass silently.
// The kernels report the last overflow through a host-visible word; every call that advances the environment returns
// CA_ERANGE from then on (like a sticky device error: the call AFTER the kernel that overflowed has finished sees it, and the
// calls that synchronise -- ca_sync, ca_step_packed -- see it at once), until ca_reset_stats clears it or the caller accepts
// the truncation with ca_allow_obstacle_overflow(env, 1).  ca_get / ca_get_stats keep working (obst_overflow counts).
static int overflow_status(ca_env* e, const char* where) {
    if (e->allow_overflow || !e->ovf_host) return CA_OK;
    const unsigned long long v = *(volatile unsigned long long*)e->ovf_host;
    if (!(v >> 63)) return CA_OK;
    return fail(e, CA_ERANGE, "%s: an obstacle-neighbour list overflowed: arena %lld, agent %d had %d%s obstacle edges in range but "
                "max_obst_neighbors=%d, so the farthest were dropped (RVO2 keeps every edge in range: collision_avoidence_env.py:249, "
                "301-318).  Raise max_obst_neighbors (at most %d), coarsen the world's polylines, or accept the truncation with "
                "ca_allow_obstacle_overflow(env, 1); ca_reset_stats clears this status", where,
                // (a tiled handle's word has a wider agent field: ca_tiled.h note_overflow_tiled)
                (long long)(e->tiled ? (v >> 24) & 0xFFFFFFFFFull : (v >> 20) & 0xFFFFFFFFFFull),
                (int)(e->tiled ? (v >> 8) & 0xFFFF : (v >> 8) & 0x7FF), (int)(v & 0xFF), (v & 0xFF) == 255 ? "+" : "",
                e->S, CA_MAX_OBST_NEIGHBORS);
}

enum { KIND_NBR = 0, KIND_STEP = 1, KIND_OBS = 2, KIND_RESET = 3 };   // (KIND_NBR: the neighbour search has no launch of its own)
enum { CA_ROLLOUT_MAX_T = 256 };  // steps per launch of the one-launch rollout (ca_rollout)  // KIND_RESET also times the small ALAN kernels
static hipEvent_t prof_event(ca_env* e) {
    if (!e->free_events.empty()) { hipEvent_t ev = e->free_events.back(); e->free_events.pop_back(); return ev; }
    hipEvent_t ev = nullptr;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    return ev;
}
// Kernel times: a sampled launch carries a start and a stop event ON ITS OWN DISPATCH (hipExtLaunchKernel: the
// timestamps of the dispatch packet's completion signal), not events recorded around it in the stream -- a recorded event
// is a barrier packet of its own and costs the step loop ~2.5 us each, 4 % of a C3 step when every second step is sampled.
struct ProfScope {
    ca_env* e; hipEvent_t t0 = nullptr, t1 = nullptr; int kind; int steps;
    ProfScope(ca_env* env, int k, int n_steps = 1) : e(env), kind(k), steps(n_steps) {
        if (!e->profiling) return;
        t0 = prof_event(e);
        t1 = t0 ? prof_event(e) : nullptr;
        if (t0 && !t1) { e->free_events.push_back(t0); t0 = nullptr; }
    }
    ~ProfScope() {
        if (t0) e->spans.push_back({t0, t1, kind, steps});
    }
};
template <class... Args>
static void launch_k(const ProfScope& ps, void (*kernel)(Args...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                     Args... args) {
    if (ps.t0) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, ps.t0, ps.t1, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}

// The sampling cadence of ca_profile(period > 1): the launches that follow are timed when the handle's step count, in units of `unit`
// steps, is a multiple of the period.  unit = 1: a step; CA_ROLLOUT_MAX_T: a launch of the one-launch rollout.
static void prof_cadence(ca_env* e, int unit) {
    if (e->prof_period > 1) e->profiling = (e->steps_done / (uint64_t)unit) % (uint64_t)e->prof_period == 0;
}

static size_t AN(const ca_env* e) { return (size_t)e->cfg.n_arenas * e->cfg.n_agents; }

struct FieldInfo {
    void* ptr;
    size_t bytes;
    bool writable;
};
static FieldInfo field_info(ca_env* e, int f) {
    const size_t an = AN(e), A = e->cfg.n_arenas;
    switch (f) {
        case CA_FLD_POS_X: return {e->pos_x, an * 4, true};
        case CA_FLD_POS_Y: return {e->pos_y, an * 4, true};
        case CA_FLD_VEL_X: return {e->vel_x, an * 4, true};
        case CA_FLD_VEL_Y: return {e->vel_y, an * 4, true};
        case CA_FLD_PREF_X: return {e->pref_x, an * 4, true};
        case CA_FLD_PREF_Y: return {e->pref_y, an * 4, true};
        case CA_FLD_GOAL_X: return {e->goal_x, an * 8, true};
        case CA_FLD_GOAL_Y: return {e->goal_y, an * 8, true};
        case CA_FLD_GOAL2_X: return {e->goal2_x, an * 8, true};
        case CA_FLD_GOAL2_Y: return {e->goal2_y, an * 8, true};
        case CA_FLD_REWARD: return {e->reward, an * 4, true};   // (writable for set_state: a frozen arena keeps its last reward)
        case CA_FLD_AGENT_DONE: return {e->agent_done, an * 4, true};
        case CA_FLD_ARRIVE_STEP: return {e->arrive_step, an * 4, true};
        // packed in device memory; the ABI shows them as i32 (ca_get / ca_set convert, ca_field_ptr refuses)
        case CA_FLD_NB_COUNT: return {e->counts, an * 4, true};
        case CA_FLD_NB_IDX: return {e->nb_idx, an * 4 * (size_t)(e->K > 0 ? e->K : 1), true};
        case CA_FLD_OBST_COUNT: return {e->counts, an * 4, true};
        case CA_FLD_OBST_IDX: return {e->obst_idx, an * 4 * (size_t)e->S, true};
        case CA_FLD_OBS: return {e->obs, an * CA_OBS_DIM * 4, true};   // (writable: ca_policy_actions reads the buffer as it stands)
        case CA_FLD_STEP_COUNT: return {e->step_count, A * 4, true};
        case CA_FLD_ARENA_DONE: return {e->arena_done, A * 4, true};
        case CA_FLD_EPISODE: return {e->episode, A * 4, true};
        case CA_FLD_REGOAL_COUNT: return {e->regoal_count, an * 4, true};
        case CA_FLD_ALAN_WEIGHTS: return {e->alan_w, an * 8 * (size_t)e->n_actions, true};
        case CA_FLD_ALAN_TIMES: return {e->alan_t, an * 8 * (size_t)e->n_actions, true};
        case CA_FLD_ALAN_ACTION: return {e->alan_action, an * 4, true};   // (writable for set_state: a frozen arena keeps its last action)
        case CA_FLD_ARENA_STATS: return {e->arena_stats, A * ST_STRIDE * 8, false};
        default: return {nullptr, 0, false};
    }
}

static void host_tables(ca_env* e) {
    // env.py:321-332 ray end points; env.py:335-350 octagon chords (fp64 like the reference's
    // Python floats, then rounded once to fp32)
    const double nd = (double)e->cfg.neighbor_dist, r = (double)e->cfg.radius;
    for (int i = 0; i < 16; ++i) {
        const double th = i * (2.0 * M_PI / 16);
        e->rays[2 * i] = (float)(nd * std::cos(th));
        e->rays[2 * i + 1] = (float)(-nd * std::sin(th));
    }
    double first[2] = {r * std::cos(0.0), -r * std::sin(0.0)}, cur[2] = {first[0], first[1]};
    int k = 0;
    for (int i = 1; i < 8; ++i, ++k) {
        const double th = i * (2.0 * M_PI / 8);
        const double nx = r * std::cos(th), ny = -r * std::sin(th);
        e->oct[4 * k] = (float)cur[0]; e->oct[4 * k + 1] = (float)cur[1];
        e->oct[4 * k + 2] = (float)nx; e->oct[4 * k + 3] = (float)ny;
        cur[0] = nx; cur[1] = ny;
    }
    e->oct[4 * k] = (float)cur[0]; e->oct[4 * k + 1] = (float)cur[1];
    e->oct[4 * k + 2] = (float)first[0]; e->oct[4 * k + 3] = (float)first[1];
}

// the per-handle block of epilogue arguments (ca_common.h StepCold); written once, at the end of ca_create
static void fill_cold(const ca_env* e, StepCold& c) {
    const ca_config& g = e->cfg;
    c.pos_x = e->pos_x; c.pos_y = e->pos_y; c.vel_x = e->vel_x; c.vel_y = e->vel_y;
    c.pref_x = e->pref_x; c.pref_y = e->pref_y; c.goal_x = e->goal_x; c.goal_y = e->goal_y;
    c.goal2_x = e->goal2_x; c.goal2_y = e->goal2_y; c.reward = e->reward;
    c.orient_x = e->orient_x; c.orient_y = e->orient_y;
    c.agent_done = e->agent_done; c.arrive_step = e->arrive_step; c.regoal_count = e->regoal_count;
    c.step_count = e->step_count; c.arena_done = e->arena_done; c.episode = e->episode;
    c.arena_stats = e->arena_stats; c.arena_steps = e->arena_steps; c.ovf_word = e->ovf_host;
    c.reward_scale = g.reward_scale; c.seed = g.seed; c.arena_offset = g.arena_offset;
    c.max_step = g.max_step; c.done_mode = g.done_mode; c.done_x_thresh = g.done_x_thresh;
    c.spawn_x0 = g.spawn_x0; c.spawn_x1 = g.spawn_x1; c.spawn_y0 = g.spawn_y0; c.spawn_y1 = g.spawn_y1;
    c.goal_x0 = g.goal_x0; c.goal_x1 = g.goal_x1; c.goal_y0 = g.goal_y0; c.goal_y1 = g.goal_y1;
    c.ap_radius = e->ap ? e->d_ap[0] : nullptr; c.ap_max_speed = e->ap ? e->d_ap[1] : nullptr;
    c.ap_time_horizon = e->ap ? e->d_ap[2] : nullptr; c.ap_time_horizon_obst = e->ap ? e->d_ap[3] : nullptr;
    c.agent_counts = e->ac ? e->d_counts : nullptr;
    c.trace = e->d_trace;
    c.actseq = e->d_actseq;
    c.as_neighbor_dist = e->sens ? e->d_as_nd : nullptr; c.as_max_neighbors = e->sens ? e->d_as_k : nullptr;
}

static void fill_args(ca_env* e, StepArgs& a, const float* actions, uint32_t flags) {
    const ca_config& c = e->cfg;
    a.pos_x = e->pos_x; a.pos_y = e->pos_y; a.vel_x = e->vel_x; a.vel_y = e->vel_y;
    a.pref_x = e->pref_x; a.pref_y = e->pref_y; a.goal_x = e->goal_x; a.goal_y = e->goal_y;
    a.counts = e->counts; a.nb_idx = e->nb_idx; a.obst_idx = e->obst_idx;
    a.arena_done = e->arena_done; a.arena_stats = e->arena_stats; a.cold = e->d_cold;
    a.obst = e->d_obst; a.tab_off = e->d_tab_off; a.actions = actions; a.alan = nullptr; a.alan_u = nullptr;
#ifdef CA_STAMPS
    a.order = e->d_order;
#endif
    a.reset_px = nullptr; a.reset_py = nullptr; a.reset_mask = nullptr; a.dbg = e->dbg;
    a.n_obst = e->h_tab_off.empty() ? (int)e->h_obst.size() : 0; a.A = c.n_arenas; a.N = c.n_agents; a.P = e->P; a.logP = e->logP;
    a.K = e->K; a.S = e->S; a.flags = flags; a.a0 = 0; a.a1 = c.n_arenas; a.T = 1;
    a.LS = e->LS; a.apb = e->apb; a.linv = e->linv; a.dense = e->dense; a.nb_hint = e->lists_trusted ? 1 : 0;
    a.time_step = c.time_step; a.neighbor_dist = c.neighbor_dist; a.time_horizon = c.time_horizon;
    a.time_horizon_obst = c.time_horizon_obst; a.radius = c.radius; a.max_speed = c.max_speed;
}

// ---- the solve launch of a step ----------------------------------------------------------------------------------------
// The one place where the variant the handle chose (pick_variant, alan_pick, the quad switches of ca_create) becomes a kernel
// instantiation, a grid, a block and a dynamic LDS size: launch_step launches what solve_launch returns, apply_variant_attributes
// and alan_pick raise the dynamic-LDS limit of exactly these kernels, and ca_launch_info reports the plain single-step form.
struct SolveLaunch { const void* fn; dim3 grid, block; size_t lds; bool seeded = false, paired = false; };   // seeded: fn is a SeededScan kernel (ca_nbr.h); paired: ... and a PairedLp3 one (ca_lp.h)
template <class F> static const void* fn_ptr(F* f) { return reinterpret_cast<const void*>(f); }
// one lane per agent: register lines (ST = 4) or the LDS line table (ST = 0); the ALAN instantiations exist for one and two waves
// seed: the handle asks for the seeded agent scan, which the one-wave kernels have a twin for under the SeededScan tag (ca_nbr.h:
// the untagged kernels, their ALAN forms -- with an action set per arena too -- and the ArenaCounts kernels below); *seeded: a twin it is
// pairs: the handle asks for the paired LP3 round, which the seeded register-line kernels with obstacle lists of 4 have a twin for
// under the PairedLp3 tag (ca_lp.h); *paired: that twin it is
template <int KMAX, int ST, int SMX, bool ALAN, class... PER>
static const void* step_fn_for(int BS, bool seed, bool* seeded, bool pairs = false, bool* paired = nullptr) {
#if CA_NBR_SEED
    if (seed && BS == 64) {
        *seeded = true;
#if CA_LP3_PAIRS
        if constexpr (ST > 0 && SMX == ST && !ALAN && sizeof...(PER) == 0) {
            if (pairs && paired) { *paired = true; return fn_ptr(&step_kernel<KMAX, 64, ST, SMX, false, SeededScan, PairedLp3>); }
        }
#endif
        return fn_ptr(&step_kernel<KMAX, 64, ST, SMX, ALAN, PER..., SeededScan>);
    }
#endif
    if constexpr (ALAN) {
        return BS == 64 ? fn_ptr(&step_kernel<KMAX, 64, ST, SMX, true, PER...>) : fn_ptr(&step_kernel<KMAX, 128, ST, SMX, true, PER...>);
    } else {
        switch (BS) {
            case 64: return fn_ptr(&step_kernel<KMAX, 64, ST, SMX>);
            case 128: return fn_ptr(&step_kernel<KMAX, 128, ST, SMX>);
            case 256: return fn_ptr(&step_kernel<KMAX, 256, ST, SMX>);
            case 512: return fn_ptr(&step_kernel<KMAX, 512, ST, SMX>);
            default: return fn_ptr(&step_kernel<KMAX, 1024, ST, SMX>);
        }
    }
}
template <int KMAX>
static const void* pair_fn_for(int BS) {
    return BS == 256 ? fn_ptr(&pair_kernel<KMAX, 256>) : fn_ptr(&pair_kernel<KMAX, 512>);
}
template <int KMAX, int SQ, bool ALAN, class... PER>
static const void* quad_fn_for(int BS) {
    switch (BS) {
        case 64: return fn_ptr(&quad_kernel<KMAX, 64, SQ, ALAN, PER...>);
        case 128: return fn_ptr(&quad_kernel<KMAX, 128, SQ, ALAN, PER...>);
        case 256: return fn_ptr(&quad_kernel<KMAX, 256, SQ, ALAN, PER...>);
        default: return fn_ptr(&quad_kernel<KMAX, 512, SQ, ALAN, PER...>);
    }
}
// the wide LDS-table kernel (obstacle lists of 17 .. 64): arenas of at most 128 agents, no ALAN form
template <int KMAX>
static const void* wide_fn_for(int BS) {
    return BS == 64 ? fn_ptr(&step_kernel<KMAX, 64, 0, SWIDE>) : fn_ptr(&step_kernel<KMAX, 128, 0, SWIDE>);
}
// per-agent parameters (ca_set_agent_params): the LDS line table with lists of up to 16, any arena size that fits; no ALAN form
template <int KMAX>
static const void* ap_fn_for(int BS) {
    switch (BS) {
        case 64: return fn_ptr(&step_kernel<KMAX, 64, 0, SMAX, false, AgentParams>);
        case 128: return fn_ptr(&step_kernel<KMAX, 128, 0, SMAX, false, AgentParams>);
        case 256: return fn_ptr(&step_kernel<KMAX, 256, 0, SMAX, false, AgentParams>);
        case 512: return fn_ptr(&step_kernel<KMAX, 512, 0, SMAX, false, AgentParams>);
        default: return fn_ptr(&step_kernel<KMAX, 1024, 0, SMAX, false, AgentParams>);
    }
}
// ... and agent counts per arena (ca_set_agent_counts): the same kernel under the ArenaCounts tag, which includes AgentParams
template <int KMAX>
static const void* ac_fn_for(int BS, bool seed, bool* seeded) {
#if CA_NBR_SEED
    if (seed && BS == 64) { *seeded = true; return fn_ptr(&step_kernel<KMAX, 64, 0, SMAX, false, ArenaCounts, SeededScan>); }
#endif
    switch (BS) {
        case 64: return fn_ptr(&step_kernel<KMAX, 64, 0, SMAX, false, ArenaCounts>);
        case 128: return fn_ptr(&step_kernel<KMAX, 128, 0, SMAX, false, ArenaCounts>);
        case 256: return fn_ptr(&step_kernel<KMAX, 256, 0, SMAX, false, ArenaCounts>);
        case 512: return fn_ptr(&step_kernel<KMAX, 512, 0, SMAX, false, ArenaCounts>);
        default: return fn_ptr(&step_kernel<KMAX, 1024, 0, SMAX, false, ArenaCounts>);
    }
}
// ... and either of the two with neighbor_dist and max_neighbors per agent (ca_set_agent_sensing): the AgentSensing tag
// (the tag includes AgentParams and stands without it; with counts per arena, behind ArenaCounts)
template <int KMAX, class... TAGS>
static const void* sens_fn_for(int BS) {
    switch (BS) {
        case 64: return fn_ptr(&step_kernel<KMAX, 64, 0, SMAX, false, TAGS...>);
        case 128: return fn_ptr(&step_kernel<KMAX, 128, 0, SMAX, false, TAGS...>);
        case 256: return fn_ptr(&step_kernel<KMAX, 256, 0, SMAX, false, TAGS...>);
        case 512: return fn_ptr(&step_kernel<KMAX, 512, 0, SMAX, false, TAGS...>);
        default: return fn_ptr(&step_kernel<KMAX, 1024, 0, SMAX, false, TAGS...>);
    }
}
template <class... TAGS>
static const void* sens_fn_of(const ca_env* e) {
    return e->KT == 5 ? sens_fn_for<5, TAGS...>(e->BS) : (e->KT == 16 ? sens_fn_for<16, TAGS...>(e->BS) : sens_fn_for<10, TAGS...>(e->BS));
}
// the lane kernel of the handle's KMAX and line storage: register lines with obstacle lists of 4, or of 16 (the rare agent with
// more than 4 is solved apart), else the LDS line table; K = 16 has the table only, and no ALAN form
template <bool ALAN, class... PER>
static const void* lane_fn_for(const ca_env* e, bool* seeded, bool* paired) {
    const bool sd = e->sw.nbr_seed != 0;   // (CA_NBR_SEED=0 in the environment, latched by ca_create: the unseeded agent scan)
    const bool pl = e->sw.lp3_pairs < 0 ? CA_LP3_PAIRS_DEFAULT != 0 : e->sw.lp3_pairs != 0;   // (CA_LP3_PAIRS=0 / 1 in the environment, latched by ca_create)
    if (e->sens) return e->ac ? sens_fn_of<ArenaCounts, AgentSensing>(e) : sens_fn_of<AgentSensing>(e);   // (ap is on with it; no ALAN form either)
    if (e->ac) return e->KT == 5 ? ac_fn_for<5>(e->BS, sd, seeded) : (e->KT == 16 ? ac_fn_for<16>(e->BS, sd, seeded) : ac_fn_for<10>(e->BS, sd, seeded));   // (refused by the ALAN calls)
    if (e->ap) return e->KT == 5 ? ap_fn_for<5>(e->BS) : (e->KT == 16 ? ap_fn_for<16>(e->BS) : ap_fn_for<10>(e->BS));   // (alan_pick never asks for an ALAN form of it)
    if (e->SMX > SMAX) return e->KT == 5 ? wide_fn_for<5>(e->BS) : (e->KT == 16 ? wide_fn_for<16>(e->BS) : wide_fn_for<10>(e->BS));   // (alan_pick never asks for an ALAN form of it)
    if (e->ST > 0 && e->SMX > 4) return e->KT == 5 ? step_fn_for<5, 4, 16, ALAN, PER...>(e->BS, sd, seeded) : step_fn_for<10, 4, 16, ALAN, PER...>(e->BS, sd, seeded);
    if (e->ST > 0) return e->KT == 5 ? step_fn_for<5, 4, 4, ALAN, PER...>(e->BS, sd, seeded, pl, paired) : step_fn_for<10, 4, 4, ALAN, PER...>(e->BS, sd, seeded, pl, paired);
    if (e->KT == 5) return step_fn_for<5, 0, SMAX, ALAN, PER...>(e->BS, sd, seeded);
    if constexpr (!ALAN) { if (e->KT == 16) return step_fn_for<16, 0, SMAX, false>(e->BS, sd, seeded); }
    return step_fn_for<10, 0, SMAX, ALAN, PER...>(e->BS, sd, seeded);
}
template <bool ALAN, class... PER>
static const void* quad_fn_for(const ca_env* e) {   // (K <= 10)
    if (e->SQ > 4) return e->KT == 5 ? quad_fn_for<5, 16, ALAN, PER...>(e->BSq) : quad_fn_for<10, 16, ALAN, PER...>(e->BSq);
    return e->KT == 5 ? quad_fn_for<5, 4, ALAN, PER...>(e->BSq) : quad_fn_for<10, 4, ALAN, PER...>(e->BSq);
}
// the tiled path's solve launch (ca_tiled.h): KMAX class x TILE, written once for every search and parameter form
template <int KMAX, int SEARCH, class... PER>
static const void* tiled_solve_fn_for(int TILE) {
    switch (TILE) {
        case 64: return fn_ptr(&tiled_solve_kernel<KMAX, 64, SEARCH, PER...>);
        case 256: return fn_ptr(&tiled_solve_kernel<KMAX, 256, SEARCH, PER...>);
        default: return fn_ptr(&tiled_solve_kernel<KMAX, 128, SEARCH, PER...>);
    }
}
template <int SEARCH, class... PER>
static const void* tiled_solve_fn_for(const ca_env* e) {
    return e->KT == 5 ? tiled_solve_fn_for<5, SEARCH, PER...>(e->TILE)
                      : (e->KT == 16 ? tiled_solve_fn_for<16, SEARCH, PER...>(e->TILE) : tiled_solve_fn_for<10, SEARCH, PER...>(e->TILE));
}
enum { TILED_SORT_LAUNCHES = 3 };   // bin, scan, scatter
// the solve launch of a tiled handle, with the static edge grid on or off (egrid: a grid handle only); AgentParams while
// ca_set_agent_params is in force (CA_CREATE_TILED_PARAMS); WideObstLists for obstacle lists above 16 (CA_CREATE_TILED_WIDE)
static const void* tiled_solve_fn(const ca_env* e, bool egrid) {
    if (e->S > SMAX) {   // (CA_CREATE_TILED_WIDE: never with per-agent parameters)
        if (e->tgrid && egrid) return tiled_solve_fn_for<SEARCH_GRID_EDGES, WideObstLists>(e);
        return e->tgrid ? tiled_solve_fn_for<SEARCH_GRID, WideObstLists>(e) : tiled_solve_fn_for<SEARCH_ALL, WideObstLists>(e);
    }
    if (e->sens) {   // (ca_set_agent_sensing on a handle made with CA_CREATE_TILED_PARAMS: ap is on with it)
        if (e->tgrid && egrid) return tiled_solve_fn_for<SEARCH_GRID_EDGES, AgentSensing>(e);
        return e->tgrid ? tiled_solve_fn_for<SEARCH_GRID, AgentSensing>(e) : tiled_solve_fn_for<SEARCH_ALL, AgentSensing>(e);
    }
    if (e->tgrid && egrid) return e->ap ? tiled_solve_fn_for<SEARCH_GRID_EDGES, AgentParams>(e) : tiled_solve_fn_for<SEARCH_GRID_EDGES>(e);
    if (e->tgrid) return e->ap ? tiled_solve_fn_for<SEARCH_GRID, AgentParams>(e) : tiled_solve_fn_for<SEARCH_GRID>(e);
    return e->ap ? tiled_solve_fn_for<SEARCH_ALL, AgentParams>(e) : tiled_solve_fn_for<SEARCH_ALL>(e);
}
// ... its advance and close launches (with AgentParams the close launch takes TiledCloseParamsArgs)
static const void* tiled_advance_fn(const ca_env* e) {
    if (e->ap) return e->egrid ? fn_ptr(&tiled_advance_kernel<true, AgentParams>) : fn_ptr(&tiled_advance_kernel<false, AgentParams>);
    return e->egrid ? fn_ptr(&tiled_advance_kernel<true>) : fn_ptr(&tiled_advance_kernel<false>);
}
static const void* tiled_close_fn(const ca_env* e) {
    if (e->sens) return fn_ptr(&tiled_close_kernel<AgentSensing>);   // (the list shortcut of the pair count takes the lane's own range and K)
    return e->ap ? fn_ptr(&tiled_close_kernel<AgentParams>) : fn_ptr(&tiled_close_kernel<>);
}
// alan: the ALAN bandit runs inside the launch (ca_alan_step, ca_alan_rollout); rollout: the launch advances a.T > 1 steps;
// trace: ... and records them (the Trace instantiations of the four-lanes kernel: the ORCA-only rollout and the fused ALAN rollout with
// one action set; the callers ask for nothing else); actseq: ... under the caller's action tensor (the ActionSeq instantiations, without
// ALAN: ca_rollout_actions asks for them on the handles whose rollout is this kernel, with rollout = true whatever a.T is)
static SolveLaunch solve_launch(const ca_env* e, bool alan, bool rollout, bool trace = false, bool actseq = false) {
    if (e->tiled)   // (the solve launch of a step's sequence; no ALAN and no rollout form)
        return {tiled_solve_fn(e, e->egrid), dim3(e->grid), dim3(e->TILE), e->lds};
    const bool per = alan && e->alan_per;   // (an action set per arena: the AlanArenaSets instantiations)
    if (e->quad || (rollout && e->quad_roll) || (alan && !e->alan_lane)) {   // four lanes per agent (ca_quad.h)
        const void* f = actseq ? quad_fn_for<false, ActionSeq>(e)
                      : trace ? (alan ? quad_fn_for<true, Trace>(e) : quad_fn_for<false, Trace>(e))
                              : (per ? quad_fn_for<true, AlanArenaSets>(e) : (alan ? quad_fn_for<true>(e) : quad_fn_for<false>(e)));
        return {f, dim3(e->grid_q), dim3(e->BSq), alan ? quad_lds_bytes(e->BSq, e->KT, e->SQ, e->n_actions) : e->lds_q};
    }
    if (e->pair)   // two lanes per agent (ca_pair.h): one arena per workgroup of 2 P lanes
        return {e->KT == 5 ? pair_fn_for<5>(e->BS) : pair_fn_for<10>(e->BS), dim3(e->grid), dim3(2 * e->BS), e->lds_p};
    bool seeded = false, paired = false;
    const void* f = per ? lane_fn_for<true, AlanArenaSets>(e, &seeded, &paired) : (alan ? lane_fn_for<true>(e, &seeded, &paired) : lane_fn_for<false>(e, &seeded, &paired));
    return {f, dim3(e->grid), dim3(e->BS), e->lds, seeded, paired};
}
// (above the 48 KiB that every kernel may take, a kernel's dynamic LDS needs its limit raised before the launch)
static hipError_t allow_lds(const SolveLaunch& s) {
    return s.lds > 48 * 1024 ? hipFuncSetAttribute(s.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds) : hipSuccess;
}
// neighbour search + lines + LP + integration + reward/done (+ the ALAN bandit), a.T steps
static hipError_t launch_step(ca_env* e, const StepArgs& a) {
    const SolveLaunch s = solve_launch(e, a.alan != nullptr, a.T > 1 || e->actseq_on, e->trace_on && a.T > 1, e->actseq_on);
    if (!(a.flags & CA_F_FREEZE)) e->lists_trusted = true;   // every arena's lists are this launch's now (frozen arenas keep theirs)
    if (e->tiled) {   // [bin -> scan -> scatter ->] solve -> advance -> close: the kernel boundaries on the stream are the arena-wide barriers (ca_tiled.h)
        // one block for every launch but one: a kernel reads the base of TiledEdgeArgs that it declares (fields a handle does not have stay null / zero)
        TiledEdgeArgs ta;
        ta.s = a; ta.nv_x = e->nv_x; ta.nv_y = e->nv_y; ta.scr = e->tscr; ta.tiles = e->tiles;
        ta.cell_count = e->tg_count; ta.cell_start = e->tg_start; ta.key = e->tg_key;
        ta.sx = e->tg_sx; ta.sy = e->tg_sy; ta.sidx = e->tg_sidx;
        ta.gx = e->tgx; ta.gy = e->tgy; ta.ics = e->tics;
        ta.eg = e->eg.d_desc; ta.eg_cells = e->eg.d_cells; ta.eg_entries = e->eg.d_entries;
        TiledCloseParamsArgs ca;   // (per-agent parameters: the close launch takes the largest radius behind TiledArgs)
        static_cast<TiledArgs&>(ca) = ta; ca.r_max = e->ap_rmax;
        void* params[] = {&ta};
        void* cparams[] = {&ca};
        const struct { const void* fn; dim3 grid, block; size_t lds; void** args; } seq[TILED_SORT_LAUNCHES + 3] = {
            {fn_ptr(&tiled_bin_kernel), s.grid, s.block, 0, params},
            {fn_ptr(&tiled_scan_kernel), dim3(e->cfg.n_arenas), dim3(1024), 0, params},
            {fn_ptr(&tiled_scatter_kernel), s.grid, s.block, 0, params},
            {s.fn, s.grid, s.block, s.lds, params},
            {tiled_advance_fn(e), s.grid, s.block, 0, params},
            {tiled_close_fn(e), s.grid, s.block, tiled_close_lds_bytes(e->TILE, e->ap), e->ap ? cparams : params}};
        for (int k = e->tgrid ? 0 : TILED_SORT_LAUNCHES; k < TILED_SORT_LAUNCHES + 3; ++k) {   // (each launch timed on its own dispatch, kind 1)
            ProfScope ps(e, KIND_STEP);
            const hipError_t r = ps.t0 ? hipExtLaunchKernel(seq[k].fn, seq[k].grid, seq[k].block, seq[k].args, seq[k].lds, e->stream, ps.t0, ps.t1, 0)
                                       : hipLaunchKernel(seq[k].fn, seq[k].grid, seq[k].block, seq[k].args, seq[k].lds, e->stream);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
    ProfScope ps(e, KIND_STEP, a.T > 1 ? a.T : 1);
    StepArgs arg = a;
    void* params[] = {&arg};
    if (ps.t0) return hipExtLaunchKernel(s.fn, s.grid, s.block, params, s.lds, e->stream, ps.t0, ps.t1, 0);
    return hipLaunchKernel(s.fn, s.grid, s.block, params, s.lds, e->stream);
}

typedef void (*obs_fn_t)(const ObsArgs);
static obs_fn_t obs_fn(int obs_bs, bool w16, bool dense = false, bool wide = false, bool ap = false, bool ac = false) {  // workgroup size x width of the stored agent-neighbour ids
    // (agent counts per arena: the per-agent-parameter kernel under the ArenaCounts tag)
    if (ac) return dense ? obs_kernel<256, false, true, ArenaCounts> : (w16 ? obs_kernel<256, true, false, ArenaCounts> : obs_kernel<256, false, false, ArenaCounts>);
    // (per-agent parameters: 256 lanes, what obs_block_threads gives every arena size; never with obstacle lists above 16)
    if (ap) return dense ? obs_kernel<256, false, true, AgentParams> : (w16 ? obs_kernel<256, true, false, AgentParams> : obs_kernel<256, false, false, AgentParams>);
    // (obstacle lists above 16: arenas of at most 128 agents -- 256 lanes, 8-bit ids; ca_create checks that -- or a tiled handle made
    // with CA_CREATE_TILED_WIDE: 16-bit ids, the neighbours gathered from global memory)
    if (wide) return dense ? obs_kernel<256, false, true, WideObstLists> : (w16 ? obs_kernel<256, true, false, WideObstLists> : obs_kernel<256, false, false, WideObstLists>);
    if (dense) return obs_kernel<256, false, true>;   // (arenas of fewer than 16 agents: 256 lanes, 8-bit ids)
    switch (obs_bs) {
        case 1024: return w16 ? obs_kernel<1024, true> : obs_kernel<1024, false>;
        case 512: return w16 ? obs_kernel<512, true> : obs_kernel<512, false>;
        case 128: return w16 ? obs_kernel<128, true> : obs_kernel<128, false>;
        case 64: return w16 ? obs_kernel<64, true> : obs_kernel<64, false>;
        default: return w16 ? obs_kernel<256, true> : obs_kernel<256, false>;
    }
}

// Arenas of fewer than 16 agents: the 16 agent groups of an observation workgroup take 16 consecutive agents of the batch (the
// reference env's own 10-agent arenas would otherwise leave 6 of 16 groups idle).  CA_OBS_DENSE=0: one arena per workgroup.
static bool obs_dense(const ca_env* e) { return e->obs_dense_on; }   // (latched by ca_create)
// (a tiled handle: obs_kernel<256, true> gathers its neighbours from global memory and never touches the staged arrays -- none are
// carved out, at 16384 agents they would be 256 KB)
static int obs_nstage(const ca_env* e) { return e->tiled ? 0 : (obs_dense(e) ? 16 + 2 * e->cfg.n_agents : e->cfg.n_agents); }
static bool obs_wide(const ca_env* e) { return e->S > SMAX; }   // more than 16 obstacle ids per agent (ca_obs.h WIDE)
static size_t obs_lds(const ca_env* e, int obs_bs) {
    if (e->ap) return obs_lds_bytes_ap(obs_nstage(e), obs_bs, 16 * (e->K + e->S));
    return obs_lds_bytes(obs_nstage(e), obs_bs, 16 * (e->K + e->S), obs_wide(e) ? e->S : 16);
}
static obs_fn_t obs_fn_of(const ca_env* e) { return obs_fn(obs_block_threads(e->cfg.n_agents), e->nidx16 != 0, obs_dense(e), obs_wide(e), e->ap, e->ac); }
// (above the 48 KiB that every kernel may take, the observation kernel's dynamic LDS needs its limit raised before the launch)
static hipError_t allow_obs_lds(const ca_env* e) {
    const size_t ol = obs_lds(e, obs_block_threads(e->cfg.n_agents));
    return ol > 48 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void*>(obs_fn_of(e)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ol) : hipSuccess;
}

static hipError_t launch_obs(ca_env* e) {
    if (!e->orient_valid) {  // positions or goals were edited from outside: re-derive the frame
        StepArgs a;
        fill_args(e, a, nullptr, 0);
        const unsigned an = (unsigned)AN(e);
        hipLaunchKernelGGL(orient_kernel, dim3((an + 255) / 256), dim3(256), 0, e->stream, a);
        hipError_t r = hipGetLastError();
        if (r != hipSuccess) return r;
        e->orient_valid = true;
    }
    ObsArgs o;
    o.pos_x = e->pos_x; o.pos_y = e->pos_y; o.vel_x = e->vel_x; o.vel_y = e->vel_y;
    o.orient_x = e->orient_x; o.orient_y = e->orient_y; o.counts = e->counts; o.nb_idx = e->nb_idx;
    o.obst_idx = e->obst_idx; o.obst = e->d_obst; o.tab_off = e->d_tab_off;
    o.obs = e->obs;
    o.A = e->cfg.n_arenas; o.N = e->cfg.n_agents; o.S = e->S;
    o.K = e->K > 0 ? e->K : 1;  // nb_idx is allocated with one column when K == 0; counts are all zero
    const int obs_bs = obs_block_threads(o.N), apb = obs_bs / 16;
    o.bpa = (o.N + apb - 1) / apb;
    o.paircap = 16 * (e->K + e->S);
    o.a0 = 0; o.dbg = e->dbg_obs;
    o.dense = obs_dense(e) ? 1 : 0;
    o.nstage_max = obs_nstage(e);
    o.xcd = (o.A % 8 == 0 && !o.dense) ? 1 : 0;  // the arena's observation on the XCD (workgroup index mod 8) whose solve workgroup wrote its state
    o.radius = e->cfg.radius;
    memcpy(o.rays, e->rays, sizeof o.rays);
    memcpy(o.oct, e->oct, sizeof o.oct);
    o.ap_oct = e->ap ? e->d_ap_oct : nullptr;
    o.agent_counts = e->ac ? e->d_counts : nullptr;
    const dim3 grid(o.dense ? (unsigned)(((size_t)o.A * o.N + apb - 1) / apb) : (unsigned)((size_t)o.A * o.bpa)), block(obs_bs);
    const size_t lds = obs_lds(e, obs_bs);
    ProfScope ps(e, KIND_OBS);
    launch_k(ps, obs_fn_of(e), grid, block, lds, e->stream, o);
    return hipGetLastError();
}

// The contact report of the current state (ca_contact.h): one launch on the handle's stream, behind whatever left that state, timed
// under kind 3 like the other small kernels.  The buffer is the handle's, allocated on first use.
static hipError_t contact_buffer(ca_env* e) {
    if (e->contact) return hipSuccess;
    return hipMalloc((void**)&e->contact, 5 * AN(e) * 4);
}
static hipError_t launch_contacts(ca_env* e) {
    hipError_t r = contact_buffer(e);
    if (r != hipSuccess) return r;
    ContactArgs c;
    c.pos_x = e->pos_x; c.pos_y = e->pos_y;
    c.ap_radius = e->ap ? e->d_ap[0] : nullptr;      // (what fill_cold puts into StepCold::ap_radius / agent_counts)
    c.agent_counts = e->ac ? e->d_counts : nullptr;
    c.obst = e->d_obst; c.tab_off = e->d_tab_off;
    c.out = e->contact;
    c.an = (unsigned)AN(e);
    c.n_obst = e->h_tab_off.empty() ? (int)e->h_obst.size() : 0; c.A = e->cfg.n_arenas; c.N = e->cfg.n_agents;
    c.apb = c.N <= CONTACT_BS ? CONTACT_BS / c.N : 0;
    c.tiles = c.N <= CONTACT_BS ? 0 : (c.N + CONTACT_BS - 1) / CONTACT_BS;
    c.radius = e->cfg.radius;
    const unsigned grid = c.apb ? (unsigned)((c.A + c.apb - 1) / c.apb) : (unsigned)((size_t)c.A * c.tiles);
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, contact_kernel, dim3(grid), dim3(CONTACT_BS), 0, e->stream, c);
    r = hipGetLastError();
    if (r == hipSuccess) e->contact_valid = true;
    return r;
}
// CA_F_CONTACT is consumed on the host: the entry points strip it, make their call, and leave the report of the state that call
// left -- one launch behind the last launch of the call (a rollout: behind its last step).  No kernel's `flags` word sees the bit.
static int contacts_behind(ca_env* e, int rc) {
    if (rc) return rc;
    HIPCHK(e, launch_contacts(e));
    return CA_OK;
}
// The tail of a call that strips CA_F_OBS and CA_F_CONTACT from its steps' flags: the observation and the contact report of the state
// its last step left, one launch each.  (The entry points above these -- the steps, the resets, ca_rollout, ca_alan_rollout and the two
// trace calls -- consume CA_F_CONTACT through contacts_behind instead, ahead of their own refusals: DESIGN.md 7q.)
static int launch_tail(ca_env* e, uint32_t flags) {
    if (flags & CA_F_OBS) HIPCHK(e, launch_obs(e));
    if (flags & CA_F_CONTACT) HIPCHK(e, launch_contacts(e));
    return CA_OK;
}

// reset_kernel + reset_arena_kernel, each timed on its own dispatch (kind 3) when the step is sampled
static hipError_t launch_reset(ca_env* e, const StepArgs& a) {
    const unsigned an = (unsigned)AN(e);
    {
        ProfScope ps(e, KIND_RESET);
        launch_k(ps, e->ac ? reset_counts_kernel : reset_kernel, dim3((an + 255) / 256), dim3(256), 0, e->stream, a);
    }
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) return r;
    {
        ProfScope ps(e, KIND_RESET);
        launch_k(ps, reset_arena_kernel, dim3((e->cfg.n_arenas + 255) / 256), dim3(256), 0, e->stream, a);
    }
    return hipGetLastError();
}

// What sim.processObstacles() (env.py:123, ALAN:209) does to the vertex table in the RVO2 library: its
// obstacle BSP tree picks, per node, the edge whose supporting line balances the remaining edges best
// (smallest (max(left, right), min(left, right)), first one wins) and cuts every edge that crosses that
// line; the cut points become new vertices at the end of the table (convex, direction of the edge they
// sit on) and are what getObstacleVertex / getNextObstacleVertexNo (env.py:307-311) and the neighbour
// query see afterwards.  The kernels scan edges brute force, so only the cuts are kept, not the tree.
// Work list instead of recursion; a node's left set is expanded before its right set, which is the
// order in which the library numbers the new vertices.
static void split_crossing_edges(std::vector<ObstDev>& tab) {
    struct Side { int left, right; };
    auto sides = [&](int split, int edge, float* a, float* b) {
        const V2 s1 = mk(tab[split].px, tab[split].py), s2 = mk(tab[tab[split].next].px, tab[tab[split].next].py);
        *a = leftOf(s1, s2, mk(tab[edge].px, tab[edge].py));
        *b = leftOf(s1, s2, mk(tab[tab[edge].next].px, tab[tab[edge].next].py));
    };
    auto worse_or_equal = [](Side x, Side y) {  // (max, min) of x >= (max, min) of y
        const int xm = x.left > x.right ? x.left : x.right, xn = x.left < x.right ? x.left : x.right;
        const int ym = y.left > y.right ? y.left : y.right, yn = y.left < y.right ? y.left : y.right;
        return xm > ym || (xm == ym && xn >= yn);
    };
    std::vector<std::vector<int>> work(1);
    for (int i = 0; i < (int)tab.size(); ++i) work[0].push_back(i);
    while (!work.empty()) {
        const std::vector<int> edges = std::move(work.back());
        work.pop_back();
        const int n = (int)edges.size();
        if (n == 0) continue;
        int pick = 0;
        Side best = {n, n};
        for (int i = 0; i < n; ++i) {
            Side c = {0, 0};
            for (int j = 0; j < n; ++j) {
                if (j == i) continue;
                float a, b;
                sides(edges[i], edges[j], &a, &b);
                if (a >= -EPS && b >= -EPS) ++c.left;
                else if (a <= EPS && b <= EPS) ++c.right;
                else { ++c.left; ++c.right; }
                if (worse_or_equal(c, best)) break;
            }
            if (!worse_or_equal(c, best)) { best = c; pick = i; }
        }
        std::vector<int> lhs, rhs;
        const int sp = edges[pick];
        const V2 s1 = mk(tab[sp].px, tab[sp].py), s2 = mk(tab[tab[sp].next].px, tab[tab[sp].next].py);
        for (int j = 0; j < n; ++j) {
            if (j == pick) continue;
            const int e1 = edges[j], e2 = tab[e1].next;
            float a, b;
            sides(sp, e1, &a, &b);
            if (a >= -EPS && b >= -EPS) { lhs.push_back(e1); continue; }
            if (a <= EPS && b <= EPS) { rhs.push_back(e1); continue; }
            const V2 p1 = mk(tab[e1].px, tab[e1].py), p2 = mk(tab[e2].px, tab[e2].py);
            const float t = det(s2 - s1, p1 - s1) / det(s2 - s1, p1 - p2);
            const V2 cut = p1 + t * (p2 - p1);
            ObstDev o;
            memset(&o, 0, sizeof o);
            o.px = cut.x; o.py = cut.y; o.ux = tab[e1].ux; o.uy = tab[e1].uy;
            o.prev = e1; o.next = e2; o.convex = 1;
            const int id = (int)tab.size();
            tab.push_back(o);
            tab[e1].next = id; tab[e2].prev = id;
            if (a > 0.0f) { lhs.push_back(e1); rhs.push_back(id); }
            else { rhs.push_back(e1); lhs.push_back(id); }
        }
        work.push_back(std::move(rhs));  // popped after the whole left subtree
        work.push_back(std::move(lhs));
    }
}

// Stream discipline: a handle's own stream is hipStreamNonBlocking, i.e. NOT ordered against the legacy
// null stream, and a fill of device memory through the blocking API is still asynchronous on the device
// (and split into a bulk and a tail command for sizes that are not a multiple of 8 bytes).  So nothing in
// this file touches the null stream: every fill and copy is the *Async form on the handle's stream, and
// an entry point that hands memory to later calls finishes with hipStreamSynchronize(e->stream).
template <class T>
static hipError_t dalloc(ca_env* e, T** p, size_t n, bool zero = true) {
    hipError_t r = hipMalloc((void**)p, n * sizeof(T));
    if (r != hipSuccess || !zero) return r;
    return hipMemsetAsync(*p, 0, n * sizeof(T), e->stream);
}
static hipError_t upload(ca_env* e, void* dst, const void* src, size_t bytes) {  // host -> device, complete on return
    hipError_t r = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream);
    return r != hipSuccess ? r : hipStreamSynchronize(e->stream);
}
static hipError_t download(ca_env* e, void* dst, const void* src, size_t bytes) {  // device -> host, complete on return
    hipError_t r = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream);
    return r != hipSuccess ? r : hipStreamSynchronize(e->stream);
}

// + the statically allocated LDS of the fused neighbour search: positions, and for >= 256 lanes the grid tables
static size_t lds_static_bytes(const ca_env* e) {
    return (size_t)e->BS * 8 +
           (e->BS >= 1024 ? (size_t)e->BS * 2 + 16 + 1024 + 1028 : (e->BS >= 256 ? (size_t)e->BS * 2 + (size_t)e->BS * 8 + 16 + 4096 + 4100 : 0)) + 64;
}

// Which solve kernel (lane-per-agent family) serves this handle.  Register-resident ORCA lines (ST = 4 obstacle slots + KMAX
// neighbour slots, LP2 / LP1 unrolled, no scratch) when K <= 10 and
//   * the obstacle-neighbour list holds at most 4 entries (the synthetic crowds: one boundary polygon), or
//   * it holds up to 16 and the world is SMALL (at most 16 edges per arena: the reference env's own doorway world, 14 edges
//     after processObstacles, env.py:117-122; "congested", ALAN:195-208) -- there an agent practically never has more than
//     four edges in range (none in 3.8e5 sampled agent-steps of either world), and the one that does is solved apart, exactly
//     (ca_step.h solve_many_obstacles), so the list capacity stays RVO2's "every edge in range" --, or
//   * the LDS line table would not fit (arenas above 256 agents with many obstacle neighbours), or the batch would not be resident
//     with it (below).
// max_obst_neighbors > 16 ALWAYS means the wide LDS line table (ST = 0, SMX = SWIDE: lists of up to 64, K + S lines per lane), whatever
// the switches say: no register lines (not even when the batch is not resident with the table -- it then runs in rounds), no
// two-lanes and no four-lanes kernel (ca_create) exist for such lists.
// Else the LDS line table (ST = 0): worlds like the two-way tube ("deadlock": 42 edges, 17 % of the agent-steps with more
// than four in range).  Called by ca_create (no table yet) and again whenever tables are installed: every variant computes
// the same bits, so a handle may change variant between steps.
static void pick_variant(ca_env* e) {
    // (CA_REG_LINES, latched by ca_create: 0 forces the LDS line table, 1 the register lines wherever they exist)
    const bool allow = e->sw.reg_lines != 0, force = e->sw.reg_lines == 1;
    e->KT = e->K <= 5 ? 5 : (e->K <= 10 ? 10 : 16);
    if (e->tiled) {   // one kernel family whatever the world: the LDS line table of a tile, lists of up to 16 (CA_CREATE_TILED_WIDE: 64)
        e->ST = 0; e->SMX = e->S > SMAX ? SWIDE : SMAX; e->pair = false;
        e->lds = tiled_lds_bytes(e->TILE, e->K, e->S);
        return;
    }
    const size_t table_per_wg = step_lds_bytes(e->BS, e->K, e->S, 0, e->KT) + lds_static_bytes(e);
    const bool table_fits = table_per_wg <= 160 * 1024;
    const bool small_world = e->max_edges <= 16;
    // ... or the batch is larger than the chip holds at once WITH the table: a 64-lane workgroup of the table kernel needs 28 KB of
    // LDS (K = 10, S = 16), five fit a CU, and from the 1281st workgroup on the launch runs in rounds of a kernel that is a third
    // occupied -- there the register lines win even in the two-way tube, where every sixth agent is solved apart (measured:
    // deadlock x 50 agents, 1280 arenas 49.6 us (table) / 64.8 us (registers) per ORCA step, 1536 arenas 81.6 / 67.7, 4096 arenas
    // 157.8 / 76.3; blocks x 20 agents, 8192 arenas 126.9 / 75.4; profiles/r04_g_many_edge_worlds.txt)
    const bool table_resident = table_fits && (long)e->grid <= (long)e->n_cus * (long)((160 * 1024) / table_per_wg);
    if (e->S > SMAX) { e->ST = 0; e->SMX = SWIDE; }
    else if (e->ap) { e->ST = 0; e->SMX = SMAX; }   // per-agent parameters: always the LDS line table, whatever the switches, the world and the batch say
    else if (allow && e->K <= 10 && e->S <= 4) { e->ST = 4; e->SMX = 4; }
    else if (allow && e->K <= 10 && (small_world || force || !table_resident)) { e->ST = 4; e->SMX = 16; }
    else { e->ST = 0; e->SMX = 16; }
    e->lds = e->ap ? step_lds_bytes_ap(e->BS, e->K, e->S) : step_lds_bytes(e->BS, e->K, e->S, e->ST, e->KT);
    // two lanes per agent for the whole step (ca_pair.h), arenas of 129 .. 512 agents on register lines: a 512-agent arena is 8
    // waves of one lane per agent on its CU -- two per SIMD, each a long dependent chain; 16 waves with half the chain each fill it
    // (CA_PAIR=0: the one-lane register-line kernel; arenas of 65 .. 128 agents, two waves, measured faster on it: ca_pair.h)
    e->pair = e->sw.pair != 0 && e->ST > 0 && e->SMX == 4 && (e->BS == 256 || e->BS == 512) && e->K > 0;
    e->lds_p = pair_lds_bytes(e->BS, e->KT);
}

// the dynamic-LDS limits of the kernels pick_variant chose -- and, for BOTH callers (ca_create, and install_tables whenever a
// world is installed and the variant may change), the check that the chosen kernel fits the CU's 160 KiB: the lane kernels by
// their dynamic part + the statically declared arrays of the neighbour search, the two-lanes kernel by what the
// compiled kernel itself reports (hipFuncGetAttributes).  *misfit = the kernel does not fit (the callers turn it into CA_ERANGE);
// the return value carries genuine HIP failures only.
static const size_t LDS_PER_CU = 160 * 1024;
static hipError_t apply_variant_attributes(ca_env* e, bool* misfit) {
    const SolveLaunch plain = solve_launch(e, false, false);
    if (e->tiled) {   // (at most 256 lanes x (32 lines x 16 B + 8 B) = 130 KiB, wide lists: ca_create_ex has checked the tile; a grid handle: its edge-grid twin too, whichever is on)
        *misfit = e->lds > LDS_PER_CU;
        if (*misfit) return hipSuccess;
        hipError_t r = allow_lds(plain);
        if (r == hipSuccess && e->tgrid) {
            SolveLaunch other = plain;
            other.fn = tiled_solve_fn(e, !e->egrid);
            r = allow_lds(other);
        }
        return r;
    }
    *misfit = !e->pair && e->lds + lds_static_bytes(e) > LDS_PER_CU;
    hipError_t r = hipSuccess;
    if (e->pair) {
        hipFuncAttributes fa;
        r = hipFuncGetAttributes(&fa, plain.fn);
        *misfit = r == hipSuccess && fa.sharedSizeBytes + plain.lds > LDS_PER_CU;
    }
    if (r != hipSuccess || *misfit) return r;
    r = allow_lds(plain);
    if (r == hipSuccess) r = allow_lds(solve_launch(e, false, true));   // (ca_rollout's one-launch form, where the handle has one)
    return r;
}

// Which form the ALAN online step takes on this handle (ca_alan_configure, and again whenever pick_variant has run: the world decides
// the solve kernel).  One launch of the four-lanes kernel (alan_fused), one launch of a lane kernel of one or two waves (alan_lane:
// the softmax terms wait in the wave's LP3 pool -- 4 + KMAX doubles per lane -- or, LDS line table, in the table itself -- 2 (K + S)
// per lane), else select -> solve -> update.
static int alan_pick(ca_env* e) {
    e->alan_fused = e->alan_lane = false;
    if (e->n_actions <= 0 || e->tiled) return CA_OK;   // (a tiled handle: select -> tiled solve -> update)
    const size_t lq = quad_lds_bytes(e->BSq, e->KT, e->SQ, e->n_actions);
    const bool on = e->sw.alan_fused != 0;   // (CA_ALAN_FUSED=0: the three-launch form everywhere)
    e->alan_fused = on && (e->quad || e->quad_roll) && lq <= 64 * 1024;
    // (obstacle lists above 16: the wide table kernel has no ALAN instantiation and no four-lanes form -- select -> solve -> update)
    // (per-agent parameters: the same -- quad and quad_roll are off there, and the AgentParams kernel has no ALAN instantiation)
    e->alan_lane = on && !e->ap && !e->quad && !e->pair && e->BS <= 128 && e->K <= 10 && e->S <= SMAX &&
                   e->n_actions <= (e->ST > 0 ? 4 + e->KT : 2 * (e->K + e->S));
    if (e->alan_fused) HIPCHK(e, allow_lds(solve_launch(e, true, true)));   // (the ALAN rollout; on a quad handle the ALAN step too)
    if (e->alan_lane) HIPCHK(e, allow_lds(solve_launch(e, true, false)));
    return CA_OK;
}

extern "C" {

const char* ca_last_error(const ca_env* env) { return env ? env->err.c_str() : g_create_err.c_str(); }

int ca_create(const ca_config* cfg, int device, void* stream, ca_env** out) { return ca_create_ex(cfg, 0u, device, stream, out); }

int ca_create_ex(const ca_config* cfg, uint32_t create_flags, int device, void* stream, ca_env** out) {
    if (!cfg || !out) return fail(nullptr, CA_EINVAL, "ca_create: null argument");
    *out = nullptr;
    if (create_flags & ~(CA_CREATE_TILED | CA_CREATE_TILED_GRID | CA_CREATE_TILED_PARAMS | CA_CREATE_TILED_WIDE))
        return fail(nullptr, CA_EINVAL, "ca_create_ex: unknown create_flags 0x%x", create_flags);
    const bool tiled = (create_flags & CA_CREATE_TILED) != 0;
    const bool tgrid = (create_flags & CA_CREATE_TILED_GRID) != 0;
    const bool tparams = (create_flags & CA_CREATE_TILED_PARAMS) != 0;
    const bool twide = (create_flags & CA_CREATE_TILED_WIDE) != 0;
    if (twide && !tiled)
        return fail(nullptr, CA_EINVAL, "ca_create_ex: CA_CREATE_TILED_WIDE (create_flags 0x%x) without CA_CREATE_TILED: it selects the tiled "
                    "path's wide-obstacle-list kernels (an ordinary handle takes max_obst_neighbors up to %d as it is)", create_flags, CA_MAX_OBST_NEIGHBORS);
    if (twide && tparams)
        return fail(nullptr, CA_EINVAL, "ca_create_ex: CA_CREATE_TILED_WIDE together with CA_CREATE_TILED_PARAMS (create_flags 0x%x): per-agent "
                    "parameters go with obstacle lists of up to %d, as on ordinary handles", create_flags, SMAX);
    if (tparams && !tiled)
        return fail(nullptr, CA_EINVAL, "ca_create_ex: CA_CREATE_TILED_PARAMS (create_flags 0x%x) without CA_CREATE_TILED: it selects the tiled "
                    "path's per-agent-parameter kernels (an ordinary handle takes ca_set_agent_params as it is)", create_flags);
    if (tgrid && !tiled)
        return fail(nullptr, CA_EINVAL, "ca_create_ex: CA_CREATE_TILED_GRID (create_flags 0x%x) without CA_CREATE_TILED: the uniform grid "
                    "is the tiled path's neighbour search", create_flags);
    const int max_agents = tiled ? CA_MAX_AGENTS_LARGE : CA_MAX_AGENTS;
    if (cfg->n_arenas <= 0 || cfg->n_agents <= 0 || cfg->n_agents > max_agents)
        return fail(nullptr, CA_ERANGE, "ca_create: n_arenas=%d n_agents=%d out of range (agents 1..%d)",
                    cfg->n_arenas, cfg->n_agents, max_agents);
    if (tiled && !twide && cfg->max_obst_neighbors > SMAX)
        return fail(nullptr, CA_ERANGE, "ca_create_ex: max_obst_neighbors=%d: wide obstacle lists (above %d) have no tiled form",
                    cfg->max_obst_neighbors, SMAX);
    if (cfg->max_neighbors < 0 || cfg->max_neighbors > CA_MAX_NEIGHBORS)
        return fail(nullptr, CA_ERANGE, "ca_create: max_neighbors=%d out of range 0..%d", cfg->max_neighbors,
                    CA_MAX_NEIGHBORS);
    if (cfg->max_obst_neighbors < 1 || cfg->max_obst_neighbors > CA_MAX_OBST_NEIGHBORS)
        return fail(nullptr, CA_ERANGE, "ca_create: max_obst_neighbors=%d out of range 1..%d",
                    cfg->max_obst_neighbors, CA_MAX_OBST_NEIGHBORS);
    if (cfg->done_mode < 0 || cfg->done_mode > 2) return fail(nullptr, CA_EINVAL, "ca_create: bad done_mode");
    {   // the supported magnitudes (include/ca_env.h "Units and magnitudes"): the kernels' division and square root run without
        // their range-scaling instructions (ca_math.h) -- exact for worlds of O(1) units, not for metres-as-nanometres
        const struct { const char* name; float v, lo, hi; } rng[] = {
            {"time_step", cfg->time_step, CA_MIN_TIME_STEP, CA_MAX_TIME_STEP}, {"neighbor_dist", cfg->neighbor_dist, CA_MIN_LENGTH, CA_MAX_LENGTH},
            {"time_horizon", cfg->time_horizon, CA_MIN_LENGTH, CA_MAX_LENGTH}, {"time_horizon_obst", cfg->time_horizon_obst, CA_MIN_LENGTH, CA_MAX_LENGTH},
            {"radius", cfg->radius, CA_MIN_LENGTH, CA_MAX_LENGTH}, {"max_speed", cfg->max_speed, CA_MIN_LENGTH, CA_MAX_LENGTH}};
        for (const auto& q : rng)
            if (!(q.v >= q.lo && q.v <= q.hi))   // (also false for NaN)
                return fail(nullptr, CA_ERANGE, "ca_create: %s=%g outside the supported range [%g, %g]", q.name, (double)q.v, (double)q.lo, (double)q.hi);
        const float box[] = {cfg->spawn_x0, cfg->spawn_x1, cfg->spawn_y0, cfg->spawn_y1, cfg->goal_x0, cfg->goal_x1, cfg->goal_y0, cfg->goal_y1,
                             cfg->done_x_thresh};
        for (float v : box)
            if (!(fabsf(v) <= CA_MAX_COORD)) return fail(nullptr, CA_ERANGE, "ca_create: a spawn / goal box coordinate (%g) is beyond %g or not a number", (double)v, (double)CA_MAX_COORD);
    }
    if ((size_t)cfg->n_arenas * cfg->n_agents > (size_t)1 << 30)
        return fail(nullptr, CA_ERANGE, "ca_create: more than 2^30 agents on one handle");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, CA_ENODEV, "ca_create: no HIP device (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(nullptr, CA_ENODEV, "ca_create: device %d of %d", device, ndev);
    ca_env* e = new ca_env();
    e->cfg = *cfg;
    e->device = device;
    hipError_t r = hipSetDevice(device);
    if (r == hipSuccess) {
        if (stream) e->stream = (hipStream_t)stream;
        else { r = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking); e->own_stream = true; }
    }
    {   // the diagnostic switches, once
        auto digit = [](const char* name) { const char* v = getenv(name); return (v && v[0] >= '0' && v[0] <= '9') ? v[0] - '0' : -1; };
        e->sw.reg_lines = digit("CA_REG_LINES"); e->sw.pair = digit("CA_PAIR"); e->sw.alan_fused = digit("CA_ALAN_FUSED");
        e->sw.nbr_seed = digit("CA_NBR_SEED"); e->sw.lp3_pairs = digit("CA_LP3_PAIRS");
        const char* nb = getenv("CA_NAV_BLOCK");   // 256 / 1024 forces the field kernel's block (tools/nav_cost.py measures both)
        e->sw.nav_block = nb ? atoi(nb) : 0;
    }
    e->tiled = tiled;
    e->twide = twide;
    if (tiled) {   // CA_TILE = 64 | 128 | 256 (diagnostic switch, tools/tiled_cost.py): the tile of the tiled path; anything else: 128
        const char* v = getenv("CA_TILE");
        const int want = v ? atoi(v) : 0;
        e->TILE = (want == 64 || want == 256) ? want : 128;
        // obstacle lists above 16 (CA_CREATE_TILED_WIDE): 64 unless CA_TILE names one of the three.  The line table bounds the
        // residency by LDS per lane whatever the tile, and the smaller tile wastes less of a CU to rounding; a tile
        // whose table does not fit a CU is refused here -- nothing is launched above the limit
        if (cfg->max_obst_neighbors > SMAX) {
            e->TILE = (want == 64 || want == 128 || want == 256) ? want : 64;
            const size_t need = tiled_lds_bytes(e->TILE, cfg->max_neighbors, cfg->max_obst_neighbors);
            if (need > LDS_PER_CU) {
                fail(nullptr, CA_ERANGE, "ca_create_ex: the tiled solve kernel for a tile of %d agents (CA_TILE), max_neighbors=%d, max_obst_neighbors=%d "
                     "does not fit the 160 KiB of LDS of a CU (%zu B: max_neighbors + max_obst_neighbors lines per lane)", e->TILE,
                     cfg->max_neighbors, cfg->max_obst_neighbors, need);
                if (e->own_stream && e->stream) hipStreamDestroy(e->stream);
                delete e;
                return CA_ERANGE;
            }
        }
        e->tiles = (cfg->n_agents + e->TILE - 1) / e->TILE;
    }
    e->tgrid = tgrid;
    e->tparams = tparams;
    if (tgrid) {   // the cell table: g x g cells, g the power of two with n_agents / 2 <= g^2 (about one agent per cell where the arena
                   // is as wide as the table), 8 <= g <= 128: the scan launch sums 128 x 128 cells in one workgroup.
                   // CA_TILED_CELLS = 8 | 16 | 32 | 64 | 128 (diagnostic switch, tests): that side; anything else: the rule
        int g = 8;
        while (g < 128 && 2 * g * g < cfg->n_agents) g <<= 1;
        const char* v = getenv("CA_TILED_CELLS");
        const int want = v ? atoi(v) : 0;
        if (want == 8 || want == 16 || want == 32 || want == 64 || want == 128) g = want;
        e->tgx = e->tgy = g;
        e->tcs = 0.5f * cfg->neighbor_dist;
        e->tics = 1.0f / e->tcs;
    }
    // launch geometry: P lanes per arena (power of two >= N), one or more whole arenas per block
    int P = 1, logP = 0;
    while (P < cfg->n_agents) { P <<= 1; ++logP; }
    e->P = P; e->logP = logP;
    e->BS = P > 64 ? P : 64;
    e->LS = P; e->apb = e->BS / P; e->linv = 65536 / P; e->dense = 0;   // (P a power of two: exact)
    e->grid = (cfg->n_arenas + e->apb - 1) / e->apb;
    if (tiled) {   // a workgroup is a tile: the lane -> (arena, agent) fields of StepArgs are not read by the tiled kernels
        if ((size_t)cfg->n_arenas * e->tiles > (size_t)0x7FFFFFFF) {
            fail(nullptr, CA_ERANGE, "ca_create_ex: n_arenas=%d x %d tiles per arena is more workgroups than a launch holds", cfg->n_arenas, e->tiles);
            if (e->own_stream && e->stream) hipStreamDestroy(e->stream);
            delete e;
            return CA_ERANGE;
        }
        e->BS = e->TILE; e->LS = e->TILE; e->apb = 1; e->linv = 65536 / e->TILE;
        e->grid = cfg->n_arenas * e->tiles;
    }
    {
        const char* v = getenv("CA_OBS_DENSE");  // diagnostic switch: 0 = one arena per observation workgroup
        e->obs_dense_on = !tiled && cfg->n_agents < 16 && !(v && v[0] == '0');
    }
    {   // arenas within one wave whose N is no power of two: N lanes each, back to back, where that packs more arenas into the
        // wave than P lanes each (the reference env's own 10-agent arenas: six per wave instead of four)
        const char* v = getenv("CA_DENSE");  // diagnostic switch: 0 = P lanes per arena
        const int N = cfg->n_agents;
        if (!tiled && !(v && v[0] == '0') && e->BS == 64 && P < 64 && 64 / N > 64 / P) {
            const int linv = (65536 + N - 1) / N;
            bool exact = true;
            for (int t = 0; t < 64; ++t) exact = exact && ((t * linv) >> 16) == t / N;
            if (exact) {
                e->LS = N; e->apb = 64 / N; e->linv = linv; e->dense = 1;
                e->grid = (cfg->n_arenas + e->apb - 1) / e->apb;
            }
        }
    }
    e->K = cfg->max_neighbors;
    e->S = cfg->max_obst_neighbors;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) e->n_cus = cus;
    }
    pick_variant(e);
    {   // four lanes per agent (ca_quad.h) where one lane per agent would leave SIMDs without a wave: fewer than 1024
        // waves.  Measured crossover (profiles/r03_d_lane_vs_quad_by_batch_size.txt): 16-agent arenas -- quad ahead up to
        // 2048 arenas (512 lane-waves), behind from 4096 (1024); 64-agent arenas -- ahead up to 512 arenas, level at 1024.
        const char* v = getenv("CA_QUAD");  // 0 / 1 forces the choice (tests run the parity suite both ways)
        e->SQ = e->S <= 4 ? 4 : 16;
        // (register budget: a 1024-lane workgroup caps the kernel at 128 VGPRs, a 512-lane one at 256 -- the variant with 16
        // obstacle neighbours and K = 10 needs all 256 already at 256 lanes)
        // (... and it holds obstacle lists of 4 or 16: a handle with max_obst_neighbors > 16 never takes it, CA_QUAD=1 or not)
        const bool fits = !tiled && e->S <= SMAX && e->K <= 10 && 4 * P <= ((e->SQ == 16 && e->KT == 10) ? 256 : 512);
        // (counted at P lanes per arena, the layout the crossover was measured with, whatever the packing is now)
        const long lane_waves = tiled ? 0 : (long)((cfg->n_arenas + e->BS / P - 1) / (e->BS / P)) * (e->BS / 64);   // (tiled: BS is a tile, fits is false)
        e->quad = fits && (v ? v[0] == '1' : lane_waves < 1024);
        e->quad_roll = fits && (v ? v[0] == '1' : lane_waves <= 1024);  // T steps per launch: ahead at 1024 lane-waves too
        e->BSq = 4 * P > 64 ? 4 * P : 64;
        const int apbq = (e->BSq / 4) / P;
        e->grid_q = (cfg->n_arenas + apbq - 1) / apbq;
        e->lds_q = quad_lds_bytes(e->BSq, e->KT, e->SQ);
        e->quad_cfg = e->quad; e->quad_roll_cfg = e->quad_roll;
    }
    if (!tiled && e->S > SMAX && (e->lds + lds_static_bytes(e) > LDS_PER_CU || e->BS > 128 || obs_block_threads(cfg->n_agents) != 256)) {
        // obstacle lists above 16 live in the LDS line table, K + S lines per lane: 64 lanes with K <= 16, 128 lanes with K <= 10 at S = 64
        if (e->lds + lds_static_bytes(e) > LDS_PER_CU)
            fail(nullptr, CA_ERANGE, "ca_create: the solve kernel for n_agents=%d, max_neighbors=%d, max_obst_neighbors=%d does not fit the "
                 "160 KiB of LDS of a CU (%zu B: obstacle lists above %d take the LDS line table, max_neighbors + max_obst_neighbors lines "
                 "per lane)", cfg->n_agents, e->K, e->S, e->lds + lds_static_bytes(e), SMAX);
        else
            fail(nullptr, CA_ERANGE, "ca_create: max_obst_neighbors=%d: obstacle lists above %d are built for arenas of at most 128 agents "
                 "(n_agents=%d)", e->S, SMAX, cfg->n_agents);
        if (e->own_stream && e->stream) hipStreamDestroy(e->stream);
        delete e;
        return CA_ERANGE;
    }
    if (!tiled && !e->pair && e->lds + lds_static_bytes(e) > LDS_PER_CU) {
        fail(nullptr, CA_ERANGE, "ca_create: the solve kernel would need %zu B of LDS (> 160 KiB) for n_agents=%d, "
             "max_neighbors=%d, max_obst_neighbors=%d: arenas above 256 agents need max_neighbors <= 10 "
             "(register-line variant)", e->lds + lds_static_bytes(e), cfg->n_agents, e->K, e->S);
        if (e->own_stream && e->stream) hipStreamDestroy(e->stream);
        delete e;
        return CA_ERANGE;
    }
    host_tables(e);
    const size_t an = AN(e), A = cfg->n_arenas;
    float** f32s[] = {&e->pos_x, &e->pos_y, &e->vel_x, &e->vel_y, &e->pref_x, &e->pref_y,
                      &e->tmp_x, &e->tmp_y, &e->orient_x, &e->orient_y};
    for (auto p : f32s) if (r == hipSuccess) r = dalloc(e, p, an);
    double** f64s[] = {&e->goal_x, &e->goal_y, &e->goal2_x, &e->goal2_y};
    for (auto p : f64s) if (r == hipSuccess) r = dalloc(e, p, an);
    int** i32s[] = {&e->agent_done, &e->arrive_step, &e->regoal_count};
    for (auto p : i32s) if (r == hipSuccess) r = dalloc(e, p, an);
    if (tiled) {
        if (r == hipSuccess) r = dalloc(e, &e->nv_x, an);
        if (r == hipSuccess) r = dalloc(e, &e->nv_y, an);
        if (r == hipSuccess) r = dalloc(e, &e->tscr, A * (size_t)TS_STRIDE);
    }
    if (tgrid) {   // (all zero-filled: the counts must be, and the sorted arrays hold ids below n_agents from the first step on)
        const size_t cells = (size_t)e->tgx * e->tgy;
        if (r == hipSuccess) r = dalloc(e, &e->tg_count, A * cells);
        if (r == hipSuccess) r = dalloc(e, &e->tg_start, A * (cells + 1));
        if (r == hipSuccess) r = dalloc(e, &e->tg_key, an);
        if (r == hipSuccess) r = dalloc(e, &e->tg_sx, an);
        if (r == hipSuccess) r = dalloc(e, &e->tg_sy, an);
        if (r == hipSuccess) r = dalloc(e, &e->tg_sidx, an);
    }
    e->nidx16 = (tiled || CA_NBW16(e->BS)) ? 1 : 0;  // u8 indices address 256 agents (BS = max(64, pow2 >= N): the kernels' compile-time test)
    if (r == hipSuccess) r = dalloc(e, &e->counts, an);
    if (r == hipSuccess) r = dalloc(e, reinterpret_cast<unsigned char**>(&e->nb_idx),
                                    an * (size_t)(e->K > 0 ? e->K : 1) * (e->nidx16 ? 2 : 1));
    if (r == hipSuccess) r = dalloc(e, &e->obst_idx, an * (size_t)e->S);
    if (r == hipSuccess) r = dalloc(e, &e->slab, an * CA_OBS_DIM + an + 2 * A);   // observation | reward | arena_done | step_count
    if (r == hipSuccess) {
        e->obs = e->slab; e->reward = e->slab + an * CA_OBS_DIM;
        e->arena_done = reinterpret_cast<int*>(e->reward + an); e->step_count = e->arena_done + A;
    }
    if (r == hipSuccess) r = dalloc(e, &e->episode, A);
    if (r == hipSuccess) r = dalloc(e, &e->arena_stats, A * ST_STRIDE);
    if (r == hipSuccess) r = dalloc(e, &e->arena_steps, A);
    if (r == hipSuccess) r = dalloc(e, &e->d_obst, (size_t)1);
#ifdef CA_STAMPS
    if (r == hipSuccess) r = dalloc(e, &e->dbg, (size_t)std::max(e->grid * (2 * e->BS / 64), e->grid_q * (e->BSq / 64)) * 16);
    if (r == hipSuccess) r = dalloc(e, &e->dbg_obs, (size_t)cfg->n_arenas * ((cfg->n_agents + 15) / 16 + 16) * 4 * 16);
#endif
    bool lds_misfit = false;
    if (r == hipSuccess) r = apply_variant_attributes(e, &lds_misfit);
    if (r == hipSuccess) r = allow_obs_lds(e);
    if (r == hipSuccess) {
        r = hipHostMalloc((void**)&e->ovf_host, sizeof(unsigned long long), hipHostMallocDefault);
        if (r == hipSuccess) *e->ovf_host = 0ull;
    }
    if (r == hipSuccess) r = dalloc(e, &e->d_trace, (size_t)1);
    if (r == hipSuccess) r = dalloc(e, &e->d_actseq, (size_t)1);
    if (r == hipSuccess) r = hipMalloc((void**)&e->d_cold, sizeof(StepCold));
    if (r == hipSuccess) {
        StepCold hc;
        fill_cold(e, hc);
        r = upload(e, e->d_cold, &hc, sizeof hc);
    }
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);  // the zero fills are done before the handle is handed out
    if (r == hipSuccess && lds_misfit) {
        fail(nullptr, CA_ERANGE, "ca_create: the solve kernel for n_agents=%d, max_neighbors=%d, max_obst_neighbors=%d does not fit the "
             "160 KiB of LDS of a CU", cfg->n_agents, e->K, e->S);
        ca_destroy(e);
        return CA_ERANGE;
    }
    if (r != hipSuccess) {
        fail(nullptr, CA_EHIP, "ca_create: %s", hipGetErrorString(r));
        ca_destroy(e);
        return CA_EHIP;
    }
    *out = e;
    return CA_OK;
}

int ca_destroy(ca_env* e) {
    if (!e) return CA_OK;
    hipSetDevice(e->device);
    if (e->stream) hipStreamSynchronize(e->stream);
    void* bufs[] = {e->pos_x, e->pos_y, e->vel_x, e->vel_y, e->pref_x, e->pref_y, e->goal_x, e->goal_y,
                    e->goal2_x, e->goal2_y, e->slab, e->tmp_x, e->tmp_y, e->orient_x, e->orient_y,
                    e->agent_done, e->arrive_step,
                    e->regoal_count, e->counts, e->nb_idx, e->obst_idx, e->cvt_buf, e->d_tab_off, e->d_cold, e->d_trace, e->d_actseq, e->actseq_words, e->d_order,
                    e->pol.d_wp, e->pol.d_bp, e->pol.act, e->pol.d_set, e->heads.d_wp, e->heads.d_bp, e->heads.rr, e->heads.words, e->nav.d_dist, e->nav.d_next, e->nav.d_class, e->nav_keep, e->nav_advance, e->rew.d_w, e->rew.saved, e->rew.advance, e->rew.parts,
                    e->episode, e->arena_stats, e->arena_steps, e->d_obst, e->dbg, e->dbg_obs,
                    e->alan_w, e->alan_t, e->alan_dirs, e->alan_u, e->alan_action, e->d_alan, e->mask_buf,
                    e->d_act_tab, e->d_act_n, e->d_ap[0], e->d_ap[1], e->d_ap[2], e->d_ap[3], e->d_ap_oct, e->d_counts, e->d_as_nd, e->d_as_k,
                    e->nv_x, e->nv_y, e->tscr, e->tg_count, e->tg_start, e->tg_key, e->tg_sx, e->tg_sy, e->tg_sidx,
                    e->eg.d_desc, e->eg.d_cells, e->eg.d_entries, e->contact, e->fork_scratch.base, e->fork_scratch.alan, e->fork_idx};
    for (void* b : bufs) if (b) hipFree(b);
    for (ca_snapshot* sn : e->snapshots) {   // (a snapshot the caller still holds dangles from here on, like the handle itself)
        if (sn->set.base) hipFree(sn->set.base);
        if (sn->set.alan) hipFree(sn->set.alan);
        delete sn;
    }
    for (const auto& h : e->host_allocs) hipHostFree(h.first);
    if (e->ovf_host) hipHostFree(e->ovf_host);
    for (const ca_env::Span& sp : e->spans) { hipEventDestroy(sp.t0); hipEventDestroy(sp.t1); }
    for (hipEvent_t ev : e->free_events) hipEventDestroy(ev);
    if (e->own_stream && e->stream) hipStreamDestroy(e->stream);
    delete e;
    return CA_OK;
}

int ca_set_stream(ca_env* e, void* stream) {
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->own_stream && e->stream) HIPCHK(e, hipStreamDestroy(e->stream));
    e->stream = (hipStream_t)stream;
    e->own_stream = false;
    return CA_OK;
}

// addObstacle for every polygon + processObstacles (env.py:118-123, 143-149): one processed edge table
static int build_table(ca_env* e, const float* verts_xy, const int32_t* poly_sizes, int n_poly, std::vector<ObstDev>& tab) {
    size_t off = 0;
    for (int pi = 0; pi < n_poly; ++pi) {
        const int n = poly_sizes[pi];
        if (n < 2) return fail(e, CA_EINVAL, "ca_set_obstacles: polygon %d has %d vertices (need >= 2)", pi, n);
        const int base = (int)tab.size();
        for (int i = 0; i < n; ++i) {  // SURVEY App. A.2 "Obstacle vertex attributes at addObstacle"
            const int in = (i == n - 1) ? 0 : i + 1, ip = (i == 0) ? n - 1 : i - 1;
            const V2 pt = mk(verts_xy[2 * (off + i)], verts_xy[2 * (off + i) + 1]);
            const V2 pn = mk(verts_xy[2 * (off + in)], verts_xy[2 * (off + in) + 1]);
            const V2 pp = mk(verts_xy[2 * (off + ip)], verts_xy[2 * (off + ip) + 1]);
            if (!(fabsf(pt.x) <= CA_MAX_COORD && fabsf(pt.y) <= CA_MAX_COORD))   // (also false for NaN)
                return fail(e, CA_ERANGE, "ca_set_obstacles: polygon %d vertex %d = (%g, %g) is beyond %g or not a number", pi, i,
                            (double)pt.x, (double)pt.y, (double)CA_MAX_COORD);
            if (pn.x == pt.x && pn.y == pt.y)
                return fail(e, CA_EINVAL, "ca_set_obstacles: polygon %d has an edge of length zero (vertex %d twice)", pi, i);
            if (absSq(pn - pt) < CA_MIN_EDGE * CA_MIN_EDGE)
                return fail(e, CA_ERANGE, "ca_set_obstacles: polygon %d edge %d is shorter than %g", pi, i, (double)CA_MIN_EDGE);
            const V2 u = normalize(pn - pt);
            ObstDev o;
            memset(&o, 0, sizeof o);
            o.px = pt.x; o.py = pt.y; o.ux = u.x; o.uy = u.y;
            o.next = base + in; o.prev = base + ip;
            o.convex = (n == 2) ? 1 : (leftOf(pp, pt, pn) >= 0.0f ? 1 : 0);
            tab.push_back(o);
        }
        off += n;
    }
    split_crossing_edges(tab);  // processObstacles (env.py:123)
    for (ObstDev& o : tab) {  // denormalise: each edge record also carries its two neighbours
        const ObstDev& nx = tab[o.next];
        const ObstDev& pv = tab[o.prev];
        o.qx = nx.px; o.qy = nx.py; o.qux = nx.ux; o.quy = nx.uy; o.qconvex = nx.convex;
        o.pux = pv.ux; o.puy = pv.uy;
    }
    return CA_OK;
}

// the obstacle-neighbour lists of the last step name edges of the OLD table(s): drop them (high byte of `counts`)
__global__ void clear_obst_counts_kernel(unsigned short* counts, size_t n) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) counts[q] &= 0x00FFu;
}

// ---- the static edge grids (ca_tiled_edge_grid; ca_edge_grid_host.h builds one table's grid, ca_tiled.h walks it) ----------------------
static void free_edge_grids(ca_env::EdgeGrids& g) {
    if (g.d_desc) hipFree(g.d_desc);
    if (g.d_cells) hipFree(g.d_cells);
    if (g.d_entries) hipFree(g.d_entries);
    g = ca_env::EdgeGrids();
}
// the obstacle range the grids are built for -- it sets the cell size and the margin of an edge's bounding box: the kernels' expression
// on the handle's constants, or, with per-agent parameters `ap` (radius | max_speed | time_horizon | time_horizon_obst, as
// ca_env::h_ap), the largest tho_i * ms_i + r_i over all agents, evaluated in fp32 as the kernels evaluate it.  The corner rule of
// the walk does not depend on the cell size: an agent of a smaller range walks fewer cells of the same table.
static float edge_grid_range(const ca_env* e, const std::vector<float>* ap) {
    if (!ap) return e->cfg.time_horizon_obst * e->cfg.max_speed + e->cfg.radius;
    float range = 0.0f;
    for (size_t q = 0; q < ap[0].size(); ++q) {
        const float v = ap[3][q] * ap[1][q] + ap[0][q];
        range = v > range ? v : range;
    }
    return range;
}
static const std::vector<float>* agent_params_of(const ca_env* e) { return e->ap_user ? e->h_ap : nullptr; }
// the grids of the tables `all` / `offs` (install_tables' arguments) for obstacle range `range` into `out`, uploaded; a failure leaves
// `out` empty and the handle as it was.  `who`: the call the message names.
static int make_edge_grids(ca_env* e, const std::vector<ObstDev>& all, const std::vector<int>& offs, float range, ca_env::EdgeGrids& out, const char* who) {
    const int tables = offs.empty() ? 1 : (int)offs.size() - 1;
    std::vector<uint32_t> cells, entries, cs, en;
    std::vector<float> pq;
    out.desc.clear();
    for (int k = 0; k < tables; ++k) {
        const int t0 = offs.empty() ? 0 : offs[k], n = offs.empty() ? (int)all.size() : offs[k + 1] - offs[k];
        pq.resize((size_t)4 * n);
        for (int i = 0; i < n; ++i) {
            const ObstDev& o = all[(size_t)t0 + i];
            pq[4 * i] = o.px; pq[4 * i + 1] = o.py; pq[4 * i + 2] = o.qx; pq[4 * i + 3] = o.qy;
        }
        ca_edge_grid::Desc d;
        const ca_edge_grid::Result r = ca_edge_grid::build(pq.data(), n, range, d, &cs, &en);
        if (r == ca_edge_grid::TOO_MANY_EDGES)
            return fail(e, CA_ERANGE, "%s: the edge grid holds at most %d edges per table, table %d has %d; the handle stays as "
                        "it was", who, (int)ca_edge_grid::MAX_EDGES, k, n);
        if (r == ca_edge_grid::TOO_MANY_ENTRIES)
            return fail(e, CA_ERANGE, "%s: the edge grid of table %d would hold %d%s entries (at most %d): long walls cover many cells -- "
                        "subdivide the walls; the handle stays as it was", who, k, (int)d.n_entries,
                        d.n_entries == 0x7FFFFFFF ? "+" : "", (int)ca_edge_grid::MAX_ENTRIES);
        if (r != ca_edge_grid::OK)
            return fail(e, CA_ERANGE, "%s: obstacle range %g (time_horizon_obst * max_speed + radius) is not a positive number", who, (double)range);
        if (cells.size() + cs.size() > 0x7FFFFFFFull || entries.size() + en.size() > 0x7FFFFFFFull)
            return fail(e, CA_ERANGE, "%s: the edge grids of %d tables are too large; subdivide the walls", who, tables);
        EdgeGridDev g;
        g.x0 = d.x0; g.y0 = d.y0; g.ics_x = d.ics_x; g.ics_y = d.ics_y; g.gx = d.gx; g.gy = d.gy;
        g.n_entries = (unsigned)d.n_entries; g.cells_off = (unsigned)cells.size(); g.entries_off = (unsigned)entries.size(); g.pad = 0u;
        out.desc.push_back(g);
        cells.insert(cells.end(), cs.begin(), cs.end());
        entries.insert(entries.end(), en.begin(), en.end());
    }
    hipError_t r = hipMalloc((void**)&out.d_desc, out.desc.size() * sizeof(EdgeGridDev));
    if (r == hipSuccess) r = upload(e, out.d_desc, out.desc.data(), out.desc.size() * sizeof(EdgeGridDev));
    if (r == hipSuccess) r = hipMalloc((void**)&out.d_cells, cells.size() * sizeof(uint32_t));
    if (r == hipSuccess) r = upload(e, out.d_cells, cells.data(), cells.size() * sizeof(uint32_t));
    if (r == hipSuccess) r = hipMalloc((void**)&out.d_entries, (entries.size() + 1) * sizeof(uint32_t));
    if (r == hipSuccess && !entries.empty()) r = upload(e, out.d_entries, entries.data(), entries.size() * sizeof(uint32_t));
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    if (r != hipSuccess) {
        free_edge_grids(out);
        return fail(e, CA_EHIP, "%s: %s (the edge grids; the handle is as it was)", who, hipGetErrorString(r));
    }
    return CA_OK;
}

// drops the navigation (ca_nav_clear; install_tables: fields of the old tables would be stale).  The stream is idle.
static void nav_release(ca_env* e) {
    if (e->nav.d_dist) hipFree(e->nav.d_dist);
    if (e->nav.d_next) hipFree(e->nav.d_next);
    if (e->nav.d_class) hipFree(e->nav.d_class);
    e->nav = ca_env::Nav();
}

// installs the table(s): `all` = every table concatenated, `offs` empty (one table for all arenas) or [A + 1].
// The new tables are allocated and uploaded first and swapped in only when everything succeeded: a failure leaves the
// handle as it was.  The obstacle-neighbour lists left by the last step refer to the old tables, so their counts are
// cleared (an observation or reset before the next step then sees no obstacle segments instead of stale edge ids).
static int install_tables(ca_env* e, std::vector<ObstDev>& all, std::vector<int>& offs) {
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    ca_env::EdgeGrids n_eg;   // (the static edge grid is on: the new tables' grids first -- a world it refuses is not installed)
    if (e->egrid) {
        const int rc = make_edge_grids(e, all, offs, edge_grid_range(e, agent_params_of(e)), n_eg, "ca_set_obstacles");
        if (rc) return rc;
    }
    ObstDev* n_obst = nullptr;
    int* n_off = nullptr;
    hipError_t r = hipMalloc((void**)&n_obst, (all.size() + 1) * sizeof(ObstDev));
    if (r == hipSuccess && !all.empty()) r = upload(e, n_obst, all.data(), all.size() * sizeof(ObstDev));
    if (r == hipSuccess && !offs.empty()) {
        r = hipMalloc((void**)&n_off, offs.size() * sizeof(int));
        if (r == hipSuccess) r = upload(e, n_off, offs.data(), offs.size() * sizeof(int));
    }
    if (r == hipSuccess) {
        const size_t an = AN(e);
        hipLaunchKernelGGL(clear_obst_counts_kernel, dim3((unsigned)((an + 255) / 256)), dim3(256), 0, e->stream, e->counts, an);
        r = hipGetLastError();
        if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    }
    if (r != hipSuccess) {
        if (n_obst) hipFree(n_obst);
        if (n_off) hipFree(n_off);
        free_edge_grids(n_eg);
        return fail(e, CA_EHIP, "ca_set_obstacles: %s (the previous tables stay installed)", hipGetErrorString(r));
    }
    // the solve-kernel variant depends on the size of the world (pick_variant): the variant the NEW world selects is chosen and
    // checked against the CU's LDS while the old tables are still installed; a world whose kernel does not fit leaves the
    // handle exactly as it was (tables, variant, ALAN form)
    int me = 0;
    if (offs.empty()) me = (int)all.size();
    else for (size_t a = 0; a + 1 < offs.size(); ++a) me = std::max(me, offs[a + 1] - offs[a]);
    struct { int ST, SMX, KT, max_edges; bool pair; size_t lds, lds_p; } old_v = {e->ST, e->SMX, e->KT, e->max_edges, e->pair, e->lds, e->lds_p};
    e->max_edges = me;
    pick_variant(e);
    bool misfit = false;
    const hipError_t ra = apply_variant_attributes(e, &misfit);
    if (misfit || ra != hipSuccess) {
        e->ST = old_v.ST; e->SMX = old_v.SMX; e->KT = old_v.KT; e->max_edges = old_v.max_edges; e->pair = old_v.pair;
        e->lds = old_v.lds; e->lds_p = old_v.lds_p;
        bool dummy = false;
        (void)apply_variant_attributes(e, &dummy);   // (the previous variant's limits again: the attribute calls are idempotent)
        hipFree(n_obst);
        if (n_off) hipFree(n_off);
        free_edge_grids(n_eg);
        if (misfit)
            return fail(e, CA_ERANGE, "ca_set_obstacles: the solve kernel this world selects does not fit the 160 KiB of LDS of a CU "
                        "(n_agents=%d, max_neighbors=%d, max_obst_neighbors=%d); the previous tables stay installed", e->cfg.n_agents, e->K, e->S);
        return fail(e, CA_EHIP, "ca_set_obstacles: %s (the previous tables stay installed)", hipGetErrorString(ra));
    }
    if (e->d_obst) hipFree(e->d_obst);
    if (e->d_tab_off) hipFree(e->d_tab_off);
    e->d_obst = n_obst;
    e->d_tab_off = n_off;
    e->h_obst.swap(all);
    e->h_tab_off.swap(offs);
    if (e->egrid) {
        free_edge_grids(e->eg);
        e->eg = n_eg;
    }
    nav_release(e);   // (the fields were relaxed round the old tables' edges)
    return alan_pick(e);   // (the form of the ALAN step follows the solve kernel)
}

int ca_set_obstacles(ca_env* e, const float* verts_xy, const int32_t* poly_sizes, int32_t n_poly) {
    if (!e || n_poly < 0 || (n_poly > 0 && (!verts_xy || !poly_sizes))) return fail(e, CA_EINVAL, "ca_set_obstacles: bad argument");
    std::vector<ObstDev> tab;
    const int rc = build_table(e, verts_xy, poly_sizes, n_poly, tab);
    if (rc) return rc;
    if (tab.size() > 65536) return fail(e, CA_ERANGE, "ca_set_obstacles: %zu edges (at most 65536)", tab.size());
    std::vector<int> none;
    return install_tables(e, tab, none);
}

int ca_set_obstacles_per_arena(ca_env* e, const float* verts_xy, const int32_t* poly_sizes, const int32_t* n_poly) {
    if (!e || !n_poly) return fail(e, CA_EINVAL, "ca_set_obstacles_per_arena: null argument");
    const int A = e->cfg.n_arenas;
    std::vector<ObstDev> all;
    std::vector<int> offs(1, 0);
    size_t voff = 0, poff = 0;
    for (int a = 0; a < A; ++a) {
        if (n_poly[a] < 0 || (n_poly[a] > 0 && (!verts_xy || !poly_sizes)))
            return fail(e, CA_EINVAL, "ca_set_obstacles_per_arena: bad argument for arena %d", a);
        std::vector<ObstDev> tab;
        const int rc = build_table(e, verts_xy ? verts_xy + 2 * voff : nullptr, poly_sizes ? poly_sizes + poff : nullptr,
                                   n_poly[a], tab);
        if (rc) return rc;
        for (int k = 0; k < n_poly[a]; ++k) voff += (size_t)poly_sizes[poff + k];
        poff += (size_t)n_poly[a];
        if (tab.size() > 65536) return fail(e, CA_ERANGE, "ca_set_obstacles_per_arena: arena %d has %zu edges (at most 65536)", a, tab.size());
        all.insert(all.end(), tab.begin(), tab.end());  // next / prev stay local to the arena's table
        if (all.size() > (size_t)0x7FFFFFFF) return fail(e, CA_ERANGE, "ca_set_obstacles_per_arena: too many edges");
        offs.push_back((int)all.size());
    }
    return install_tables(e, all, offs);
}

static int get_table(ca_env* e, int arena, float* verts_xy, int32_t* next, int32_t* convex, int32_t cap, int32_t* n_out) {
    const bool per = !e->h_tab_off.empty();
    const int t0 = per ? e->h_tab_off[arena] : 0;
    const int n = per ? e->h_tab_off[arena + 1] - t0 : (int)e->h_obst.size();
    *n_out = n;
    for (int i = 0; i < n && i < cap; ++i) {
        const ObstDev& o = e->h_obst[t0 + i];
        if (verts_xy) { verts_xy[2 * i] = o.px; verts_xy[2 * i + 1] = o.py; }
        if (next) next[i] = o.next;
        if (convex) convex[i] = o.convex;
    }
    return CA_OK;
}

int ca_get_obstacles(ca_env* e, float* verts_xy, int32_t* next, int32_t* convex, int32_t cap, int32_t* n_out) {
    if (!e || !n_out) return fail(e, CA_EINVAL, "ca_get_obstacles: null argument");
    return get_table(e, 0, verts_xy, next, convex, cap, n_out);
}

int ca_get_obstacles_arena(ca_env* e, int32_t arena, float* verts_xy, int32_t* next, int32_t* convex, int32_t cap,
                           int32_t* n_out) {
    if (!e || !n_out) return fail(e, CA_EINVAL, "ca_get_obstacles_arena: null argument");
    if (arena < 0 || arena >= e->cfg.n_arenas) return fail(e, CA_ERANGE, "ca_get_obstacles_arena: arena %d of %d", arena, e->cfg.n_arenas);
    return get_table(e, arena, verts_xy, next, convex, cap, n_out);
}

}  // extern "C" (the per-agent parameters and the scenario generators below are plain C++ around their entry points)

// ---- per-agent ORCA parameters (sim.addAgent's per-agent arguments, env.py:126-133; setAgentRadius / setAgentMaxSpeed /
// setAgentTimeHorizon / setAgentTimeHorizonObst) ----
// every agent's octagon as the observation sees it (env.py:335-350): vertex e = (r cos(e pi/4), -(r sin(e pi/4))) in fp64 from the
// fp32 radius, rounded once to fp32 -- host_tables' chain, per agent; cos / sin are libm's, as there
static void agent_octagons(const std::vector<float>& radius, std::vector<float>& oct) {
    double cs[8], sn[8];
    for (int i = 0; i < 8; ++i) { const double th = i * (2.0 * M_PI / 8); cs[i] = std::cos(th); sn[i] = std::sin(th); }
    oct.resize(radius.size() * 16);
    for (size_t q = 0; q < radius.size(); ++q) {
        const double r = (double)radius[q];
        for (int i = 0; i < 8; ++i) { oct[q * 16 + 2 * i] = (float)(r * cs[i]); oct[q * 16 + 2 * i + 1] = (float)(-r * sn[i]); }
    }
}

// the handle's variant state that per-agent parameters change (saved before a prospective pick_variant, restored on failure)
struct VariantState { bool ap, ap_user, ac, sens, quad, quad_roll, pair; int ST, SMX, KT; size_t lds, lds_p; };
static VariantState save_variant(const ca_env* e) { return {e->ap, e->ap_user, e->ac, e->sens, e->quad, e->quad_roll, e->pair, e->ST, e->SMX, e->KT, e->lds, e->lds_p}; }
static void restore_variant(ca_env* e, const VariantState& v) {
    e->ap = v.ap; e->ap_user = v.ap_user; e->ac = v.ac; e->sens = v.sens; e->quad = v.quad; e->quad_roll = v.quad_roll; e->pair = v.pair; e->ST = v.ST; e->SMX = v.SMX; e->KT = v.KT;
    e->lds = v.lds; e->lds_p = v.lds_p;
}
// switch the handle to the kernels of (parameters of the caller's: ap_user, agent counts per arena: ac) -- the AgentParams kernels
// if either is set, with the ArenaCounts tag if ac, else the uniform ones: variant and dynamic-LDS limits, checked against the CU's
// LDS before anything is swapped (as install_tables does).  *misfit: the kernel does not fit; the handle is then left as it was.
// sens (per-agent sensing, ca_set_agent_sensing) selects the AgentSensing twin of whichever of the two it is, and switches them on by itself.
static hipError_t switch_agent_params(ca_env* e, bool ap_user, bool ac, bool sens, bool* misfit) {
    const VariantState old_v = save_variant(e);
    const bool on = ap_user || ac || sens;
    e->ap = on; e->ap_user = ap_user; e->ac = ac; e->sens = sens;
    e->quad = on ? false : e->quad_cfg;
    e->quad_roll = on ? false : e->quad_roll_cfg;
    pick_variant(e);
    hipError_t r = apply_variant_attributes(e, misfit);
    if (r == hipSuccess && !*misfit) r = allow_obs_lds(e);
    if (r != hipSuccess || *misfit) {
        restore_variant(e, old_v);
        bool dummy = false;
        (void)apply_variant_attributes(e, &dummy);   // (the previous variant's limits again: the attribute calls are idempotent)
    }
    return r;
}

// the device arrays of the AgentParams kernels (the first call allocates them; they stay until ca_destroy)
static int alloc_agent_params(ca_env* e) {
    const size_t an = AN(e);
    for (int k = 0; k < 4; ++k) if (!e->d_ap[k]) HIPCHK(e, hipMalloc((void**)&e->d_ap[k], an * 4));
    if (!e->d_ap_oct) HIPCHK(e, hipMalloc((void**)&e->d_ap_oct, an * 64));
    return CA_OK;
}
// the four arrays and the octagons of their radii into them; complete on return (the host vectors may go)
static hipError_t push_agent_params(ca_env* e, const std::vector<float> (&h)[4]) {
    const size_t an = AN(e);
    std::vector<float> oct;
    agent_octagons(h[0], oct);
    hipError_t r = hipSuccess;
    for (int k = 0; k < 4 && r == hipSuccess; ++k) r = hipMemcpyAsync(e->d_ap[k], h[k].data(), an * 4, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(e->d_ap_oct, oct.data(), an * 64, hipMemcpyHostToDevice, e->stream);
    return r != hipSuccess ? r : hipStreamSynchronize(e->stream);
}

// ---- agents per arena (the reference's one constructor argument, Collision_Avoidance_Env(numAgents), env.py:23-60, per arena) ----
// ca_stats.agent_steps = steps an arena was advanced x its agents: the kernels count the steps (arena_steps), so the product so far
// is folded into a host counter whenever the agents per arena change
static int fold_agent_steps(ca_env* e) {
    const size_t A = e->cfg.n_arenas;
    std::vector<unsigned long long> hs(A);
    HIPCHK(e, download(e, hs.data(), e->arena_steps, A * 8));
    for (size_t a = 0; a < A; ++a) e->agent_steps_base += hs[a] * (uint64_t)(e->ac ? e->h_counts[a] : e->cfg.n_agents);
    HIPCHK(e, hipMemsetAsync(e->arena_steps, 0, A * 8, e->stream));
    return CA_OK;
}
// what an absent row shows from the call on: a reward of 0 and an observation row of zeros
__global__ void clear_absent_kernel(const int* counts, int A, int N, float* reward, float* obs) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // one lane per (row, ray)
    const size_t q = t >> 4;
    if (q >= (size_t)A * N) return;
    const int a = (int)(q / N), i = (int)(q - (size_t)a * N), r = (int)(t & 15);
    if (i < counts[a]) return;
    reinterpret_cast<float4*>(obs)[q * 16 + r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r == 0) reward[q] = 0.0f;
}
// ca_set_agent_sensing: the agent-neighbour half (low byte) of every packed count reads 0 -- a list of the previous lengths may be
// longer than its agent's new K_i; the obstacle half stays
__global__ void clear_agent_nbr_counts_kernel(unsigned short* counts, size_t n) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) counts[q] &= (unsigned short)0xFF00u;
}

extern "C" {

int ca_set_agent_counts(ca_env* e, const int32_t* counts, size_t bytes, int32_t src_is_device) {
    if (!e) return CA_EINVAL;
    if (e->tiled)
        return fail(e, CA_EINVAL, "ca_set_agent_counts: not on a tiled handle (CA_CREATE_TILED): the tiled kernels have no per-arena-count form");
    HIPCHK(e, hipSetDevice(e->device));
    const int A = e->cfg.n_arenas, N = e->cfg.n_agents;
    const size_t an = AN(e);
    std::vector<int> h;
    if (counts) {
        if (e->S > SMAX)
            return fail(e, CA_EINVAL, "ca_set_agent_counts: not together with wide obstacle lists (max_obst_neighbors=%d > %d)", e->S, SMAX);
        if (bytes != (size_t)A * 4) return fail(e, CA_ESIZE, "ca_set_agent_counts: the array holds %zu bytes, got %zu", (size_t)A * 4, bytes);
        h.resize(A);
        if (src_is_device) HIPCHK(e, download(e, h.data(), counts, (size_t)A * 4));
        else memcpy(h.data(), counts, (size_t)A * 4);
        for (int a = 0; a < A; ++a)
            if (h[a] < 1 || h[a] > N)
                return fail(e, CA_ERANGE, "ca_set_agent_counts: arena %d has a count of %d, outside [1, n_agents=%d]", a, h[a], N);
        if (!e->d_counts) HIPCHK(e, hipMalloc((void**)&e->d_counts, (size_t)A * 4));
        { const int rc = alloc_agent_params(e); if (rc) return rc; }
    } else if (!e->ac) {
        return CA_OK;
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));   // steps in flight read the previous counts
    if (e->ac != (counts != nullptr)) {   // the prospective kernels are chosen and checked against the CU's LDS before anything is swapped
        bool misfit = false;
        const hipError_t r = switch_agent_params(e, e->ap_user, counts != nullptr, e->sens, &misfit);
        if (r != hipSuccess) return fail(e, CA_EHIP, "ca_set_agent_counts: %s (the handle keeps its previous counts)", hipGetErrorString(r));
        if (misfit)
            return fail(e, CA_ERANGE, "ca_set_agent_counts: the %s solve kernel does not fit the 160 KiB of LDS of a CU for n_agents=%d, max_neighbors=%d, "
                        "max_obst_neighbors=%d (with counts: the LDS line table, max_neighbors + max_obst_neighbors lines per lane); the handle keeps "
                        "its previous counts", counts ? "per-arena-count" : "uniform", N, e->K, e->S);
        e->ac = !e->ac;   // (the steps counted so far belong to the previous counts)
        const int rc = fold_agent_steps(e);
        e->ac = !e->ac;
        if (rc) return rc;
    } else {
        const int rc = fold_agent_steps(e);
        if (rc) return rc;
    }
    hipError_t r = hipSuccess;
    if (counts) {
        r = hipMemcpyAsync(e->d_counts, h.data(), (size_t)A * 4, hipMemcpyHostToDevice, e->stream);
        if (r == hipSuccess && !e->ap_user) {   // no parameters of the caller's: the per-agent arrays hold the ca_config values
            const float defaults[4] = {e->cfg.radius, e->cfg.max_speed, e->cfg.time_horizon, e->cfg.time_horizon_obst};
            std::vector<float> hp[4];
            for (int k = 0; k < 4; ++k) hp[k].assign(an, defaults[k]);
            r = push_agent_params(e, hp);
        }
    }
    // the lists of the last step may name agents that are gone, and a fresh simulator has none: both counts of every row read 0
    if (r == hipSuccess) r = hipMemsetAsync(e->counts, 0, an * sizeof(unsigned short), e->stream);
    if (r == hipSuccess && counts) {
        hipLaunchKernelGGL(clear_absent_kernel, dim3((unsigned)((an * 16 + 255) / 256)), dim3(256), 0, e->stream, e->d_counts, A, N, e->reward, e->obs);
        r = hipGetLastError();
    }
    e->h_counts.swap(h);
    e->lists_trusted = false;
    StepCold hc;
    fill_cold(e, hc);
    if (r == hipSuccess) r = upload(e, e->d_cold, &hc, sizeof hc);   // (synchronises)
    if (r != hipSuccess) return fail(e, CA_EHIP, "ca_set_agent_counts: %s", hipGetErrorString(r));
    return alan_pick(e);   // (the form of the ALAN step follows the solve kernel)
}

int ca_get_agent_counts(ca_env* e, int32_t* counts, size_t bytes, int32_t dst_is_device) {
    if (!e || !counts) return fail(e, CA_EINVAL, "ca_get_agent_counts: null argument");
    const size_t A = e->cfg.n_arenas;
    if (bytes != A * 4) return fail(e, CA_ESIZE, "ca_get_agent_counts: the array holds %zu bytes, got %zu", A * 4, bytes);
    HIPCHK(e, hipSetDevice(e->device));
    std::vector<int> uni;
    if (!e->ac) uni.assign(A, e->cfg.n_agents);
    const int* s = e->ac ? e->h_counts.data() : uni.data();
    if (dst_is_device) { HIPCHK(e, upload(e, counts, s, A * 4)); }
    else memcpy(counts, s, A * 4);
    return CA_OK;
}

int ca_agent_counts_info(ca_env* e, int32_t* per_arena) {
    if (!e) return CA_EINVAL;
    if (per_arena) *per_arena = e->ac ? 1 : 0;
    return CA_OK;
}

int ca_set_agent_params(ca_env* e, const float* radius, const float* max_speed, const float* time_horizon,
                        const float* time_horizon_obst, size_t bytes_each, int32_t src_is_device) {
    if (!e) return CA_EINVAL;
    const float* src[4] = {radius, max_speed, time_horizon, time_horizon_obst};
    static const char* const names[4] = {"radius", "max_speed", "time_horizon", "time_horizon_obst"};
    const float defaults[4] = {e->cfg.radius, e->cfg.max_speed, e->cfg.time_horizon, e->cfg.time_horizon_obst};
    const bool any = radius || max_speed || time_horizon || time_horizon_obst;
    if (e->tiled && !e->tparams)
        return fail(e, CA_EINVAL, "ca_set_agent_params: not on a tiled handle made without CA_CREATE_TILED_PARAMS: the tiled kernels' per-agent-parameter "
                    "form is chosen at ca_create_ex (create_flags 0x11 or 0x15)");
    HIPCHK(e, hipSetDevice(e->device));
    ca_env::EdgeGrids n_eg;   // (a grid handle with the static edge grid on: the grids of the new obstacle range first, swapped in at the end)
    if (!any) {   // back to the handle's four constants and to the kernels it used with them
        if (!e->ap_user) return CA_OK;
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (e->ac || e->sens) {   // agent counts or per-agent sensing stay set: their kernels stay, the per-agent arrays return to the ca_config values
            if (e->egrid) {   // (a tiled grid handle with sensing: the edge grid returns to the handle's own obstacle range)
                const int rc = make_edge_grids(e, e->h_obst, e->h_tab_off, edge_grid_range(e, nullptr), n_eg, "ca_set_agent_params");
                if (rc) return rc;
            }
            std::vector<float> h[4];
            for (int k = 0; k < 4; ++k) h[k].assign(AN(e), defaults[k]);
            const hipError_t r = push_agent_params(e, h);
            if (r != hipSuccess) { free_edge_grids(n_eg); return fail(e, CA_EHIP, "ca_set_agent_params: %s", hipGetErrorString(r)); }
            if (e->egrid) { free_edge_grids(e->eg); e->eg = n_eg; }
            e->ap_rmax = e->cfg.radius;
            e->ap_user = false;
            for (auto& v : e->h_ap) v.clear();
            return alan_pick(e);
        }
        if (e->egrid) {
            const int rc = make_edge_grids(e, e->h_obst, e->h_tab_off, edge_grid_range(e, nullptr), n_eg, "ca_set_agent_params");
            if (rc) return rc;
        }
        bool misfit = false;
        const hipError_t r = switch_agent_params(e, false, false, false, &misfit);
        if (r != hipSuccess || misfit) free_edge_grids(n_eg);
        if (r != hipSuccess) return fail(e, CA_EHIP, "ca_set_agent_params: %s (the per-agent parameters stay)", hipGetErrorString(r));
        if (misfit) return fail(e, CA_ERANGE, "ca_set_agent_params: the uniform solve kernel does not fit the 160 KiB of LDS of a CU (the per-agent parameters stay)");
        if (e->egrid) { free_edge_grids(e->eg); e->eg = n_eg; }
        StepCold hc;
        fill_cold(e, hc);
        HIPCHK(e, upload(e, e->d_cold, &hc, sizeof hc));
        for (auto& h : e->h_ap) h.clear();
        return alan_pick(e);
    }
    if (e->S > SMAX)
        return fail(e, CA_EINVAL, "ca_set_agent_params: not together with wide obstacle lists (max_obst_neighbors=%d > %d)", e->S, SMAX);
    const size_t an = AN(e);
    if (bytes_each != an * 4) return fail(e, CA_ESIZE, "ca_set_agent_params: each array holds %zu bytes, got %zu", an * 4, bytes_each);
    // a configuration call: every value is checked (a device array is copied back for it)
    std::vector<float> h[4];
    for (int k = 0; k < 4; ++k) {
        h[k].assign(an, defaults[k]);
        if (!src[k]) continue;
        if (src_is_device) HIPCHK(e, download(e, h[k].data(), src[k], an * 4));
        else memcpy(h[k].data(), src[k], an * 4);
        for (size_t q = 0; q < an; ++q)
            if (!(h[k][q] >= CA_MIN_LENGTH && h[k][q] <= CA_MAX_LENGTH))   // (also false for NaN)
                return fail(e, CA_ERANGE, "ca_set_agent_params: %s=%g of arena %zu, agent %zu is outside the supported range [%g, %g] or not a number",
                            names[k], (double)h[k][q], q / (size_t)e->cfg.n_agents, q % (size_t)e->cfg.n_agents, (double)CA_MIN_LENGTH, (double)CA_MAX_LENGTH);
    }
    // the buffers exist before anything changes (the first call allocates them; they stay until ca_destroy)
    { const int rc = alloc_agent_params(e); if (rc) return rc; }
    HIPCHK(e, hipStreamSynchronize(e->stream));   // steps in flight read the previous values
    if (e->egrid) {   // (a refused rebuild fails the whole call: the handle keeps its parameters, kernels and grids)
        const int rc = make_edge_grids(e, e->h_obst, e->h_tab_off, edge_grid_range(e, h), n_eg, "ca_set_agent_params");
        if (rc) return rc;
    }
    if (!e->ap) {   // the prospective variant is chosen and checked against the CU's LDS before anything is swapped
        bool misfit = false;
        const hipError_t r = switch_agent_params(e, true, false, false, &misfit);
        if (r != hipSuccess || misfit) free_edge_grids(n_eg);
        if (r != hipSuccess) return fail(e, CA_EHIP, "ca_set_agent_params: %s (the handle keeps its uniform parameters)", hipGetErrorString(r));
        if (misfit)
            return fail(e, CA_ERANGE, "ca_set_agent_params: the per-agent solve kernel (LDS line table, max_neighbors + max_obst_neighbors lines per lane) "
                        "does not fit the 160 KiB of LDS of a CU for n_agents=%d, max_neighbors=%d, max_obst_neighbors=%d; the handle keeps its "
                        "uniform parameters", e->cfg.n_agents, e->K, e->S);
    }
    hipError_t r = push_agent_params(e, h);
    StepCold hc;
    fill_cold(e, hc);
    if (r == hipSuccess) r = upload(e, e->d_cold, &hc, sizeof hc);
    if (r != hipSuccess) { free_edge_grids(n_eg); return fail(e, CA_EHIP, "ca_set_agent_params: %s", hipGetErrorString(r)); }
    if (e->egrid) { free_edge_grids(e->eg); e->eg = n_eg; }
    e->ap_rmax = 0.0f;   // (the pair count's bound on a tiled handle: ca_tiled.h TiledCloseParamsArgs)
    for (size_t q = 0; q < an; ++q) e->ap_rmax = h[0][q] > e->ap_rmax ? h[0][q] : e->ap_rmax;
    for (int k = 0; k < 4; ++k) e->h_ap[k].swap(h[k]);
    e->ap_user = true;   // (a handle with agent counts ran these kernels already, on the ca_config values)
    return alan_pick(e);   // (the form of the ALAN step follows the solve kernel)
}

int ca_get_agent_params(ca_env* e, float* radius, float* max_speed, float* time_horizon, float* time_horizon_obst,
                        size_t bytes_each, int32_t dst_is_device) {
    if (!e) return CA_EINVAL;
    float* dst[4] = {radius, max_speed, time_horizon, time_horizon_obst};
    const float defaults[4] = {e->cfg.radius, e->cfg.max_speed, e->cfg.time_horizon, e->cfg.time_horizon_obst};
    const size_t an = AN(e);
    if (bytes_each != an * 4) return fail(e, CA_ESIZE, "ca_get_agent_params: each array holds %zu bytes, got %zu", an * 4, bytes_each);
    HIPCHK(e, hipSetDevice(e->device));
    for (int k = 0; k < 4; ++k) {
        if (!dst[k]) continue;
        std::vector<float> uni;
        if (!e->ap_user) uni.assign(an, defaults[k]);   // uniform parameters: the handle's constant for every agent
        const float* s = e->ap_user ? e->h_ap[k].data() : uni.data();
        if (dst_is_device) { HIPCHK(e, upload(e, dst[k], s, an * 4)); }
        else memcpy(dst[k], s, an * 4);
    }
    return CA_OK;
}

int ca_agent_params_info(ca_env* e, int32_t* per_agent) {
    if (!e) return CA_EINVAL;
    if (per_agent) *per_agent = e->ap_user ? 1 : 0;
    return CA_OK;
}

// ---- per-agent sensing: the two remaining per-agent arguments of sim.addAgent (neighborDist, maxNeighbors; env.py:126-133, ALAN:81-87) ----
int ca_set_agent_sensing(ca_env* e, const float* neighbor_dist, const int32_t* max_neighbors, size_t bytes_each, int32_t src_is_device) {
    if (!e) return CA_EINVAL;
    if (e->tiled && !e->tparams)
        return fail(e, CA_EINVAL, "ca_set_agent_sensing: not on a tiled handle made without CA_CREATE_TILED_PARAMS: the tiled kernels' per-agent "
                    "form is chosen at ca_create_ex (create_flags 0x11 or 0x15)");
    HIPCHK(e, hipSetDevice(e->device));
    const size_t an = AN(e), N = (size_t)e->cfg.n_agents;
    const bool any = neighbor_dist || max_neighbors;
    std::vector<float> hn;
    std::vector<int> hk;
    std::vector<unsigned char> hk8;
    if (any) {
        if (e->S > SMAX)
            return fail(e, CA_EINVAL, "ca_set_agent_sensing: not together with wide obstacle lists (max_obst_neighbors=%d > %d)", e->S, SMAX);
        if (bytes_each != an * 4) return fail(e, CA_ESIZE, "ca_set_agent_sensing: each array holds %zu bytes, got %zu", an * 4, bytes_each);
        // a configuration call: every value is checked (a device array is copied back for it), absent rows' too.  The ca_config values
        // are the capacities: they size the K class, the list layout, the grids and the composite-key image
        hn.assign(an, e->cfg.neighbor_dist);
        hk.assign(an, e->cfg.max_neighbors);
        if (neighbor_dist) {
            if (src_is_device) HIPCHK(e, download(e, hn.data(), neighbor_dist, an * 4));
            else memcpy(hn.data(), neighbor_dist, an * 4);
            for (size_t q = 0; q < an; ++q)
                if (!(hn[q] >= CA_MIN_LENGTH && hn[q] <= e->cfg.neighbor_dist))   // (also false for NaN)
                    return fail(e, CA_ERANGE, "ca_set_agent_sensing: neighbor_dist=%g of arena %zu, agent %zu is outside [%g, the handle's neighbor_dist=%g] "
                                "or not a number", (double)hn[q], q / N, q % N, (double)CA_MIN_LENGTH, (double)e->cfg.neighbor_dist);
        }
        if (max_neighbors) {
            if (src_is_device) HIPCHK(e, download(e, hk.data(), max_neighbors, an * 4));
            else memcpy(hk.data(), max_neighbors, an * 4);
            for (size_t q = 0; q < an; ++q)
                if (hk[q] < 0 || hk[q] > e->cfg.max_neighbors)
                    return fail(e, CA_ERANGE, "ca_set_agent_sensing: max_neighbors=%d of arena %zu, agent %zu is outside [0, the handle's max_neighbors=%d]",
                                hk[q], q / N, q % N, e->cfg.max_neighbors);
        }
        hk8.resize(an);
        for (size_t q = 0; q < an; ++q) hk8[q] = (unsigned char)hk[q];
        // the buffers exist before anything changes (the first call allocates them; they stay until ca_destroy)
        if (!e->d_as_nd) HIPCHK(e, hipMalloc((void**)&e->d_as_nd, an * 4));
        if (!e->d_as_k) HIPCHK(e, hipMalloc((void**)&e->d_as_k, an));
        { const int rc = alloc_agent_params(e); if (rc) return rc; }
    } else if (!e->sens) {
        return CA_OK;
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));   // steps in flight read the previous values
    if (e->sens != any) {   // the prospective kernels are chosen and checked against the CU's LDS before anything is swapped
        bool misfit = false;
        const hipError_t r = switch_agent_params(e, e->ap_user, e->ac, any, &misfit);
        if (r != hipSuccess) return fail(e, CA_EHIP, "ca_set_agent_sensing: %s (the handle keeps what it had)", hipGetErrorString(r));
        if (misfit)
            return fail(e, CA_ERANGE, "ca_set_agent_sensing: the %s solve kernel does not fit the 160 KiB of LDS of a CU for n_agents=%d, max_neighbors=%d, "
                        "max_obst_neighbors=%d (with per-agent sensing: the LDS line table, max_neighbors + max_obst_neighbors lines per lane); the handle "
                        "keeps what it had", any ? "per-agent" : "uniform", e->cfg.n_agents, e->K, e->S);
    }
    hipError_t r = hipSuccess;
    if (any) {
        if (!e->ap_user) {   // no parameters of the caller's: the per-agent arrays hold the ca_config values
            const float defaults[4] = {e->cfg.radius, e->cfg.max_speed, e->cfg.time_horizon, e->cfg.time_horizon_obst};
            std::vector<float> hp[4];
            for (int k = 0; k < 4; ++k) hp[k].assign(an, defaults[k]);
            r = push_agent_params(e, hp);
            e->ap_rmax = e->cfg.radius;
        }
        if (r == hipSuccess) r = hipMemcpyAsync(e->d_as_nd, hn.data(), an * 4, hipMemcpyHostToDevice, e->stream);
        if (r == hipSuccess) r = hipMemcpyAsync(e->d_as_k, hk8.data(), an, hipMemcpyHostToDevice, e->stream);
    }
    // a list of the previous lengths may be longer than its agent's K_i: the agent-neighbour count of every row reads 0
    if (r == hipSuccess) {
        hipLaunchKernelGGL(clear_agent_nbr_counts_kernel, dim3((unsigned)((an + 255) / 256)), dim3(256), 0, e->stream, e->counts, an);
        r = hipGetLastError();
    }
    e->h_as_nd.swap(hn);   // (both empty when the call clears)
    e->h_as_k.swap(hk);
    e->lists_trusted = false;
    StepCold hc;
    fill_cold(e, hc);
    if (r == hipSuccess) r = upload(e, e->d_cold, &hc, sizeof hc);   // (synchronises: the host vectors may go)
    if (r != hipSuccess) return fail(e, CA_EHIP, "ca_set_agent_sensing: %s", hipGetErrorString(r));
    return alan_pick(e);   // (the form of the ALAN step follows the solve kernel)
}

int ca_get_agent_sensing(ca_env* e, float* neighbor_dist, int32_t* max_neighbors, size_t bytes_each, int32_t dst_is_device) {
    if (!e) return CA_EINVAL;
    const size_t an = AN(e);
    if (bytes_each != an * 4) return fail(e, CA_ESIZE, "ca_get_agent_sensing: each array holds %zu bytes, got %zu", an * 4, bytes_each);
    HIPCHK(e, hipSetDevice(e->device));
    if (neighbor_dist) {
        std::vector<float> uni;
        if (!e->sens) uni.assign(an, e->cfg.neighbor_dist);   // without per-agent sensing: the handle's constant for every agent
        const float* s = e->sens ? e->h_as_nd.data() : uni.data();
        if (dst_is_device) { HIPCHK(e, upload(e, neighbor_dist, s, an * 4)); }
        else memcpy(neighbor_dist, s, an * 4);
    }
    if (max_neighbors) {
        std::vector<int> uni;
        if (!e->sens) uni.assign(an, e->cfg.max_neighbors);
        const int* s = e->sens ? e->h_as_k.data() : uni.data();
        if (dst_is_device) { HIPCHK(e, upload(e, max_neighbors, s, an * 4)); }
        else memcpy(max_neighbors, s, an * 4);
    }
    return CA_OK;
}

int ca_agent_sensing_info(ca_env* e, int32_t* per_agent) {
    if (!e) return CA_EINVAL;
    if (per_agent) *per_agent = e->sens ? 1 : 0;
    return CA_OK;
}

int ca_nbr_seed_info(ca_env* e, int32_t* seeded) {
    if (!e) return CA_EINVAL;
    if (seeded) *seeded = solve_launch(e, false, false).seeded ? 1 : 0;   // (the plain single-step form, as ca_launch_info reports it)
    return CA_OK;
}

int ca_lp3_pairs_info(ca_env* e, int32_t* paired) {
    if (!e) return CA_EINVAL;
    if (paired) *paired = solve_launch(e, false, false).paired ? 1 : 0;   // (the plain single-step form, as above)
    return CA_OK;
}

}  // extern "C"


// The scenario generators (env.py:86-97, ALAN:175-457) on the host, for arenas [0, An): An = n_arenas for the one scenario
// whose draws are sequential per arena (rejection-sampled starts), An = 1 for the per-agent TABLE of the others -- their
// layout either does not depend on the arena at all (circle, incoming, blocks, deadlock: libm's cos / sin / sqrt stay on the
// host) or only through counter-based draws, which init_scenario_kernel makes on the device.
static void host_scenario(const ca_env* e, int scenario, int An, std::vector<float>& px, std::vector<float>& py, std::vector<float>& vx,
                          std::vector<float>& vy, std::vector<float>& fx, std::vector<float>& fy, std::vector<double>& gx,
                          std::vector<double>& gy, std::vector<double>& g2x, std::vector<double>& g2y) {
    const ca_config& c = e->cfg;
    const int A = An, N = c.n_agents;
    const size_t an = (size_t)An * N;
    px.assign(an, 0.0f); py.assign(an, 0.0f); vx.assign(an, 0.0f); vy.assign(an, 0.0f); fx.assign(an, 0.0f); fy.assign(an, 0.0f);
    gx.assign(an, 0.0); gy.assign(an, 0.0); g2x.assign(an, 0.0); g2y.assign(an, 0.0);
    const double r = (double)c.radius;
    for (int a = 0; a < A; ++a) {
        const int64_t g = c.arena_offset + a;
        double theta = 0.0;
        for (int i = 0; i < N; ++i) {
            const size_t q = (size_t)a * N + i;
            double u0, u1, s, cs;
            rng2(c.seed, g, i, RNG_HEADING, 0, &u0, &u1);
            sincos64(uniform64(0.0, 2.0 * M_PI, u0), &s, &cs);  // env.py:89-90 / ALAN:276-277
            vx[q] = (float)cs; vy[q] = (float)s;
            if (scenario == CA_SCN_CROWD || scenario == CA_SCN_CROWD_SEPARATED) {  // ALAN:270-283
                const double E = std::sqrt(2.0 * r * N) * 2.0;
                // SURVEY 8d "rejection-sampled non-overlapping variant": the draw is repeated (sequence number
                // 1, 2, ...) until the start keeps 2 r from the starts of the agents before it; 64 tries at most
                const int tries = scenario == CA_SCN_CROWD_SEPARATED ? 64 : 1;
                const float minSq = sqr(c.radius + c.radius);
                for (int t = 0; t < tries; ++t) {
                    rng2(c.seed, g, i, RNG_POS, (uint32_t)t, &u0, &u1);
                    px[q] = (float)uniform64(0.0, E, u0); py[q] = (float)uniform64(0.0, E, u1);
                    bool clear = true;
                    for (int j = 0; j < i && clear; ++j)
                        clear = !(absSq(mk(px[q], py[q]) - mk(px[q - i + j], py[q - i + j])) < minSq);
                    if (clear) break;
                }
                rng2(c.seed, g, i, RNG_GOAL, 0, &u0, &u1);
                gx[q] = uniform64(0.0, E, u0); gy[q] = uniform64(0.0, E, u1);
                g2x[q] = gx[q]; g2y[q] = gy[q];
            } else if (scenario == CA_SCN_CIRCLE) {  // ALAN:297-322
                const double R = (r * 3 * N) / (2.0 * M_PI);
                const double E = 2.0 * R + 4.0 * r;
                px[q] = (float)(E / 2 + R * std::cos(theta)); py[q] = (float)(E / 2 + R * std::sin(theta));
                gx[q] = E / 2 + R * std::cos(theta + M_PI);
                gy[q] = E / 2 + R * std::sin(theta + M_PI);
                g2x[q] = gx[q]; g2y[q] = gy[q];
                theta += (2.0 * M_PI) / N;
            } else if (scenario >= CA_SCN_CONGESTED) {  // ALAN:175-193, 213-258, 333-357, 377-416
                const double E = (scenario == CA_SCN_CONGESTED) ? std::sqrt(2 * r * N) * 3
                               : (scenario == CA_SCN_BLOCKS) ? 3 * r * N : std::sqrt(2 * r * N) * 10;
                double x = 0, y = 0, tx = 0, ty = 0, t2x = 0, t2y = 0;
                if (scenario == CA_SCN_CONGESTED) {
                    rng2(c.seed, g, i, RNG_POS, 0, &u0, &u1);
                    x = uniform64(E * 0.2, E, u0); y = uniform64(0.0, E, u1);
                    tx = 0.1 * E - 1.0; ty = E / 2; t2x = 0.1 * E - E; t2y = E / 2;
                } else if (scenario == CA_SCN_INCOMING) {
                    if (i == 0) {
                        x = 0.1 * E; y = E / 2; tx = t2x = 0.9 * E; ty = t2y = E / 2;
                    } else {  // the block of N-1 agents, column by column (ALAN:232-258)
                        const double len = std::sqrt((double)(N - 1)), x_inc = 3 * r, y_inc = 2.1 * r;
                        const double y_start = E / 2 - ((y_inc * len) / 2);
                        double x_pos = 0.8 * E, y_pos = y_start;
                        for (int k = 1; k < i; ++k) {
                            y_pos += y_inc;
                            if (y_pos > y_start + y_inc * len) { x_pos += x_inc; y_pos = y_start; }
                        }
                        x = x_pos; y = y_pos; tx = t2x = x_pos - 0.7 * E; ty = t2y = y_pos;
                    }
                } else if (scenario == CA_SCN_BLOCKS) {
                    double y_pos = 1.5 * r;
                    for (int k = 0; k < i; ++k) y_pos += 3 * r;
                    x = 1.5 * r; y = y_pos; tx = t2x = E - 1.5 * r; ty = t2y = y_pos;
                } else {  // deadlock: two queues facing each other through a tube
                    const int half = N / 2;
                    if (i < half) {
                        double pos_x = 0.2 * E;
                        for (int k = 0; k < i; ++k) pos_x += -3 * r;
                        x = pos_x; tx = 0.9 * E; t2x = 0.9 * E + E;
                    } else {
                        double pos_x = 0.8 * E;
                        for (int k = half; k < i; ++k) pos_x += 3 * r;
                        x = pos_x; tx = 0.1 * E; t2x = 0.1 * E - E;
                    }
                    y = E / 2; ty = t2y = E / 2;
                }
                px[q] = (float)x; py[q] = (float)y; gx[q] = tx; gy[q] = ty;
                g2x[q] = t2x; g2y[q] = t2y;
            } else {  // env.py:86-95, 361
                const double E = 10.0;
                rng2(c.seed, g, i, RNG_POS, 0, &u0, &u1);
                px[q] = (float)uniform64(E * 0.5, E, u0); py[q] = (float)uniform64(0.0, E, u1);
                gx[q] = 1.0; gy[q] = 5.0; g2x[q] = -10.0; g2y[q] = 5.0;
            }
            double dx, dy;  // env.py:97 update_pref_vel
            pref_dir64(px[q], py[q], gx[q], gy[q], &dx, &dy);
            fx[q] = (float)dx; fy[q] = (float)dy;
        }
    }
}

struct InitArgs {
    float *pos_x, *pos_y, *vel_x, *vel_y, *pref_x, *pref_y;
    double *goal_x, *goal_y, *goal2_x, *goal2_y;
    const float *tpx, *tpy;                      // [N] table: start of agent i (arena-independent scenarios)
    const double *tgx, *tgy, *tg2x, *tg2y;       // [N] table: targets of agent i
    double x0, x1, y0, y1;                       // box of the drawn starts (pos_rng)
    double ge;                                   // drawn goals: uniform in (0, ge)^2 (goal_rng)
    uint64_t seed;
    int64_t arena_offset;
    int A, N, pos_rng, goal_rng;
};
// every agent of every arena: heading drawn (env.py:89-90 / ALAN:276-277), start and targets drawn or from the table,
// preferred velocity towards the target (env.py:97) -- the same counter-based streams and the same fp64 operations as the host
// path (ca_math.h), so the state is the host path's bit for bit
__global__ void init_scenario_kernel(const InitArgs p) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (size_t)p.A * p.N) return;
    const int a = (int)(q / p.N), i = (int)(q - (size_t)a * p.N);
    const int64_t g = p.arena_offset + a;
    double u0, u1, s, cs;
    rng2(p.seed, g, i, RNG_HEADING, 0, &u0, &u1);
    sincos64(uniform64(0.0, 2.0 * M_PI, u0), &s, &cs);
    p.vel_x[q] = (float)cs; p.vel_y[q] = (float)s;
    float px = p.tpx[i], py = p.tpy[i];
    double gx = p.tgx[i], gy = p.tgy[i], g2x = p.tg2x[i], g2y = p.tg2y[i];
    if (p.pos_rng) {
        rng2(p.seed, g, i, RNG_POS, 0, &u0, &u1);
        px = (float)uniform64(p.x0, p.x1, u0); py = (float)uniform64(p.y0, p.y1, u1);
    }
    if (p.goal_rng) {
        rng2(p.seed, g, i, RNG_GOAL, 0, &u0, &u1);
        gx = uniform64(0.0, p.ge, u0); gy = uniform64(0.0, p.ge, u1);
        g2x = gx; g2y = gy;
    }
    double dx, dy;
    pref_dir64(px, py, gx, gy, &dx, &dy);
    p.pos_x[q] = px; p.pos_y[q] = py; p.pref_x[q] = (float)dx; p.pref_y[q] = (float)dy;
    p.goal_x[q] = gx; p.goal_y[q] = gy; p.goal2_x[q] = g2x; p.goal2_y[q] = g2y;
}

extern "C" {

int ca_init_scenario(ca_env* e, int32_t scenario) {
    if (!e) return CA_EINVAL;
    if (scenario < 0 || scenario > CA_SCN_CROWD_SEPARATED)
        return fail(e, CA_EINVAL, "ca_init_scenario: unknown scenario %d", scenario);
    if (e->ac && scenario != CA_SCN_DOORWAY)
        return fail(e, CA_EINVAL, "ca_init_scenario: scenario %d is not supported while per-arena agent counts are set (its geometry is a function "
                    "of the number of agents; CA_SCN_DOORWAY is not)", scenario);
    const ca_config& c = e->cfg;
    const int A = c.n_arenas, N = c.n_agents;
    const size_t an = AN(e);
    const bool on_host = scenario == CA_SCN_CROWD_SEPARATED;   // sequential draws per arena (each start depends on the ones before)
    std::vector<float> px, py, vx, vy, fx, fy;
    std::vector<double> gx, gy, g2x, g2y;
    host_scenario(e, scenario, on_host ? A : 1, px, py, vx, vy, fx, fy, gx, gy, g2x, g2y);
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;  // everything below is ordered on the handle's stream (see dalloc)
    if (on_host) {
        struct { float* d; std::vector<float>* h; } up[] = {{e->pos_x, &px}, {e->pos_y, &py}, {e->vel_x, &vx},
            {e->vel_y, &vy}, {e->pref_x, &fx}, {e->pref_y, &fy}};
        struct { double* d; std::vector<double>* h; } upd[] = {{e->goal_x, &gx}, {e->goal_y, &gy},
            {e->goal2_x, &g2x}, {e->goal2_y, &g2y}};
        for (auto& u : up) HIPCHK(e, hipMemcpyAsync(u.d, u.h->data(), an * 4, hipMemcpyHostToDevice, st));
        for (auto& u : upd) HIPCHK(e, hipMemcpyAsync(u.d, u.h->data(), an * 8, hipMemcpyHostToDevice, st));
    } else {   // the per-agent table (N entries) goes up, the kernel fills A x N agents
        char* tab = nullptr;
        const size_t nb = (size_t)N * (2 * 4 + 4 * 8);
        HIPCHK(e, hipMalloc((void**)&tab, nb));
        std::vector<char> h(nb);
        memcpy(h.data(), px.data(), (size_t)N * 4); memcpy(h.data() + (size_t)N * 4, py.data(), (size_t)N * 4);
        memcpy(h.data() + (size_t)N * 8, gx.data(), (size_t)N * 8); memcpy(h.data() + (size_t)N * 16, gy.data(), (size_t)N * 8);
        memcpy(h.data() + (size_t)N * 24, g2x.data(), (size_t)N * 8); memcpy(h.data() + (size_t)N * 32, g2y.data(), (size_t)N * 8);
        hipError_t r = hipMemcpyAsync(tab, h.data(), nb, hipMemcpyHostToDevice, st);
        if (r == hipSuccess) {
            InitArgs ia;
            ia.pos_x = e->pos_x; ia.pos_y = e->pos_y; ia.vel_x = e->vel_x; ia.vel_y = e->vel_y; ia.pref_x = e->pref_x; ia.pref_y = e->pref_y;
            ia.goal_x = e->goal_x; ia.goal_y = e->goal_y; ia.goal2_x = e->goal2_x; ia.goal2_y = e->goal2_y;
            ia.tpx = (const float*)tab; ia.tpy = (const float*)(tab + (size_t)N * 4);
            ia.tgx = (const double*)(tab + (size_t)N * 8); ia.tgy = (const double*)(tab + (size_t)N * 16);
            ia.tg2x = (const double*)(tab + (size_t)N * 24); ia.tg2y = (const double*)(tab + (size_t)N * 32);
            const double r2 = (double)c.radius;
            ia.pos_rng = (scenario == CA_SCN_CROWD || scenario == CA_SCN_CONGESTED || scenario == CA_SCN_DOORWAY) ? 1 : 0;
            ia.goal_rng = scenario == CA_SCN_CROWD ? 1 : 0;
            ia.x0 = 0.0; ia.x1 = 0.0; ia.y0 = 0.0; ia.y1 = 0.0; ia.ge = 0.0;
            if (scenario == CA_SCN_CROWD) { const double E = std::sqrt(2.0 * r2 * N) * 2.0; ia.x1 = E; ia.y1 = E; ia.ge = E; }             // ALAN:270-283
            else if (scenario == CA_SCN_CONGESTED) { const double E = std::sqrt(2 * r2 * N) * 3; ia.x0 = E * 0.2; ia.x1 = E; ia.y1 = E; }  // ALAN:177-186
            else if (scenario == CA_SCN_DOORWAY) { const double E = 10.0; ia.x0 = E * 0.5; ia.x1 = E; ia.y1 = E; }                        // env.py:86-95
            ia.seed = c.seed; ia.arena_offset = c.arena_offset; ia.A = A; ia.N = N;
            hipLaunchKernelGGL(init_scenario_kernel, dim3((unsigned)((an + 255) / 256)), dim3(256), 0, st, ia);
            r = hipGetLastError();
        }
        if (r == hipSuccess) r = hipStreamSynchronize(st);   // the table and the host staging go away
        hipFree(tab);
        if (r != hipSuccess) return fail(e, CA_EHIP, "ca_init_scenario: %s", hipGetErrorString(r));
    }
    HIPCHK(e, hipMemsetAsync(e->agent_done, 0, an * 4, st));
    HIPCHK(e, hipMemsetAsync(e->arrive_step, 0xff, an * 4, st));
    HIPCHK(e, hipMemsetAsync(e->regoal_count, 0, an * 4, st));
    HIPCHK(e, hipMemsetAsync(e->counts, 0, an * 2, st));
    HIPCHK(e, hipMemsetAsync(e->step_count, 0, (size_t)A * 4, st));
    HIPCHK(e, hipMemsetAsync(e->arena_done, 0, (size_t)A * 4, st));
    HIPCHK(e, hipMemsetAsync(e->episode, 0, (size_t)A * 4, st));
    HIPCHK(e, hipMemsetAsync(e->obs, 0, an * CA_OBS_DIM * 4, st));
    HIPCHK(e, hipStreamSynchronize(st));  // the host vectors above go out of scope
    e->orient_valid = false;
    return CA_OK;
}

// The packed neighbour-list fields keep their ABI image (i32 arrays, include/ca_env.h) through two small kernels.
__global__ void unpack_list_kernel(const void* src, int kind, int w16, int* dst, size_t n) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    if (kind == 0) dst[q] = (int)(reinterpret_cast<const unsigned short*>(src)[q] & 0xFFu);       // agent-neighbour count
    else if (kind == 1) dst[q] = (int)(reinterpret_cast<const unsigned short*>(src)[q] >> 8);      // obstacle-neighbour count
    else dst[q] = w16 ? ld_idx_t<true>(src, q) : ld_idx_t<false>(src, q);
}
__global__ void pack_list_kernel(const int* src, int kind, int w16, void* dst, size_t n) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    unsigned short* c = reinterpret_cast<unsigned short*>(dst);
    if (kind == 0) c[q] = (unsigned short)((c[q] & 0xFF00u) | ((unsigned)src[q] & 0xFFu));
    else if (kind == 1) c[q] = (unsigned short)((c[q] & 0x00FFu) | (((unsigned)src[q] & 0xFFu) << 8));
    else if (w16) st_idx_t<true>(dst, q, src[q]);
    else st_idx_t<false>(dst, q, src[q]);
}
static bool packed_field(int f) {
    return f == CA_FLD_NB_COUNT || f == CA_FLD_OBST_COUNT || f == CA_FLD_NB_IDX || f == CA_FLD_OBST_IDX;
}
static int packed_kind(int f) { return f == CA_FLD_NB_COUNT ? 0 : (f == CA_FLD_OBST_COUNT ? 1 : 2); }
static int cvt_reserve(ca_env* e, size_t elems) {
    if (e->cvt_cap >= elems) return CA_OK;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->cvt_buf) HIPCHK(e, hipFree(e->cvt_buf));
    e->cvt_buf = nullptr; e->cvt_cap = 0;
    HIPCHK(e, hipMalloc((void**)&e->cvt_buf, elems * sizeof(int)));
    e->cvt_cap = elems;
    return CA_OK;
}

int ca_set(ca_env* e, int32_t field, const void* src, size_t bytes, int32_t src_is_device) {
    if (!e || !src) return fail(e, CA_EINVAL, "ca_set: null argument");
    const FieldInfo fi = field_info(e, field);
    if (!fi.ptr) return fail(e, CA_EINVAL, "ca_set: unknown field %d", field);
    if (!fi.writable) return fail(e, CA_EINVAL, "ca_set: field %d is read-only", field);
    if (bytes != fi.bytes) return fail(e, CA_ESIZE, "ca_set: field %d holds %zu bytes, got %zu", field, fi.bytes, bytes);
    HIPCHK(e, hipSetDevice(e->device));
    if (packed_field(field)) {
        e->lists_trusted = false;   // (until the next solve launch has rewritten them)
        const size_t n = bytes / 4;
        const int rc = cvt_reserve(e, n);
        if (rc) return rc;
        HIPCHK(e, hipMemcpyAsync(e->cvt_buf, src, bytes, src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(pack_list_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, e->cvt_buf,
                           packed_kind(field), field == CA_FLD_NB_IDX ? e->nidx16 : 1, fi.ptr, n);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipStreamSynchronize(e->stream));  // the staging buffer is free again, the caller's host array too
        return CA_OK;
    }
    HIPCHK(e, hipMemcpyAsync(fi.ptr, src, bytes, src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
    if (!src_is_device) HIPCHK(e, hipStreamSynchronize(e->stream));
    if (field == CA_FLD_POS_X || field == CA_FLD_POS_Y || field == CA_FLD_GOAL_X || field == CA_FLD_GOAL_Y)
        e->orient_valid = false;
    return CA_OK;
}

int ca_get(ca_env* e, int32_t field, void* dst, size_t bytes, int32_t dst_is_device) {
    if (!e || !dst) return fail(e, CA_EINVAL, "ca_get: null argument");
    const FieldInfo fi = field_info(e, field);
    if (!fi.ptr) return fail(e, CA_EINVAL, "ca_get: unknown field %d", field);
    if (bytes != fi.bytes) return fail(e, CA_ESIZE, "ca_get: field %d holds %zu bytes, got %zu", field, fi.bytes, bytes);
    HIPCHK(e, hipSetDevice(e->device));
    if (packed_field(field)) {
        const size_t n = bytes / 4;
        const int rc = cvt_reserve(e, n);
        if (rc) return rc;
        hipLaunchKernelGGL(unpack_list_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, fi.ptr,
                           packed_kind(field), field == CA_FLD_NB_IDX ? e->nidx16 : 1, e->cvt_buf, n);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipMemcpyAsync(dst, e->cvt_buf, bytes, dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        return CA_OK;
    }
    HIPCHK(e, hipMemcpyAsync(dst, fi.ptr, bytes, dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
    if (!dst_is_device) HIPCHK(e, hipStreamSynchronize(e->stream));
    return CA_OK;
}

int ca_field_ptr(ca_env* e, int32_t field, void** dev_ptr, size_t* bytes) {
    if (!e || !dev_ptr) return fail(e, CA_EINVAL, "ca_field_ptr: null argument");
    const FieldInfo fi = field_info(e, field);
    if (!fi.ptr) return fail(e, CA_EINVAL, "ca_field_ptr: unknown field %d", field);
    if (packed_field(field))
        return fail(e, CA_EINVAL, "ca_field_ptr: field %d is stored packed (u8/u16); read it through ca_get", field);
    *dev_ptr = fi.ptr;
    if (bytes) *bytes = fi.bytes;
    return CA_OK;
}

int ca_bind_obs(ca_env* e, void* dev_ptr, size_t bytes) {
    if (!e || !dev_ptr) return fail(e, CA_EINVAL, "ca_bind_obs: null argument");
    if (bytes != AN(e) * CA_OBS_DIM * 4)
        return fail(e, CA_ESIZE, "ca_bind_obs: need %zu bytes, got %zu", AN(e) * CA_OBS_DIM * 4, bytes);
    if (((uintptr_t)dev_ptr & 15) != 0) return fail(e, CA_EINVAL, "ca_bind_obs: buffer must be 16-byte aligned");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->obs = (float*)dev_ptr;   // (the library's own observation buffer is part of the result slab and stays allocated)
    e->obs_external = true;
    return CA_OK;
}

int ca_reset(ca_env* e, const float* pos_x, const float* pos_y, int32_t pos_is_device, uint32_t flags) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_reset(e, pos_x, pos_y, pos_is_device, flags & ~CA_F_CONTACT));
    if (!e) return CA_EINVAL;
    if ((pos_x == nullptr) != (pos_y == nullptr)) return fail(e, CA_EINVAL, "ca_reset: pos_x and pos_y go together");
    HIPCHK(e, hipSetDevice(e->device));
    StepArgs a;
    fill_args(e, a, nullptr, flags);
    if (pos_x) {
        if (pos_is_device) { a.reset_px = pos_x; a.reset_py = pos_y; }
        else {
            HIPCHK(e, hipMemcpyAsync(e->tmp_x, pos_x, AN(e) * 4, hipMemcpyHostToDevice, e->stream));
            HIPCHK(e, hipMemcpyAsync(e->tmp_y, pos_y, AN(e) * 4, hipMemcpyHostToDevice, e->stream));
            HIPCHK(e, hipStreamSynchronize(e->stream));  // the caller's host buffers may go away
            a.reset_px = e->tmp_x; a.reset_py = e->tmp_y;
        }
    }
    HIPCHK(e, launch_reset(e, a));
    HIPCHK(e, hipGetLastError());
    e->orient_valid = true;
    if (flags & CA_F_OBS) HIPCHK(e, launch_obs(e));
    return CA_OK;
}

int ca_reset_masked(ca_env* e, const int32_t* mask, int32_t mask_is_device, uint32_t flags) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_reset_masked(e, mask, mask_is_device, flags & ~CA_F_CONTACT));
    if (!e || !mask) return fail(e, CA_EINVAL, "ca_reset_masked: null argument");
    HIPCHK(e, hipSetDevice(e->device));
    const int A = e->cfg.n_arenas;
    if (!mask_is_device) {
        if (!e->mask_buf) HIPCHK(e, dalloc(e, &e->mask_buf, (size_t)A, /*zero=*/false));  // fully overwritten below
        HIPCHK(e, upload(e, e->mask_buf, mask, (size_t)A * 4));
        mask = e->mask_buf;
    }
    StepArgs a;
    fill_args(e, a, nullptr, flags);
    a.reset_mask = mask;
    HIPCHK(e, launch_reset(e, a));
    HIPCHK(e, hipGetLastError());
    if (flags & CA_F_OBS) HIPCHK(e, launch_obs(e));
    return CA_OK;
}

// The reward terms round a step (ca_reward.h; kind 3 for ca_profile): reward_begin_kernel in front of its launches, reward_terms_kernel
// behind them -- or, parts_only, the one launch of ca_reward_parts for the state as it stands.
static hipError_t reward_buffers(ca_env* e) {
    if (!e->rew.saved) { const hipError_t r = dalloc(e, &e->rew.saved, AN(e)); if (r != hipSuccess) return r; }
    if (!e->rew.advance) { const hipError_t r = dalloc(e, &e->rew.advance, (size_t)e->cfg.n_arenas); if (r != hipSuccess) return r; }
    if (!e->rew.parts) { const hipError_t r = dalloc(e, &e->rew.parts, (size_t)REWARD_N_TERMS * AN(e)); if (r != hipSuccess) return r; }
    return hipSuccess;
}
static hipError_t launch_reward_begin(ca_env* e, uint32_t flags) {
    const hipError_t r = reward_buffers(e);
    if (r != hipSuccess) return r;
    RewardBeginArgs b;
    b.word = e->cfg.done_mode == CA_DONE_REGOAL ? e->regoal_count : e->agent_done;
    b.arena_done = e->arena_done; b.saved = e->rew.saved; b.advance = e->rew.advance;
    b.an = (unsigned)AN(e); b.N = e->cfg.n_agents; b.freeze = (flags & CA_F_FREEZE) ? 1 : 0;
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, reward_begin_kernel, dim3((b.an + 255) / 256), dim3(256), 0, e->stream, b);
    return hipGetLastError();
}
static hipError_t launch_reward_terms(ca_env* e, uint32_t flags, bool parts_only) {
    hipError_t r = reward_buffers(e);
    if (r != hipSuccess) return r;
    RewardTermsArgs c;
    c.pos_x = e->pos_x; c.pos_y = e->pos_y;
    c.ap_radius = e->ap ? e->d_ap[0] : nullptr;      // (as launch_contacts)
    c.agent_counts = e->ac ? e->d_counts : nullptr;
    c.obst = e->d_obst; c.tab_off = e->d_tab_off;
    c.an = (unsigned)AN(e);
    c.n_obst = e->h_tab_off.empty() ? (int)e->h_obst.size() : 0; c.A = e->cfg.n_arenas; c.N = e->cfg.n_agents;
    c.apb = c.N <= REWARD_BS ? REWARD_BS / c.N : 0;
    c.tiles = c.N <= REWARD_BS ? 0 : (c.N + REWARD_BS - 1) / REWARD_BS;
    c.radius = e->cfg.radius;
    c.weights = e->rew.d_w; c.margin = e->rew.margin;
    c.reward = e->reward; c.parts = e->rew.parts; c.saved = e->rew.saved; c.advance = e->rew.advance;
    c.agent_done = e->agent_done; c.regoal_count = e->regoal_count; c.arena_done = e->arena_done; c.arena_stats = e->arena_stats;
    c.regoal = e->cfg.done_mode == CA_DONE_REGOAL ? 1 : 0;
    c.autoreset = (flags & CA_F_AUTORESET) ? 1 : 0; c.stats = (!parts_only && (flags & CA_F_STATS)) ? 1 : 0;
    c.need_mask = e->rew.need_mask;
    c.need_pairs = (c.need_mask & ((1 << CA_REWARD_COLLISION) | (1 << CA_REWARD_NEAR))) ? 1 : 0;
    c.need_walls = (c.need_mask & ((1 << CA_REWARD_WALL) | (1 << CA_REWARD_WALL_NEAR))) ? 1 : 0;
    c.parts_only = parts_only ? 1 : 0;
    const unsigned grid = c.apb ? (unsigned)((c.A + c.apb - 1) / c.apb) : (unsigned)((size_t)c.A * c.tiles);
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, reward_terms_kernel, dim3(grid), dim3(REWARD_BS), 0, e->stream, c);
    r = hipGetLastError();
    if (r == hipSuccess) e->rew.parts_valid = true;
    return r;
}

static int do_step(ca_env* e, const float* actions, uint32_t flags) {
    { const int rs = overflow_status(e, "step"); if (rs) return rs; }
    prof_cadence(e, 1);
    const bool terms = actions != nullptr && e->rew.on;   // (a step that writes the reward from actions: ca_reward_configure)
    if (terms) HIPCHK(e, launch_reward_begin(e, flags));
    StepArgs a;
    fill_args(e, a, actions, flags);
    HIPCHK(e, launch_step(e, a));
    if (terms) HIPCHK(e, launch_reward_terms(e, flags, false));
    e->orient_valid = true;
    if (flags & CA_F_OBS) HIPCHK(e, launch_obs(e));
    e->steps_done += 1;
    return CA_OK;
}

// The one-launch rollout's loop, for every call that has one (DESIGN.md 7q lists them and their conditions): `steps` steps in launches
// of at most CA_ROLLOUT_MAX_T, the workgroup that owns an arena keeping it in registers / LDS for all the steps of a launch
// (ca_quad.h).  Bounded, so that a long rollout stays a sequence of kernels of a few milliseconds (a kernel cannot be interrupted, and
// a watchdog may reset a GPU over one that runs for seconds).  chunk(done) launches a.T steps behind the `done` the call has made;
// lone(done) makes a last launch of one step, which is a step and not a rollout: the caller passes `chunk` again where the same launch
// serves.  Both return a CA_ code.  The loop owns the sampling cadence, a.T, steps_done and orient_valid.
extern "C++" {   // (templates)
template <class Chunk, class Lone>
static int rollout_chunks(ca_env* e, StepArgs& a, int steps, const Chunk& chunk, const Lone& lone) {
    const uint64_t before = e->steps_done;
    for (int done = 0; done < steps; done += CA_ROLLOUT_MAX_T) {
        prof_cadence(e, CA_ROLLOUT_MAX_T);
        a.T = steps - done < CA_ROLLOUT_MAX_T ? steps - done : CA_ROLLOUT_MAX_T;
        const int rc = a.T == 1 ? lone(done) : chunk(done);
        if (rc) return rc;
        e->steps_done = before + (uint64_t)(done + a.T);   // (set, not added: a lone step that went through ca_alan_step has counted itself)
        e->orient_valid = true;
    }
    return CA_OK;
}
}  // extern "C++"

int ca_step(ca_env* e, const float* actions, uint32_t flags) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_step(e, actions, flags & ~CA_F_CONTACT));
    if (!e) return CA_EINVAL;
    if (!actions) return fail(e, CA_EINVAL, "ca_step: actions is null (use ca_orca_step for the ORCA-only step)");
    if (flags & CA_F_NODONE) return fail(e, CA_EINVAL, "ca_step: CA_F_NODONE applies to ca_orca_step only");
    HIPCHK(e, hipSetDevice(e->device));
    return do_step(e, actions, flags);
}

int ca_step_host(ca_env* e, const float* actions_host, uint32_t flags) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_step_host(e, actions_host, flags & ~CA_F_CONTACT));
    if (!e) return CA_EINVAL;
    if (!actions_host) return fail(e, CA_EINVAL, "ca_step_host: actions is null");
    if (flags & CA_F_NODONE) return fail(e, CA_EINVAL, "ca_step_host: CA_F_NODONE applies to ca_orca_step only");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(e->tmp_x, actions_host, AN(e) * 4, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // the caller's buffer may be reused right away
    return do_step(e, e->tmp_x, flags);
}

/* The host-array form of a step with ONE round trip: actions in (or NULL: the ORCA-only step), then observation | reward |
 * arena_done | step_count out in one copy, one synchronisation at the end.  The shape the reference's callers use -- one
 * environment per worker, results wanted on the host every step (run_rllib.py:77, 108; env.py:367-416) -- is latency:
 * ca_step_host + three ca_get cost four synchronisations.  Buffers from ca_host_alloc are page-locked AND device-visible: such
 * an action buffer is read by the kernel where it lies (no staging copy). */
int ca_step_packed(ca_env* e, const float* actions_host, uint32_t flags, void* out_host, size_t out_bytes) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_step_packed(e, actions_host, flags & ~CA_F_CONTACT, out_host, out_bytes));
    if (!e || !out_host) return fail(e, CA_EINVAL, "ca_step_packed: null argument");
    const size_t an = AN(e), A = (size_t)e->cfg.n_arenas;
    const size_t obs_b = an * CA_OBS_DIM * 4, rest_b = an * 4 + 2 * A * 4;
    if (out_bytes != obs_b + rest_b) return fail(e, CA_ESIZE, "ca_step_packed: need %zu bytes, got %zu", obs_b + rest_b, out_bytes);
    if (actions_host && (flags & CA_F_NODONE)) return fail(e, CA_EINVAL, "ca_step_packed: CA_F_NODONE applies to the ORCA-only step");
    HIPCHK(e, hipSetDevice(e->device));
    const float* act = nullptr;
    if (actions_host) {
        bool mapped = false;
        for (const auto& h : e->host_allocs)   // a ca_host_alloc buffer holding the whole action array: device-visible as it is
            if ((const char*)actions_host >= (const char*)h.first && (const char*)actions_host + an * 4 <= (const char*)h.first + h.second) { mapped = true; break; }
        if (mapped) act = actions_host;
        else {
            HIPCHK(e, hipMemcpyAsync(e->tmp_x, actions_host, an * 4, hipMemcpyHostToDevice, e->stream));
            act = e->tmp_x;
        }
    }
    const int rc = do_step(e, act, flags);
    if (rc) return rc;
    char* out = (char*)out_host;
    if (!e->obs_external) {
        HIPCHK(e, hipMemcpyAsync(out, e->slab, obs_b + rest_b, hipMemcpyDeviceToHost, e->stream));
    } else {
        HIPCHK(e, hipMemcpyAsync(out, e->obs, obs_b, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipMemcpyAsync(out + obs_b, e->reward, rest_b, hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));   // (also the point from which the caller may reuse its action buffer)
    return overflow_status(e, "ca_step_packed");       // (this very step's lists included: the stream is idle)
}

int ca_orca_step(ca_env* e, uint32_t flags) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_orca_step(e, flags & ~CA_F_CONTACT));
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    return do_step(e, nullptr, flags);
}

// (cos, sin) of atan2(y, x) = the normalised vector (ALAN:592-595); a zero-length action keeps the goal direction
static void alan_unit(double x, double y, double* c, double* s) {
    const double len = std::sqrt(x * x + y * y);
    *c = len == 0.0 ? 1.0 : x / len;
    *s = len == 0.0 ? 0.0 : y / len;
}

// Fresh bandit state for nA actions per agent (weights and times zeroed), then the kernels' arguments; the caller has filled
// act_c / act_s (one set) or h_act_tab / h_act_n (per arena) and set alan_per.
static int alan_install(ca_env* e, int nA, double temp, double timewindow, double time_step) {
    for (double** b : {&e->alan_w, &e->alan_t, &e->alan_dirs, &e->alan_u}) { if (*b) hipFree(*b); *b = nullptr; }
    if (e->alan_action) { hipFree(e->alan_action); e->alan_action = nullptr; }
    const size_t an = AN(e);
    HIPCHK(e, dalloc(e, &e->alan_w, an * (size_t)nA));
    HIPCHK(e, dalloc(e, &e->alan_t, an * (size_t)nA));
    HIPCHK(e, dalloc(e, &e->alan_dirs, an * 4));
    HIPCHK(e, dalloc(e, &e->alan_u, an));
    HIPCHK(e, dalloc(e, &e->alan_action, an));
    if (e->alan_per) {
        const size_t A = (size_t)e->cfg.n_arenas;
        if (!e->d_act_tab) HIPCHK(e, hipMalloc((void**)&e->d_act_tab, A * CA_ALAN_MAX_ACTIONS * sizeof(double2)));
        if (!e->d_act_n) HIPCHK(e, hipMalloc((void**)&e->d_act_n, A * sizeof(int)));
        HIPCHK(e, hipMemcpyAsync(e->d_act_tab, e->h_act_tab.data(), A * CA_ALAN_MAX_ACTIONS * sizeof(double2),
                                 hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipMemcpyAsync(e->d_act_n, e->h_act_n.data(), A * sizeof(int), hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->n_actions = nA;
    e->alan_temp = temp; e->alan_window = timewindow; e->alan_dt = time_step;
    {   // the same arguments for the kernels that run the bandit inside their launch (ca_quad.h, ca_step.h)
        if (!e->d_alan) HIPCHK(e, hipMalloc((void**)&e->d_alan, sizeof(AlanCold)));
        AlanCold h;
        memset(&h, 0, sizeof h);
        h.w = e->alan_w; h.t = e->alan_t; h.action = e->alan_action; h.reward = e->reward;
        memcpy(h.act_c, e->act_c, sizeof h.act_c); memcpy(h.act_s, e->act_s, sizeof h.act_s);
        h.temp = temp; h.window = timewindow; h.dt = time_step; h.reward_scale = e->cfg.reward_scale; h.nA = nA;
        h.tab = e->alan_per ? e->d_act_tab : nullptr;
        h.tab_n = e->alan_per ? e->d_act_n : nullptr;
        HIPCHK(e, upload(e, e->d_alan, &h, sizeof h));
    }
    return alan_pick(e);
}

int ca_alan_configure(ca_env* e, const double* actions_xy, int32_t n_actions, double temp, double timewindow,
                      double time_step) {
    if (!e || !actions_xy) return fail(e, CA_EINVAL, "ca_alan_configure: null argument");
    if (e->ac) return fail(e, CA_EINVAL, "ca_alan_configure: ALAN is not supported while per-arena agent counts are set");
    if (n_actions < 1 || n_actions > CA_ALAN_MAX_ACTIONS)
        return fail(e, CA_ERANGE, "ca_alan_configure: n_actions=%d out of range 1..%d", n_actions, CA_ALAN_MAX_ACTIONS);
    if (!(temp > 0.0) || !(timewindow > 0.0) || !(time_step > 0.0))
        return fail(e, CA_EINVAL, "ca_alan_configure: temp, timewindow and time_step must be positive");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->n_actions = 0;
    for (int k = 0; k < n_actions; ++k) alan_unit(actions_xy[2 * k], actions_xy[2 * k + 1], &e->act_c[k], &e->act_s[k]);
    e->alan_per = false;   // (back to one set for every arena)
    return alan_install(e, n_actions, temp, timewindow, time_step);
}

int ca_alan_configure_per_arena(ca_env* e, const double* actions_xy, const int32_t* n_actions, double temp, double timewindow,
                                double time_step) {
    if (!e || !actions_xy || !n_actions) return fail(e, CA_EINVAL, "ca_alan_configure_per_arena: null argument");
    if (e->ac) return fail(e, CA_EINVAL, "ca_alan_configure_per_arena: ALAN is not supported while per-arena agent counts are set");
    const int A = e->cfg.n_arenas;
    int nmax = 0;
    for (int a = 0; a < A; ++a) {
        if (n_actions[a] < 1 || n_actions[a] > CA_ALAN_MAX_ACTIONS)
            return fail(e, CA_ERANGE, "ca_alan_configure_per_arena: n_actions[%d]=%d out of range 1..%d", a, n_actions[a],
                        CA_ALAN_MAX_ACTIONS);
        nmax = n_actions[a] > nmax ? n_actions[a] : nmax;
    }
    if (!(temp > 0.0) || !(timewindow > 0.0) || !(time_step > 0.0))
        return fail(e, CA_EINVAL, "ca_alan_configure_per_arena: temp, timewindow and time_step must be positive");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->n_actions = 0;
    e->h_act_tab.assign((size_t)A * CA_ALAN_MAX_ACTIONS * 2, 0.0);
    e->h_act_n.assign(n_actions, n_actions + A);
    size_t off = 0;
    for (int a = 0; a < A; ++a)
        for (int k = 0; k < n_actions[a]; ++k, ++off) {
            double* cs = &e->h_act_tab[((size_t)a * CA_ALAN_MAX_ACTIONS + k) * 2];
            alan_unit(actions_xy[2 * off], actions_xy[2 * off + 1], cs, cs + 1);
        }
    e->alan_per = true;
    return alan_install(e, nmax, temp, timewindow, time_step);
}

int ca_alan_actions_arena(ca_env* e, int32_t arena, double* cs_xy, int32_t cap, int32_t* n_out) {
    if (!e || !n_out) return fail(e, CA_EINVAL, "ca_alan_actions_arena: null argument");
    if (arena < 0 || arena >= e->cfg.n_arenas)
        return fail(e, CA_ERANGE, "ca_alan_actions_arena: arena %d of %d", arena, e->cfg.n_arenas);
    if (e->n_actions <= 0) return fail(e, CA_EINVAL, "ca_alan_actions_arena: call ca_alan_configure first");
    const int n = e->alan_per ? e->h_act_n[arena] : e->n_actions;
    *n_out = n;
    if (!cs_xy) return CA_OK;
    for (int k = 0; k < n && k < cap; ++k) {
        if (e->alan_per) {
            cs_xy[2 * k] = e->h_act_tab[((size_t)arena * CA_ALAN_MAX_ACTIONS + k) * 2];
            cs_xy[2 * k + 1] = e->h_act_tab[((size_t)arena * CA_ALAN_MAX_ACTIONS + k) * 2 + 1];
        } else {
            cs_xy[2 * k] = e->act_c[k]; cs_xy[2 * k + 1] = e->act_s[k];
        }
    }
    return CA_OK;
}

// the refusals of an ALAN step, for the calls that make them up front (ca_alan_rollout makes the first alone and leaves the others to
// the steps it falls back to)
static int alan_refusals(ca_env* e, const char* who, uint32_t flags) {
    if (e->ac) return fail(e, CA_EINVAL, "%s: ALAN is not supported while per-arena agent counts are set", who);
    if (e->n_actions <= 0) return fail(e, CA_EINVAL, "%s: call ca_alan_configure first", who);
    if (flags & (CA_F_AUTORESET | CA_F_NODONE)) return fail(e, CA_EINVAL, "%s: CA_F_AUTORESET / CA_F_NODONE do not apply (ALAN:106-123)", who);
    return CA_OK;
}

int ca_alan_step(ca_env* e, const double* u, int32_t u_is_device, uint32_t flags) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_alan_step(e, u, u_is_device, flags & ~CA_F_CONTACT));
    if (!e) return CA_EINVAL;
    { const int rc = alan_refusals(e, "ca_alan_step", flags); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    { const int rs = overflow_status(e, "ca_alan_step"); if (rs) return rs; }
    if (u && !u_is_device) {  // stage the caller's host uniforms
        HIPCHK(e, hipMemcpyAsync(e->alan_u, u, AN(e) * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        u = e->alan_u;
    }
    prof_cadence(e, 1);
    if ((e->alan_fused && e->quad) || e->alan_lane) {   // ONE launch: the bandit runs inside the solve kernel (ca_quad.h / ca_step.h)
        StepArgs a;
        fill_args(e, a, nullptr, flags);
        a.alan = e->d_alan; a.alan_u = u;
        HIPCHK(e, launch_step(e, a));
        e->orient_valid = true;
        if (flags & CA_F_OBS) HIPCHK(e, launch_obs(e));
        e->steps_done += 1;
        return CA_OK;
    }
    const ca_config& c = e->cfg;
    AlanArgs p;
    p.pos_x = e->pos_x; p.pos_y = e->pos_y; p.vel_x = e->vel_x; p.vel_y = e->vel_y;
    p.goal_x = e->goal_x; p.goal_y = e->goal_y; p.pref_x = e->pref_x; p.pref_y = e->pref_y; p.reward = e->reward;
    p.w = e->alan_w; p.t = e->alan_t; p.action = e->alan_action; p.dirs = e->alan_dirs; p.u = u;
    p.step_count = e->step_count; p.arena_done = e->arena_done; p.episode = e->episode; p.arena_stats = e->arena_stats;
    memcpy(p.act_c, e->act_c, sizeof p.act_c);
    memcpy(p.act_s, e->act_s, sizeof p.act_s);
    p.tab = e->alan_per ? e->d_act_tab : nullptr; p.tab_n = e->alan_per ? e->d_act_n : nullptr;
    p.temp = e->alan_temp; p.window = e->alan_window; p.dt = e->alan_dt; p.reward_scale = c.reward_scale;
    p.seed = c.seed; p.arena_offset = c.arena_offset; p.A = c.n_arenas; p.N = c.n_agents; p.nA = e->n_actions;
    p.flags = flags;
    const dim3 grid((unsigned)((AN(e) + ALAN_BS - 1) / ALAN_BS)), block(ALAN_BS);
    {
        ProfScope ps(e, KIND_RESET);
        if (e->alan_per) launch_k(ps, alan_select_kernel<2>, grid, block, (size_t)e->n_actions * ALAN_BS * 8, e->stream, p);
        else launch_k(ps, alan_select_kernel<1>, grid, block, (size_t)e->n_actions * ALAN_BS * 8, e->stream, p);
    }
    HIPCHK(e, hipGetLastError());
    StepArgs a;
    fill_args(e, a, nullptr, flags);  // sim.doStep() + ALAN:118-121 = the ORCA-mode step
    HIPCHK(e, launch_step(e, a));
    {
        ProfScope ps(e, KIND_RESET);
        if (e->alan_per) launch_k(ps, alan_update_kernel<2>, grid, block, 0, e->stream, p);
        else launch_k(ps, alan_update_kernel<1>, grid, block, 0, e->stream, p);
    }
    HIPCHK(e, hipGetLastError());
    e->orient_valid = true;
    if (flags & CA_F_OBS) HIPCHK(e, launch_obs(e));
    e->steps_done += 1;
    return CA_OK;
}

// a lone last step of a fused ALAN rollout (a.T == 1) is a step, not a rollout: the handle's step kernel takes it -- ca_alan_step, unless
// that kernel is the four-lanes one the rollout runs on anyway
static int alan_lone_step(ca_env* e, const StepArgs& a, uint32_t flags) {
    if (!e->quad) return ca_alan_step(e, nullptr, 0, flags);
    HIPCHK(e, launch_step(e, a));
    return CA_OK;
}

int ca_alan_rollout(ca_env* e, int32_t steps, uint32_t flags) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_alan_rollout(e, steps, flags & ~CA_F_CONTACT));
    if (!e || steps < 0) return fail(e, CA_EINVAL, "ca_alan_rollout: bad argument");
    if (e->ac) return fail(e, CA_EINVAL, "ca_alan_rollout: ALAN is not supported while per-arena agent counts are set");
    { const int rs = overflow_status(e, "ca_alan_rollout"); if (rs) return rs; }
    if (e->n_actions > 0 && e->alan_fused && e->quad_roll && !(flags & (CA_F_OBS | CA_F_AUTORESET | CA_F_NODONE)) && steps > 1) {
        // run_sim(mode=1) (ALAN:106-123) as ONE launch per CA_ROLLOUT_MAX_T steps: select -> doStep -> update for every step
        // inside the four-lanes kernel, weights and times resident in LDS (ca_quad.h)
        HIPCHK(e, hipSetDevice(e->device));
        StepArgs a;
        fill_args(e, a, nullptr, flags);
        a.alan = e->d_alan;
        return rollout_chunks(e, a, steps, [&](int) -> int { HIPCHK(e, launch_step(e, a)); return CA_OK; },   // (the four-lanes kernel: alan_fused)
                              [&](int) -> int { return alan_lone_step(e, a, flags); });
    }
    for (int s = 0; s < steps; ++s) {
        const int rc = ca_alan_step(e, nullptr, 0, flags);
        if (rc) return rc;
    }
    return CA_OK;
}

int ca_observe(ca_env* e) {
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_obs(e));
    return CA_OK;
}

int ca_contacts(ca_env* e) {
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_contacts(e));
    return CA_OK;
}

int ca_get_contacts(ca_env* e, int32_t* agents, int32_t* wall, int32_t* nearest, float* nearest_d2, float* wall_d2, size_t bytes_each,
                    int32_t dst_is_device) {
    if (!e) return CA_EINVAL;
    const size_t an = AN(e);
    if (bytes_each != an * 4) return fail(e, CA_ESIZE, "ca_get_contacts: a plane holds %zu bytes, got %zu", an * 4, bytes_each);
    if (!e->contact_valid)
        return fail(e, CA_EINVAL, "ca_get_contacts: no contact report has been computed on this handle (ca_contacts, or a step with "
                                  "CA_F_CONTACT)");
    HIPCHK(e, hipSetDevice(e->device));
    void* dst[5] = {agents, wall, nearest, nearest_d2, wall_d2};
    for (int k = 0; k < 5; ++k)
        if (dst[k])
            HIPCHK(e, hipMemcpyAsync(dst[k], e->contact + (size_t)k * an, bytes_each,
                                     dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, e->stream));
    if (!dst_is_device) HIPCHK(e, hipStreamSynchronize(e->stream));
    return CA_OK;
}

int ca_contacts_ptr(ca_env* e, void** dev_ptr, size_t* bytes) {
    if (!e || !dev_ptr) return fail(e, CA_EINVAL, "ca_contacts_ptr: null argument");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, contact_buffer(e));
    *dev_ptr = e->contact;
    if (bytes) *bytes = 5 * AN(e) * 4;
    return CA_OK;
}

int ca_rollout(ca_env* e, int32_t steps, uint32_t flags) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_rollout(e, steps, flags & ~CA_F_CONTACT));
    if (!e || steps < 0) return fail(e, CA_EINVAL, "ca_rollout: bad argument");
    HIPCHK(e, hipSetDevice(e->device));
    { const int rs = overflow_status(e, "ca_rollout"); if (rs) return rs; }
    if (e->quad_roll && !(flags & CA_F_OBS) && steps > 1) {   // ONE launch per CA_ROLLOUT_MAX_T steps (rollout_chunks)
        StepArgs a;
        fill_args(e, a, nullptr, flags);
        const auto chunk = [&](int) -> int { HIPCHK(e, launch_step(e, a)); return CA_OK; };
        return rollout_chunks(e, a, steps, chunk, chunk);
    }
    for (int s = 0; s < steps; ++s) {
        const int rc = do_step(e, nullptr, flags);
        if (rc) return rc;
    }
    return CA_OK;
}

// ---- recording rollouts (include/ca_env.h ca_trace) -------------------------------------------------------------------------
struct TracePlan { int R, C; };
// every refusal of the two calls, before anything is launched
static int trace_check(ca_env* e, const char* who, int32_t steps, const ca_trace* tr, TracePlan* pl) {
    if (!e || steps < 0) return fail(e, CA_EINVAL, "%s: bad argument", who);
    if (!tr || !tr->agents) return fail(e, CA_EINVAL, "%s: the trace or its agents buffer is null", who);
    if (tr->every < 1) return fail(e, CA_EINVAL, "%s: every=%d, must be at least 1", who, tr->every);
    if (tr->channels == 0u || (tr->channels & ~(CA_TRACE_POS | CA_TRACE_VEL)) != 0u)
        return fail(e, CA_EINVAL, "%s: channels=0x%x, must be CA_TRACE_POS (1), CA_TRACE_VEL (2) or both", who, tr->channels);
    pl->R = steps / tr->every;
    pl->C = ((tr->channels & CA_TRACE_POS) ? 2 : 0) + ((tr->channels & CA_TRACE_VEL) ? 2 : 0);
    const size_t need_ag = (size_t)pl->R * (size_t)pl->C * AN(e) * 4, need_ar = (size_t)pl->R * 3 * (size_t)e->cfg.n_arenas * 4;
    if (tr->agents_bytes < need_ag)
        return fail(e, CA_ESIZE, "%s: the agents buffer needs %zu bytes (f32 [R=%d, C=%d, A=%d, N=%d]), got %zu", who, need_ag, pl->R, pl->C,
                    e->cfg.n_arenas, e->cfg.n_agents, tr->agents_bytes);
    if (tr->arenas && tr->arenas_bytes < need_ar)
        return fail(e, CA_ESIZE, "%s: the arenas buffer needs %zu bytes (i32 [R=%d, 3, A=%d]), got %zu", who, need_ar, pl->R, e->cfg.n_arenas,
                    tr->arenas_bytes);
    return CA_OK;
}
// record r by the record kernel: behind the launches of a step (kind 3 for ca_profile)
static hipError_t launch_trace_record(ca_env* e, const ca_trace* tr, const TracePlan& pl, int r) {
    if (r >= pl.R) return hipSuccess;
    TraceRecArgs t;
    int c = 0;
    for (int k = 0; k < 4; ++k) t.src[k] = nullptr;
    if (tr->channels & CA_TRACE_POS) { t.src[c++] = e->pos_x; t.src[c++] = e->pos_y; }
    if (tr->channels & CA_TRACE_VEL) { t.src[c++] = e->vel_x; t.src[c++] = e->vel_y; }
    t.words[0] = e->step_count; t.words[1] = e->arena_done; t.words[2] = e->episode;
    t.an = (unsigned)AN(e); t.A = e->cfg.n_arenas; t.C = pl.C;
    t.agents = (float*)tr->agents + (size_t)r * pl.C * t.an;
    t.arenas = tr->arenas ? (int*)tr->arenas + (size_t)r * 3 * t.A : nullptr;
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, trace_record_kernel, dim3((t.an + 255) / 256), dim3(256), 0, e->stream, t);
    return hipGetLastError();
}
// behind the launches of step s of a call that makes a step at a time: the record kernel behind every `every`-th
static hipError_t launch_trace_behind(ca_env* e, const ca_trace* tr, const TracePlan& pl, int s) {
    return (s + 1) % tr->every == 0 ? launch_trace_record(e, tr, pl, (s + 1) / tr->every - 1) : hipSuccess;
}
// the cursor of a Trace launch of the four-lanes kernel that follows `done` steps of the rollout
static hipError_t launch_trace_setup(ca_env* e, const ca_trace* tr, const TracePlan& pl, int done) {
    TraceDev v;
    v.agents = (float*)tr->agents; v.arenas = (int*)tr->arenas; v.an = (unsigned)AN(e); v.A = e->cfg.n_arenas;
    v.R = pl.R; v.C = pl.C; v.channels = tr->channels; v.every = tr->every;
    v.next = done / tr->every; v.countdown = tr->every - done % tr->every;
    hipLaunchKernelGGL(trace_setup_kernel, dim3(1), dim3(64), 0, e->stream, e->d_trace, v);
    return hipGetLastError();
}
// a T-step launch of the four-lanes kernel that records (a.T > 1)
static hipError_t launch_step_traced(ca_env* e, const StepArgs& a, const ca_trace* tr, const TracePlan& pl, int done) {
    hipError_t r = allow_lds(solve_launch(e, a.alan != nullptr, true, true));
    if (r == hipSuccess) r = launch_trace_setup(e, tr, pl, done);
    if (r != hipSuccess) return r;
    e->trace_on = true;
    r = launch_step(e, a);
    e->trace_on = false;
    return r;
}

int ca_rollout_trace(ca_env* e, int32_t steps, uint32_t flags, const ca_trace* tr) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_rollout_trace(e, steps, flags & ~CA_F_CONTACT, tr));
    TracePlan pl;
    { const int rc = trace_check(e, "ca_rollout_trace", steps, tr, &pl); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    { const int rs = overflow_status(e, "ca_rollout_trace"); if (rs) return rs; }
    if (e->quad_roll && !(flags & CA_F_OBS) && steps > 1) {   // ca_rollout's one-launch form, its Trace instantiation
        StepArgs a;
        fill_args(e, a, nullptr, flags);
        return rollout_chunks(e, a, steps, [&](int done) -> int { HIPCHK(e, launch_step_traced(e, a, tr, pl, done)); return CA_OK; },
                              [&](int done) -> int {   // (a lone last step is the launch ca_rollout makes, and the record kernel behind it)
                                  HIPCHK(e, launch_step(e, a));
                                  HIPCHK(e, launch_trace_behind(e, tr, pl, done));
                                  return CA_OK;
                              });
    }
    for (int s = 0; s < steps; ++s) {   // a sequence of launches per step: the record kernel behind those of every `every`-th
        const int rc = do_step(e, nullptr, flags);
        if (rc) return rc;
        HIPCHK(e, launch_trace_behind(e, tr, pl, s));
    }
    return CA_OK;
}

int ca_alan_rollout_trace(ca_env* e, int32_t steps, uint32_t flags, const ca_trace* tr) {
    if (e && (flags & CA_F_CONTACT)) return contacts_behind(e, ca_alan_rollout_trace(e, steps, flags & ~CA_F_CONTACT, tr));
    TracePlan pl;
    { const int rc = trace_check(e, "ca_alan_rollout_trace", steps, tr, &pl); if (rc) return rc; }
    { const int rc = alan_refusals(e, "ca_alan_rollout_trace", flags); if (rc) return rc; }
    { const int rs = overflow_status(e, "ca_alan_rollout_trace"); if (rs) return rs; }
    // (an action set per arena records in the per-step form: no Trace twin of the AlanArenaSets instantiations)
    if (e->alan_fused && e->quad_roll && !e->alan_per && !(flags & CA_F_OBS) && steps > 1) {
        HIPCHK(e, hipSetDevice(e->device));
        StepArgs a;
        fill_args(e, a, nullptr, flags);
        a.alan = e->d_alan;
        return rollout_chunks(e, a, steps, [&](int done) -> int { HIPCHK(e, launch_step_traced(e, a, tr, pl, done)); return CA_OK; },
                              [&](int done) -> int {   // (a lone last step: what ca_alan_rollout does with it, and the record kernel behind it)
                                  const int rc = alan_lone_step(e, a, flags);
                                  if (rc) return rc;
                                  HIPCHK(e, launch_trace_behind(e, tr, pl, done));
                                  return CA_OK;
                              });
    }
    for (int s = 0; s < steps; ++s) {
        const int rc = ca_alan_step(e, nullptr, 0, flags);
        if (rc) return rc;
        HIPCHK(e, launch_trace_behind(e, tr, pl, s));
    }
    return CA_OK;
}

// ---- action-sequence rollouts (include/ca_env.h ca_action_seq) --------------------------------------------------------------
struct ActSeqPlan { int* first_done; int* entry_frozen; };
// The refusals that the sequence calls share -- ca_rollout_actions, ca_rollout_policy and their navigated forms, `who` -- in the two
// groups and the order that all of them make them in; Seq is ca_action_seq or ca_policy_seq, whose members of one name mean one thing.
extern "C++" {   // (templates)
template <class Seq>
static int seq_check_call(ca_env* e, const char* who, int32_t steps, uint32_t flags, const Seq* seq) {
    if (steps < 0) return fail(e, CA_EINVAL, "%s: steps=%d", who, steps);
    if (seq->hold < 1) return fail(e, CA_EINVAL, "%s: hold=%d, must be at least 1", who, seq->hold);
    if (flags & CA_F_NODONE) return fail(e, CA_EINVAL, "%s: CA_F_NODONE applies to ca_orca_step only", who);
    if (flags & ~(CA_F_OBS | CA_F_STATS | CA_F_AUTORESET | CA_F_FREEZE | CA_F_CONTACT))
        return fail(e, CA_EINVAL, "%s: flags=0x%x holds a bit this call does not know", who, flags);
    return CA_OK;
}
template <class Seq>
static int seq_check_results(ca_env* e, const char* who, int32_t steps, const Seq* seq) {
    const size_t A = (size_t)e->cfg.n_arenas, an = AN(e), T = (size_t)steps;
    const int Ai = e->cfg.n_arenas, Ni = e->cfg.n_agents;
    if (seq->weights && seq->weights_bytes < T * 4)
        return fail(e, CA_ESIZE, "%s: the weights buffer needs %zu bytes (f32 [steps=%d]), got %zu", who, T * 4, steps, seq->weights_bytes);
    if (seq->returns && seq->returns_bytes < an * 4)
        return fail(e, CA_ESIZE, "%s: the returns buffer needs %zu bytes (f32 [A=%d, N=%d]), got %zu", who, an * 4, Ai, Ni, seq->returns_bytes);
    if (seq->first_done && seq->first_done_bytes < A * 4)
        return fail(e, CA_ESIZE, "%s: the first_done buffer needs %zu bytes (i32 [A=%d]), got %zu", who, A * 4, Ai, seq->first_done_bytes);
    return CA_OK;
}
}  // extern "C++"
// every refusal of an action-sequence call, before anything is launched
static int actseq_check(ca_env* e, const char* who, int32_t steps, uint32_t flags, const ca_action_seq* seq) {
    if (!seq || !seq->actions) return fail(e, CA_EINVAL, "%s: the sequence or its actions buffer is null", who);
    { const int rc = seq_check_call(e, who, steps, flags, seq); if (rc) return rc; }
    const size_t R = ((size_t)steps + (size_t)seq->hold - 1) / (size_t)seq->hold;
    if (seq->actions_bytes < R * AN(e) * 4)
        return fail(e, CA_ESIZE, "%s: the actions buffer needs %zu bytes (f32 [R=%zu, A=%d, N=%d], R = ceil(steps / hold)), got %zu", who,
                    R * AN(e) * 4, R, e->cfg.n_arenas, e->cfg.n_agents, seq->actions_bytes);
    return seq_check_results(e, who, steps, seq);
}
// In front of the first step of a sequence call: the handle's words on first use, the plan -- first_done is the caller's or the handle's
// own, entry_frozen only where a launch behind each step reads it --, the sampling cadence and the set-up launch: returns = +0,
// first_done = -1, the arenas frozen at entry (kind 3 for ca_profile, like the record kernel).
static int actseq_prologue(ca_env* e, uint32_t flags, float* returns, int32_t* first_done, bool entry_frozen, ActSeqPlan* pl) {
    const size_t A = (size_t)e->cfg.n_arenas;
    if (!e->actseq_words) HIPCHK(e, dalloc(e, &e->actseq_words, 2 * A));
    pl->first_done = first_done ? (int*)first_done : e->actseq_words;
    pl->entry_frozen = entry_frozen ? e->actseq_words + A : nullptr;
    prof_cadence(e, 1);
    ActSeqBeginArgs b;
    b.arena_done = e->arena_done; b.returns = returns; b.first_done = pl->first_done; b.entry_frozen = pl->entry_frozen;
    b.an = (unsigned)AN(e); b.A = e->cfg.n_arenas; b.freeze = (flags & CA_F_FREEZE) ? 1 : 0;
    const unsigned n = b.an > (unsigned)b.A ? b.an : (unsigned)b.A;
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, actseq_begin_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, b);
    HIPCHK(e, hipGetLastError());
    return CA_OK;
}
// What a sequence call hands the launch behind its step t, whichever kernel that is (null members: not wanted): the one description
// that actseq_accumulate_kernel, policy_record_kernel and nav_reward_kernel take their share of the arguments of actseq_account from.
struct StepRec { const ActSeqPlan* pl; const float* weights; float* returns; float* rewards_out; int32_t* done_out; int t; uint32_t flags; };
extern "C++" {   // (templates)
template <class Args>   // (rec null: the launch behind a single step -- nav_reward_kernel knows it by a null first_done)
static void fill_step_rec(const ca_env* e, const StepRec* rec, Args& c) {
    c.arena_done = e->arena_done; c.entry_frozen = rec ? rec->pl->entry_frozen : nullptr;
    c.agent_counts = e->ac ? e->d_counts : nullptr;
    c.weight = rec && rec->weights ? rec->weights + rec->t : nullptr;
    c.returns = rec ? rec->returns : nullptr; c.first_done = rec ? rec->pl->first_done : nullptr;
    c.an = (unsigned)AN(e); c.N = e->cfg.n_agents; c.t = rec ? rec->t : 0; c.freeze = rec && (rec->flags & CA_F_FREEZE) ? 1 : 0;
}
template <class Args>   // (the kernels with the records of a policy rollout)
static void fill_step_records(const ca_env* e, const StepRec& rec, Args& c) {
    c.rewards_rec = rec.rewards_out ? rec.rewards_out + (size_t)rec.t * AN(e) : nullptr;
    c.done_rec = rec.done_out ? (int*)rec.done_out + (size_t)rec.t * e->cfg.n_arenas : nullptr;
}
}  // extern "C++"
// behind the launches of step t of the per-step form
static hipError_t launch_actseq_accumulate(ca_env* e, const StepRec& rec) {
    ActSeqAccArgs c;
    fill_step_rec(e, &rec, c);
    c.reward = e->reward; c.A = e->cfg.n_arenas;
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, actseq_accumulate_kernel, dim3((c.an + 255) / 256), dim3(256), 0, e->stream, c);
    return hipGetLastError();
}
// an ActionSeq launch of the four-lanes kernel that follows `done` steps of the call (a.T steps of it)
static hipError_t launch_step_actseq(ca_env* e, const StepArgs& a, const ca_action_seq* seq, const ActSeqPlan& pl, int done) {
    hipError_t r = allow_lds(solve_launch(e, false, true, false, true));
    if (r != hipSuccess) return r;
    ActSeqDev v;
    v.actions = seq->actions; v.weights = seq->weights; v.returns = seq->returns; v.first_done = pl.first_done;
    v.an = (unsigned)AN(e); v.hold = seq->hold; v.t0 = done; v.row = done / seq->hold; v.countdown = seq->hold - done % seq->hold;
    {
        ProfScope ps(e, KIND_RESET);
        launch_k(ps, actseq_setup_kernel, dim3(1), dim3(64), 0, e->stream, e->d_actseq, v);
    }
    r = hipGetLastError();
    if (r != hipSuccess) return r;
    e->actseq_on = true;
    r = launch_step(e, a);
    e->actseq_on = false;
    return r;
}

int ca_rollout_actions(ca_env* e, int32_t steps, uint32_t flags, const ca_action_seq* seq) {
    if (!e) return CA_EINVAL;
    { const int rc = actseq_check(e, "ca_rollout_actions", steps, flags, seq); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    { const int rs = overflow_status(e, "ca_rollout_actions"); if (rs) return rs; }
    const bool one_launch = e->quad_roll && !e->rew.on;   // (ca_solver_info: rollout_one_launch; an ALAN-configured handle steps without the bandit here; reward terms need the state between steps)
    ActSeqPlan pl;
    { const int rc = actseq_prologue(e, flags, seq->returns, seq->first_done, !one_launch, &pl); if (rc) return rc; }
    const uint32_t sf = flags & ~(CA_F_OBS | CA_F_CONTACT);   // (both: one launch behind the last step, launch_tail)
    if (one_launch) {
        // one launch per CA_ROLLOUT_MAX_T steps, as ca_rollout: the arena stays in registers / LDS, each step reads its own action
        StepArgs a;
        fill_args(e, a, seq->actions, sf);
        const auto chunk = [&](int done) -> int { HIPCHK(e, launch_step_actseq(e, a, seq, pl, done)); return CA_OK; };
        const int rc = rollout_chunks(e, a, steps, chunk, chunk);
        if (rc) return rc;
    } else {
        StepRec rec = {&pl, seq->weights, seq->returns, nullptr, nullptr, 0, flags};
        for (rec.t = 0; rec.t < steps; ++rec.t) {   // the launches of ca_step with this step's row, the accumulate kernel behind them
            const int rc = do_step(e, seq->actions + (size_t)(rec.t / seq->hold) * AN(e), sf);
            if (rc) return rc;
            HIPCHK(e, launch_actseq_accumulate(e, rec));
        }
    }
    return launch_tail(e, flags);
}

// ---- the policy and its rollouts (include/ca_env.h ca_policy_desc, ca_policy_seq) ---------------------------------------------------
// the heads go with the policy they were packed for (the stream is drained where this is called); the row-record buffers stay
static void drop_heads(ca_env* e) {
    if (e->heads.d_wp) hipFree(e->heads.d_wp);
    if (e->heads.d_bp) hipFree(e->heads.d_bp);
    e->heads.d_wp = e->heads.d_bp = nullptr;
    e->heads.on = e->heads.has_value = e->heads.has_logstd = false;
}
int ca_policy_configure(ca_env* e, const ca_policy_desc* d) {
    const char* who = "ca_policy_configure";
    if (!e || !d) return fail(e, CA_EINVAL, "%s: null argument", who);
    const int L = d->n_layers, A = e->cfg.n_arenas;
    if (L < 2 || L > CA_POLICY_MAX_LAYERS) return fail(e, CA_EINVAL, "%s: n_layers=%d, must be 2 .. %d", who, L, CA_POLICY_MAX_LAYERS);
    if (d->width[0] != CA_OBS_DIM) return fail(e, CA_EINVAL, "%s: width[0]=%d, must be CA_OBS_DIM = %d", who, d->width[0], CA_OBS_DIM);
    for (int l = 1; l < L; ++l)
        if (d->width[l] < 16 || d->width[l] > CA_POLICY_MAX_WIDTH || d->width[l] % 16 != 0)
            return fail(e, CA_EINVAL, "%s: width[%d]=%d, a hidden width is a multiple of 16 in 16 .. %d", who, l, d->width[l], CA_POLICY_MAX_WIDTH);
    if (d->width[L] != 1) return fail(e, CA_EINVAL, "%s: width[%d]=%d, the output layer has one unit", who, L, d->width[L]);
    if (d->out_mode != CA_POLICY_OUT_IDENTITY && d->out_mode != CA_POLICY_OUT_CLIP)
        return fail(e, CA_EINVAL, "%s: out_mode=%d", who, d->out_mode);
    if (d->out_mode == CA_POLICY_OUT_CLIP && !(d->out_limit >= 0.0f && std::isfinite(d->out_limit)))
        return fail(e, CA_EINVAL, "%s: out_limit=%g, must be finite and not negative", who, (double)d->out_limit);
    const int P = d->n_sets;
    if (P < 1) return fail(e, CA_EINVAL, "%s: n_sets=%d, must be at least 1", who, P);
    if (P > 1 && !d->set_of_arena) return fail(e, CA_EINVAL, "%s: n_sets=%d needs set_of_arena", who, P);
    for (int l = 0; l < L; ++l) {
        if (!d->weights[l] || !d->bias[l]) return fail(e, CA_EINVAL, "%s: weights[%d] or bias[%d] is null", who, l, l);
        const size_t wb = (size_t)P * d->width[l + 1] * d->width[l] * 4, bb = (size_t)P * d->width[l + 1] * 4;
        if (d->weights_bytes[l] < wb)
            return fail(e, CA_ESIZE, "%s: weights[%d] needs %zu bytes (f32 [P=%d, %d, %d]), got %zu", who, l, wb, P, d->width[l + 1], d->width[l], d->weights_bytes[l]);
        if (d->bias_bytes[l] < bb)
            return fail(e, CA_ESIZE, "%s: bias[%d] needs %zu bytes (f32 [P=%d, %d]), got %zu", who, l, bb, P, d->width[l + 1], d->bias_bytes[l]);
    }
    if (d->set_of_arena) {
        if (d->set_of_arena_bytes < (size_t)A * 4)
            return fail(e, CA_ESIZE, "%s: set_of_arena needs %zu bytes (i32 [A=%d]), got %zu", who, (size_t)A * 4, A, d->set_of_arena_bytes);
        for (int a = 0; a < A; ++a)
            if (d->set_of_arena[a] < 0 || d->set_of_arena[a] >= P)
                return fail(e, CA_ERANGE, "%s: arena %d asks for set %d of %d", who, a, d->set_of_arena[a], P);
    }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    // the caller's arrays on the host, checked; then the kernel's layout: a set is its layers one behind the other, a layer its
    // 16-column tiles (the output layer: one tile, columns 1 .. 15 zero), a tile its k-steps, a k-step 64 lanes
    std::vector<float> hw[CA_POLICY_MAX_LAYERS], hb[CA_POLICY_MAX_LAYERS];
    ca_env::Policy n;
    n.L = L; n.P = P; n.out_mode = d->out_mode; n.limit = d->out_limit;
    for (int l = 0; l <= L; ++l) { n.width[l] = d->width[l]; if (l < L && d->width[l] > n.maxw) n.maxw = d->width[l]; }
    for (int l = 0; l < L; ++l) {
        const size_t nw = (size_t)P * d->width[l + 1] * d->width[l], nb = (size_t)P * d->width[l + 1];
        hw[l].resize(nw); hb[l].resize(nb);
        if (d->src_is_device) {
            HIPCHK(e, download(e, hw[l].data(), d->weights[l], nw * 4));
            HIPCHK(e, download(e, hb[l].data(), d->bias[l], nb * 4));
        } else {
            memcpy(hw[l].data(), d->weights[l], nw * 4);
            memcpy(hb[l].data(), d->bias[l], nb * 4);
        }
        const size_t per = (size_t)d->width[l + 1] * d->width[l];
        for (size_t k = 0; k < nw; ++k)
            if (!std::isfinite(hw[l][k]))
                return fail(e, CA_ERANGE, "%s: layer %d, set %zu: weight [%zu, %zu] is not finite", who, l, k / per, (k % per) / d->width[l], k % d->width[l]);
        for (size_t k = 0; k < nb; ++k)
            if (!std::isfinite(hb[l][k]))
                return fail(e, CA_ERANGE, "%s: layer %d, set %zu: bias [%zu] is not finite", who, l, k / d->width[l + 1], k % d->width[l + 1]);
        const unsigned opad = l == L - 1 ? 16u : (unsigned)d->width[l + 1];
        n.wp_off[l] = n.wset; n.bp_off[l] = n.bset;
        n.wset += opad * (unsigned)d->width[l]; n.bset += opad;
    }
    std::vector<float> wp((size_t)P * n.wset, 0.0f), bp((size_t)P * n.bset, 0.0f);
    for (int p = 0; p < P; ++p)
        for (int l = 0; l < L; ++l) {
            const int K = d->width[l], O = d->width[l + 1], opad = l == L - 1 ? 16 : O;
            const float* W = hw[l].data() + (size_t)p * O * K;
            float* dst = wp.data() + (size_t)p * n.wset + n.wp_off[l];
            for (int jt = 0; jt < opad / 16; ++jt)
                for (int s = 0; s < K / 4; ++s)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int j = jt * 16 + (lane & 15), k = 4 * s + (lane >> 4);
                        dst[((size_t)jt * (K / 4) + s) * 64 + lane] = j < O ? W[(size_t)j * K + k] : 0.0f;
                    }
            for (int j = 0; j < O; ++j) bp[(size_t)p * n.bset + n.bp_off[l] + j] = hb[l][(size_t)p * O + j];
        }
    hipError_t r = hipMalloc((void**)&n.d_wp, wp.size() * 4);
    if (r == hipSuccess) r = hipMalloc((void**)&n.d_bp, bp.size() * 4);
    if (r == hipSuccess && P > 1) r = hipMalloc((void**)&n.d_set, (size_t)A * 4);
    if (r == hipSuccess) r = upload(e, n.d_wp, wp.data(), wp.size() * 4);
    if (r == hipSuccess) r = upload(e, n.d_bp, bp.data(), bp.size() * 4);
    if (r == hipSuccess && P > 1) r = upload(e, n.d_set, d->set_of_arena, (size_t)A * 4);
    n.act = e->pol.act;
    if (r == hipSuccess && !n.act) r = dalloc(e, &n.act, AN(e));
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    if (r != hipSuccess) {
        if (n.d_wp) hipFree(n.d_wp);
        if (n.d_bp) hipFree(n.d_bp);
        if (n.d_set) hipFree(n.d_set);
        if (n.act && !e->pol.act) hipFree(n.act);
        return fail(e, CA_EHIP, "%s: installing the weights failed: %s", who, hipGetErrorString(r));
    }
    if (e->pol.d_wp) hipFree(e->pol.d_wp);
    if (e->pol.d_bp) hipFree(e->pol.d_bp);
    if (e->pol.d_set) hipFree(e->pol.d_set);
    n.on = true;
    e->pol = n;
    drop_heads(e);
    return CA_OK;
}

int ca_policy_clear(ca_env* e) {
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->pol.d_wp) hipFree(e->pol.d_wp);
    if (e->pol.d_bp) hipFree(e->pol.d_bp);
    if (e->pol.d_set) hipFree(e->pol.d_set);
    float* act = e->pol.act;   // (kept for the next policy)
    e->pol = ca_env::Policy();
    e->pol.act = act;
    drop_heads(e);
    return CA_OK;
}

int ca_policy_info(ca_env* e, int32_t* configured, int32_t* n_layers, int32_t* width, int32_t* n_sets) {
    if (!e) return CA_EINVAL;
    if (configured) *configured = e->pol.on ? 1 : 0;
    if (n_layers) *n_layers = e->pol.on ? e->pol.L : 0;
    if (n_sets) *n_sets = e->pol.on ? e->pol.P : 0;
    if (width) for (int l = 0; l <= CA_POLICY_MAX_LAYERS; ++l) width[l] = e->pol.on && l <= e->pol.L ? e->pol.width[l] : 0;
    return CA_OK;
}

// the four rows of a policy launch (null members: not wanted; actions may be null for the heads only)
struct PolicyRows { const float* noise; float* actions; float* actions_rec; float* obs_rec; };
// The policy launch (kind 3 for ca_profile) for both instances of policy_kernel: the handle's observation buffer through the sets
// wp / bp (the policy's own, or the ones with the heads' output tile) into the rows; c is the argument block, p the PolicyArgs in it.
extern "C++" {   // (a template)
template <class Args>
static hipError_t launch_policy_args(ca_env* e, void (*kernel)(Args), Args& c, PolicyArgs& p, const float* wp, const float* bp, const PolicyRows& rows) {
    const ca_env::Policy& q = e->pol;
    p.obs = e->obs; p.wp = wp; p.bp = bp; p.set_of_arena = q.P > 1 ? q.d_set : nullptr;
    p.noise = rows.noise; p.actions = rows.actions; p.actions_rec = rows.actions_rec; p.obs_rec = rows.obs_rec;
    for (int l = 0; l < POLICY_MAX_LAYERS; ++l) { p.wp_off[l] = q.wp_off[l]; p.bp_off[l] = q.bp_off[l]; }
    for (int l = 0; l <= POLICY_MAX_LAYERS; ++l) p.width[l] = q.width[l];
    p.wset = q.wset; p.bset = q.bset;
    p.an = (unsigned)AN(e); p.N = e->cfg.n_agents;
    // one set: tiles of consecutive rows across arenas; a set per arena: a tile holds rows of one arena, padded (the same bits)
    p.tpa = q.P > 1 ? (p.N + POLICY_ROWS - 1) / POLICY_ROWS : 0;
    p.n_layers = q.L; p.stride = q.maxw + POLICY_PAD;
    p.clip = q.out_mode == CA_POLICY_OUT_CLIP ? 1 : 0; p.limit = q.limit;
    const unsigned grid = p.tpa ? (unsigned)e->cfg.n_arenas * (unsigned)p.tpa : (p.an + POLICY_ROWS - 1) / POLICY_ROWS;
    const size_t lds = (size_t)2 * POLICY_ROWS * p.stride * 4;
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, kernel, dim3(grid), dim3(64), lds, e->stream, c);
    return hipGetLastError();
}
}  // extern "C++"
static hipError_t launch_policy(ca_env* e, const PolicyRows& rows) {
    PolicyArgs p;
    return launch_policy_args(e, policy_kernel<false>, p, p, e->pol.d_wp, e->pol.d_bp, rows);
}
// the same on the sets with the heads' output tile: the records of ca_policy_eval, or the value column alone
static hipError_t launch_heads(ca_env* e, const PolicyRows& rows, const ca_policy_eval& o, bool values_only) {
    ActorCriticArgs c;
    c.logp = o.logp; c.value = o.value; c.mean = o.mean; c.log_std = o.log_std;
    c.has_logstd = e->heads.has_logstd ? 1 : 0; c.values_only = values_only ? 1 : 0;
    return launch_policy_args(e, policy_kernel<true>, c, c.p, e->heads.d_wp, e->heads.d_bp, rows);
}

int ca_policy_actions(ca_env* e, const float* noise, float* actions_out) {
    if (!e) return CA_EINVAL;
    if (!e->pol.on) return fail(e, CA_EINVAL, "ca_policy_actions: call ca_policy_configure first");
    if (!actions_out) return fail(e, CA_EINVAL, "ca_policy_actions: actions_out is null");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_policy(e, {noise, actions_out, nullptr, nullptr}));
    return CA_OK;
}

// every refusal of a policy-rollout call, before anything is launched
extern "C++" {   // (a template: Seq is ca_policy_seq or ca_policy_sample_seq, whose members of one name mean one thing)
template <class Seq>
static int policy_seq_check(ca_env* e, const char* who, int32_t steps, uint32_t flags, const Seq* seq) {
    if (!seq) return fail(e, CA_EINVAL, "%s: the sequence is null", who);
    if (!e->pol.on) return fail(e, CA_EINVAL, "%s: call ca_policy_configure first", who);
    { const int rc = seq_check_call(e, who, steps, flags, seq); if (rc) return rc; }
    if (seq->obs_out && ((uintptr_t)seq->obs_out & 15) != 0) return fail(e, CA_EINVAL, "%s: the obs_out buffer must be 16-byte aligned", who);
    const size_t R = ((size_t)steps + (size_t)seq->hold - 1) / (size_t)seq->hold, A = (size_t)e->cfg.n_arenas, an = AN(e), T = (size_t)steps;
    const int Ai = e->cfg.n_arenas, Ni = e->cfg.n_agents;
    if (seq->noise && seq->noise_bytes < R * an * 4)
        return fail(e, CA_ESIZE, "%s: the noise buffer needs %zu bytes (f32 [R=%zu, A=%d, N=%d], R = ceil(steps / hold)), got %zu", who, R * an * 4, R, Ai, Ni, seq->noise_bytes);
    { const int rc = seq_check_results(e, who, steps, seq); if (rc) return rc; }
    if (seq->obs_out && seq->obs_out_bytes < R * an * CA_OBS_DIM * 4)
        return fail(e, CA_ESIZE, "%s: the obs_out buffer needs %zu bytes (f32 [R=%zu, A=%d, N=%d, %d]), got %zu", who, R * an * CA_OBS_DIM * 4, R, Ai, Ni, CA_OBS_DIM, seq->obs_out_bytes);
    if (seq->actions_out && seq->actions_out_bytes < R * an * 4)
        return fail(e, CA_ESIZE, "%s: the actions_out buffer needs %zu bytes (f32 [R=%zu, A=%d, N=%d]), got %zu", who, R * an * 4, R, Ai, Ni, seq->actions_out_bytes);
    if (seq->rewards_out && seq->rewards_out_bytes < T * an * 4)
        return fail(e, CA_ESIZE, "%s: the rewards_out buffer needs %zu bytes (f32 [steps=%d, A=%d, N=%d]), got %zu", who, T * an * 4, steps, Ai, Ni, seq->rewards_out_bytes);
    if (seq->done_out && seq->done_out_bytes < T * A * 4)
        return fail(e, CA_ESIZE, "%s: the done_out buffer needs %zu bytes (i32 [steps=%d, A=%d]), got %zu", who, T * A * 4, steps, Ai, seq->done_out_bytes);
    return CA_OK;
}
}  // extern "C++"
// The row of actions that starts at step t (t a multiple of hold): what ca_observe launches, then the policy on what it left, into the
// handle's action buffer and the row's records.  heads: row t / hold of the records of a sampling rollout, which launches the heads
// (null: the policy alone).
extern "C++" {   // (templates: Seq as for policy_seq_check; the record launches lie between them)
template <class Seq>
static hipError_t launch_policy_row(ca_env* e, const Seq* seq, int t, const ca_policy_eval* heads) {
    const size_t r = (size_t)(t / seq->hold), an = AN(e);
    prof_cadence(e, 1);
    const hipError_t rc = launch_obs(e);
    if (rc != hipSuccess) return rc;
    const PolicyRows rows = {seq->noise ? seq->noise + r * an : nullptr, e->pol.act, seq->actions_out ? seq->actions_out + r * an : nullptr,
                             seq->obs_out ? seq->obs_out + r * an * CA_OBS_DIM : nullptr};
    return heads ? launch_heads(e, rows, *heads, false) : launch_policy(e, rows);
}
// behind the launches of step t: the return, first_done and the step's records (both record kernels take these)
static void fill_policy_rec(const ca_env* e, const StepRec& rec, PolicyRecArgs& c) {
    fill_step_rec(e, &rec, c);
    fill_step_records(e, rec, c);
    c.reward = e->reward; c.A = e->cfg.n_arenas;
}
static hipError_t launch_policy_record(ca_env* e, const StepRec& rec) {
    PolicyRecArgs c;
    fill_policy_rec(e, rec, c);
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, policy_record_kernel, dim3((c.an + 255) / 256), dim3(256), 0, e->stream, c);
    return hipGetLastError();
}
// the same behind a step of a sampling rollout, with row t / hold of the row records (null: not wanted)
static hipError_t launch_sample_record(ca_env* e, const StepRec& rec, int hold, float* row_rewards, int* row_done, int* row_valid) {
    const size_t r = (size_t)(rec.t / hold), an = AN(e), A = (size_t)e->cfg.n_arenas;
    SampleRecArgs c;
    fill_policy_rec(e, rec, c.s);
    c.row_rewards = row_rewards ? row_rewards + r * an : nullptr; c.row_done = row_done ? row_done + r * A : nullptr;
    c.row_valid = row_valid ? row_valid + r * A : nullptr; c.first = rec.t % hold == 0 ? 1 : 0;
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, sample_record_kernel, dim3((c.s.an + 255) / 256), dim3(256), 0, e->stream, c);
    return hipGetLastError();
}
// The loop of a policy rollout, for the three calls that have one: the set-up launch, then for every step the row where a row starts,
// the step and the record behind it.  row(t) is launch_policy_row; step(sf, rec) launches step t on the handle's action buffer and
// returns a CA_ code; record(rec) is the launch behind it.  The caller's launch_tail follows (the sampling rollout has launches in between).
template <class Seq, class Row, class Step, class Record>
static int policy_rollout_steps(ca_env* e, int steps, uint32_t flags, const Seq* seq, const Row& row, const Step& step, const Record& record) {
    ActSeqPlan pl;
    { const int rc = actseq_prologue(e, flags, seq->returns, seq->first_done, true, &pl); if (rc) return rc; }
    const uint32_t sf = flags & (CA_F_STATS | CA_F_AUTORESET | CA_F_FREEZE);   // (observation and contacts: one launch behind the last step, launch_tail)
    StepRec rec = {&pl, seq->weights, seq->returns, seq->rewards_out, seq->done_out, 0, flags};
    for (rec.t = 0; rec.t < steps; ++rec.t) {
        if (rec.t % seq->hold == 0) HIPCHK(e, row(rec.t));
        const int rc = step(sf, rec);
        if (rc) return rc;
        HIPCHK(e, record(rec));
    }
    return CA_OK;
}
}  // extern "C++"

int ca_rollout_policy(ca_env* e, int32_t steps, uint32_t flags, const ca_policy_seq* seq) {
    if (!e) return CA_EINVAL;
    { const int rc = policy_seq_check(e, "ca_rollout_policy", steps, flags, seq); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    { const int rs = overflow_status(e, "ca_rollout_policy"); if (rs) return rs; }
    const int rc = policy_rollout_steps(e, steps, flags, seq, [&](int t) { return launch_policy_row(e, seq, t, nullptr); },
                                        [&](uint32_t sf, const StepRec&) { return do_step(e, e->pol.act, sf); },
                                        [&](const StepRec& rec) { return launch_policy_record(e, rec); });
    return rc ? rc : launch_tail(e, flags);
}

// ---- PPO sample collection (include/ca_env.h ca_policy_heads, ca_policy_sample_seq, ca_gae_desc) -------------------
int ca_policy_set_heads(ca_env* e, const ca_policy_heads* d) {
    const char* who = "ca_policy_set_heads";
    if (!e || !d) return fail(e, CA_EINVAL, "%s: null argument", who);
    if (!e->pol.on) return fail(e, CA_EINVAL, "%s: call ca_policy_configure first", who);
    const ca_env::Policy& q = e->pol;
    const int P = q.P, K = q.width[q.L - 1];
    if (!d->value_b && !d->logstd_b) return fail(e, CA_EINVAL, "%s: neither head is given (value_b and logstd_b are null)", who);
    if (d->value_b && !d->value_w) return fail(e, CA_EINVAL, "%s: value_b without value_w", who);
    if (d->value_w && !d->value_b) return fail(e, CA_EINVAL, "%s: value_w without value_b", who);
    if (d->logstd_w && !d->logstd_b) return fail(e, CA_EINVAL, "%s: logstd_w without logstd_b", who);
    const size_t wb = (size_t)P * K * 4, bb = (size_t)P * 4;
    struct { const char* name; const float* w; size_t w_bytes; const float* b; size_t b_bytes; int col; } hd[2] = {
        {"value", d->value_w, d->value_w_bytes, d->value_b, d->value_b_bytes, 2}, {"logstd", d->logstd_w, d->logstd_w_bytes, d->logstd_b, d->logstd_b_bytes, 1}};
    for (const auto& h : hd) {
        if (!h.b) continue;
        if (h.w && h.w_bytes < wb) return fail(e, CA_ESIZE, "%s: %s_w needs %zu bytes (f32 [P=%d, %d]), got %zu", who, h.name, wb, P, K, h.w_bytes);
        if (h.b_bytes < bb) return fail(e, CA_ESIZE, "%s: %s_b needs %zu bytes (f32 [P=%d]), got %zu", who, h.name, bb, P, h.b_bytes);
        for (size_t k = 0; h.w && k < (size_t)P * K; ++k)
            if (!std::isfinite(h.w[k])) return fail(e, CA_ERANGE, "%s: %s head, set %zu: weight [%zu] is not finite", who, h.name, k / K, k % K);
        for (int p = 0; p < P; ++p)
            if (!std::isfinite(h.b[p])) return fail(e, CA_ERANGE, "%s: %s head, set %d: the bias is not finite", who, h.name, p);
    }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    // the policy's own packed sets, and into the output tile of each: lane l of k-step s holds W[column l & 15][4 s + (l >> 4)]
    std::vector<float> wp((size_t)P * q.wset), bp((size_t)P * q.bset);
    HIPCHK(e, download(e, wp.data(), q.d_wp, wp.size() * 4));
    HIPCHK(e, download(e, bp.data(), q.d_bp, bp.size() * 4));
    for (const auto& h : hd) {
        if (!h.b) continue;
        for (int p = 0; p < P; ++p) {
            float* dst = wp.data() + (size_t)p * q.wset + q.wp_off[q.L - 1];
            for (int k = 0; k < K; ++k) dst[(size_t)(k >> 2) * 64 + (size_t)(k & 3) * 16 + h.col] = h.w ? h.w[(size_t)p * K + k] : 0.0f;
            bp[(size_t)p * q.bset + q.bp_off[q.L - 1] + h.col] = h.b[p];
        }
    }
    float *nw = nullptr, *nb = nullptr;
    hipError_t r = hipMalloc((void**)&nw, wp.size() * 4);
    if (r == hipSuccess) r = hipMalloc((void**)&nb, bp.size() * 4);
    if (r == hipSuccess) r = upload(e, nw, wp.data(), wp.size() * 4);
    if (r == hipSuccess) r = upload(e, nb, bp.data(), bp.size() * 4);
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    if (r != hipSuccess) {
        if (nw) hipFree(nw);
        if (nb) hipFree(nb);
        return fail(e, CA_EHIP, "%s: installing the heads failed: %s", who, hipGetErrorString(r));
    }
    drop_heads(e);
    e->heads.d_wp = nw; e->heads.d_bp = nb;
    e->heads.has_value = d->value_b != nullptr; e->heads.has_logstd = d->logstd_b != nullptr;
    e->heads.on = true;
    return CA_OK;
}

int ca_policy_clear_heads(ca_env* e) {
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    drop_heads(e);
    return CA_OK;
}

int ca_policy_heads_info(ca_env* e, int32_t* has_value, int32_t* has_logstd) {
    if (!e) return CA_EINVAL;
    if (has_value) *has_value = e->heads.on && e->heads.has_value ? 1 : 0;
    if (has_logstd) *has_logstd = e->heads.on && e->heads.has_logstd ? 1 : 0;
    return CA_OK;
}

int ca_policy_evaluate(ca_env* e, const float* noise, const ca_policy_eval* out) {
    if (!e) return CA_EINVAL;
    if (!e->pol.on) return fail(e, CA_EINVAL, "ca_policy_evaluate: call ca_policy_configure first");
    if (!e->heads.on) return fail(e, CA_EINVAL, "ca_policy_evaluate: call ca_policy_set_heads first");
    if (!out) return fail(e, CA_EINVAL, "ca_policy_evaluate: out is null");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_heads(e, {noise, out->actions, nullptr, nullptr}, *out, false));
    return CA_OK;
}

static hipError_t launch_gae(ca_env* e, int R, const float* rewards, const float* values, const int* done, const int* valid, float gamma, float lambda,
                             float* adv, float* target) {
    GaeArgs g;
    g.rewards = rewards; g.values = values; g.done = done; g.valid = valid; g.adv = adv; g.target = target;
    g.an = (unsigned)AN(e); g.A = e->cfg.n_arenas; g.N = e->cfg.n_agents; g.R = R;
    g.gamma = gamma; g.gl = gamma * lambda;   // (one fp32 multiply: the library is built without contraction)
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, gae_kernel, dim3((g.an + 255) / 256), dim3(256), 0, e->stream, g);
    return hipGetLastError();
}

int ca_gae(ca_env* e, int32_t rows, const ca_gae_desc* d) {
    const char* who = "ca_gae";
    if (!e) return CA_EINVAL;
    if (!d) return fail(e, CA_EINVAL, "%s: the description is null", who);
    if (rows < 0) return fail(e, CA_EINVAL, "%s: rows=%d", who, rows);
    if (!d->rewards || !d->values || !d->done) return fail(e, CA_EINVAL, "%s: rewards, values or done is null", who);
    const size_t R = (size_t)rows, A = (size_t)e->cfg.n_arenas, an = AN(e);
    const int Ai = e->cfg.n_arenas, Ni = e->cfg.n_agents;
    if (d->rewards_bytes < R * an * 4)
        return fail(e, CA_ESIZE, "%s: the rewards buffer needs %zu bytes (f32 [R=%d, A=%d, N=%d]), got %zu", who, R * an * 4, rows, Ai, Ni, d->rewards_bytes);
    if (d->values_bytes < (R + 1) * an * 4)
        return fail(e, CA_ESIZE, "%s: the values buffer needs %zu bytes (f32 [R+1=%d, A=%d, N=%d]), got %zu", who, (R + 1) * an * 4, rows + 1, Ai, Ni, d->values_bytes);
    if (d->done_bytes < R * A * 4)
        return fail(e, CA_ESIZE, "%s: the done buffer needs %zu bytes (i32 [R=%d, A=%d]), got %zu", who, R * A * 4, rows, Ai, d->done_bytes);
    if (d->valid && d->valid_bytes < R * A * 4)
        return fail(e, CA_ESIZE, "%s: the valid buffer needs %zu bytes (i32 [R=%d, A=%d]), got %zu", who, R * A * 4, rows, Ai, d->valid_bytes);
    if (d->advantages && d->advantages_bytes < R * an * 4)
        return fail(e, CA_ESIZE, "%s: the advantages buffer needs %zu bytes (f32 [R=%d, A=%d, N=%d]), got %zu", who, R * an * 4, rows, Ai, Ni, d->advantages_bytes);
    if (d->targets && d->targets_bytes < R * an * 4)
        return fail(e, CA_ESIZE, "%s: the targets buffer needs %zu bytes (f32 [R=%d, A=%d, N=%d]), got %zu", who, R * an * 4, rows, Ai, Ni, d->targets_bytes);
    if (rows == 0) return CA_OK;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_gae(e, rows, d->rewards, d->values, (const int*)d->done, (const int*)d->valid, d->gamma, d->lambda, d->advantages, d->targets));
    return CA_OK;
}

// every refusal of a sampling rollout, before anything is launched: those of a policy rollout, then the new records'
static int sample_seq_check(ca_env* e, const char* who, int32_t steps, uint32_t flags, const ca_policy_sample_seq* seq) {
    { const int rc = policy_seq_check(e, who, steps, flags, seq); if (rc) return rc; }
    if (!e->heads.on) return fail(e, CA_EINVAL, "%s: call ca_policy_set_heads first", who);
    if ((seq->advantages_out || seq->targets_out) && !seq->values_out)
        return fail(e, CA_EINVAL, "%s: advantages_out and targets_out need values_out", who);
    const size_t R = ((size_t)steps + (size_t)seq->hold - 1) / (size_t)seq->hold, A = (size_t)e->cfg.n_arenas, an = AN(e);
    const int Ai = e->cfg.n_arenas, Ni = e->cfg.n_agents;
    const struct { const char* name; const void* p; size_t bytes, need; const char* layout; } bufs[] = {
        {"logp_out", seq->logp_out, seq->logp_out_bytes, R * an * 4, "f32 [R, A, N]"},
        {"dist_out", seq->dist_out, seq->dist_out_bytes, R * 2 * an * 4, "f32 [R, 2, A, N]"},
        {"values_out", seq->values_out, seq->values_out_bytes, (R + 1) * an * 4, "f32 [R+1, A, N]"},
        {"row_rewards_out", seq->row_rewards_out, seq->row_rewards_out_bytes, R * an * 4, "f32 [R, A, N]"},
        {"row_done_out", seq->row_done_out, seq->row_done_out_bytes, R * A * 4, "i32 [R, A]"},
        {"row_valid_out", seq->row_valid_out, seq->row_valid_out_bytes, R * A * 4, "i32 [R, A]"},
        {"advantages_out", seq->advantages_out, seq->advantages_out_bytes, R * an * 4, "f32 [R, A, N]"},
        {"targets_out", seq->targets_out, seq->targets_out_bytes, R * an * 4, "f32 [R, A, N]"}};
    for (const auto& b : bufs)
        if (b.p && b.bytes < b.need)
            return fail(e, CA_ESIZE, "%s: the %s buffer needs %zu bytes (%s with R=%zu, A=%d, N=%d), got %zu", who, b.name, b.need, b.layout, R, Ai, Ni, b.bytes);
    return CA_OK;
}

int ca_rollout_policy_sample(ca_env* e, int32_t steps, uint32_t flags, const ca_policy_sample_seq* seq) {
    const char* who = "ca_rollout_policy_sample";
    if (!e) return CA_EINVAL;
    { const int rc = sample_seq_check(e, who, steps, flags, seq); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    { const int rs = overflow_status(e, who); if (rs) return rs; }
    const size_t an = AN(e), A = (size_t)e->cfg.n_arenas;
    const int hold = seq->hold, R = (int)(((size_t)steps + (size_t)hold - 1) / (size_t)hold);
    const bool gae = (seq->advantages_out || seq->targets_out) && R > 0;
    // the row records the GAE launch reads: the caller's, or the handle's own (they only grow)
    float* rr = seq->row_rewards_out;
    int *rd = (int*)seq->row_done_out, *rv = (int*)seq->row_valid_out;
    if (gae && !rr) {
        if (e->heads.rr_rows < (size_t)R) {
            if (e->heads.rr) { HIPCHK(e, hipFree(e->heads.rr)); e->heads.rr = nullptr; e->heads.rr_rows = 0; }
            HIPCHK(e, hipMalloc((void**)&e->heads.rr, (size_t)R * an * 4));
            e->heads.rr_rows = (size_t)R;
        }
        rr = e->heads.rr;
    }
    if (gae && (!rd || !rv)) {
        if (e->heads.words_rows < (size_t)R) {
            if (e->heads.words) { HIPCHK(e, hipFree(e->heads.words)); e->heads.words = nullptr; e->heads.words_rows = 0; }
            HIPCHK(e, hipMalloc((void**)&e->heads.words, 2 * (size_t)R * A * 4));
            e->heads.words_rows = (size_t)R;
        }
        if (!rd) rd = e->heads.words;
        if (!rv) rv = e->heads.words + e->heads.words_rows * A;
    }
    const auto row = [&](int t) {   // (the heads, into row t / hold of the call's own records)
        const size_t r = (size_t)(t / hold);
        ca_policy_eval o;
        o.actions = nullptr;
        o.logp = seq->logp_out ? seq->logp_out + r * an : nullptr;
        o.value = seq->values_out ? seq->values_out + r * an : nullptr;
        o.mean = seq->dist_out ? seq->dist_out + r * 2 * an : nullptr;
        o.log_std = seq->dist_out ? seq->dist_out + r * 2 * an + an : nullptr;
        return launch_policy_row(e, seq, t, &o);
    };
    { const int rc = policy_rollout_steps(e, steps, flags, seq, row, [&](uint32_t sf, const StepRec&) { return do_step(e, e->pol.act, sf); },
                                          [&](const StepRec& rec) { return launch_sample_record(e, rec, hold, rr, rd, rv); }); if (rc) return rc; }
    if (seq->values_out) {   // the bootstrap row: the value of the state the call leaves
        HIPCHK(e, launch_obs(e));
        ca_policy_eval o = {nullptr, nullptr, seq->values_out + (size_t)R * an, nullptr, nullptr};
        HIPCHK(e, launch_heads(e, {nullptr, nullptr, nullptr, nullptr}, o, true));
    }
    if (gae) HIPCHK(e, launch_gae(e, R, rr, seq->values_out, rd, rv, seq->gamma, seq->lambda, seq->advantages_out, seq->targets_out));
    const uint32_t tail = seq->values_out ? flags & ~(uint32_t)CA_F_OBS : flags;   // (the bootstrap's observation is CA_F_OBS's)
    return launch_tail(e, tail);
}

// ---- navigation fields (include/ca_env.h ca_nav_desc; ca_nav.h, ca_nav_host.h) --------------------------------------
// the field kernel's block: one workgroup relaxes a whole grid, so a large grid wants every lane a workgroup can have, and many small
// grids want several workgroups per CU (profiles/nav_cost.txt has the two measured)
enum { NAV_BIG_CELLS = 4096 };
static int nav_block_for(const ca_env* e, int cells) {
    if (e->sw.nav_block == 256 || e->sw.nav_block == 1024) return e->sw.nav_block;
    return cells > NAV_BIG_CELLS ? 1024 : 256;
}
static hipError_t launch_nav_field(ca_env* e, const NavFieldArgs& f, int fields, int block) {
    const size_t lds = ((size_t)f.cells + (size_t)f.mw) * 4;
    void (*fn)(NavFieldArgs) = block == 1024 ? nav_field_kernel<1024> : nav_field_kernel<256>;
    if (lds > 48 * 1024) {
        const hipError_t r = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (r != hipSuccess) return r;
    }
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, fn, dim3((unsigned)fields), dim3((unsigned)block), lds, e->stream, f);
    return hipGetLastError();
}

int ca_nav_mask_build(const float* edges_pq, int32_t n_edges, float x0, float y0, float cell, int32_t gx, int32_t gy, float clearance,
                      uint8_t* blocked, int32_t cells_cap) {
    const char* who = "ca_nav_mask_build";
    if (!blocked || n_edges < 0 || (n_edges > 0 && !edges_pq)) return fail(nullptr, CA_EINVAL, "%s: bad argument", who);
    if (!ca_nav::grid_ok(gx, gy))
        return fail(nullptr, CA_EINVAL, "%s: a grid of %d x %d cells (1 .. %d per axis, at most %d in all)", who, (int)gx, (int)gy, (int)ca_nav::MAX_SIDE,
                    (int)ca_nav::MAX_CELLS);
    if (cells_cap < gx * gy) return fail(nullptr, CA_ESIZE, "%s: blocked needs %d bytes (cells_cap=%d)", who, (int)(gx * gy), (int)cells_cap);
    ca_nav::mask_build(edges_pq, n_edges, x0, y0, cell, gx, gy, clearance, blocked);
    return CA_OK;
}

int ca_nav_configure(ca_env* e, const ca_nav_desc* d) {
    const char* who = "ca_nav_configure";
    static_assert(NAV_STAY == ca_nav::STAY && NAV_NONE == ca_nav::NONE, "one pointer code");
    if (!e || !d || !d->targets || !d->agent_class) return fail(e, CA_EINVAL, "%s: null argument", who);
    const int A = e->cfg.n_arenas, N = e->cfg.n_agents, G = d->n_goals;
    const bool per = d->per_arena != 0;
    if (d->per_arena != 0 && d->per_arena != 1) return fail(e, CA_EINVAL, "%s: per_arena=%d (0 or 1)", who, (int)d->per_arena);
    if (!per && !e->h_tab_off.empty())
        return fail(e, CA_EINVAL, "%s: per_arena=0 asks for one field set, but the handle holds an obstacle table per arena (ca_set_obstacles_per_arena): "
                    "configure with per_arena=1 and targets [A, G, 2]", who);
    if (G < 1 || G > ca_nav::MAX_GOALS) return fail(e, CA_EINVAL, "%s: n_goals=%d (1 .. %d)", who, G, (int)ca_nav::MAX_GOALS);
    if (d->lookahead < 1 || d->lookahead > ca_nav::MAX_LOOKAHEAD) return fail(e, CA_EINVAL, "%s: lookahead=%d (1 .. %d)", who, (int)d->lookahead, (int)ca_nav::MAX_LOOKAHEAD);
    if (!ca_nav::grid_ok(d->gx, d->gy))
        return fail(e, CA_EINVAL, "%s: a grid of %d x %d cells (1 .. %d per axis, at most %d in all)", who, (int)d->gx, (int)d->gy, (int)ca_nav::MAX_SIDE,
                    (int)ca_nav::MAX_CELLS);
    const int sets = per ? A : 1, gx = d->gx, gy = d->gy, cells = gx * gy, fields = sets * G;
    const size_t an = AN(e);
    if (d->targets_bytes != (size_t)fields * 2 * 4)
        return fail(e, CA_ESIZE, "%s: targets holds %zu bytes (f32 %s), got %zu", who, (size_t)fields * 2 * 4, per ? "[A, G, 2]" : "[G, 2]", d->targets_bytes);
    if (d->class_bytes != an * 4) return fail(e, CA_ESIZE, "%s: agent_class holds %zu bytes (i32 [A=%d, N=%d]), got %zu", who, an * 4, A, N, d->class_bytes);
    if (!(d->cell >= CA_MIN_LENGTH && d->cell <= CA_MAX_LENGTH))   // (also false for NaN)
        return fail(e, CA_ERANGE, "%s: cell=%g is outside [%g, %g] or not a number", who, (double)d->cell, (double)CA_MIN_LENGTH, (double)CA_MAX_LENGTH);
    if (!(d->clearance == 0.0f || (d->clearance >= CA_MIN_LENGTH && d->clearance <= CA_MAX_LENGTH)))
        return fail(e, CA_ERANGE, "%s: clearance=%g is neither 0 nor inside [%g, %g]", who, (double)d->clearance, (double)CA_MIN_LENGTH, (double)CA_MAX_LENGTH);
    if (!(fabsf(d->x0) <= CA_MAX_COORD && fabsf(d->y0) <= CA_MAX_COORD))
        return fail(e, CA_ERANGE, "%s: the origin (%g, %g) is beyond %g or not a number", who, (double)d->x0, (double)d->y0, (double)CA_MAX_COORD);
    for (size_t q = 0; q < an; ++q)
        if (d->agent_class[q] < -1 || d->agent_class[q] >= G)
            return fail(e, CA_ERANGE, "%s: agent_class=%d of arena %zu, agent %zu is outside -1 .. %d", who, (int)d->agent_class[q], q / (size_t)N, q % (size_t)N, G - 1);
    const float cs = d->cell, ics = 1.0f / cs;
    // the masks and the sources, on the host
    std::vector<unsigned char> blocked((size_t)sets * cells);
    std::vector<float> pq;
    for (int s = 0; s < sets; ++s) {
        const int t0 = e->h_tab_off.empty() ? 0 : e->h_tab_off[s], n = e->h_tab_off.empty() ? (int)e->h_obst.size() : e->h_tab_off[s + 1] - e->h_tab_off[s];
        pq.resize((size_t)4 * n);
        for (int i = 0; i < n; ++i) {
            const ObstDev& o = e->h_obst[(size_t)t0 + i];
            pq[4 * i] = o.px; pq[4 * i + 1] = o.py; pq[4 * i + 2] = o.qx; pq[4 * i + 3] = o.qy;
        }
        ca_nav::mask_build(pq.data(), n, d->x0, d->y0, cs, gx, gy, d->clearance, blocked.data() + (size_t)s * cells);
    }
    std::vector<int> source((size_t)fields);
    const double bx1 = (double)d->x0 + (double)gx * (double)cs, by1 = (double)d->y0 + (double)gy * (double)cs;
    for (int f = 0; f < fields; ++f) {
        const float tx = d->targets[2 * f], ty = d->targets[2 * f + 1];
        const int s = f / G, g = f % G;
        if (!(tx >= d->x0 && (double)tx <= bx1 && ty >= d->y0 && (double)ty <= by1))   // (also false for NaN)
            return fail(e, CA_ERANGE, "%s: target (%g, %g) of arena %d, goal %d is outside the grid box [%g, %g] x [%g, %g] or not a number", who,
                        (double)tx, (double)ty, per ? s : -1, g, (double)d->x0, bx1, (double)d->y0, by1);
        const int c = ca_nav::cell(ty, d->y0, ics, gy) * gx + ca_nav::cell(tx, d->x0, ics, gx);
        if (blocked[(size_t)s * cells + c])
            return fail(e, CA_ERANGE, "%s: target (%g, %g) of arena %d, goal %d lies in a blocked cell (%d, %d): within clearance %g of an obstacle edge", who,
                        (double)tx, (double)ty, per ? s : -1, g, c % gx, c / gx, (double)d->clearance);
        source[f] = c;
    }
    const int mw = (cells + 31) / 32;
    std::vector<unsigned> bits((size_t)sets * mw, 0u);
    for (int s = 0; s < sets; ++s)
        for (int c = 0; c < cells; ++c)
            if (blocked[(size_t)s * cells + c]) bits[(size_t)s * mw + (c >> 5)] |= 1u << (c & 31);
    // the new buffers, the upload, the relaxation; swapped in only when all of it succeeded
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    ca_env::Nav n;
    unsigned* d_bits = nullptr;
    int *d_src = nullptr, *d_sweeps = nullptr;
    std::vector<int> sweeps((size_t)fields, 0);
    hipError_t r = hipMalloc((void**)&n.d_dist, (size_t)fields * cells * 4);
    if (r == hipSuccess) r = hipMalloc((void**)&n.d_next, (size_t)fields * cells);
    if (r == hipSuccess) r = hipMalloc((void**)&n.d_class, an * 4);
    if (r == hipSuccess) r = hipMalloc((void**)&d_bits, bits.size() * 4);
    if (r == hipSuccess) r = hipMalloc((void**)&d_src, (size_t)fields * 4);
    if (r == hipSuccess) r = hipMalloc((void**)&d_sweeps, (size_t)fields * 4);
    if (r == hipSuccess) r = hipMemcpyAsync(n.d_class, d->agent_class, an * 4, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(d_bits, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) r = hipMemcpyAsync(d_src, source.data(), (size_t)fields * 4, hipMemcpyHostToDevice, e->stream);
    n.block = nav_block_for(e, cells);
    if (r == hipSuccess) {
        NavFieldArgs f;
        f.mask = d_bits; f.source = d_src; f.dist = n.d_dist; f.next = n.d_next; f.sweeps = d_sweeps;
        f.gx = gx; f.gy = gy; f.cells = cells; f.mw = mw; f.G = G;
        f.w_axis = cs; f.w_diag = cs * 1.41421354f;
        r = launch_nav_field(e, f, fields, n.block);
    }
    if (r == hipSuccess) r = hipMemcpyAsync(sweeps.data(), d_sweeps, (size_t)fields * 4, hipMemcpyDeviceToHost, e->stream);
    if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
    if (d_bits) hipFree(d_bits);
    if (d_src) hipFree(d_src);
    if (d_sweeps) hipFree(d_sweeps);
    if (r != hipSuccess) {
        if (n.d_dist) hipFree(n.d_dist);
        if (n.d_next) hipFree(n.d_next);
        if (n.d_class) hipFree(n.d_class);
        return fail(e, CA_EHIP, "%s: %s (the handle's navigation is as it was)", who, hipGetErrorString(r));
    }
    n.on = true;
    n.x0 = d->x0; n.y0 = d->y0; n.cell = cs; n.ics = ics; n.clearance = d->clearance;
    n.gx = gx; n.gy = gy; n.G = G; n.sets = sets; n.per_arena = per ? 1 : 0; n.lookahead = d->lookahead;
    for (int f = 0; f < fields; ++f) n.sweeps_max = std::max(n.sweeps_max, sweeps[f]);
    n.h_blocked.swap(blocked);
    nav_release(e);
    e->nav = std::move(n);
    return CA_OK;
}

int ca_nav_clear(ca_env* e) {
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    nav_release(e);
    return CA_OK;
}

int ca_nav_info(ca_env* e, int32_t* configured, int32_t* gx, int32_t* gy, int32_t* n_goals, int32_t* n_sets, int32_t* sweeps_max) {
    if (!e) return CA_EINVAL;
    const ca_env::Nav& n = e->nav;
    if (configured) *configured = n.on ? 1 : 0;
    if (gx) *gx = n.gx;
    if (gy) *gy = n.gy;
    if (n_goals) *n_goals = n.G;
    if (n_sets) *n_sets = n.sets;
    if (sweeps_max) *sweeps_max = n.sweeps_max;
    return CA_OK;
}

int ca_nav_get_field(ca_env* e, int32_t arena, int32_t goal, float* dist, uint8_t* next, uint8_t* blocked, int32_t cells_cap) {
    const char* who = "ca_nav_get_field";
    if (!e) return CA_EINVAL;
    const ca_env::Nav& n = e->nav;
    if (!n.on) return fail(e, CA_EINVAL, "%s: call ca_nav_configure first", who);
    if (arena < 0 || arena >= e->cfg.n_arenas) return fail(e, CA_ERANGE, "%s: arena %d of %d", who, (int)arena, e->cfg.n_arenas);
    if (goal < 0 || goal >= n.G) return fail(e, CA_ERANGE, "%s: goal %d of %d", who, (int)goal, n.G);
    const int cells = n.gx * n.gy, set = n.per_arena ? arena : 0;
    if (cells_cap < cells) return fail(e, CA_ESIZE, "%s: a field holds %d cells (cells_cap=%d)", who, cells, (int)cells_cap);
    const size_t f = (size_t)set * n.G + (size_t)goal;
    HIPCHK(e, hipSetDevice(e->device));
    if (dist) HIPCHK(e, hipMemcpyAsync(dist, n.d_dist + f * cells, (size_t)cells * 4, hipMemcpyDeviceToHost, e->stream));
    if (next) HIPCHK(e, hipMemcpyAsync(next, n.d_next + f * cells, (size_t)cells, hipMemcpyDeviceToHost, e->stream));
    if (dist || next) HIPCHK(e, hipStreamSynchronize(e->stream));
    if (blocked) memcpy(blocked, n.h_blocked.data() + (size_t)set * cells, (size_t)cells);
    return CA_OK;
}

// what the per-step kernels read of the state and the navigation
static NavPrefArgs nav_pref_args(ca_env* e, float* dist_out, bool freeze) {
    const ca_env::Nav& n = e->nav;
    NavPrefArgs p;
    p.pos_x = e->pos_x; p.pos_y = e->pos_y; p.goal_x = e->goal_x; p.goal_y = e->goal_y;
    p.agent_done = e->agent_done; p.arena_done = e->arena_done; p.agent_counts = e->ac ? e->d_counts : nullptr;
    p.cls = n.d_class; p.dist = n.d_dist; p.next = n.d_next;
    p.pref_x = e->pref_x; p.pref_y = e->pref_y; p.dist_out = dist_out;
    p.an = (unsigned)AN(e); p.N = e->cfg.n_agents; p.G = n.G; p.gx = n.gx; p.gy = n.gy; p.cells = n.gx * n.gy;
    p.per_arena = n.per_arena; p.lookahead = n.lookahead; p.freeze = freeze ? 1 : 0;
    p.x0 = n.x0; p.y0 = n.y0; p.cell = n.cell; p.ics = n.ics;
    return p;
}
// the preferred-velocity launch (kind 3 for ca_profile)
static hipError_t launch_nav_pref(ca_env* e, float* dist_out, bool freeze) {
    const NavPrefArgs p = nav_pref_args(e, dist_out, freeze);
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, nav_pref_kernel, dim3((p.an + 255) / 256), dim3(256), 0, e->stream, p);
    return hipGetLastError();
}

int ca_nav_pref(ca_env* e, float* dist_out, uint32_t flags) {
    if (!e) return CA_EINVAL;
    if (!e->nav.on) return fail(e, CA_EINVAL, "ca_nav_pref: call ca_nav_configure first");
    if (flags & ~CA_F_FREEZE) return fail(e, CA_EINVAL, "ca_nav_pref: flags=0x%x (0 or CA_F_FREEZE)", flags);
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_nav_pref(e, dist_out, (flags & CA_F_FREEZE) != 0));
    return CA_OK;
}

int ca_rollout_nav(ca_env* e, int32_t steps, uint32_t flags, const ca_trace* tr) {
    const char* who = "ca_rollout_nav";
    if (!e) return CA_EINVAL;
    if (!e->nav.on) return fail(e, CA_EINVAL, "%s: call ca_nav_configure first", who);
    if (steps < 0) return fail(e, CA_EINVAL, "%s: steps=%d", who, (int)steps);
    if (flags & ~(CA_F_OBS | CA_F_STATS | CA_F_AUTORESET | CA_F_NODONE | CA_F_FREEZE | CA_F_CONTACT))
        return fail(e, CA_EINVAL, "%s: flags=0x%x holds a bit this call does not know", who, flags);
    TracePlan pl = {0, 0};
    if (tr) { const int rc = trace_check(e, who, steps, tr, &pl); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    { const int rs = overflow_status(e, who); if (rs) return rs; }
    const uint32_t sf = flags & ~(CA_F_OBS | CA_F_CONTACT);   // (both: one launch behind the last step, launch_tail)
    for (int s = 0; s < steps; ++s) {   // the launch of ca_nav_pref, the launches of ca_orca_step, the record kernel behind every `every`-th
        prof_cadence(e, 1);
        HIPCHK(e, launch_nav_pref(e, nullptr, (flags & CA_F_FREEZE) != 0));
        const int rc = do_step(e, nullptr, sf);
        if (rc) return rc;
        if (tr) HIPCHK(e, launch_trace_behind(e, tr, pl, s));
    }
    return launch_tail(e, flags);
}

// ---- action steps steered by the navigation (include/ca_env.h ca_nav_act, ca_nav_step; ca_nav.h) -----------------------
static hipError_t nav_step_buffers(ca_env* e) {
    if (!e->nav_keep) { const hipError_t r = dalloc(e, &e->nav_keep, 4 * AN(e)); if (r != hipSuccess) return r; }
    if (!e->nav_advance) { const hipError_t r = dalloc(e, &e->nav_advance, (size_t)e->cfg.n_arenas); if (r != hipSuccess) return r; }
    return hipSuccess;
}
// the launch in front of the step (kind 3 for ca_profile)
static hipError_t launch_nav_act(ca_env* e, const float* actions, float* heading_out, float* dist_out, bool freeze) {
    NavActArgs q;
    q.n = nav_pref_args(e, dist_out, freeze);
    q.actions = actions; q.keep = e->nav_keep; q.heading_out = heading_out; q.advance = e->nav_advance;
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, nav_act_kernel, dim3((q.n.an + 255) / 256), dim3(256), 0, e->stream, q);
    return hipGetLastError();
}
// the launch behind the step (kind 3): the reward, the arena's sum under CA_F_STATS, a rollout's return, first_done and records
static hipError_t launch_nav_reward(ca_env* e, uint32_t flags, const StepRec* rec) {
    NavRewardArgs c = {};
    fill_step_rec(e, rec, c);
    if (rec) fill_step_records(e, *rec, c);
    c.vel_x = e->vel_x; c.vel_y = e->vel_y; c.keep = e->nav_keep; c.advance = e->nav_advance;
    c.reward = e->reward; c.arena_stats = (flags & CA_F_STATS) ? e->arena_stats : nullptr;
    c.reward_scale = e->cfg.reward_scale;
    ProfScope ps(e, KIND_RESET);
    launch_k(ps, nav_reward_kernel, dim3((c.an + 255) / 256), dim3(256), 0, e->stream, c);
    return hipGetLastError();
}
// one navigated action step: nav_act_kernel, the launches of the ORCA-only step, nav_reward_kernel
static int nav_do_step(ca_env* e, const float* actions, uint32_t sf, const StepRec* rec) {
    prof_cadence(e, 1);
    const bool terms = e->rew.on;
    if (terms) HIPCHK(e, launch_reward_begin(e, sf));
    HIPCHK(e, launch_nav_act(e, actions, nullptr, nullptr, (sf & CA_F_FREEZE) != 0));
    const int rc = do_step(e, nullptr, sf);
    if (rc) return rc;
    if (!terms) {
        HIPCHK(e, launch_nav_reward(e, sf, rec));
        return CA_OK;
    }
    // reward terms: nav_reward_kernel in its single-step form, the terms, then a rollout's ordinary accounting of the shaped reward
    HIPCHK(e, launch_nav_reward(e, sf, nullptr));
    HIPCHK(e, launch_reward_terms(e, sf, false));
    if (rec) HIPCHK(e, (rec->rewards_out || rec->done_out) ? launch_policy_record(e, *rec) : launch_actseq_accumulate(e, *rec));
    return CA_OK;
}

int ca_nav_act(ca_env* e, const float* actions, float* heading_out, float* dist_out, uint32_t flags) {
    if (!e) return CA_EINVAL;
    if (!e->nav.on) return fail(e, CA_EINVAL, "ca_nav_act: call ca_nav_configure first");
    if (!actions) return fail(e, CA_EINVAL, "ca_nav_act: actions is null");
    if (flags & ~CA_F_FREEZE) return fail(e, CA_EINVAL, "ca_nav_act: flags=0x%x (0 or CA_F_FREEZE)", flags);
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, nav_step_buffers(e));
    HIPCHK(e, launch_nav_act(e, actions, heading_out, dist_out, (flags & CA_F_FREEZE) != 0));
    return CA_OK;
}

int ca_nav_step(ca_env* e, const float* actions, uint32_t flags) {
    const char* who = "ca_nav_step";
    if (!e) return CA_EINVAL;
    if (!e->nav.on) return fail(e, CA_EINVAL, "%s: call ca_nav_configure first", who);
    if (!actions) return fail(e, CA_EINVAL, "%s: actions is null (ca_rollout_nav is the ORCA-only navigated step)", who);
    if (flags & CA_F_NODONE) return fail(e, CA_EINVAL, "%s: CA_F_NODONE applies to ca_orca_step only", who);
    if (flags & ~(CA_F_OBS | CA_F_STATS | CA_F_AUTORESET | CA_F_FREEZE | CA_F_CONTACT))
        return fail(e, CA_EINVAL, "%s: flags=0x%x holds a bit this call does not know", who, flags);
    HIPCHK(e, hipSetDevice(e->device));
    { const int rs = overflow_status(e, who); if (rs) return rs; }
    HIPCHK(e, nav_step_buffers(e));
    { const int rc = nav_do_step(e, actions, flags & (CA_F_STATS | CA_F_AUTORESET | CA_F_FREEZE), nullptr); if (rc) return rc; }
    return launch_tail(e, flags);
}

int ca_rollout_nav_actions(ca_env* e, int32_t steps, uint32_t flags, const ca_action_seq* seq) {
    if (!e) return CA_EINVAL;
    if (!e->nav.on) return fail(e, CA_EINVAL, "ca_rollout_nav_actions: call ca_nav_configure first");
    { const int rc = actseq_check(e, "ca_rollout_nav_actions", steps, flags, seq); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    { const int rs = overflow_status(e, "ca_rollout_nav_actions"); if (rs) return rs; }
    HIPCHK(e, nav_step_buffers(e));
    ActSeqPlan pl;
    { const int rc = actseq_prologue(e, flags, seq->returns, seq->first_done, true, &pl); if (rc) return rc; }
    const uint32_t sf = flags & (CA_F_STATS | CA_F_AUTORESET | CA_F_FREEZE);   // (observation and contacts: one launch behind the last step, launch_tail)
    StepRec rec = {&pl, seq->weights, seq->returns, nullptr, nullptr, 0, flags};
    for (rec.t = 0; rec.t < steps; ++rec.t) {   // always the per-step form, as ca_rollout_nav
        const int rc = nav_do_step(e, seq->actions + (size_t)(rec.t / seq->hold) * AN(e), sf, &rec);
        if (rc) return rc;
    }
    return launch_tail(e, flags);
}

int ca_rollout_nav_policy(ca_env* e, int32_t steps, uint32_t flags, const ca_policy_seq* seq) {
    if (!e) return CA_EINVAL;
    if (!e->nav.on) return fail(e, CA_EINVAL, "ca_rollout_nav_policy: call ca_nav_configure first");
    { const int rc = policy_seq_check(e, "ca_rollout_nav_policy", steps, flags, seq); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    { const int rs = overflow_status(e, "ca_rollout_nav_policy"); if (rs) return rs; }
    HIPCHK(e, nav_step_buffers(e));
    const int rc = policy_rollout_steps(e, steps, flags, seq, [&](int t) { return launch_policy_row(e, seq, t, nullptr); },
                                        [&](uint32_t sf, const StepRec& rec) { return nav_do_step(e, e->pol.act, sf, &rec); },
                                        [](const StepRec&) { return hipSuccess; });   // (nav_do_step launches its record itself)
    return rc ? rc : launch_tail(e, flags);
}

// ---- reward terms (include/ca_env.h ca_reward_desc; ca_reward.h) ------------------------------------------------------
int ca_reward_configure(ca_env* e, const ca_reward_desc* d) {
    const char* who = "ca_reward_configure";
    if (!e) return CA_EINVAL;
    if (!d || !d->weights) return fail(e, CA_EINVAL, "%s: the description or its weights are null", who);
    if (d->per_arena != 0 && d->per_arena != 1) return fail(e, CA_EINVAL, "%s: per_arena=%d (0 or 1)", who, d->per_arena);
    const size_t A = (size_t)e->cfg.n_arenas, rows = d->per_arena ? A : 1, need = rows * CA_REWARD_N_TERMS * 4;
    if (d->weights_bytes != need)
        return fail(e, CA_ESIZE, "%s: the weights hold %zu bytes (f32 [%s%d]), got %zu", who, need, d->per_arena ? "A, " : "", CA_REWARD_N_TERMS, d->weights_bytes);
    for (size_t a = 0; a < rows; ++a)
        for (int k = 0; k < CA_REWARD_N_TERMS; ++k)
            if (!std::isfinite(d->weights[a * CA_REWARD_N_TERMS + k]))
                return fail(e, CA_ERANGE, "%s: the weight of arena %zu, term %d is not finite", who, a, k);
    if (!std::isfinite(d->margin) || d->margin < 0.0f || d->margin > CA_MAX_LENGTH)
        return fail(e, CA_ERANGE, "%s: margin=%g outside [0, %g]", who, (double)d->margin, (double)CA_MAX_LENGTH);
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));   // (launches in flight read the weights being replaced)
    if (!e->rew.d_w) HIPCHK(e, dalloc(e, &e->rew.d_w, A * CA_REWARD_N_TERMS));
    std::vector<float> w(A * CA_REWARD_N_TERMS);
    int mask = 0;
    for (size_t a = 0; a < A; ++a)
        for (int k = 0; k < CA_REWARD_N_TERMS; ++k) {
            const float v = d->weights[(d->per_arena ? a : 0) * CA_REWARD_N_TERMS + k];
            w[a * CA_REWARD_N_TERMS + k] = v;
            if (v != 0.0f) mask |= 1 << k;
        }
    HIPCHK(e, upload(e, e->rew.d_w, w.data(), w.size() * 4));
    e->rew.h_w.swap(w);
    e->rew.need_mask = mask; e->rew.per_arena = d->per_arena; e->rew.margin = d->margin; e->rew.on = true;
    return CA_OK;
}

int ca_reward_clear(ca_env* e) {
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->rew.on = false;
    return CA_OK;
}

int ca_reward_info(ca_env* e, int32_t* configured, int32_t* per_arena, float* margin) {
    if (!e) return CA_EINVAL;
    if (configured) *configured = e->rew.on ? 1 : 0;
    if (per_arena) *per_arena = e->rew.on ? e->rew.per_arena : 0;
    if (margin) *margin = e->rew.on ? e->rew.margin : 0.0f;
    return CA_OK;
}

int ca_reward_get_weights(ca_env* e, float* weights, size_t bytes) {
    if (!e) return CA_EINVAL;
    if (!weights) return fail(e, CA_EINVAL, "ca_reward_get_weights: weights is null");
    if (!e->rew.on) return fail(e, CA_EINVAL, "ca_reward_get_weights: no reward terms are configured (ca_reward_configure)");
    if (bytes != e->rew.h_w.size() * 4)
        return fail(e, CA_ESIZE, "ca_reward_get_weights: the weights hold %zu bytes (f32 [A, %d]), got %zu", e->rew.h_w.size() * 4, CA_REWARD_N_TERMS, bytes);
    memcpy(weights, e->rew.h_w.data(), bytes);
    return CA_OK;
}

int ca_reward_parts(ca_env* e) {
    if (!e) return CA_EINVAL;
    if (!e->rew.on) return fail(e, CA_EINVAL, "ca_reward_parts: no reward terms are configured (ca_reward_configure)");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, launch_reward_terms(e, 0, true));
    return CA_OK;
}

int ca_get_reward_parts(ca_env* e, float* ref, int32_t* counts, size_t ref_bytes, size_t counts_bytes, int32_t dst_is_device) {
    if (!e) return CA_EINVAL;
    const size_t an = AN(e);
    if (ref && ref_bytes != an * 4) return fail(e, CA_ESIZE, "ca_get_reward_parts: the reference plane holds %zu bytes, got %zu", an * 4, ref_bytes);
    if (counts && counts_bytes != (CA_REWARD_N_TERMS - 1) * an * 4)
        return fail(e, CA_ESIZE, "ca_get_reward_parts: the count planes hold %zu bytes, got %zu", (CA_REWARD_N_TERMS - 1) * an * 4, counts_bytes);
    if (!e->rew.parts_valid)
        return fail(e, CA_EINVAL, "ca_get_reward_parts: no reward parts have been computed on this handle (ca_reward_parts, or a step "
                                  "under configured terms)");
    HIPCHK(e, hipSetDevice(e->device));
    const hipMemcpyKind kind = dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (ref) HIPCHK(e, hipMemcpyAsync(ref, e->rew.parts, ref_bytes, kind, e->stream));
    if (counts) HIPCHK(e, hipMemcpyAsync(counts, e->rew.parts + an, counts_bytes, kind, e->stream));
    if (!dst_is_device) HIPCHK(e, hipStreamSynchronize(e->stream));
    return CA_OK;
}

int ca_reward_parts_ptr(ca_env* e, void** dev_ptr, size_t* bytes) {
    if (!e || !dev_ptr) return fail(e, CA_EINVAL, "ca_reward_parts_ptr: null argument");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, reward_buffers(e));
    *dev_ptr = e->rew.parts;
    if (bytes) *bytes = (size_t)CA_REWARD_N_TERMS * AN(e) * 4;
    return CA_OK;
}

int ca_sync(ca_env* e) {
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return overflow_status(e, "ca_sync");
}

int ca_allow_obstacle_overflow(ca_env* e, int32_t allow) {
    if (!e) return CA_EINVAL;
    e->allow_overflow = allow != 0;
    return CA_OK;
}

int ca_get_stats(ca_env* e, ca_stats* out) {
    if (!e || !out) return fail(e, CA_EINVAL, "ca_get_stats: null argument");
    HIPCHK(e, hipSetDevice(e->device));
    const size_t A = e->cfg.n_arenas;
    std::vector<unsigned long long> h(A * ST_STRIDE);
    HIPCHK(e, hipMemcpyAsync(h.data(), e->arena_stats, h.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    ca_stats s;
    memset(&s, 0, sizeof s);
    for (size_t a = 0; a < A; ++a) {
        const unsigned long long* r = &h[a * ST_STRIDE];
        s.episodes += r[ST_EPISODES]; s.collisions += r[ST_COLL]; s.obst_collisions += r[ST_OBST_COLL];
        s.goals_reached += r[ST_GOALS]; s.obst_overflow += r[ST_OVERFLOW];
        double d;
        memcpy(&d, &r[ST_SUMREW], 8);
        s.sum_reward += d;
    }
    // agent-steps: counted by the kernels (every solve launch adds, per arena it advanced, the steps it advanced it by)
    std::vector<unsigned long long> hs(A);
    HIPCHK(e, hipMemcpyAsync(hs.data(), e->arena_steps, A * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    unsigned long long arena_steps = 0;
    for (size_t a = 0; a < A; ++a) arena_steps += hs[a] * (uint64_t)(e->ac ? e->h_counts[a] : e->cfg.n_agents);   // x the arena's agents
    s.agent_steps = e->agent_steps_base + arena_steps;
    *out = s;
    return CA_OK;
}

int ca_reset_stats(ca_env* e) {
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemsetAsync(e->arena_stats, 0, (size_t)e->cfg.n_arenas * ST_STRIDE * 8, e->stream));
    HIPCHK(e, hipMemsetAsync(e->arena_steps, 0, (size_t)e->cfg.n_arenas * 8, e->stream));
    e->steps_done = 0;
    e->agent_steps_base = 0;
    if (e->ovf_host && (*(volatile unsigned long long*)e->ovf_host >> 63)) {   // the sticky overflow status goes with the counters; a step
        HIPCHK(e, hipStreamSynchronize(e->stream));                              // still in flight must not set it again behind the clear
        *(volatile unsigned long long*)e->ovf_host = 0ull;
    }
    return CA_OK;
}

int ca_debug_math(ca_env* e, int32_t op, const void* in, void* out, int32_t n) {
    if (!e || !in || !out || n <= 0 || op < 0 || op > 7) return fail(e, CA_EINVAL, "ca_debug_math: bad argument");
    static const size_t in_b[] = {4, 8, 8, 16, 16, 8, 8, 4}, out_b[] = {4, 4, 16, 16, 16, 8, 4, 4};
    HIPCHK(e, hipSetDevice(e->device));
    void *di = nullptr, *dout = nullptr;
    HIPCHK(e, hipMalloc(&di, in_b[op] * n));
    HIPCHK(e, hipMalloc(&dout, out_b[op] * n));
    HIPCHK(e, upload(e, di, in, in_b[op] * n));
    hipLaunchKernelGGL(debug_math_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, op, di, dout, n, e->cfg.seed);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, download(e, out, dout, out_b[op] * n));
    hipFree(di);
    hipFree(dout);
    return CA_OK;
}

#ifdef CA_STAMPS  // the two entry points below exist in the CA_STAMPS diagnostic build only (tools/stamps.py, tools/diag/placement.py)
/* Diagnostic (not declared in include/ca_env.h): install a block order for the solve kernel -- workgroup b then works on
 * the arenas of block order[b] (a permutation of 0 .. grid-1; host array) -- or remove it (NULL).  Results do not depend on it. */
int ca_debug_set_order(ca_env* e, const int32_t* order) {
    if (!e) return CA_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->d_order) { HIPCHK(e, hipFree(e->d_order)); e->d_order = nullptr; }
    if (!order) return CA_OK;
    std::vector<char> seen((size_t)e->grid, 0);
    for (int b = 0; b < e->grid; ++b) {
        if (order[b] < 0 || order[b] >= e->grid || seen[order[b]]) return fail(e, CA_EINVAL, "ca_debug_set_order: not a permutation");
        seen[order[b]] = 1;
    }
    HIPCHK(e, hipMalloc((void**)&e->d_order, (size_t)e->grid * sizeof(int)));
    HIPCHK(e, upload(e, e->d_order, order, (size_t)e->grid * sizeof(int)));
    return CA_OK;
}

/* CA_STAMPS diagnostic build only: the pieces of the dispatch timeline of tools/diag/timeline.py.  ca_debug_clock launches a
 * one-wave kernel on the handle's stream that writes the device-wide 100 MHz counter at its start and end into slot `slot`
 * (in-stream fences around a dispatch: the kernel before it has ended, the kernel after it has not begun);
 * ca_debug_empty launches a kernel of the solve kernel's grid, block and LDS size whose waves only stamp their start and end. */
__global__ void debug_clock_kernel(unsigned long long* out) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (threadIdx.x == 0) out[0] = t0;
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (threadIdx.x == 0) out[1] = t1;
}
__global__ void debug_empty_kernel(unsigned long long* dbg, int waves_per_block) {
    extern __shared__ float4 smem4[];
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (threadIdx.x == 4096) smem4[0] = make_float4(0.f, 0.f, 0.f, 0.f);   // (keeps the LDS allocation)
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* r = dbg + ((size_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6)) * 16;
        r[12] = t0; r[11] = t1;
    }
}
static unsigned long long* g_dbg_clock = nullptr;
int ca_debug_clock(ca_env* e, int32_t slot) {
    if (!e || slot < 0 || slot >= 64) return fail(e, CA_EINVAL, "ca_debug_clock: bad argument");
    HIPCHK(e, hipSetDevice(e->device));
    if (!g_dbg_clock) HIPCHK(e, hipMalloc((void**)&g_dbg_clock, 64 * 2 * 8));
    hipLaunchKernelGGL(debug_clock_kernel, dim3(1), dim3(64), 0, e->stream, g_dbg_clock + 2 * slot);
    return CA_OK;
}
int ca_debug_clock_read(ca_env* e, unsigned long long* out, int32_t n_slots) {
    if (!e || !g_dbg_clock || n_slots > 64) return fail(e, CA_EINVAL, "ca_debug_clock_read: bad argument");
    HIPCHK(e, download(e, out, g_dbg_clock, (size_t)n_slots * 2 * 8));
    return CA_OK;
}
int ca_debug_empty(ca_env* e) {
    if (!e || !e->dbg) return fail(e, CA_EINVAL, "ca_debug_empty: not a CA_STAMPS build");
    HIPCHK(e, hipSetDevice(e->device));
    ProfScope ps(e, KIND_RESET);   // (timed under "reset_kernels": the step launch in front of it keeps "step_kernel")
    launch_k(ps, debug_empty_kernel, dim3(e->grid), dim3(e->BS), (size_t)e->lds, e->stream, e->dbg, e->BS / 64);
    return CA_OK;
}

/* CA_STAMPS diagnostic build only (not declared in include/ca_env.h): per-wave phase time stamps
 * of the last step kernel, [waves][16] u64. */
int ca_debug_stamps(ca_env* e, unsigned long long* out, int32_t max_waves, int32_t* n_waves) {
    if (!e || !e->dbg) return fail(e, CA_EINVAL, "ca_debug_stamps: not a CA_STAMPS build");
    const bool obs = max_waves < 0;  // negative: the observation kernel's stamps
    if (obs) max_waves = -max_waves;
    const int nw = obs ? e->cfg.n_arenas * ((e->cfg.n_agents + 15) / 16) * 4 : (e->quad ? e->grid_q * (e->BSq / 64) : e->grid * ((e->pair ? 2 : 1) * e->BS / 64));
    if (n_waves) *n_waves = nw;
    // (a one-lane solve launch owns twice its waves' rows -- the allocation above: the second half holds what a wave counts
    // besides its time stamps, row n_waves + w for wave w: the seeded neighbour scan's candidate trips and network runs, ca_nbr.h)
    const int have = (!obs && !e->quad && !e->pair) ? 2 * nw : nw;
    const int n = have < max_waves ? have : max_waves;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, download(e, out, obs ? e->dbg_obs : e->dbg, (size_t)n * 16 * 8));
    return CA_OK;
}
#endif  // CA_STAMPS

/* Page-locked host memory for the results of the host-array calls (ca_get / ca_step_host into the same buffers every step:
 * the reference hands out the same dict objects every call, env.py:463-466).  A pageable destination takes the 67-MB
 * observation of 4096 x 64 agents at ~10 GB/s, a pinned one at the link's rate.  Owned by the handle. */
int ca_host_alloc(ca_env* e, size_t bytes, void** out) {
    if (!e || !out || bytes == 0) return fail(e, CA_EINVAL, "ca_host_alloc: bad argument");
    *out = nullptr;
    HIPCHK(e, hipSetDevice(e->device));
    void* p = nullptr;
    HIPCHK(e, hipHostMalloc(&p, bytes, hipHostMallocDefault));
    e->host_allocs.push_back({p, bytes});
    *out = p;
    return CA_OK;
}
int ca_host_free(ca_env* e, void* p) {
    if (!e || !p) return fail(e, CA_EINVAL, "ca_host_free: bad argument");
    for (size_t k = 0; k < e->host_allocs.size(); ++k)
        if (e->host_allocs[k].first == p) {
            e->host_allocs.erase(e->host_allocs.begin() + k);
            HIPCHK(e, hipHostFree(p));
            return CA_OK;
        }
    return fail(e, CA_EINVAL, "ca_host_free: not a buffer of this handle");
}

int ca_profile(ca_env* e, int32_t period) {
    if (!e || period < 0) return fail(e, CA_EINVAL, "ca_profile: bad argument");
    e->prof_period = period;
    e->profiling = period == 1;
    if (period > 0) {  // the events of the first sampled steps exist before the caller's timed region starts
        HIPCHK(e, hipSetDevice(e->device));
        while (e->free_events.size() < 256) {
            hipEvent_t ev = nullptr;
            if (hipEventCreate(&ev) != hipSuccess) break;
            e->free_events.push_back(ev);
        }
    }
    return CA_OK;
}

int ca_profile_read(ca_env* e, int32_t counts[4], float mean_ms[4]) {
    if (!e || !counts || !mean_ms) return fail(e, CA_EINVAL, "ca_profile_read: null argument");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    double sum[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    for (const ca_env::Span& sp : e->spans) {
        float ms = 0.0f;
        // (a launch that advanced T steps -- ca_rollout's one-launch form -- is reported per step, like the others)
        if (hipEventElapsedTime(&ms, sp.t0, sp.t1) == hipSuccess) { sum[sp.kind] += ms / (sp.steps > 0 ? sp.steps : 1); counts[sp.kind] += 1; }
        e->free_events.push_back(sp.t0);
        e->free_events.push_back(sp.t1);
    }
    e->spans.clear();
    for (int k = 0; k < 4; ++k) mean_ms[k] = counts[k] ? (float)(sum[k] / counts[k]) : 0.0f;
    return CA_OK;
}

int ca_launch_info(ca_env* e, int32_t* block, int32_t* grid, int32_t* lds_bytes, int32_t* obs_grid) {
    if (!e) return CA_EINVAL;
    const SolveLaunch s = solve_launch(e, false, false);   // (what a plain ca_step launches)
    if (block) *block = (int32_t)s.block.x;
    if (grid) *grid = (int32_t)s.grid.x;
    if (lds_bytes) *lds_bytes = e->tgrid ? 0 : (int32_t)s.lds;   // (a grid handle: the bin launch, the solve launch's geometry without its LDS)
    if (obs_grid) {
        const int apb = obs_block_threads(e->cfg.n_agents) / 16;
        *obs_grid = obs_dense(e) ? (int32_t)(((size_t)e->cfg.n_arenas * e->cfg.n_agents + apb - 1) / apb)
                                 : (int32_t)((size_t)e->cfg.n_arenas * ((e->cfg.n_agents + apb - 1) / apb));
    }
    return CA_OK;
}

#ifndef CA_SRC_SHA
#define CA_SRC_SHA "unknown"
#endif
const char* ca_source_sha(void) { return CA_SRC_SHA; }

int ca_solver_info(ca_env* e, int32_t* lanes_per_agent, int32_t* rollout_one_launch) {
    if (!e) return CA_EINVAL;
    if (lanes_per_agent) *lanes_per_agent = e->quad ? 4 : (e->pair ? 2 : 1);
    if (rollout_one_launch) *rollout_one_launch = e->quad_roll ? 1 : 0;
    return CA_OK;
}

int ca_tiled_info(ca_env* e, int32_t* tiled, int32_t* tile_agents, int32_t* tiles_per_arena, int32_t* launches_per_step) {
    if (!e) return CA_EINVAL;
    if (tiled) *tiled = e->tiled ? 1 : 0;
    if (tile_agents) *tile_agents = e->tiled ? e->TILE : 0;
    if (tiles_per_arena) *tiles_per_arena = e->tiled ? e->tiles : 0;
    if (launches_per_step) *launches_per_step = e->tiled ? (e->tgrid ? TILED_SORT_LAUNCHES + 3 : 3) : 0;
    return CA_OK;
}

int ca_tiled_grid_info(ca_env* e, int32_t* grid, int32_t* cells_x, int32_t* cells_y, float* cell_size, int32_t* sort_launches) {
    if (!e) return CA_EINVAL;
    if (grid) *grid = e->tgrid ? 1 : 0;
    if (cells_x) *cells_x = e->tgrid ? e->tgx : 0;
    if (cells_y) *cells_y = e->tgrid ? e->tgy : 0;
    if (cell_size) *cell_size = e->tgrid ? e->tcs : 0.0f;
    if (sort_launches) *sort_launches = e->tgrid ? TILED_SORT_LAUNCHES : 0;
    return CA_OK;
}

int ca_tiled_edge_grid(ca_env* e, int32_t on) {
    if (!e) return CA_EINVAL;
    if (!(e->tiled && e->tgrid))
        return fail(e, CA_EINVAL, "ca_tiled_edge_grid: the static edge grid belongs to a grid handle (ca_create_ex with create_flags 0x5 = "
                    "CA_CREATE_TILED | CA_CREATE_TILED_GRID, with CA_CREATE_TILED_PARAMS or CA_CREATE_TILED_WIDE or not); this handle was made "
                    "without CA_CREATE_TILED_GRID (create_flags 0x%x)", e->tiled ? (e->twide ? 0x21 : (e->tparams ? 0x11 : 0x1)) : 0x0);
    if (on != 0 && on != 1) return fail(e, CA_EINVAL, "ca_tiled_edge_grid: on=%d (0 or 1)", (int)on);
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (on) {
        ca_env::EdgeGrids n_eg;
        const int rc = make_edge_grids(e, e->h_obst, e->h_tab_off, edge_grid_range(e, agent_params_of(e)), n_eg, "ca_tiled_edge_grid");
        if (rc) return rc;
        free_edge_grids(e->eg);
        e->eg = n_eg;
        e->egrid = true;
    } else {
        e->egrid = false;
        free_edge_grids(e->eg);
    }
    return CA_OK;
}

int ca_tiled_edge_grid_info(ca_env* e, int32_t arena, int32_t* on, int32_t* cells_x, int32_t* cells_y, float* cell_size_x, float* cell_size_y,
                            int32_t* entries) {
    if (!e) return CA_EINVAL;
    if (arena < 0 || arena >= e->cfg.n_arenas) return fail(e, CA_ERANGE, "ca_tiled_edge_grid_info: arena %d of %d", (int)arena, e->cfg.n_arenas);
    const EdgeGridDev* g = e->egrid ? &e->eg.desc[e->eg.desc.size() > 1 ? (size_t)arena : 0] : nullptr;
    if (on) *on = g ? 1 : 0;
    if (cells_x) *cells_x = g ? g->gx : 0;
    if (cells_y) *cells_y = g ? g->gy : 0;
    if (cell_size_x) *cell_size_x = g ? 1.0f / g->ics_x : 0.0f;
    if (cell_size_y) *cell_size_y = g ? 1.0f / g->ics_y : 0.0f;
    if (entries) *entries = g ? (int32_t)g->n_entries : 0;
    return CA_OK;
}

int ca_edge_grid_build(const float* edges_pq, int32_t n_edges, float range, ca_edge_grid_desc* desc, uint32_t* cell_start, int32_t cell_cap,
                       uint32_t* entries, int32_t entry_cap) {
    if (!desc || n_edges < 0 || (n_edges > 0 && !edges_pq)) return fail(nullptr, CA_EINVAL, "ca_edge_grid_build: bad argument");
    static_assert(sizeof(ca_edge_grid_desc) == sizeof(ca_edge_grid::Desc), "one layout");
    static_assert(CA_EDGE_GRID_MAX_EDGES == ca_edge_grid::MAX_EDGES && CA_EDGE_GRID_MAX_ENTRIES == ca_edge_grid::MAX_ENTRIES, "one set of caps");
    ca_edge_grid::Desc d;
    std::vector<uint32_t> cs, en;
    const bool fill = cell_start != nullptr && entries != nullptr;
    const ca_edge_grid::Result r = ca_edge_grid::build(edges_pq, n_edges, range, d, fill ? &cs : nullptr, fill ? &en : nullptr);
    memcpy(desc, &d, sizeof d);
    if (r == ca_edge_grid::TOO_MANY_EDGES)
        return fail(nullptr, CA_ERANGE, "ca_edge_grid_build: the edge grid holds at most %d edges per table, this one has %d", (int)ca_edge_grid::MAX_EDGES,
                    (int)n_edges);
    if (r == ca_edge_grid::TOO_MANY_ENTRIES)
        return fail(nullptr, CA_ERANGE, "ca_edge_grid_build: the edge grid would hold %d%s entries (at most %d): long walls cover many cells -- "
                    "subdivide the walls", (int)d.n_entries, d.n_entries == 0x7FFFFFFF ? "+" : "", (int)ca_edge_grid::MAX_ENTRIES);
    if (r != ca_edge_grid::OK) return fail(nullptr, CA_ERANGE, "ca_edge_grid_build: range %g is not a positive number", (double)range);
    if (!fill) return CA_OK;
    if (cell_cap < 0 || entry_cap < 0 || (size_t)cell_cap < cs.size() || (size_t)entry_cap < en.size())
        return fail(nullptr, CA_ESIZE, "ca_edge_grid_build: cell_start needs %zu words (cell_cap=%d), entries %zu (entry_cap=%d)", cs.size(), (int)cell_cap,
                    en.size(), (int)entry_cap);
    memcpy(cell_start, cs.data(), cs.size() * sizeof(uint32_t));
    if (!en.empty()) memcpy(entries, en.data(), en.size() * sizeof(uint32_t));
    return CA_OK;
}

}  // extern "C"

// ---- forking and rewinding arenas: ca_arena_gather, ca_snapshot_* (ca_fork.h) ---------------------------------------
// THE list of what an arena's state is: every plane that moves, as [A][rows][n] elements of esize bytes.  The scratch set, the
// snapshots and the kernel's descriptor table are all laid out from it, and the header's list of moved fields (include/ca_env.h,
// "State that moves") and VecCollisionAvoidanceEnv._STATE_FIELDS name the same fields (tests/test_fork_cpu.py holds the three
// together).  What is not here stays with the slot: configuration (obstacle tables, per-agent parameters, counts and sensing, ALAN
// action sets, the edge grid), statistics, the contact report, the observation, and seed / arena_offset + a, which key the draws.
// The sort buffers, nv_x / nv_y and tscr of a tiled handle, alan_dirs / alan_u and orient_x / orient_y are scratch or derived.
struct StatePlane { const char* fields; void* ptr; unsigned esize, n, rows; bool per_agent, alan; };
static int state_planes(const ca_env* e, StatePlane* out) {
    const unsigned N = (unsigned)e->cfg.n_agents, K = (unsigned)(e->K > 0 ? e->K : 1), S = (unsigned)e->S, nA = (unsigned)e->n_actions;
    const StatePlane all[] = {
        {"POS_X", e->pos_x, 4, N, 1, true, false},
        {"POS_Y", e->pos_y, 4, N, 1, true, false},
        {"VEL_X", e->vel_x, 4, N, 1, true, false},
        {"VEL_Y", e->vel_y, 4, N, 1, true, false},
        {"PREF_X", e->pref_x, 4, N, 1, true, false},
        {"PREF_Y", e->pref_y, 4, N, 1, true, false},
        {"GOAL_X", e->goal_x, 8, N, 1, true, false},
        {"GOAL_Y", e->goal_y, 8, N, 1, true, false},
        {"GOAL2_X", e->goal2_x, 8, N, 1, true, false},
        {"GOAL2_Y", e->goal2_y, 8, N, 1, true, false},
        {"REWARD", e->reward, 4, N, 1, true, false},
        {"AGENT_DONE", e->agent_done, 4, N, 1, true, false},
        {"ARRIVE_STEP", e->arrive_step, 4, N, 1, true, false},
        {"REGOAL_COUNT", e->regoal_count, 4, N, 1, true, false},
        {"NB_COUNT OBST_COUNT", e->counts, 2, N, 1, true, false},   // one packed u16: agent-neighbour count | obstacle-neighbour count << 8
        {"NB_IDX", e->nb_idx, e->nidx16 ? 2u : 1u, N, K, true, false},
        {"OBST_IDX", e->obst_idx, 2, N, S, true, false},
        {"STEP_COUNT", e->step_count, 4, 1, 1, false, false},
        {"ARENA_DONE", e->arena_done, 4, 1, 1, false, false},
        {"EPISODE", e->episode, 4, 1, 1, false, false},
        {"ALAN_WEIGHTS", e->alan_w, 8, N, nA, true, true},
        {"ALAN_TIMES", e->alan_t, 8, N, nA, true, true},
        {"ALAN_ACTION", e->alan_action, 4, N, 1, true, true},
    };
    static_assert(sizeof all / sizeof all[0] <= FORK_MAX_PLANES, "ca_fork.h ForkArgs holds every plane");
    int n = 0;
    for (const StatePlane& p : all)
        if (!p.alan || e->n_actions > 0) out[n++] = p;
    return n;
}
static size_t state_plane_bytes(const ca_env* e, const StatePlane& p) {
    return (size_t)e->cfg.n_arenas * p.esize * p.n * p.rows;
}
static size_t fork_align(size_t v) { return (v + 255) & ~(size_t)255; }

// the buffers of a set for the handle's present shape; the bandit's part follows n_actions (a change drains the stream first)
static int state_set_reserve(ca_env* e, StateSet& s, const char* who) {
    StatePlane pl[FORK_MAX_PLANES];
    const int n = state_planes(e, pl);
    size_t base = 0, alan = 0;
    for (int k = 0; k < n; ++k) (pl[k].alan ? alan : base) += fork_align(state_plane_bytes(e, pl[k]));
    if (!s.base) {
        const hipError_t r = hipMalloc((void**)&s.base, base);
        if (r != hipSuccess) { s.base = nullptr; return fail(e, CA_EHIP, "%s: %zu bytes for a second set of the state buffers: %s", who, base, hipGetErrorString(r)); }
    }
    if (s.alan_nA != e->n_actions) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (s.alan) HIPCHK(e, hipFree(s.alan));
        s.alan = nullptr; s.alan_nA = 0;
        if (e->n_actions > 0) {
            const hipError_t r = hipMalloc((void**)&s.alan, alan);
            if (r != hipSuccess) { s.alan = nullptr; return fail(e, CA_EHIP, "%s: %zu bytes for the bandit's state: %s", who, alan, hipGetErrorString(r)); }
            s.alan_nA = e->n_actions;
        }
    }
    return CA_OK;
}

// One launch of fork_kernel over every plane.  save: handle -> set, every arena, no index.  Else set -> handle: arena a takes arena
// idx[a] of the set (idx == nullptr: arena a), negative entries -- and with keep_self idx[a] == a -- are not written; the two clearing
// rules and the per-arena counts apply to what is written.
static hipError_t launch_fork(ca_env* e, const StateSet& s, bool save, const int* idx, bool keep_self) {
    StatePlane pl[FORK_MAX_PLANES];
    const int n = state_planes(e, pl);
    ForkArgs f;
    memset(&f, 0, sizeof f);
    size_t off[2] = {0, 0}, most = 0;
    unsigned keep_counts = 0xFFFFu;
    if (!save && !e->h_tab_off.empty()) keep_counts &= 0x00FFu;   // a world per arena: obstacle ids are local to a table, the moved list is void
    if (!save && e->sens) keep_counts &= 0xFF00u;                 // per-agent sensing: a copied list may be longer than its new owner's max_neighbors
    const bool counts = !save && e->ac;
    for (int k = 0; k < n; ++k) {
        unsigned char* in_set = (pl[k].alan ? s.alan : s.base) + off[pl[k].alan];
        off[pl[k].alan] += fork_align(state_plane_bytes(e, pl[k]));
        ForkPlane& p = f.p[k];
        p.src = save ? (const unsigned char*)pl[k].ptr : in_set;
        p.dst = save ? in_set : (unsigned char*)pl[k].ptr;
        p.esize = pl[k].esize; p.n = pl[k].n; p.rows = pl[k].rows;
        p.per_agent = pl[k].per_agent ? 1u : 0u;
        p.keep = pl[k].ptr == (void*)e->counts ? (keep_counts | keep_counts << 16) : 0xFFFFFFFFu;
        const size_t arena_bytes = (size_t)p.esize * p.n * p.rows;
        p.vec = (arena_bytes % 16 == 0 && (uintptr_t)p.src % 16 == 0 && (uintptr_t)p.dst % 16 == 0 && !(counts && pl[k].per_agent)) ? 1u : 0u;
        p.items = (unsigned)(p.vec ? arena_bytes / 16 : (size_t)p.n * p.rows);
        most = std::max(most, (size_t)e->cfg.n_arenas * p.items);
    }
    f.idx = idx; f.counts = counts ? e->d_counts : nullptr; f.A = e->cfg.n_arenas; f.keep_self = keep_self ? 1 : 0;
    // a grid-stride loop: enough workgroups to fill the chip, no more than the largest plane has items for
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((most + FORK_BS - 1) / FORK_BS, (size_t)e->n_cus * 8));
    const dim3 grid(gx, (unsigned)n), block(FORK_BS);
    ProfScope ps(e, KIND_RESET);
    if (idx) {
        if (counts) launch_k(ps, fork_kernel<true, true>, grid, block, 0, e->stream, f);
        else launch_k(ps, fork_kernel<true, false>, grid, block, 0, e->stream, f);
    } else {
        if (counts) launch_k(ps, fork_kernel<false, true>, grid, block, 0, e->stream, f);
        else launch_k(ps, fork_kernel<false, false>, grid, block, 0, e->stream, f);
    }
    return hipGetLastError();
}

// the index array of a gather / load on the host, checked: lo = 0 (gather) or -1 (load: -1 keeps the arena)
static int fork_index(ca_env* e, const char* who, const int32_t* src, size_t bytes, int32_t src_is_device, int lo, std::vector<int>& h) {
    const int A = e->cfg.n_arenas;
    if (bytes != (size_t)A * 4) return fail(e, CA_ESIZE, "%s: the index array holds %zu bytes, got %zu", who, (size_t)A * 4, bytes);
    h.resize(A);
    if (src_is_device) HIPCHK(e, download(e, h.data(), src, (size_t)A * 4));   // (drains the stream)
    else memcpy(h.data(), src, (size_t)A * 4);
    for (int a = 0; a < A; ++a)
        if (h[a] < lo || h[a] >= A)
            return fail(e, CA_ERANGE, "%s: arena %d takes arena %d, outside [%d, n_arenas=%d)", who, a, h[a], lo, A);
    return CA_OK;
}
// per-arena counts: an arena takes the state of an arena of the same size only (from: the counts the source set was saved under)
static int fork_counts_match(ca_env* e, const char* who, const std::vector<int>& h, const std::vector<int>& from, bool keep_self) {
    if (!e->ac && from.empty()) return CA_OK;
    if (e->ac != !from.empty())
        return fail(e, CA_EINVAL, "%s: the snapshot was saved %s per-arena agent counts and the handle now runs %s them", who,
                    from.empty() ? "without" : "with", e->ac ? "with" : "without");
    for (int a = 0; a < (int)h.size(); ++a) {
        if (h[a] < 0 || (keep_self && h[a] == a)) continue;
        if (from[h[a]] != e->h_counts[a])
            return fail(e, CA_EINVAL, "%s: arena %d holds %d agents and would take arena %d, which holds %d (ca_set_agent_counts: an arena "
                        "takes the state of an arena of its own size)", who, a, e->h_counts[a], h[a], from[h[a]]);
    }
    return CA_OK;
}
static int fork_flags(ca_env* e, const char* who, uint32_t flags) {
    if (flags & ~(CA_F_OBS | CA_F_CONTACT)) return fail(e, CA_EINVAL, "%s: flags=0x%x: CA_F_OBS and CA_F_CONTACT only", who, flags);
    return CA_OK;
}
// the state has been written from outside the step kernels: the observation's frame is re-derived, the seeded scan sanitises the lists
static int fork_after(ca_env* e, uint32_t flags) {
    e->orient_valid = false;
    e->lists_trusted = false;
    if (flags & CA_F_OBS) HIPCHK(e, launch_obs(e));
    if (flags & CA_F_CONTACT) HIPCHK(e, launch_contacts(e));
    return CA_OK;
}
static int fork_upload_index(ca_env* e, const std::vector<int>& h) {
    if (!e->fork_idx) HIPCHK(e, hipMalloc((void**)&e->fork_idx, h.size() * 4));
    HIPCHK(e, upload(e, e->fork_idx, h.data(), h.size() * 4));
    return CA_OK;
}

extern "C" {

int ca_arena_gather(ca_env* e, const int32_t* src, size_t bytes, int32_t src_is_device, uint32_t flags) {
    if (!e) return CA_EINVAL;
    if (!src) return fail(e, CA_EINVAL, "ca_arena_gather: null argument");
    { const int rc = fork_flags(e, "ca_arena_gather", flags); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    std::vector<int> h;
    { const int rc = fork_index(e, "ca_arena_gather", src, bytes, src_is_device, 0, h); if (rc) return rc; }
    { const int rc = fork_counts_match(e, "ca_arena_gather", h, e->h_counts, true); if (rc) return rc; }
    { const int rc = state_set_reserve(e, e->fork_scratch, "ca_arena_gather"); if (rc) return rc; }
    { const int rc = fork_upload_index(e, h); if (rc) return rc; }
    HIPCHK(e, launch_fork(e, e->fork_scratch, true, nullptr, false));
    HIPCHK(e, launch_fork(e, e->fork_scratch, false, e->fork_idx, true));
    return fork_after(e, flags);
}

int ca_snapshot_create(ca_env* e, ca_snapshot** out) {
    if (!e) return CA_EINVAL;
    if (!out) return fail(e, CA_EINVAL, "ca_snapshot_create: null argument");
    HIPCHK(e, hipSetDevice(e->device));
    ca_snapshot* sn = new ca_snapshot();
    sn->owner = e;
    const int rc = state_set_reserve(e, sn->set, "ca_snapshot_create");
    if (rc) {
        if (sn->set.base) hipFree(sn->set.base);
        if (sn->set.alan) hipFree(sn->set.alan);
        delete sn;
        return rc;
    }
    e->snapshots.push_back(sn);
    *out = sn;
    return CA_OK;
}

static int snapshot_of(ca_env* e, const char* who, const ca_snapshot* sn) {
    if (!sn) return fail(e, CA_EINVAL, "%s: null argument", who);
    if (std::find(e->snapshots.begin(), e->snapshots.end(), sn) == e->snapshots.end())
        return fail(e, CA_EINVAL, "%s: the snapshot is not one of this handle's (a snapshot belongs to the handle it was created on)", who);
    return CA_OK;
}

int ca_snapshot_save(ca_env* e, ca_snapshot* sn) {
    if (!e) return CA_EINVAL;
    { const int rc = snapshot_of(e, "ca_snapshot_save", sn); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    { const int rc = state_set_reserve(e, sn->set, "ca_snapshot_save"); if (rc) return rc; }
    HIPCHK(e, launch_fork(e, sn->set, true, nullptr, false));
    sn->saved = true;
    sn->n_actions = e->n_actions;
    sn->counts = e->ac ? e->h_counts : std::vector<int>();
    return CA_OK;
}

int ca_snapshot_load(ca_env* e, const ca_snapshot* sn, const int32_t* src, size_t bytes, int32_t src_is_device, uint32_t flags) {
    if (!e) return CA_EINVAL;
    { const int rc = snapshot_of(e, "ca_snapshot_load", sn); if (rc) return rc; }
    { const int rc = fork_flags(e, "ca_snapshot_load", flags); if (rc) return rc; }
    if (!sn->saved) return fail(e, CA_EINVAL, "ca_snapshot_load: nothing has been saved into the snapshot (ca_snapshot_save)");
    if (sn->n_actions != e->n_actions)
        return fail(e, CA_EINVAL, "ca_snapshot_load: the snapshot was saved with n_actions=%d and the handle now has n_actions=%d (ca_alan_configure* "
                    "changed the shape of the bandit's state)", sn->n_actions, e->n_actions);
    HIPCHK(e, hipSetDevice(e->device));
    std::vector<int> h;
    if (src) {
        const int rc = fork_index(e, "ca_snapshot_load", src, bytes, src_is_device, -1, h);
        if (rc) return rc;
    } else {
        h.resize(e->cfg.n_arenas);
        for (int a = 0; a < e->cfg.n_arenas; ++a) h[a] = a;
    }
    { const int rc = fork_counts_match(e, "ca_snapshot_load", h, sn->counts, false); if (rc) return rc; }
    if (src) { const int rc = fork_upload_index(e, h); if (rc) return rc; }
    HIPCHK(e, launch_fork(e, sn->set, false, src ? e->fork_idx : nullptr, false));
    return fork_after(e, flags);
}

int ca_snapshot_destroy(ca_env* e, ca_snapshot* sn) {
    if (!e) return CA_EINVAL;
    { const int rc = snapshot_of(e, "ca_snapshot_destroy", sn); if (rc) return rc; }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));   // a save or a load may still be in flight
    if (sn->set.base) hipFree(sn->set.base);
    if (sn->set.alan) hipFree(sn->set.alan);
    e->snapshots.erase(std::find(e->snapshots.begin(), e->snapshots.end(), sn));
    delete sn;
    return CA_OK;
}

// (diagnostic for tools/fork_cost.py: the bytes of ONE arena that the plane descriptors move, i.e. what a save reads and writes once each)
int ca_fork_bytes_per_arena(ca_env* e, size_t* out) {
    if (!e || !out) return fail(e, CA_EINVAL, "ca_fork_bytes_per_arena: null argument");
    StatePlane pl[FORK_MAX_PLANES];
    const int n = state_planes(e, pl);
    size_t b = 0;
    for (int k = 0; k < n; ++k) b += (size_t)pl[k].esize * pl[k].n * pl[k].rows;
    *out = b;
    return CA_OK;
}

}  // extern "C"
