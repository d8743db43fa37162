/*
 * ca_env.h -- C ABI of libcaenv.so: the MI355X (gfx950) batched collision-avoidance environment.
 *
 * This is the drop-in boundary for the hot path of navallo/collision_avoidance: one call
 * advances A independent arenas x N agents through what the reference does per agent in Python
 * plus per-scalar calls into the external `rvo2` extension.  Citations (file:line) are into
 * /root/reference/collision_avoidance/ : env.py = envs/collision_avoidence_env.py,
 * utils.py = envs/utils.py, ALAN = ALAN/ALAN_true.py.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success, a negative CA_E* code on failure;
 *     ca_last_error() returns the message of the last failure on that handle (NULL handle: of the
 *     last failed ca_create on this thread).
 *   - a handle is bound to one HIP device and one stream; calls are asynchronous on that stream
 *     unless stated otherwise.  A handle is not thread-safe; distinct handles are independent.
 *   - all per-agent arrays are struct-of-arrays fp32/int32 (targets: fp64) of shape [A, N] (agent index
 *     fastest).
 *   - there is NO CPU fallback: without a HIP device ca_create fails with CA_ENODEV.
 */
#ifndef CA_ENV_H
#define CA_ENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CA_OBS_DIM 64 /* env.py:34,53: 16 rays x (hit x, hit y, vel x, vel y) */
#define CA_N_RAYS 16
#define CA_MAX_NEIGHBORS 16      /* largest supported max_neighbors       */
#define CA_MAX_OBST_NEIGHBORS 64 /* largest supported max_obst_neighbors: RVO2 keeps every edge in range (env.py:249,
                                    301-318); 16 covers the reference's own worlds, 64 polyline worlds (subdivided walls,
                                    pillar halls).  Lists above 16 take a kernel of their own (ca_solver_info) and need
                                    n_agents <= 128 and max_neighbors + max_obst_neighbors lines per lane in a CU's LDS:
                                    at 64, n_agents <= 64 with any max_neighbors, n_agents <= 128 with max_neighbors <= 10.
                                    Larger crowds: a tiled handle made with CA_CREATE_TILED_WIDE (ca_create_ex), up to
                                    CA_MAX_AGENTS_LARGE agents with lists of up to 64 and any max_neighbors.
                                    A list that meets more edges in range
                                    than it holds drops the farthest, counts it (ca_stats.obst_overflow) AND makes every
                                    later step call fail with CA_ERANGE: see ca_allow_obstacle_overflow */
#define CA_MAX_AGENTS 1024       /* one workgroup owns one arena; above 256 agents max_neighbors <= 10
                                    is required (LDS capacity: the register-line solve kernels)         */
#define CA_MAX_AGENTS_LARGE 16384 /* agents per arena on a tiled handle (ca_create_ex, CA_CREATE_TILED): an arena
                                    spread over several workgroups                                       */

/* create flags for ca_create_ex */
#define CA_CREATE_TILED 1u /* the tiled solve path: n_agents 1..CA_MAX_AGENTS_LARGE, see ca_create_ex */
#define CA_CREATE_TILED_GRID 4u /* with CA_CREATE_TILED only (flags == 5): the tiled path finds the agent neighbours through a uniform
                                   grid sorted across workgroups, see ca_create_ex.  Bit 2u is NOT a flag: it stays unknown
                                   (CA_EINVAL), as does bit 8u and every bit above 32u */
#define CA_CREATE_TILED_PARAMS 16u /* with CA_CREATE_TILED only (flags == 17 or 21): the tiled handle takes ca_set_agent_params, see
                                      ca_create_ex */
#define CA_CREATE_TILED_WIDE 32u /* with CA_CREATE_TILED only (flags == 33 or 37), never with CA_CREATE_TILED_PARAMS: the tiled handle
                                    takes max_obst_neighbors up to CA_MAX_OBST_NEIGHBORS, see ca_create_ex */

/* error codes */
#define CA_OK 0
#define CA_EINVAL (-1)
#define CA_ENODEV (-2)
#define CA_EHIP (-3)
#define CA_ESIZE (-4)
#define CA_ERANGE (-5)

/* done_mode: who decides that an agent has finished */
#define CA_DONE_XLESS 0  /* env.py:352-365: pos.x < done_x_thresh -> done, goal <- goal2      */
#define CA_DONE_GOAL 1   /* ALAN:547-566: |pos - goal| < 2 r -> done, goal <- goal2           */
#define CA_DONE_REGOAL 2 /* synthetic workload: |pos - goal| < 2 r -> draw a new goal         */

/* step flags */
#define CA_F_OBS 1u       /* write the laser observation (env.py:231-277, utils.py:42-113)     */
#define CA_F_STATS 2u     /* count collisions (build-defined)                   */
#define CA_F_AUTORESET 4u /* arenas that finished are reset (env.py:461-488) inside the call   */
#define CA_F_NODONE 8u    /* ca_orca_step only: no done test, no step counter (env.py:447-450) */
#define CA_F_FREEZE 16u   /* an arena whose arena_done flag is set is not advanced any more: the
                             `break` of the reference's episode loops (ALAN:121-123), per arena,
                             without a host round trip.  ca_reset clears the flag.                */
#define CA_F_CONTACT 32u  /* leave the per-agent contact report of the state this call leaves (ca_get_contacts): one small
                             launch behind the call's own, consumed on the host -- no kernel sees the bit            */
#define CA_ALAN_MAX_ACTIONS 32

/* scenarios for ca_init_scenario */
#define CA_SCN_CROWD 0   /* ALAN:270-294 random start / random goal                            */
#define CA_SCN_CIRCLE 1  /* ALAN:297-330 circle swap                                           */
#define CA_SCN_DOORWAY 2 /* env.py:77-123 the reference env's own world                        */
#define CA_SCN_CONGESTED 3 /* ALAN:175-210 */
#define CA_SCN_INCOMING 4  /* ALAN:213-267 */
#define CA_SCN_BLOCKS 5    /* ALAN:333-374 (block obstacles come through ca_set_obstacles)       */
#define CA_SCN_DEADLOCK 6  /* ALAN:377-457 */
#define CA_SCN_CROWD_SEPARATED 7 /* the crowd with rejection-sampled starts >= 2 r apart (SURVEY 8d bench variant) */

/* fields for ca_get / ca_set / ca_field_ptr */
enum ca_field {
    CA_FLD_POS_X = 0, CA_FLD_POS_Y, CA_FLD_VEL_X, CA_FLD_VEL_Y, CA_FLD_PREF_X, CA_FLD_PREF_Y,
    CA_FLD_GOAL_X, CA_FLD_GOAL_Y, CA_FLD_GOAL2_X, CA_FLD_GOAL2_Y, /* f64 [A,N]: the reference keeps its
                                   targets as Python floats (env.py:94, ALAN:186) and derives the
                                   preferred velocity from them in fp64 */
    CA_FLD_REWARD,       /* f32 [A,N]                                             */
    CA_FLD_AGENT_DONE,   /* i32 [A,N]                                             */
    CA_FLD_ARRIVE_STEP,  /* i32 [A,N]                                             */
    /* the neighbour lists left by the last doStep (sim.getAgentNumAgentNeighbors / getAgentAgentNeighbor /
       getAgentNumObstacleNeighbors / getAgentObstacleNeighbor, env.py:246-249, 283-285, 305-306).  i32 at this
       boundary; the device keeps them packed (u16 counts, u8 / u16 ids), so ca_get / ca_set convert and
       ca_field_ptr refuses them */
    CA_FLD_NB_COUNT,     /* i32 [A,N]   ORCA agent-neighbour count                */
    CA_FLD_NB_IDX,       /* i32 [A,K,N] ORCA agent neighbours, nearest first      */
    CA_FLD_OBST_COUNT,   /* i32 [A,N]                                             */
    CA_FLD_OBST_IDX,     /* i32 [A,S,N] ORCA obstacle-edge neighbours: edge ids of the arena's processed table */
    CA_FLD_OBS,          /* f32 [A,N,64]                                          */
    CA_FLD_STEP_COUNT,   /* i32 [A]                                               */
    CA_FLD_ARENA_DONE,   /* i32 [A]                                               */
    CA_FLD_EPISODE,      /* i32 [A]                                               */
    CA_FLD_REGOAL_COUNT, /* i32 [A,N]                                             */
    CA_FLD_ALAN_WEIGHTS, /* f64 [A,n_actions,N] ALAN:75 self.weights (after ca_alan_configure);
                            agent index fastest like every other per-agent array                  */
    CA_FLD_ALAN_TIMES,   /* f64 [A,n_actions,N] ALAN:76 self.times                                 */
    CA_FLD_ALAN_ACTION,  /* i32 [A,N] the action executed by the last ca_alan_step (read-only)     */
    CA_FLD_ARENA_STATS,  /* u64 [A,8] per-arena counters (read-only): episodes, collisions, obst_collisions,
                            goals_reached, obst_overflow, sum_reward (f64 bits), steps sat out under
                            CA_F_FREEZE, last finished episode (length << 32 | agents that arrived)   */
    CA_FLD__COUNT
};

/* Units and magnitudes.  The kernels compute in fp32 with a correctly rounded division and square root that omit the
 * range-scaling steps of the general sequences (exact where quotients, discriminants and lengths stay well inside the normal
 * range: csrc/ca_math.h).  That holds for worlds in units of O(1) -- the reference's are metres and seconds: radius 0.5,
 * max_speed 1, time_step 1/60, arenas of 10-50 (env.py:26-44, ALAN_true.py:14-20) -- and is ENFORCED at the boundary:
 * ca_create refuses (CA_ERANGE) a configuration outside the ranges below, ca_set_obstacles a vertex beyond CA_MAX_COORD
 * or an edge shorter than CA_MIN_EDGE.  Positions and targets handed in through ca_set / ca_reset are device data and are
 * not checked: keep them within CA_MAX_COORD of the origin. */
#define CA_MIN_LENGTH 1e-3f      /* radius, max_speed, neighbor_dist, time_horizon, time_horizon_obst: [1e-3, 1e3] */
#define CA_MAX_LENGTH 1e3f
#define CA_MIN_TIME_STEP 1e-4f   /* time_step: [1e-4, 10] */
#define CA_MAX_TIME_STEP 10.0f
#define CA_MAX_COORD 1e5f        /* obstacle vertices, spawn / goal boxes: |x|, |y| <= 1e5 */
#define CA_MIN_EDGE 1e-4f        /* an obstacle edge is at least this long */

/* Replaces the constants the reference hard-codes in Collision_Avoidance_Env.__init__
 * (env.py:27-44), the literal at env.py:130, and the per-call arguments of
 * rvo2.PyRVOSimulator / addAgent (env.py:62-68, 126-133; ALAN:22-28). */
typedef struct ca_config {
    int32_t n_arenas;           /* arenas owned by this handle (this GPU's shard)             */
    int32_t n_agents;           /* agents per arena, 1..CA_MAX_AGENTS                         */
    int64_t arena_offset;       /* global id of arena 0: keys the scenario RNG, so results do
                                   not depend on how arenas are sharded over GPUs             */
    uint64_t seed;
    double reward_scale;        /* env.py:396 (0.3); ALAN:47 gamma (0.6)                      */
    float time_step;            /* env.py:27                                                  */
    float neighbor_dist;        /* env.py:28 / ALAN:16                                        */
    int32_t max_neighbors;      /* env.py:29 / ALAN:17, 0..CA_MAX_NEIGHBORS                   */
    float time_horizon;         /* env.py:30                                                  */
    float time_horizon_obst;    /* env.py:130                                                 */
    float radius;               /* env.py:31                                                  */
    float max_speed;            /* env.py:32                                                  */
    int32_t max_obst_neighbors; /* capacity of the obstacle-neighbour list, 1..CA_MAX_OBST_NEIGHBORS (64);
                                   above 16: ca_create returns CA_ERANGE for shapes whose line table
                                   does not fit a CU's LDS (see CA_MAX_OBST_NEIGHBORS);
                                   overflow is counted in ca_stats.obst_overflow and is an error
                                   (CA_ERANGE) unless ca_allow_obstacle_overflow accepted it    */
    int32_t max_step;           /* env.py:44; <= 0: no cap                                    */
    int32_t done_mode;
    float done_x_thresh;        /* env.py:359                                                 */
    float spawn_x0, spawn_x1, spawn_y0, spawn_y1; /* reset() spawn box, env.py:478            */
    float goal_x0, goal_x1, goal_y0, goal_y1;     /* CA_DONE_REGOAL draw box                  */
} ca_config;

typedef struct ca_stats {
    uint64_t agent_steps;     /* counted IN the solve kernels: per arena, the steps it was really advanced, x its agents */
    uint64_t episodes;
    uint64_t collisions;      /* overlapping agent pairs after the update, summed over steps  */
    uint64_t obst_collisions; /* agents overlapping an obstacle edge, summed over steps       */
    uint64_t goals_reached;
    uint64_t obst_overflow;
    double sum_reward;
} ca_stats;

typedef struct ca_env ca_env;

/* Replaces Collision_Avoidance_Env.__init__ + rvo2.PyRVOSimulator(...) (env.py:26-74, 62-68).
 * device: HIP device ordinal.  stream: a hipStream_t to run on (e.g. PyTorch's current stream),
 * or NULL to let the handle create its own. */
int ca_create(const ca_config* cfg, int device, void* stream, ca_env** out);
/* ca_create with create flags; ca_create(cfg, ...) is ca_create_ex(cfg, 0, ...).  Unknown flag bits -> CA_EINVAL.
 * CA_CREATE_TILED: one large crowd in one world (the reference's Collision_Avoidance_Env(numAgents) / Collision_Avoidance_Sim(numAgents)
 * take any number).  n_agents may be 1..CA_MAX_AGENTS_LARGE (above -> CA_ERANGE, "out of range"); max_obst_neighbors <= 16 (above,
 * without CA_CREATE_TILED_WIDE -> CA_ERANGE: wide lists have no tiled form; with it, below: up to 64); max_neighbors 0..16 at any size.
 *   - The handle runs the tiled kernels whatever its size (below 1025 agents: for comparison and tests): one lane per agent, an
 *     arena spread over ceil(n_agents / tile) workgroups, a step in three launches on the handle's stream -- solve (neighbour
 *     search over the whole arena, N^2 per arena; lines; LP), advance (integration, reward, goal / wall tests), close (pair count,
 *     end of episode, in-kernel reset) -- ca_tiled_info.  Results are the CPU oracle's and the ordinary handle's bit for bit;
 *     ca_stats.sum_reward is added in another order (1e-9 relative).
 *   - Every step, reset, scenario, field, obstacle-table and ALAN call works as on an ordinary handle, with all step flags and the
 *     sticky overflow error; ca_rollout is T times the three launches, ca_alan_step / ca_alan_rollout take the three-launch form
 *     around them (select, solve, update); neighbour ids are 16 bits on the device.
 *   - ca_set_agent_params (without CA_CREATE_TILED_PARAMS, below) and ca_set_agent_counts -> CA_EINVAL; the handle keeps working.
 *   - ca_solver_info reports lanes_per_agent = 1, rollout_one_launch = 0; ca_launch_info the first of the three launches;
 *     ca_profile counts each of the three launches on its own under kind 1.
 * CA_CREATE_TILED | CA_CREATE_TILED_GRID (flags == 5; CA_CREATE_TILED_GRID alone -> CA_EINVAL: the grid is the tiled path's): a tiled
 * handle in every respect above -- limits, refusals, 16-bit ids, step flags, sticky overflow error, ALAN in the three-launch form
 * around the solve, ca_rollout = T times the launches of a step -- that differs in three ways:
 *   - the agent-neighbour list is found through a uniform grid instead of the scan of the whole arena: a fixed, wrapped table of
 *     cells_x x cells_y cells (powers of two chosen from n_agents), cells half a neighbour range wide (ca_tiled_grid_info), the
 *     arena's agents counting-sorted by cell every step, an agent testing the cells its range touches.  The lists it leaves
 *     (CA_FLD_NB_*, CA_FLD_OBST_*) are the same, order included: the same K smallest (distance, index) keys;
 *   - a step is sort_launches more launches in front of the solve (bin, scan, scatter): ca_tiled_info reports
 *     launches_per_step = sort_launches + 3, and ca_profile counts each under kind 1;
 *   - ca_launch_info reports the first launch of the sequence (the bin launch: no dynamic LDS).
 *   The sort's buffers belong to the handle and are no part of its state (no field reads them).  CA_TILED_CELLS=<g> (a power of
 *   two, 8 .. 128; diagnostic switch latched here, like CA_TILE) forces a g x g table.
 * CA_CREATE_TILED_PARAMS, together with CA_CREATE_TILED (flags == 17: the plain tiled handle, 21: the grid handle; without
 * CA_CREATE_TILED, or with bit 2u or 8u -> CA_EINVAL): the tiled handle of those flags that also takes ca_set_agent_params --
 * a heterogeneous crowd of up to CA_MAX_AGENTS_LARGE agents in one world.  Opt-in at create, like the grid: the tiled path fixes
 * its kernel family when the handle is made, and a handle made without the flag keeps refusing the call.
 *   - Until parameters are set the handle runs the uniform tiled kernels: the launches and the bits of flags 1 / 5.
 *   - ca_set_agent_params behaves as on an ordinary handle (value checks, CA_ESIZE, drains the stream, configuration that survives
 *     resets and scenarios, a failure leaves the handle as it was, four NULLs return to the uniform kernels; ca_get_agent_params,
 *     ca_agent_params_info).  No LDS misfit exists: the tile's line table is sized at create.
 *   - While parameters are set the solve, advance and close launches are their per-agent twins (the same number of launches;
 *     results are the ordinary per-agent handle's and the oracle's bit for bit), every call of a tiled handle works, and the
 *     observation takes every neighbour's own octagon.  The pair count (CA_F_STATS) counts a pair within r_i + r_j.
 *   - The static edge grid (ca_tiled_edge_grid) is built for the LARGEST obstacle range tho_i * ms_i + r_i of the handle, in fp32:
 *     that range is the cell size and the margin of an edge's bounding box.  Setting and clearing the parameters rebuild the grids
 *     while the edge grid is on (a refused rebuild fails the call and changes nothing); switching it on afterwards uses the same
 *     range.  The walk's corner rule does not depend on the cell size, so an agent of a smaller range walks fewer cells.
 *   - ca_set_agent_counts stays CA_EINVAL; neighbor_dist and max_neighbors per agent come through ca_set_agent_sensing, which these
 *     handles (and no other tiled handle) accept.
 * CA_CREATE_TILED_WIDE, together with CA_CREATE_TILED (flags == 33: the plain tiled handle, 37: the grid handle; without
 * CA_CREATE_TILED, with CA_CREATE_TILED_PARAMS -- per-agent parameters go with lists of up to 16, as on ordinary handles --, or with
 * bit 2u or 8u -> CA_EINVAL): the tiled handle of those flags with max_obst_neighbors 1..CA_MAX_OBST_NEIGHBORS -- a large crowd in a
 * polyline world (a pillar hall puts 30 to 60 edges in range of an agent) without truncated obstacle lists.  Opt-in at create, like
 * the grid: the tiled path fixes its kernel family when the handle is made.
 *   - With max_obst_neighbors <= 16 the handle IS the handle of flags 1 / 5: the same kernels, launches and bits.
 *   - With max_obst_neighbors > 16 the solve launch and the observation are their wide twins: the sorted obstacle list is built in
 *     the tile's LDS line table (max_neighbors + max_obst_neighbors lines per lane), the results are the oracle's and the ordinary
 *     wide handle's bit for bit, the lists (CA_FLD_OBST_*) the same, order included.  The number of launches does not change, nor
 *     does anything else of a tiled handle: limits, 16-bit ids, step flags, the sticky overflow error, ca_rollout, ALAN in the
 *     three-launch form, per-arena obstacle tables, ca_tiled_edge_grid on the grid handle, the two refusals above.  Installing small
 *     or large worlds does not change its kernels.
 *   - The tile of such a handle is 64 agents (ca_tiled_info; the table is bounded by LDS per lane: DESIGN.md 7i).  CA_TILE=128 or 256
 *     is honoured where tile x ((max_neighbors + max_obst_neighbors) x 16 + 8) bytes fit the 160 KiB of LDS of a CU; where they do
 *     not, ca_create_ex -> CA_ERANGE.  Nothing is launched above the limit. */
int ca_create_ex(const ca_config* cfg, uint32_t create_flags, int device, void* stream, ca_env** out);
int ca_destroy(ca_env* env);
const char* ca_last_error(const ca_env* env);
/* Run on the caller's stream from now on (hipStream_t; NULL = the device's default stream).
 * The previous stream is drained first. */
int ca_set_stream(ca_env* env, void* stream);

/* Replaces sim.addObstacle + sim.processObstacles (env.py:118-123, 143-149): the same polygons
 * for every arena (see ca_set_obstacles_per_arena for a world per arena).  verts_xy: host array [sum(poly_sizes), 2].  Like the RVO2 library's
 * processObstacles, edges that cross the supporting line of a splitting edge of its obstacle tree are cut
 * there; the cut points are appended to the vertex table behind the caller's vertices. */
int ca_set_obstacles(ca_env* env, const float* verts_xy, const int32_t* poly_sizes, int32_t n_poly);
/* Replaces sim.getObstacleVertex / getNextObstacleVertexNo (env.py:148, 208, 307-311): the processed
 * vertex table.  Edge i runs from vertex i to vertex next[i]; these are the ids in CA_FLD_OBST_IDX.
 * Host arrays of capacity `cap` (each may be NULL); *n_out = number of vertices. */
int ca_get_obstacles(ca_env* env, float* verts_xy, int32_t* next, int32_t* convex, int32_t cap, int32_t* n_out);
/* A world of its own for every arena: the reference builds a simulator per environment and draws the four blocks of
 * the "blocks" world anew for each (ALAN:359-372: addObstacle x 5 + processObstacles per simulator; reset() redraws
 * them, ALAN:92-100; the trainer averages over such worlds, Train_ALAN_action_space.py:53-66).
 * n_poly: host array [A], polygons of arena a; poly_sizes / verts_xy: all arenas' polygons back to back.
 * Each arena gets its own processed table; obstacle-neighbour ids (CA_FLD_OBST_IDX) are local to it. */
int ca_set_obstacles_per_arena(ca_env* env, const float* verts_xy, const int32_t* poly_sizes, const int32_t* n_poly);
/* ca_get_obstacles for the table of one arena (the common table if ca_set_obstacles installed one). */
int ca_get_obstacles_arena(ca_env* env, int32_t arena, float* verts_xy, int32_t* next, int32_t* convex, int32_t cap,
                           int32_t* n_out);

/* Replaces the per-agent arguments of sim.addAgent (env.py:126-133; ALAN:81-87) / setAgentRadius, setAgentMaxSpeed,
 * setAgentTimeHorizon, setAgentTimeHorizonObst: a crowd of large and small, slow and fast agents, or arenas that differ in these
 * values (domain randomisation).  Each array: f32 [A,N] (host or device), or NULL = every agent keeps the handle's ca_config value
 * for that parameter.  All four NULL: the handle returns to uniform parameters and to the kernels it used before.
 *   - Configuration, like the obstacle tables, not state: the values persist across ca_reset, ca_reset_masked, CA_F_AUTORESET and
 *     ca_init_scenario, and are not a ca_field.  The scenario generators and the spawn boxes keep using ca_config.radius.
 *   - neighbor_dist and max_neighbors stay per handle in this call: they size the neighbour-key image, the search grid, the ray
 *     table of the observation and the kernels' K classes.  ca_set_agent_sensing (below) takes them per agent, with the handle's
 *     values as capacities.
 *   - Every value is checked (a device array is copied back for the check): a value that is not finite or lies outside
 *     [CA_MIN_LENGTH, CA_MAX_LENGTH] -> CA_ERANGE (ca_last_error names the parameter, the arena and the agent);
 *     bytes_each != A*N*4 -> CA_ESIZE; a handle with max_obst_neighbors > 16 -> CA_EINVAL (not together with wide obstacle lists);
 *     a shape whose LDS line table does not fit a CU (lanes x (16 (max_neighbors + max_obst_neighbors) + 36) bytes plus the
 *     neighbour search's arrays > 160 KiB: e.g. 512 agents with max_neighbors 10 and lists of 16) -> CA_ERANGE.  On any failure the
 *     handle keeps its previous parameters and kernels.
 *   - While the parameters are set the handle runs one lane per agent on the LDS line table, an instantiation of its own, whatever
 *     the world and the batch size (CA_QUAD / CA_PAIR / CA_REG_LINES are ignored): ca_solver_info reports lanes_per_agent = 1,
 *     rollout_one_launch = 0, ca_rollout is T launches, ca_alan_step / ca_alan_rollout take the three-launch form (select, solve,
 *     update; one action set or one per arena).  The observation sees neighbour j as the octagon of radius r_j (env.py:335-350).
 *     Results are the CPU oracle's with these values per agent, bit for bit; arrays equal to the ca_config values give the
 *     uniform handle's bits. */
int ca_set_agent_params(ca_env* env, const float* radius, const float* max_speed, const float* time_horizon,
                        const float* time_horizon_obst, size_t bytes_each, int32_t src_is_device);
/* The four arrays as the kernels use them (the ca_config value for every agent on a handle with uniform parameters); any may be NULL. */
int ca_get_agent_params(ca_env* env, float* radius, float* max_speed, float* time_horizon,
                        float* time_horizon_obst, size_t bytes_each, int32_t dst_is_device);
/* *per_agent = 1 while per-agent parameters are set (the AgentParams kernels run), else 0. */
int ca_agent_params_info(ca_env* env, int32_t* per_agent);

/* Arenas of different crowd sizes in one batch: the reference's one constructor argument, Collision_Avoidance_Env(numAgents)
 * (env.py:23-60), per arena.  counts: i32 [A], host or device; NULL = every arena holds n_agents again and the handle returns to
 * the kernels it used before.
 *   - Layout: every array keeps its shape and strides ([A,N], [A,K,N], [A,N,64]; N = ca_config.n_agents, now a capacity).  Arena a
 *     consists of agents 0 .. counts[a]-1; rows i >= counts[a] are absent.
 *   - An absent agent is nobody's neighbour and casts no octagon into anybody's observation.  It is not in the done test (an
 *     arena's episode is over when all of its counts[a] agents are done, or at the step cap) and in no statistic:
 *     ca_stats.agent_steps grows by counts[a] per step of arena a, and the "agents that arrived" half of the last-episode word is
 *     out of counts[a].
 *   - From the call on the observation row and the reward of an absent row read 0, and its two list counts read 0.  No kernel
 *     writes any other field of an absent row -- not ca_step / ca_orca_step / ca_rollout, not ca_reset (the caller's position
 *     arrays included), ca_reset_masked or CA_F_AUTORESET: an absent row keeps what the caller last put there.
 *   - Configuration, like the agent parameters and the obstacle tables, not state: the counts persist across ca_reset*,
 *     CA_F_AUTORESET and ca_init_scenario, and are not a ca_field.
 *   - The call drains the stream and clears the agent- and obstacle-neighbour counts of EVERY arena (the old lists may name agents
 *     that are gone; a fresh simulator has empty lists).  It touches nothing else.  counts[a] == n_agents for every arena is
 *     allowed and still selects the kernels described below.
 *   - bytes != A*4 -> CA_ESIZE; a count outside [1, n_agents] -> CA_ERANGE (ca_last_error names the arena and the value); a handle
 *     with max_obst_neighbors > 16 -> CA_EINVAL; a shape whose LDS line table does not fit a CU -> CA_ERANGE (as for
 *     ca_set_agent_params).  On any failure the handle keeps its previous counts and kernels.
 *   - Not supported while counts are set (CA_EINVAL, the message says so): ca_init_scenario for every scenario but CA_SCN_DOORWAY
 *     (the other generators' geometry is a function of the number of agents; the doorway's is not and works unchanged, for all N
 *     rows), ca_alan_configure*, ca_alan_step and ca_alan_rollout.
 *   - Composes with ca_set_agent_params, in either order; clearing one keeps the other.
 *   - While counts are set the handle runs one lane per agent on the LDS line table (the per-agent-parameter kernels with a count
 *     per arena; without parameters of the caller's the per-agent arrays hold the ca_config values, whose bits are the uniform
 *     handle's): ca_solver_info reports lanes_per_agent = 1, rollout_one_launch = 0, ca_rollout is T launches.  An arena keeps its
 *     N-lane slot and absent lanes idle.  CA_F_FREEZE, ca_step_packed and the overflow error work as before.  Arena a computes
 *     what a handle of one arena with n_agents = counts[a] and arena_offset + a computes, bit for bit (no random stream is keyed
 *     by n_agents); sum_reward is added in another order (1e-9 relative). */
int ca_set_agent_counts(ca_env* env, const int32_t* counts, size_t bytes, int32_t src_is_device);
/* The counts as the kernels use them (n_agents everywhere on a uniform handle). */
int ca_get_agent_counts(ca_env* env, int32_t* counts, size_t bytes, int32_t dst_is_device);
/* *per_arena = 1 while counts are set (the ArenaCounts kernels run), else 0. */
int ca_agent_counts_info(ca_env* env, int32_t* per_arena);

/* The two remaining per-agent arguments of sim.addAgent (env.py:126-133; ALAN:81-87), neighborDist and maxNeighbors: how far an agent
 * looks and how many others it attends to -- attentive and distracted pedestrians in one crowd, or a perception range per arena.
 * neighbor_dist: f32 [A,N], max_neighbors: i32 [A,N] (host or device); NULL = every agent keeps the handle's ca_config value for
 * that parameter.  Both NULL: the handle returns to the kernels it ran before.
 *   - The ca_config values become CAPACITIES, as n_agents does under ca_set_agent_counts: neighbor_dist_i must be finite and lie in
 *     [CA_MIN_LENGTH, ca_config.neighbor_dist], max_neighbors_i in [0, ca_config.max_neighbors]; anything else -> CA_ERANGE
 *     (ca_last_error names the parameter, the arena and the agent).  The capacities keep sizing the kernels' K class, the [A,K,N]
 *     list layout, the LDS line table, the search grids and the neighbour-key image.
 *   - Semantics, exactly RVO2's computeAgentNeighbors: agent i's list holds the max_neighbors_i smallest (squared distance, index)
 *     keys among the other agents j with fl(dx^2) + fl(dy^2) < fl(neighbor_dist_i * neighbor_dist_i) (fp32), nearest first, ties to the
 *     lower index; slots at or beyond the count read -1.  Lists are asymmetric: i may see j while j does not see i.
 *   - The observation's laser range stays ca_config.neighbor_dist: the ray table belongs to the environment (env.py:321-332), not
 *     to the agent.  The observation enumerates the lists (env.py:283-285) and so follows them with no rule of its own.
 *   - Configuration, not state: it persists across ca_reset, ca_reset_masked, CA_F_AUTORESET and ca_init_scenario and is not a ca_field.
 *   - The call drains the stream and clears the agent-neighbour count of every row of every arena (a list left by the last step may
 *     be longer than its agent's new max_neighbors; the next step rebuilds them).  It touches nothing else.
 *   - bytes_each != A*N*4 -> CA_ESIZE; a handle with max_obst_neighbors > 16 -> CA_EINVAL; a shape whose LDS line table does not fit
 *     a CU -> CA_ERANGE (as for ca_set_agent_params); a NULL handle -> CA_EINVAL.  On any failure the handle keeps what it had.
 *   - While set, an ordinary handle runs the one-lane LDS-line-table kernels of ca_set_agent_params, in an instantiation of their
 *     own (ca_solver_info: lanes_per_agent = 1, rollout_one_launch = 0; ALAN in the three-launch form); the four per-agent
 *     parameter arrays hold the ca_config values unless the caller set them, as under counts.
 *   - Composes with ca_set_agent_params and ca_set_agent_counts in any order; clearing one keeps the others.  An absent row's values
 *     are checked but never read.
 *   - Tiled handles: only those made with CA_CREATE_TILED_PARAMS (flags 17 and 21) accept it, every other tiled handle -> CA_EINVAL
 *     and keeps working.  The number of launches does not change and the sort launches are the uniform handle's (the cells stay
 *     half the handle's neighbor_dist wide; an agent walks the cells of its own range).  The pair count's shortcut through the
 *     lists takes the agent's own range and list length.
 * Results are the CPU oracle's with these values per agent, bit for bit; arrays equal to the ca_config values give the bits of the
 * same handle without them. */
int ca_set_agent_sensing(ca_env* env, const float* neighbor_dist, const int32_t* max_neighbors, size_t bytes_each, int32_t src_is_device);
/* The two arrays as the kernels use them (the ca_config value for every agent on a handle without per-agent sensing); either may be NULL. */
int ca_get_agent_sensing(ca_env* env, float* neighbor_dist, int32_t* max_neighbors, size_t bytes_each, int32_t dst_is_device);
/* *per_agent = 1 while per-agent sensing is set (the AgentSensing kernels run), else 0. */
int ca_agent_sensing_info(ca_env* env, int32_t* per_agent);

/* The agent-neighbour scan of arenas of at most 64 agents starts each agent's list from the one the last step left in memory and runs
 * the sorted insertion only for candidates that some agent of the wave can still take (the SeededScan kernels).  Results are the
 * same bits; lists written through ca_set, or left by a reset or another state, are sanitised, never trusted.  *seeded = 1 if a plain
 * ca_step of this handle launches such a kernel, else 0: arenas above 64 agents, tiled handles, handles on the four-lanes kernel,
 * per-agent parameters or sensing and obstacle lists above 16 have none.  CA_NBR_SEED=0 in the environment when the handle is made
 * (a diagnostic switch, like CA_QUAD) keeps the handle on the unseeded kernels. */
int ca_nbr_seed_info(ca_env* env, int32_t* seeded);

/* The LP3 stage of the one-wave register-line solve kernels (arenas of at most 64 agents, K <= 10, obstacle lists of 4) solves a wave's
 * infeasible agents cooperatively, 16 at a time with four lanes each.  The PairedLp3 kernels take a wave with 17 to 32 of them in one
 * round instead, two lanes per agent; the results are the same bits.  *paired = 1 if a plain ca_step of this handle launches such a
 * kernel, else 0.  CA_LP3_PAIRS=0 / 1 in the environment when the handle is made (a diagnostic switch, like CA_NBR_SEED) selects the
 * kernel without / with the tag on one library. */
int ca_lp3_pairs_info(ca_env* env, int32_t* paired);

/* Replaces _init_world's agent loop (env.py:86-97) / ALAN's scenario generators (ALAN:175-457).  Runs on the device: every
 * agent's heading, start and targets come from the handle's counter-based streams (keyed by the global arena id) or, for
 * the layouts that do not depend on the arena, from a per-agent table made once on the host (its cos / sin / sqrt are
 * libm's); only the rejection-sampled starts of CA_SCN_CROWD_SEPARATED are drawn on the host (sequential per arena). */
int ca_init_scenario(ca_env* env, int32_t scenario);

/* Replaces the per-scalar getters/setters (sim.getAgentPosition, setAgentPosition, ...
 * env.py:157, 237, 479): whole-array copies.  *_is_device: the caller's pointer is device memory. */
int ca_set(ca_env* env, int32_t field, const void* src, size_t bytes, int32_t src_is_device);
int ca_get(ca_env* env, int32_t field, void* dst, size_t bytes, int32_t dst_is_device);
/* Page-locked, device-visible host memory owned by the handle (freed by ca_host_free or ca_destroy): the destination of the
 * host-array calls at the link's rate instead of a pageable copy's, and an action buffer the kernels read where it lies. */
int ca_host_alloc(ca_env* env, size_t bytes, void** out);
int ca_host_free(ca_env* env, void* p);
/* Zero-copy view of a field's device buffer (valid until ca_destroy / ca_bind_obs). */
int ca_field_ptr(ca_env* env, int32_t field, void** dev_ptr, size_t* bytes);
/* Let the caller own the observation buffer (e.g. a torch tensor [A,N,64] f32 on this device). */
int ca_bind_obs(ca_env* env, void* dev_ptr, size_t bytes);

/* Replaces reset() (env.py:461-488).  pos_x/pos_y: device or host arrays [A,N] with the new
 * positions, or NULL to draw them from the spawn box with the counter-based RNG. */
int ca_reset(ca_env* env, const float* pos_x, const float* pos_y, int32_t pos_is_device, uint32_t flags);

/* The same for the arenas with mask[a] != 0 only, positions drawn from the spawn box: what a vector-env
 * front end needs for reset_at(index) / try_reset(env_id).  mask: i32 [A], device or host. */
int ca_reset_masked(ca_env* env, const int32_t* mask, int32_t mask_is_device, uint32_t flags);

/* Replaces step(action) (env.py:367-416).  actions: DEVICE array [A,N] f32 of heading offsets. */
int ca_step(ca_env* env, const float* actions, uint32_t flags);
/* Same, with the actions in HOST memory (copied to the device on the handle's stream). */
int ca_step_host(ca_env* env, const float* actions_host, uint32_t flags);
/* A whole host-side step in ONE round trip -- what one environment per worker needs (run_rllib.py:77, 108; env.py:367-416: the
 * four dictionaries every step): actions in (NULL: the ORCA-only step, env.py:447-458), then
 *   out_host = [ observation A*N*64 f32 | reward A*N f32 | arena_done A i32 | step_count A i32 ]
 * in one device-to-host copy and one synchronisation (ca_step_host + three ca_get make four).  out_bytes must be the size of
 * that layout.  Buffers from ca_host_alloc make the copy run at the link's rate; an action buffer from ca_host_alloc is read by
 * the kernel where it lies.  Without CA_F_OBS the observation part holds the last one computed. */
int ca_step_packed(ca_env* env, const float* actions_host, uint32_t flags, void* out_host, size_t out_bytes);
/* Replaces orca_step (env.py:447-458; ALAN:631-636 + the done test of ALAN:118-121). */
int ca_orca_step(ca_env* env, uint32_t flags);
/* Replaces _get_obs() alone (env.py:231-277): recompute the observation of the current state. */
int ca_observe(ca_env* env);
/* The per-agent contact report: who touches whom, the nearest neighbour, the walls -- what a per-agent `infos` entry, a collision
 * or discomfort-distance penalty or a termination rule needs, without copying the positions back for an O(N^2) scan on the host.
 * (CA_F_STATS counts the same events, per arena.)  For every agent i of every arena, of the state a call leaves, in fp32, one
 * operation per source operation, in the order of the statistics' own pair and wall tests:
 *   agents      i32  number of other present agents j of the same arena with absSq(p_i - p_j) < sqr(r_i + r_j)
 *   wall        i32  1 if distSqPointSegment(edge, p_i) < sqr(r_i) for any edge of the arena's processed table, else 0
 *   nearest     i32  the j != i with the smallest key (absSq(p_i - p_j), j) -- ties go to the smaller index --, or -1 when the arena
 *                    holds one agent
 *   nearest_d2  f32  that squared distance, or +inf when nearest is -1
 *   wall_d2     f32  the smallest distSqPointSegment over the arena's edges, or +inf when the table is empty
 *   - r_i is the agent's own radius while ca_set_agent_params is in force, else ca_config.radius.
 *   - On a handle with per-arena counts an absent row is never a j, and reports 0, 0, -1, +inf, +inf whatever the caller left in its
 *     position.
 *   - Contacts have no range limit: neighbor_dist plays no part, and on a grid handle with the static edge grid on the walls are
 *     still a scan of the whole table (wall_d2 may lie beyond any obstacle range).
 *   - Over an arena, `agents` sums to twice the pairs and `wall` to the wall hits that CA_F_STATS counts for the same state.
 * The report lives in ONE device buffer [5, A, N] of 4-byte words, the planes in the order above, agent index fastest, allocated on
 * first use.  It is no ca_field and no part of the state (nothing a later step depends on).
 * ca_contacts: recompute the report of the current state (like ca_observe: one launch on the handle's stream).
 * CA_F_CONTACT on ca_step / ca_step_host / ca_step_packed / ca_orca_step / ca_alan_step / ca_reset / ca_reset_masked: the same launch
 * behind the call's own, so the report is of the state the call leaves -- a frozen arena (CA_F_FREEZE) reports its unchanged state;
 * under CA_F_AUTORESET an arena that was reset inside the call reports its RESPAWNED state, as the observation does, while the
 * statistics of that step were counted before the reset.  The packed layout of ca_step_packed does not change.  On ca_rollout /
 * ca_alan_rollout / ca_rollout_trace / ca_alan_rollout_trace: ONE launch behind the last step, not one per step (a one-launch rollout
 * stays one launch, plus this one); no report per trace record.  ca_profile counts the launch under kind 3.  Every kind of handle
 * takes the flag and the calls; nothing else a call computes depends on it.
 * ca_get_contacts: copies the planes out ([A,N] each; any pointer may be NULL): bytes_each != A*N*4 -> CA_ESIZE; no report computed
 * yet on this handle -> CA_EINVAL (zeros would read as "no contact"); otherwise the last report computed, like CA_FLD_OBS.
 * ca_contacts_ptr: zero-copy view of the [5, A, N] buffer (allocates it if needed; valid until ca_destroy). */
int ca_contacts(ca_env* env);
int ca_get_contacts(ca_env* env, int32_t* agents, int32_t* wall, int32_t* nearest, float* nearest_d2, float* wall_d2, size_t bytes_each,
                    int32_t dst_is_device);
int ca_contacts_ptr(ca_env* env, void** dev_ptr, size_t* bytes);
/* Forking and rewinding arenas on the device: what planning by sampling (copy the real arena into every other slot, roll each copy
 * out under its own actions with ca_rollout / ca_step, pick, rewind), population-based training (overwrite the worst arenas with
 * the best) and curricula (return to a stored situation) need, without the host round trip of ca_get / ca_set per field.  The
 * reference never copies a simulator; its counterpart is rebuilding one from stored positions (env.py:461-488).
 * State that moves (CA_FLD_*): POS_X POS_Y VEL_X VEL_Y PREF_X PREF_Y GOAL_X GOAL_Y GOAL2_X GOAL2_Y REWARD AGENT_DONE ARRIVE_STEP
 *   REGOAL_COUNT NB_COUNT OBST_COUNT NB_IDX OBST_IDX STEP_COUNT ARENA_DONE EPISODE; after ca_alan_configure*: ALAN_WEIGHTS ALAN_TIMES
 *   ALAN_ACTION.
 * What stays with the slot: configuration (obstacle tables, ca_set_agent_params / _counts / _sensing values, ALAN action sets, the
 * edge grid), statistics (CA_FLD_ARENA_STATS, the per-arena step counts, ca_stats), the contact report, the observation buffer
 * (unless CA_F_OBS is given), and the identity that keys the random streams: seed and arena_offset + a.  The last is the intended
 * meaning: copies of one arena share a past and draw futures of their own -- spawn positions, re-goals and ALAN draws after the
 * call are those of the destination's arena id.
 * ca_arena_gather: arena a := arena src[a] as it was BEFORE the call, for every a, however src overlaps (a permutation, a broadcast).
 *   src: i32 [A], host or device, each in 0 .. n_arenas-1; src[a] == a leaves arena a alone: it is not written at all.
 * ca_snapshot_create: a second set of the state buffers on the handle's device, owned by the handle; it holds no state yet.
 * ca_snapshot_save: snap := the state of every arena, asynchronously on the handle's stream (one launch); may be repeated, the
 *   last save counts.  ca_snapshot_load: arena a := arena src[a] OF THE SNAPSHOT; src[a] == -1 leaves arena a as it is (not
 *   written); src == NULL (bytes ignored): every arena a := snapshot arena a.  ca_snapshot_destroy frees one (drains the stream);
 *   ca_destroy frees those still alive.
 * Rules
 *   - In place, and pointers stay: ca_field_ptr's buffers do not move.  The gather copies through a scratch set of the state buffers
 *     that the handle owns (allocated on first use, freed by ca_destroy): one launch saves into it, one loads from it with src.  A
 *     save or a load is one launch of the same kernel.  ca_profile counts these launches under kind 3.
 *   - The observation's frame is re-derived from the moved positions and goals at the next observation, and the moved neighbour
 *     lists are treated like lists written through ca_set: the seeded scan sanitises them on the next step.  Results are the bits a
 *     handle brought to the same state through ca_set computes.
 *   - flags: CA_F_OBS -- one observation launch behind the move, for the state the call leaves, as ca_reset(..., CA_F_OBS) does;
 *     CA_F_CONTACT -- the contact launch likewise.  Any other bit -> CA_EINVAL.
 *   - A world per arena (ca_set_obstacles_per_arena): obstacle-neighbour ids are local to a table, so the obstacle-neighbour count of
 *     every row of every arena that was WRITTEN reads 0 afterwards (a fresh simulator has empty lists; the next solve rebuilds
 *     them).  With one common table the lists move intact.
 *   - Per-agent sensing (ca_set_agent_sensing): the agent-neighbour count of every row of a written arena reads 0, as after that call
 *     itself (a copied list may be longer than its new owner's max_neighbors).
 *   - Per-arena counts (ca_set_agent_counts): only rows i < counts[a] are written, an absent row keeps what the caller put there.
 *     An arena takes the state of an arena of its own size only: counts[src[a]] != counts[a] -- for a load: the counts saved with
 *     the snapshot -- -> CA_EINVAL (ca_last_error names the arena and both counts).
 *   - Checks, all before anything is launched (a failure leaves the handle as it was): bytes != A*4 -> CA_ESIZE; an index outside
 *     0 .. n_arenas-1 (load: -1 .. n_arenas-1) -> CA_ERANGE (the message names the arena and the value); a snapshot of another
 *     handle, one with nothing saved, or one saved under another ALAN shape (n_actions changed since) -> CA_EINVAL; a NULL handle ->
 *     CA_EINVAL.  The index array is read before the call returns: a device src is copied back for the check, as
 *     ca_set_agent_params does with its arrays, which drains the stream (so does the upload of a host src).
 *   - These calls advance nothing, so like ca_get they do not report the sticky obstacle-overflow status.
 *   - Every kind of handle takes them: one-, two- and four-lanes kernels, wide lists, per-agent parameters, counts and sensing, tiled
 *     handles of every create flag (16-bit ids; the sort buffers and the launches' scratch are no state and do not move). */
typedef struct ca_snapshot ca_snapshot;
int ca_arena_gather(ca_env* env, const int32_t* src, size_t bytes, int32_t src_is_device, uint32_t flags);
int ca_snapshot_create(ca_env* env, ca_snapshot** out);
int ca_snapshot_save(ca_env* env, ca_snapshot* snap);
int ca_snapshot_load(ca_env* env, const ca_snapshot* snap, const int32_t* src, size_t bytes, int32_t src_is_device, uint32_t flags);
int ca_snapshot_destroy(ca_env* env, ca_snapshot* snap);
/* Diagnostic (tools/fork_cost.py): *bytes = the bytes of ONE arena in the planes listed above, as the copy kernel's descriptors
 * state them; a save reads and writes each of them once. */
int ca_fork_bytes_per_arena(ca_env* env, size_t* bytes);
/* `steps` consecutive ca_orca_step calls without returning to the host (with CA_F_FREEZE: every
 * arena runs to the end of its own episode, at most `steps` steps): the reference's ORCA-only loops, env.py:570-573
 * (`while True: orca_step()`) and ALAN:106-123 (run_sim).  One kernel launch per 256 steps where the handle uses
 * the four-lanes-per-agent kernel (ca_solver_info) and no observation is asked for (a launch is bounded so that a long
 * rollout stays a sequence of kernels of a few milliseconds; ca_profile_read reports such a launch per step). */
int ca_rollout(ca_env* env, int32_t steps, uint32_t flags);

/* ALAN online learning (ALAN_true.py:569-628 online_step + the counter / goal test of run_sim,
 * ALAN:118-121), for every agent of every arena on the device.
 * ca_alan_configure replaces the constructor's bandit state (ALAN:31-38, 47-49, 73-76):
 *   actions_xy : HOST array [n_actions, 2] of action vectors (ALAN:31-38); an action rotates the goal
 *                direction by atan2(y, x) (ALAN:592-595)
 *   temp       : softmax temperature (ALAN:49 online_temp = 0.2)
 *   timewindow : seconds after which an action's weight is forgotten (ALAN:48 = 2)
 *   time_step  : the fp64 time step the reference adds to `times` (ALAN:15 = 1/60.)
 * Weights and times start at zero.
 * ca_alan_step: softmax draw -> preferred velocity -> ORCA step -> reward -> bandit update -> step
 * counter -> goal test.  u: device or host array [A,N] f64 of uniforms in [0,1) that drive the draws (one per
 * agent, consumed like numpy's choice: first action whose normalised cdf exceeds u), or NULL to use
 * the handle's counter-based RNG keyed by (seed, global arena, agent, episode of the arena, step).  Flags: CA_F_OBS,
 * CA_F_STATS, CA_F_FREEZE. */
int ca_alan_configure(ca_env* env, const double* actions_xy, int32_t n_actions, double temp, double timewindow,
                      double time_step);
/* One action set per arena (the trainer's proposals side by side: Train_ALAN_action_space.py:53-67 evaluates one set over
 * `num` worlds; here many sets, each over arenas of its own, advance in the same launches).
 *   n_actions  : HOST array [A], each 1..CA_ALAN_MAX_ACTIONS
 *   actions_xy : HOST array [sum(n_actions), 2], all arenas' sets back to back (like ca_set_obstacles_per_arena)
 * Each action is normalised as ca_alan_configure does it; temp / timewindow / time_step as there.  Weights and times start at
 * zero and keep the shape [A, max(n_actions), N]: rows k >= n_actions[a] of arena a are zero and never touched.  Every form of
 * the step (ca_solver_info) runs with per-arena sets; the fused forms are sized by the largest set.  ca_alan_configure
 * afterwards returns the handle to one set for all arenas, and this call may follow that one. */
int ca_alan_configure_per_arena(ca_env* env, const double* actions_xy, const int32_t* n_actions, double temp,
                                double timewindow, double time_step);
/* The action set of one arena as the kernels use it (after either configure call): unit (cos, sin) pairs, host array
 * [cap, 2] (may be NULL); *n_out = the number of actions of that arena (at most cap pairs are written). */
int ca_alan_actions_arena(ca_env* env, int32_t arena, double* cs_xy, int32_t cap, int32_t* n_out);
int ca_alan_step(ca_env* env, const double* u, int32_t u_is_device, uint32_t flags);
/* `steps` consecutive ca_alan_step(env, NULL, 0, flags) calls without returning to the host: with
 * CA_F_FREEZE this is run_sim(mode=1) (ALAN:106-123) for every arena at once.  Where the handle uses the four-lanes kernel
 * (ca_solver_info: rollout_one_launch) the bandit runs INSIDE that kernel -- one launch per 256 steps, weights and times
 * resident in LDS --, and a single ca_alan_step is one launch instead of three (select, solve, update). */
int ca_alan_rollout(ca_env* env, int32_t steps, uint32_t flags);

/* Recording rollouts: ca_rollout / ca_alan_rollout that also write the states in between into buffers of the caller's -- what the
 * reference shows by drawing every step (ALAN:639-699 draw_world / draw_update), demonstration trajectories, and on a tiled handle the product of
 * the simulation itself -- without giving up the one-launch rollout and without a host round trip per step.
 *   R = steps / every records.  Record r holds what ca_get of those fields would return had the rollout been (r + 1) * every
 *   steps long:
 *     agents : DEVICE f32 [R, C, A, N], C = 2 per channel bit, the planes in the order pos_x, pos_y, vel_x, vel_y (CA_TRACE_POS
 *              alone: pos_x, pos_y; CA_TRACE_VEL alone: vel_x, vel_y)
 *     arenas : DEVICE i32 [R, 3, A] = step_count, arena_done, episode; or NULL: not recorded
 *   It follows that
 *     - an arena frozen under CA_F_FREEZE repeats its unchanged state in every later record;
 *     - under CA_F_AUTORESET the record taken at the step that ended an episode holds the respawned positions, step_count 0 and the
 *       bumped episode;
 *     - on a handle with per-arena agent counts an absent row holds what the field holds (what the caller last put there).
 *   Steps beyond R * every are advanced and not recorded.  The final state, the statistics and every other field are bit for bit
 *   those of the same call without a trace (one exception, in the last place of one sum: ca_alan_rollout_trace with an action set
 *   per arena and CA_F_STATS adds ca_stats.sum_reward step by step where ca_alan_rollout adds it per launch).
 * Asynchronous on the handle's stream like ca_rollout: the buffers are the caller's and must stay alive, and unread, until the
 * stream has passed the call (ca_sync, or work ordered behind it on the same stream).  The ca_trace struct itself is read before the
 * call returns.  Flags are those of ca_rollout / ca_alan_rollout; CA_F_OBS is allowed and takes the per-step form.  The sticky
 * overflow error works as in ca_rollout.
 * Where ca_rollout / ca_alan_rollout are one launch per 256 steps (ca_solver_info: rollout_one_launch) so are these: the four-lanes
 * kernel stores the records from its registers, and records continue across launches whatever `every` is.  (ca_alan_rollout_trace
 * with an action set per arena takes the per-step form.)  Everywhere else -- one- and two-lanes kernels, per-agent parameters,
 * per-arena counts, wide lists, tiled handles, the three-launch ALAN step, any rollout with CA_F_OBS -- a small record kernel runs
 * behind the launches of every `every`-th step; ca_profile counts it under kind 3.
 * Errors, all checked before anything is launched (a failure advances nothing): tr or tr->agents NULL, every < 1, channels zero or
 * with unknown bits -> CA_EINVAL; agents_bytes, or a non-NULL arenas' arenas_bytes, smaller than the layout -> CA_ESIZE
 * (ca_last_error names the needed size). */
#define CA_TRACE_POS 1u   /* pos_x, pos_y */
#define CA_TRACE_VEL 2u   /* vel_x, vel_y */
typedef struct ca_trace {
    void*    agents;        /* DEVICE f32 [R, C, A, N]: C = 2 per channel bit, planes in the order pos_x, pos_y, vel_x, vel_y */
    size_t   agents_bytes;
    void*    arenas;        /* DEVICE i32 [R, 3, A]: step_count, arena_done, episode; or NULL */
    size_t   arenas_bytes;
    int32_t  every;         /* >= 1 */
    uint32_t channels;      /* CA_TRACE_POS | CA_TRACE_VEL, at least one */
} ca_trace;
int ca_rollout_trace(ca_env* env, int32_t steps, uint32_t flags, const ca_trace* tr);
int ca_alan_rollout_trace(ca_env* env, int32_t steps, uint32_t flags, const ca_trace* tr);

/* Action-sequence rollouts: `steps` consecutive ca_step calls under a [R, A, N] action tensor the caller already holds, without
 * returning to the host -- the second step of a planner's round (ca_arena_gather: copy the real arena into every slot; roll each
 * copy out under its own actions; pick; ca_snapshot_load: rewind) and an agent that holds every action for `hold` steps (frame skip).
 *   Definition: the state, every field and every statistic the call leaves are, bit for bit, those of `steps` consecutive
 *   ca_step(env, actions + (t / hold) * A * N, flags) calls, t = 0 .. steps - 1.  R = ceil(steps / hold): the last row may be held
 *   for fewer than `hold` steps.
 *   returns[a, i] starts at +0.0f and takes, in step order, ret = ret + r_t (weights NULL) or ret = ret + weights[t] * r_t (two fp32
 *   operations, each rounded once, never contracted), r_t the value step t writes to CA_FLD_REWARD.  A step that did not advance
 *   the arena adds nothing: under CA_F_FREEZE every step once arena_done is set, all of them for an arena frozen at entry.  An absent
 *   row of ca_set_agent_counts stays 0.  Under CA_F_AUTORESET the sum RUNS ACROSS the episode boundary: it is the sum over the steps
 *   of the call, not of an episode (first_done says where the boundary fell).
 *   first_done[a] is the smallest t for which arena_done[a] != 0 after step t of this call, -1 if there is none; an arena frozen at
 *   entry reads -1 (its flag was there to see before the call).
 * Flags: CA_F_STATS, CA_F_AUTORESET and CA_F_FREEZE apply per step as in ca_step; CA_F_OBS and CA_F_CONTACT each add ONE launch
 * behind the last step, for the state the call leaves (both are pure functions of that state: what the `steps` calls leave);
 * CA_F_NODONE or an unknown bit -> CA_EINVAL.
 * Checks, all before anything is launched (a failure advances nothing): a NULL env, seq or seq->actions, steps < 0, hold < 1 ->
 * CA_EINVAL; a buffer smaller than its layout -> CA_ESIZE (ca_last_error names the buffer and the size it needs).  steps == 0
 * advances nothing and still writes zeros to returns and -1 to first_done where given.  The sticky overflow error works as in
 * ca_rollout.
 * Asynchronous on the handle's stream: the buffers are the caller's and must stay alive until the stream has passed the call; the
 * ca_action_seq struct itself is read before the call returns, as ca_trace is.
 * Where ca_rollout is one launch per 256 steps (ca_solver_info: rollout_one_launch; ALAN-configured handles included) so is this:
 * the four-lanes kernel reads each step's action element itself, keeps the return in a register and writes returns, first_done and
 * the last reward once per launch; sums and row indices carry on across launches, also in the middle of a hold.  Everywhere else --
 * one- and two-lanes kernels, wide lists, per-agent parameters, counts, sensing, tiled handles -- every step is the launch (sequence)
 * of ca_step with that step's row and a small accumulate kernel behind it; ca_profile counts the small kernels under kind 3. */
typedef struct ca_action_seq {
    const float* actions;    /* DEVICE f32 [R, A, N], R = ceil(steps / hold): row t / hold drives step t */
    size_t   actions_bytes;
    int32_t  hold;           /* >= 1: every row is held for `hold` consecutive steps (frame skip) */
    const float* weights;    /* DEVICE f32 [steps], or NULL = 1 for every step (discounts: the caller's gamma^t) */
    size_t   weights_bytes;
    float*   returns;        /* DEVICE f32 [A, N], or NULL: not wanted */
    size_t   returns_bytes;
    int32_t* first_done;     /* DEVICE i32 [A], or NULL: not wanted */
    size_t   first_done_bytes;
} ca_action_seq;
int ca_rollout_actions(ca_env* env, int32_t steps, uint32_t flags, const ca_action_seq* seq);

/* A policy on the device: the reference's model is a shared-weights 64-64 ReLU MLP over the 64-float laser observation that emits
 * one heading offset per agent (run_rllib.py:35-52), stepped in a loop (run_rllib.py:103-125).  Here the policy is configuration of
 * the handle and observation -> MLP -> action -> step runs for `steps` steps in one call.
 *   Definition, bit for bit.  L linear layers, 2 <= L <= 4, widths w[0] = CA_OBS_DIM, hidden widths w[1 .. L-1] each a multiple of 16
 *   in 16 .. 128, w[L] = 1.  Layer l has W_l f32 [w[l], w[l-1]] and b_l f32 [w[l]] (the torch.nn.Linear layout).  For a row x (one
 *   agent's observation), layer l and output j, in fp32:
 *       acc = b_l[j];  for k = 0 .. w[l-1]-1 ascending: acc = fmaf(x[k], W_l[j][k], acc)        (one rounding per step)
 *       hidden layers: y[j] = acc > 0 ? acc : +0.0f            output layer: mean = acc
 *       action = out(mean + noise)                               (the add only where noise is given, one fp32 add)
 *       out = identity (CA_POLICY_OUT_IDENTITY) | fminf(fmaxf(v, -limit), limit) (CA_POLICY_OUT_CLIP)
 *   A row's result depends on its observation and its arena's weight set only.
 * ca_policy_configure: n_sets = P >= 1 weight sets, weights[l] f32 [P, w[l+1], w[l]] and bias[l] f32 [P, w[l+1]] (host memory, or
 * device memory with src_is_device), set_of_arena i32 [A] HOST memory (NULL with P = 1: set 0 everywhere): arena a plays set
 * set_of_arena[a], so a population is evaluated side by side.  Every value is checked before anything changes: n_layers, a width,
 * out_mode, n_sets < 1, a NULL array, a NaN or negative out_limit under CA_POLICY_OUT_CLIP, a NULL set_of_arena with P > 1 ->
 * CA_EINVAL; an array smaller than its layout -> CA_ESIZE; a non-finite weight or bias (ca_last_error names the layer, the set and
 * the element) or a set index outside 0 .. P-1 (names the arena) -> CA_ERANGE.  The call repacks the weights for the kernel and
 * drains the stream; calling it again replaces the policy.  Configuration, like the ALAN action sets: no ca_field, it persists across
 * resets and stays with the SLOT under ca_arena_gather and ca_snapshot_load (fork arena 0 into every slot: each slot plays its own set).
 * ca_policy_clear removes it; ca_policy_info reports *configured, and where configured *n_layers, width[0 .. L] and *n_sets (any
 * pointer may be NULL).
 * ca_policy_actions: ONE launch that reads the handle's observation buffer as it stands (what ca_observe / CA_F_OBS / ca_set left, a
 * buffer bound with ca_bind_obs included) and writes actions_out, DEVICE f32 [A, N]; noise DEVICE f32 [A, N] or NULL.  No policy, or a
 * NULL actions_out -> CA_EINVAL.  Asynchronous on the handle's stream. */
#define CA_POLICY_OUT_IDENTITY 0
#define CA_POLICY_OUT_CLIP 1
#define CA_POLICY_MAX_LAYERS 4
#define CA_POLICY_MAX_WIDTH 128
typedef struct ca_policy_desc {
    int32_t  n_layers;                           /* L: 2 .. CA_POLICY_MAX_LAYERS */
    int32_t  width[CA_POLICY_MAX_LAYERS + 1];    /* w[0 .. L] */
    const float* weights[CA_POLICY_MAX_LAYERS];  /* layer l: f32 [P, w[l+1], w[l]] */
    size_t   weights_bytes[CA_POLICY_MAX_LAYERS];
    const float* bias[CA_POLICY_MAX_LAYERS];     /* layer l: f32 [P, w[l+1]] */
    size_t   bias_bytes[CA_POLICY_MAX_LAYERS];
    int32_t  src_is_device;                      /* weights and bias lie in device memory */
    int32_t  n_sets;                             /* P >= 1 */
    const int32_t* set_of_arena;                 /* HOST i32 [A], or NULL when P = 1 */
    size_t   set_of_arena_bytes;
    int32_t  out_mode;                           /* CA_POLICY_OUT_* */
    float    out_limit;                          /* CA_POLICY_OUT_CLIP: actions are clamped to [-out_limit, out_limit] */
} ca_policy_desc;
int ca_policy_configure(ca_env* env, const ca_policy_desc* desc);
int ca_policy_clear(ca_env* env);
int ca_policy_info(ca_env* env, int32_t* configured, int32_t* n_layers, int32_t* width, int32_t* n_sets);
int ca_policy_actions(ca_env* env, const float* noise, float* actions_out);

/* Closed-loop policy rollouts: `steps` steps under the configured policy without returning to the host.
 *   Definition: the state, every field, every statistic, returns and first_done are bit for bit those of the loop
 *       for t in 0 .. steps-1:
 *           if t % hold == 0: ca_observe; ca_policy_actions(noise row t / hold) -> act       (record obs row t / hold, action row t / hold)
 *           ca_step(env, act, flags & (CA_F_STATS | CA_F_AUTORESET | CA_F_FREEZE))            (record reward_t, done_t)
 *   with returns and first_done as ca_rollout_actions defines them (weights, freezing, absent rows, the sum across a respawn: the
 *   rules above apply verbatim).  R = ceil(steps / hold).  The handle's observation buffer is left holding the last row's observation
 *   (CA_F_OBS: that of the final state).
 *   Records, all optional DEVICE buffers, written for every row, arena and step: obs_out f32 [R, A, N, 64] (16-byte aligned) and
 *   actions_out f32 [R, A, N] -- what the policy read and emitted at the start of row r --, rewards_out f32 [steps, A, N] -- what
 *   CA_FLD_REWARD holds after step t -- and done_out i32 [steps, A] -- arena_done after step t.  An arena frozen under CA_F_FREEZE
 *   repeats its unchanged observation and the reward the field holds; an absent row of ca_set_agent_counts records the policy of its
 *   zero observation, which nothing reads.
 * Flags as for ca_rollout_actions: CA_F_OBS and CA_F_CONTACT each add ONE launch behind the last step; CA_F_NODONE or an unknown bit
 * -> CA_EINVAL.  Checks, all before anything is launched (a failure advances nothing): a NULL env or seq, steps < 0, hold < 1, no
 * policy configured, a misaligned obs_out -> CA_EINVAL; a buffer smaller than its layout -> CA_ESIZE (ca_last_error names the buffer
 * and the size it needs).  steps == 0 writes zeros to returns and -1 to first_done where given, and nothing else.  The sticky
 * overflow error works as in ca_rollout.  Asynchronous on the handle's stream; the struct itself is read before the call returns.
 * Every kind of handle takes the same form: per row one observation launch and one policy launch (which stores the obs and action
 * records itself), per step the launch (sequence) of ca_step and a small accumulate-and-record kernel; ca_profile counts the policy
 * kernel and the record kernel under kind 3. */
typedef struct ca_policy_seq {
    int32_t  hold;            /* >= 1: every action row is held for `hold` consecutive steps */
    const float* noise;       /* DEVICE f32 [R, A, N], or NULL: exploration noise added to the mean, drawn by the caller */
    size_t   noise_bytes;
    const float* weights;     /* DEVICE f32 [steps], or NULL = 1 for every step */
    size_t   weights_bytes;
    float*   returns;         /* DEVICE f32 [A, N], or NULL */
    size_t   returns_bytes;
    int32_t* first_done;      /* DEVICE i32 [A], or NULL */
    size_t   first_done_bytes;
    float*   obs_out;         /* DEVICE f32 [R, A, N, 64], or NULL */
    size_t   obs_out_bytes;
    float*   actions_out;     /* DEVICE f32 [R, A, N], or NULL */
    size_t   actions_out_bytes;
    float*   rewards_out;     /* DEVICE f32 [steps, A, N], or NULL */
    size_t   rewards_out_bytes;
    int32_t* done_out;        /* DEVICE i32 [steps, A], or NULL */
    size_t   done_out_bytes;
} ca_policy_seq;
int ca_rollout_policy(ca_env* env, int32_t steps, uint32_t flags, const ca_policy_seq* seq);

/* PPO sample collection: heads on the installed policy, a rollout that hands back a PPO batch, and GAE.
 * Heads.  Two optional extra rows of the output layer, read from the last hidden layer (width w[L-1]), one per weight set: the value
 * head value_w f32 [P, w[L-1]] / value_b f32 [P], and the log-std head logstd_w f32 [P, w[L-1]] (NULL: all zeros -- a
 * state-independent log-std carried by the bias) / logstd_b f32 [P]; HOST memory.  A head is given by its bias; at least one must be.
 *   Definition, bit for bit.  Per agent row, in fp32, one rounding per operation, never contracted:
 *       mean, ls_raw, value: each the k-ordered fmaf chain from its bias over the last hidden layer's activations (the rule of the mean)
 *       ls  = fminf(fmaxf(ls_raw, CA_POLICY_LOGSTD_MIN), CA_POLICY_LOGSTD_MAX);  std = (float)exp64((double)ls)     (ca_debug_math op 5)
 *             without a log-std head: ls = +0, std = 1;  without a value head: value = +0
 *       eps = the noise element, +0 where noise is NULL
 *       u   = mean + std * eps                                     (two operations)
 *       action = out(u)                                            (the policy's out mode)
 *       logp = ((-0.5f * (eps * eps)) - ls) - 0.918938533f         (left to right as written: the log-density of the UNCLIPPED u)
 * ca_policy_set_heads repacks the output tile -- column 0 the installed mean row, column 1 the log-std, column 2 the value -- and
 * drains the stream.  Refusals as ca_policy_configure's, all before anything changes: no policy installed, a NULL desc, no head at
 * all, a weight array without its bias -> CA_EINVAL; an array smaller than its layout -> CA_ESIZE; a non-finite value -> CA_ERANGE
 * (ca_last_error names the head, the set and the element).  Heads are configuration like the policy: they survive resets and stay
 * with the SLOT under ca_arena_gather / ca_snapshot_load.  ca_policy_configure and ca_policy_clear drop them (the widths may have
 * changed); ca_policy_clear_heads removes them alone; ca_policy_heads_info reports *has_value and *has_logstd (either may be NULL).
 * ca_policy_actions and ca_rollout_policy are untouched by heads: they keep reading the tile whose columns 1 .. 15 are zero.
 * ca_policy_evaluate: ONE launch on the observation buffer as it stands, the heads' counterpart of ca_policy_actions.  out holds
 * optional DEVICE f32 [A, N] pointers; noise DEVICE f32 [A, N] or NULL.  No policy, no heads or a NULL out -> CA_EINVAL. */
#define CA_POLICY_LOGSTD_MIN (-20.0f)
#define CA_POLICY_LOGSTD_MAX 2.0f
typedef struct ca_policy_heads {
    const float* value_w;     /* HOST f32 [P, w[L-1]], or NULL: no value head */
    size_t   value_w_bytes;
    const float* value_b;     /* HOST f32 [P] */
    size_t   value_b_bytes;
    const float* logstd_w;    /* HOST f32 [P, w[L-1]], or NULL: zeros */
    size_t   logstd_w_bytes;
    const float* logstd_b;    /* HOST f32 [P], or NULL: no log-std head */
    size_t   logstd_b_bytes;
} ca_policy_heads;
typedef struct ca_policy_eval {
    float*   actions;         /* DEVICE f32 [A, N] each, or NULL: not wanted */
    float*   logp;
    float*   value;
    float*   mean;
    float*   log_std;         /* the clamped log-std */
} ca_policy_eval;
int ca_policy_set_heads(ca_env* env, const ca_policy_heads* heads);
int ca_policy_clear_heads(ca_env* env);
int ca_policy_heads_info(ca_env* env, int32_t* has_value, int32_t* has_logstd);
int ca_policy_evaluate(ca_env* env, const float* noise, const ca_policy_eval* out);

/* ca_rollout_policy_sample: the loop of ca_rollout_policy, verbatim, with ca_policy_evaluate in the place of ca_policy_actions:
 *       for t in 0 .. steps-1:
 *           if t % hold == 0: ca_observe; ca_policy_evaluate(noise row t / hold) -> act         (the row's records, r = t / hold)
 *           ca_step(env, act, flags & (CA_F_STATS | CA_F_AUTORESET | CA_F_FREEZE))               (the step's and the row's records)
 *       values_out given: ca_observe; the value of the state the call leaves -> values_out row R
 *       advantages_out or targets_out given: ca_gae(R rows: row_rewards, values, row_done, row_valid; gamma, lambda)
 * The state, fields, statistics, returns, first_done and the four records of ca_policy_seq are bit for bit those of
 * ca_rollout_policy under the same effective actions.  Further optional DEVICE records, R = ceil(steps / hold):
 *   logp_out f32 [R, A, N]; dist_out f32 [R, 2, A, N]: the mean and the clamped log-std; values_out f32 [R+1, A, N]: row R is the
 *   bootstrap value, one observation launch and one heads launch behind the last step, made only where the buffer is given -- the
 *   handle's observation buffer then holds the final state's observation, as under CA_F_OBS;
 *   row_rewards_out f32 [R, A, N]: from +0, one fp32 add per step of the row that advanced the arena (ca_rollout_actions' freeze
 *   rule), in step order, unweighted (`weights` is the business of `returns`); row_done_out i32 [R, A]: the OR of the row's done_out
 *   entries; row_valid_out i32 [R, A]: 1 iff the row's first step advanced the arena;
 *   advantages_out, targets_out f32 [R, A, N]: one ca_gae launch behind everything, under gamma and lambda; they need values_out,
 *   else CA_EINVAL (row records that were not given are kept in buffers of the handle's).
 * Checks, messages and steps == 0 as ca_rollout_policy (steps == 0 with values_out: the bootstrap row alone is written); a policy
 * without heads and a misaligned obs_out are CA_EINVAL; a refusal advances nothing; the sticky overflow error works as before;
 * ca_profile counts the new kernels under kind 3. */
typedef struct ca_policy_sample_seq {
    int32_t  hold;            /* the members of ca_policy_seq, with their meaning */
    const float* noise;       /* DEVICE f32 [R, A, N], or NULL: eps */
    size_t   noise_bytes;
    const float* weights;
    size_t   weights_bytes;
    float*   returns;
    size_t   returns_bytes;
    int32_t* first_done;
    size_t   first_done_bytes;
    float*   obs_out;
    size_t   obs_out_bytes;
    float*   actions_out;
    size_t   actions_out_bytes;
    float*   rewards_out;
    size_t   rewards_out_bytes;
    int32_t* done_out;
    size_t   done_out_bytes;
    float*   logp_out;        /* DEVICE f32 [R, A, N], or NULL */
    size_t   logp_out_bytes;
    float*   dist_out;        /* DEVICE f32 [R, 2, A, N], or NULL */
    size_t   dist_out_bytes;
    float*   values_out;      /* DEVICE f32 [R+1, A, N], or NULL */
    size_t   values_out_bytes;
    float*   row_rewards_out; /* DEVICE f32 [R, A, N], or NULL */
    size_t   row_rewards_out_bytes;
    int32_t* row_done_out;    /* DEVICE i32 [R, A], or NULL */
    size_t   row_done_out_bytes;
    int32_t* row_valid_out;   /* DEVICE i32 [R, A], or NULL */
    size_t   row_valid_out_bytes;
    float*   advantages_out;  /* DEVICE f32 [R, A, N], or NULL */
    size_t   advantages_out_bytes;
    float*   targets_out;     /* DEVICE f32 [R, A, N], or NULL */
    size_t   targets_out_bytes;
    float    gamma;           /* of the GAE launch */
    float    lambda;
} ca_policy_sample_seq;
int ca_rollout_policy_sample(ca_env* env, int32_t steps, uint32_t flags, const ca_policy_sample_seq* seq);

/* ca_gae: generalised advantage estimation on buffers of the caller's, all DEVICE: rewards f32 [R, A, N], values f32 [R+1, A, N],
 * done i32 [R, A], valid i32 [R, A] or NULL for all 1; advantages and targets f32 [R, A, N], each optional.  R = rows.
 *   Definition, in fp32, gl = gamma * lambda one fp32 multiply; for r = R-1 .. 0 per (a, i):
 *       nd     = done[r, a] == 0
 *       next_v = nd ? values[r+1] : +0
 *       delta  = (rewards[r] + gamma * next_v) - values[r]                  (three operations, in that order)
 *       next_a = nd && r < R-1 ? adv[r+1] : +0
 *       adv[r] = delta + gl * next_a;     valid[r, a] == 0: adv[r] = +0
 *       target[r] = adv[r] + values[r]
 * A pure function of its inputs, no special case for absent rows; the done flag alone ends an episode, the step cap included (the
 * reference treats it as terminal, env.py:404-413).  rows == 0 launches nothing; rows < 0, a NULL desc, rewards, values or done ->
 * CA_EINVAL; a buffer smaller than its layout -> CA_ESIZE.  One launch (kind 3), asynchronous on the handle's stream. */
typedef struct ca_gae_desc {
    const float* rewards;
    size_t   rewards_bytes;
    const float* values;
    size_t   values_bytes;
    const int32_t* done;
    size_t   done_bytes;
    const int32_t* valid;     /* or NULL */
    size_t   valid_bytes;
    float*   advantages;      /* or NULL */
    size_t   advantages_bytes;
    float*   targets;         /* or NULL */
    size_t   targets_bytes;
    float    gamma;
    float    lambda;
} ca_gae_desc;
int ca_gae(ca_env* env, int32_t rows, const ca_gae_desc* desc);

/* The reference's simulator keeps EVERY obstacle edge within range of an agent (sim.getAgentNumObstacleNeighbors /
 * getAgentObstacleNeighbor, env.py:249, 301-318, iterate them all); this library's lists hold max_obst_neighbors and drop the
 * farthest edges beyond that.  So that such a deviation cannot pass unnoticed, an overflow is a sticky error of the handle:
 * once a step has met an agent with more edges in range than the list holds, ca_step / ca_step_host / ca_step_packed /
 * ca_orca_step / ca_rollout / ca_alan_step / ca_alan_rollout and ca_sync return CA_ERANGE (ca_last_error names the global arena,
 * the agent and the number of edges) -- asynchronously, like a device fault: the first call made after the kernel that
 * overflowed has finished reports it, calls that synchronise report it at once -- until ca_reset_stats clears it.
 * ca_allow_obstacle_overflow(env, 1) accepts the truncation (nearest max_obst_neighbors edges kept, counted in
 * ca_stats.obst_overflow and per arena); 0 restores the default.  ca_get / ca_get_stats always work.
 * The cure is a larger list: max_obst_neighbors up to CA_MAX_OBST_NEIGHBORS = 64 (a 9 x 9 grid of small squares at a pitch of
 * 0.65 puts 62 edges in range of an agent); the solve and the observation then carry every one of them, bit for bit RVO2's. */
int ca_allow_obstacle_overflow(ca_env* env, int32_t allow);

/* Blocks until the stream is idle, then returns the counters accumulated so far. */
int ca_get_stats(ca_env* env, ca_stats* out);
int ca_reset_stats(ca_env* env);
int ca_sync(ca_env* env);

/* Diagnostics for the numerics contract tests: evaluates device primitives on n inputs.
 * op 0: sqrtf(x)            in f32[n]        out f32[n]
 * op 1: a / b               in f32[2n]       out f32[n]
 * op 2: sincos64(x)         in f64[n]        out f64[2n]
 * op 3: pref_dir64          in f32[4n]       out f64[2n]
 * op 4: philox4x32 uniform  in u32[4n]       out f64[2n]   (key = seed of the handle)
 * op 5: exp64(x)            in f64[n]        out f64[n]
 * op 6: a / b by the in-range sequence (csrc/ca_math.h div_ir)   in f32[2n]   out f32[n]
 * op 7: sqrt(x) by the in-range sequence (csrc/ca_math.h sqrt_ir) in f32[n]    out f32[n]
 * Host pointers. */
int ca_debug_math(ca_env* env, int32_t op, const void* in, void* out, int32_t n);

/* Per-kernel timing for roofline reports.  ca_profile(env, k), k >= 1: every kernel launch of every k-th step of this
 * handle carries a start and a stop HIP event on its own dispatch (hipExtLaunchKernel on the handle's stream: the execution
 * time of the kernel, what rocprofv3 --kernel-trace reports; k = 1: every launch).  ca_profile_read synchronises and
 * returns, per kernel kind, the number of sampled launches and their mean duration in milliseconds since the last read
 * (kinds: 0 nbr_kernel -- always 0: the neighbour search is the head of step_kernel, with no launch of its own; the
 * slot keeps the numbering --, 1 step_kernel -- per STEP: a ca_rollout launch that advances T steps counts as one launch of
 * duration / T; on a tiled handle (CA_CREATE_TILED) every launch of the solve / advance / close sequence counts on its own, so a step
 * is three launches and its time three times the mean (CA_CREATE_TILED_GRID: the launches of the sort in front of them too) --, 2 obs_kernel, 3 the small kernels: reset_kernel, reset_arena_kernel, the ALAN select / update kernels, the record kernel of a
 * recording rollout, contact_kernel (ca_contacts / CA_F_CONTACT), fork_kernel (ca_arena_gather: two, ca_snapshot_save / _load: one), policy_kernel<false> and the record kernel of ca_rollout_policy, policy_kernel<true>, sample_record_kernel and gae_kernel (ca_policy_evaluate, ca_rollout_policy_sample, ca_gae), nav_field_kernel (ca_nav_configure) and nav_pref_kernel (ca_nav_pref, ca_rollout_nav), nav_act_kernel and nav_reward_kernel (ca_nav_act, ca_nav_step, ca_rollout_nav_actions, ca_rollout_nav_policy), reward_begin_kernel and reward_terms_kernel (every step from actions while ca_reward_configure's terms are set; ca_reward_parts), each launch on its own), then clears them.  ca_profile(env, 0) switches
 * it off (default).  A sampled step costs ~10 us of dispatch serialisation; results never depend on it. */
int ca_profile(ca_env* env, int32_t period);
int ca_profile_read(ca_env* env, int32_t counts[4], float mean_ms[4]);

/* Launch geometry chosen for this handle (for reports): threads per block, blocks, LDS bytes. */
int ca_launch_info(ca_env* env, int32_t* block, int32_t* grid, int32_t* lds_bytes, int32_t* obs_grid);
/* Which solve kernel the handle uses: *lanes_per_agent = 1 (one lane per agent), 2 (two lanes per agent: arenas of 129 .. 512
 * agents with max_neighbors <= 10 and max_obst_neighbors <= 4 -- one arena per workgroup is otherwise two waves per SIMD, each
 * a long dependent chain) or 4 (four lanes per agent: chosen at ca_create for batches that would otherwise leave SIMDs without
 * a wave -- fewer than 1024 waves -- when n_agents <= 128 and max_neighbors <= 10 (n_agents <= 64 when, in addition,
 * max_neighbors > 5 and max_obst_neighbors > 4)); results are identical bit for bit.  Among the one-lane kernels the ORCA
 * lines live in registers when max_neighbors <= 10 and either max_obst_neighbors <= 4 or the installed world has at most 16
 * edges per arena (the reference env's own doorway world: an agent with more than four edges in range is solved apart,
 * exactly), else in an LDS table; the choice is re-made when obstacle tables are installed.
 * max_obst_neighbors > 16 always means one lane per agent on the wide LDS table (max_neighbors + max_obst_neighbors lines per
 * lane; *lanes_per_agent = 1, *rollout_one_launch = 0, ca_launch_info's lds_bytes = block x (16 (K + S) + 32)), whatever the
 * world and the batch size: no register lines, no two- or four-lanes kernel (CA_QUAD / CA_REG_LINES are ignored), a batch
 * that is not resident with the table runs in rounds, and ca_alan_step is three launches (select, solve, update).
 * *rollout_one_launch = 1: ca_rollout(env, T, flags without CA_F_OBS) is ONE kernel launch that keeps every arena in
 * registers / LDS for its T steps (the four-lanes kernel; chosen up to 1024 waves inclusive); 0: it is T launches. */
int ca_solver_info(ca_env* env, int32_t* lanes_per_agent, int32_t* rollout_one_launch);
/* The tiled solve path of a handle made with CA_CREATE_TILED: *tiled = 1, *tile_agents = agents per workgroup, *tiles_per_arena =
 * workgroups an arena spans, *launches_per_step = kernel launches of one solve (3; with CA_CREATE_TILED_GRID the launches of the
 * sort in front of them as well: sort_launches + 3).  All zeros on an ordinary handle. */
int ca_tiled_info(ca_env* env, int32_t* tiled, int32_t* tile_agents, int32_t* tiles_per_arena, int32_t* launches_per_step);
/* The uniform grid of a handle made with CA_CREATE_TILED | CA_CREATE_TILED_GRID: *grid = 1, *cells_x / *cells_y = the sides of the
 * wrapped cell table (powers of two, at least 8), *cell_size = the width of a cell (half of neighbor_dist), *sort_launches = kernel
 * launches in front of the solve launch.  All zeros on every handle without the flag. */
int ca_tiled_grid_info(ca_env* env, int32_t* grid, int32_t* cells_x, int32_t* cells_y, float* cell_size, int32_t* sort_launches);

/* The static edge grid of a grid handle (CA_CREATE_TILED | CA_CREATE_TILED_GRID): opt-in, off by default.  Without it every agent tests
 * every edge of its arena's table in every step, for its obstacle list and (CA_F_STATS) for the wall test: O(N * E).  Obstacle edges
 * do not move, so an index over them is built once on the host when a table is installed: per table a uniform grid over the bounding
 * box of its edges, UNWRAPPED and clamped, stored as CSR -- cell_start[cells_x * cells_y + 1] and entries[] --, and the solve and
 * advance launches walk the few cells an agent's range touches.  No launch, sort or barrier per step: ca_tiled_info still reports
 * launches_per_step = 6.  Everything a step leaves -- lists, order, counts, the overflow word and its status, statistics -- is the
 * same bit for bit: an obstacle list is the max_obst_neighbors smallest (distance, edge id) keys of the in-range set, in whatever
 * order the candidates arrive.
 *   - The cell of a coordinate v along an axis with origin x0, reciprocal cell size ics and g cells, in fp32, each operation rounded once:
 *         cell(v) = (int)fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1))
 *     i.e. clamp((int)floor((v - x0) * ics), 0, g - 1), with a coordinate outside the box, an infinity or a NaN clamped into an outermost
 *     cell.  The host builder and the kernels evaluate exactly this expression.  Cells are max(range, extent / 256) wide per axis,
 *     range = time_horizon_obst * max_speed + radius, extent = the side of the edges' bounding box plus two margins: 1 .. 256 cells.
 *   - An edge is registered in every cell of its bounding box inflated by `margin` = 16 * 2^-24 * (largest |coordinate| of the table +
 *     range), which covers the fp32 rounding of the in-range test (DESIGN.md 7g derives it).  An entry is
 *     edge id | lowest column of the edge's cell rectangle << 16 | its lowest row << 24.
 *   - An agent at (x, y) walks the cells of columns cell(x - range) .. cell(x + range) and rows likewise (fp32 differences), 3 x 3
 *     at most but for a rounding of ics (then 4 along an axis), and takes an edge only in cell (max(edge's lowest column, own lowest column), max(edge's lowest row, own lowest row)):
 *     the low corner of the two rectangles' intersection, so no edge twice.
 * ca_tiled_edge_grid(env, 1): builds the grids of the installed tables (one per arena with ca_set_obstacles_per_arena, else one for all
 * arenas) and uses them from the next step; (env, 0): back to the scan.  Drains the stream.  Configuration, like the obstacle tables:
 * it persists across ca_reset*, CA_F_AUTORESET and ca_init_scenario and is no part of the state a caller saves through ca_get.  While
 * on, ca_set_obstacles and ca_set_obstacles_per_arena rebuild the grids for the new tables; if that fails the install fails as a
 * whole and the previous tables and grids stay.
 *   - not a grid handle (create_flags != 5) -> CA_EINVAL (ca_last_error names the flags); the handle keeps working;
 *   - a table of more than CA_EDGE_GRID_MAX_EDGES edges, or whose grid would hold more than CA_EDGE_GRID_MAX_ENTRIES entries (very long
 *     diagonal walls cover many cells) -> CA_ERANGE, "subdivide the walls"; the handle stays as it was (it keeps scanning). */
#define CA_EDGE_GRID_MAX_EDGES 65535
#define CA_EDGE_GRID_MAX_ENTRIES (1 << 22)
int ca_tiled_edge_grid(ca_env* env, int32_t on);
/* The static edge grid of `arena` (0 .. n_arenas - 1; a common table: the same for every arena): *on = 1, *cells_x / *cells_y = the
 * table's sides, *cell_size_x / *cell_size_y = the cells' widths, *entries = entries of the table.  All zeros while off and on every
 * other handle. */
int ca_tiled_edge_grid_info(ca_env* env, int32_t arena, int32_t* on, int32_t* cells_x, int32_t* cells_y, float* cell_size_x, float* cell_size_y,
                            int32_t* entries);
/* The builder itself, handle-free and without a device (tests, tools): the grid of the n_edges edges edges_pq[n_edges][4] = (px, py,
 * qx, qy) for obstacle range `range`.  cell_start == NULL or entries == NULL: fills *desc only, so that the caller can size its
 * buffers (gx * gy + 1 words and n_entries words); else also cell_start[gx * gy + 1] and entries[n_entries] (too small a cap ->
 * CA_ESIZE).  CA_ERANGE as for ca_tiled_edge_grid; messages through ca_last_error(NULL). */
typedef struct ca_edge_grid_desc {
    float x0, y0;        /* the table's origin */
    float ics_x, ics_y;  /* reciprocal cell sizes */
    int32_t gx, gy;      /* sides, 1 .. 256 */
    int32_t n_entries;
    float margin;        /* the inflation of an edge's bounding box (rounded up to fp32) */
} ca_edge_grid_desc;
int ca_edge_grid_build(const float* edges_pq, int32_t n_edges, float range, ca_edge_grid_desc* desc, uint32_t* cell_start, int32_t cell_cap,
                       uint32_t* entries, int32_t entry_cap);
/* Navigation fields: steering round obstacles on the device.  Every ORCA-only step steers an agent straight at its goal (the
 * preferred velocity is the unit vector towards it), and ORCA avoids only locally: an agent whose goal lies behind a wall walks into
 * the wall and stays there.  A navigation is, per target, a shortest-path distance field over a caller-given grid and a pointer per
 * cell; ca_nav_pref writes CA_FLD_PREF_X / _Y from it in front of an ORCA-only step, which reads them as its input.  No solve kernel
 * knows about it.  Every value is defined bit for bit (fp32, one rounding per operation):
 *   - Grid: origin (x0, y0), cell size `cell`, gx x gy cells (1 .. 256 per axis, gx * gy <= CA_NAV_MAX_CELLS), ics = 1.0f / cell.  The
 *     cell of a coordinate is the edge grid's expression above, cell(v) = (int)fminf(fmaxf(floorf((v - x0) * ics), 0.0f), (float)(g - 1)):
 *     a position outside the box is clamped into the outermost cell.  Cell index = cy * gx + cx; the centre of column cx is
 *     x0 + ((float)cx + 0.5f) * cell, rows alike.
 *   - Blocked: cell c is blocked iff some edge (p, q) of the obstacle table has distSqPointSegment(p, q, centre(c)) < clearance *
 *     clearance (csrc/ca_math.h; strictly, like the wall test).  Edges only, no inside test.
 *   - Field per (set, target): the target's cell is the source, d = 0.  Neighbours k = 0 .. 7 are offset by (1,0) (0,1) (-1,0) (0,-1)
 *     (1,1) (-1,1) (-1,-1) (1,-1); w_k = cell for k < 4, cell * 1.41421354f (one multiply) for k >= 4; a diagonal move is allowed only
 *     if both axis cells it passes between are in the grid and unblocked.  For an unblocked cell that is not the source,
 *     d[c] = min over in-grid, unblocked, allowed neighbours of (d[u_k] + w_k), +inf without any; a blocked cell holds +inf.  These
 *     equations have one solution, whatever order a kernel relaxes in.
 *   - Pointers, `next`, one byte per cell: the smallest k with d[u_k] + w_k == d[c] in an unblocked cell of finite distance;
 *     CA_NAV_STAY in the source; CA_NAV_NONE in an unblocked cell of infinite distance; in a blocked cell the escape pointer, the
 *     smallest (d[u_k], k) over all in-grid neighbours of finite distance (all eight, no corner rule), CA_NAV_NONE without one.
 *   - Per step: agent (a, i) is navigated if its row is present (ca_set_agent_counts), agent_done == 0, its class g =
 *     agent_class[a, i] is >= 0 and, with CA_F_FREEZE, arena_done[a] == 0.  Every other row is not written at all.  For a navigated
 *     agent: w = cell(pos); repeat `lookahead` times: k = next[w]; stop if k >= 8; else move w by offset k.  If the walk never moved
 *     or stopped on CA_NAV_STAY: pref = the unit vector towards the agent's own goal; otherwise towards the centre of w (as a double).
 *     Both through the one direction function of the step kernels (env.py:156-162).  dist_out[a, i] = d[g][cell(pos)], +inf in a
 *     blocked cell.  Nothing else is written.
 * ca_nav_configure: builds the masks on the host from the installed obstacle table(s), uploads them, relaxes every field in one launch
 * (one workgroup per field, the grid in LDS) and drains the stream.  per_arena = 0: one set of fields for all arenas, targets [G, 2];
 * needs one common table.  per_arena = 1: a set per arena from the arena's own table (or the common one), targets [A, G, 2].  Calling
 * it again replaces the navigation.  All checks run before anything changes, and a failure leaves the handle as it was:
 *   - a null argument, per_arena = 0 on a handle with tables per arena, n_goals outside 1 .. CA_NAV_MAX_GOALS, lookahead outside
 *     1 .. CA_NAV_MAX_LOOKAHEAD, a grid outside the limits -> CA_EINVAL;
 *   - targets_bytes or class_bytes not exactly the array's size -> CA_ESIZE;
 *   - cell or clearance outside [CA_MIN_LENGTH, CA_MAX_LENGTH] (clearance may also be 0) or not finite; |x0| or |y0| above CA_MAX_COORD;
 *     a target that is not finite, lies outside the box [x0, x0 + gx * cell] x [y0, y0 + gy * cell] or in a blocked cell; a class
 *     outside -1 .. n_goals - 1 -> CA_ERANGE (ca_last_error names the arena, goal or agent).
 * Navigation is configuration, like the policy and the obstacle tables: no ca_field, it survives ca_reset*, CA_F_AUTORESET and
 * ca_init_scenario, and stays with the slot under ca_arena_gather / ca_snapshot_load.  ca_set_obstacles and
 * ca_set_obstacles_per_arena CLEAR it when they install their tables: the fields were relaxed round the old edges.
 * ca_nav_info: *configured, the grid's sides, n_goals, the number of field sets (1 or n_arenas) and the largest number of sweeps a
 * field's relaxation made (below gx * gy + 1, the bound that makes the loop finite); zeros while nothing is configured.
 * ca_nav_get_field: host copies of one field -- dist f32 [gy * gx], next u8, blocked u8 (0 / 1) -- of `arena`'s set (any arena names the
 * one set of per_arena = 0); any pointer may be NULL; cells_cap < gx * gy -> CA_ESIZE.  Synchronises.
 * ca_nav_pref: one small launch; flags 0 or CA_F_FREEZE (anything else -> CA_EINVAL).  dist_out: DEVICE f32 [A, N] or NULL.
 * ca_rollout_nav(env, T, flags, tr) is the loop  for each step: ca_nav_pref(env, NULL, flags & CA_F_FREEZE); ca_orca_step(env, flags)
 * without the returns to the host, always as launches per step (also where ca_rollout is one launch).  Flags are ca_rollout's; CA_F_OBS
 * and CA_F_CONTACT each add one launch behind the last step.  tr != NULL: ca_rollout_trace's checks and records (record r = the state
 * after (r + 1) * every steps).  The sticky overflow status works as in ca_rollout.  Without a navigation -> CA_EINVAL; a refusal
 * advances nothing.
 * ca_nav_mask_build: the mask builder itself, handle-free and without a device (tests, tools), for the n_edges edges
 * edges_pq[n_edges][4] = (px, py, qx, qy): blocked[gy * gx] = 0 / 1.  cells_cap < gx * gy -> CA_ESIZE; a grid outside the limits ->
 * CA_EINVAL; messages through ca_last_error(NULL). */
#define CA_NAV_MAX_CELLS 32768
#define CA_NAV_MAX_GOALS 16
#define CA_NAV_MAX_LOOKAHEAD 8
#define CA_NAV_STAY 8
#define CA_NAV_NONE 9
typedef struct ca_nav_desc {
    float x0, y0, cell;            /* the grid's origin and cell size */
    int32_t gx, gy;                /* its sides */
    float clearance;               /* >= 0: how near an edge a cell centre may lie (a caller's usual choice: ca_config.radius) */
    int32_t n_goals;               /* G: 1 .. CA_NAV_MAX_GOALS */
    int32_t per_arena;             /* 0: one field set, targets [G, 2]; 1: a set per arena, targets [A, G, 2] */
    const float* targets;          /* HOST f32 (x, y) */
    size_t targets_bytes;
    const int32_t* agent_class;    /* HOST i32 [A, N]: the target an agent walks to, or -1: not navigated */
    size_t class_bytes;
    int32_t lookahead;             /* pointer steps per ca_nav_pref: 1 .. CA_NAV_MAX_LOOKAHEAD */
} ca_nav_desc;
int ca_nav_configure(ca_env* env, const ca_nav_desc* desc);
int ca_nav_clear(ca_env* env);
int ca_nav_info(ca_env* env, int32_t* configured, int32_t* gx, int32_t* gy, int32_t* n_goals, int32_t* n_sets, int32_t* sweeps_max);
int ca_nav_get_field(ca_env* env, int32_t arena, int32_t goal, float* dist, uint8_t* next, uint8_t* blocked, int32_t cells_cap);
int ca_nav_pref(ca_env* env, float* dist_out, uint32_t flags);
int ca_rollout_nav(ca_env* env, int32_t steps, uint32_t flags, const ca_trace* tr);
int ca_nav_mask_build(const float* edges_pq, int32_t n_edges, float x0, float y0, float cell, int32_t gx, int32_t gy, float clearance,
                      uint8_t* blocked, int32_t cells_cap);

/* Action steps steered by the navigation fields.  ca_step, ca_rollout_actions and ca_rollout_policy rotate the straight line to the
 * agent's own goal by the action, so behind a wall an action of 0 walks into the wall and the reward's progress term pays for pushing
 * against it.  Here the action rotates the navigation heading instead, and the reward counts progress along that heading.  No solve
 * kernel knows about it: every solve family reads CA_FLD_PREF_X / _Y as its input when no actions are given and leaves CA_FLD_VEL_*
 * unchanged across a respawn, so a navigated action step is a small kernel in front of the launches of ca_orca_step and a small kernel
 * behind them.  Every value is defined bit for bit: fp32 / fp64 exactly as written, one rounding per operation, no contraction.
 *
 * ca_nav_act(env, actions, heading_out, dist_out, flags): ONE launch (nav_act_kernel), one lane per agent row.  actions DEVICE f32
 * [A, N]; heading_out DEVICE f32 [2, A, N] or NULL; dist_out DEVICE f32 [A, N] or NULL; flags 0 or CA_F_FREEZE.
 *   - A row is STEERED if it is present (i < counts[a] under ca_set_agent_counts) and not (CA_F_FREEZE and arena_done[a] != 0).  A
 *     row that is not steered is not written at all.
 *   - The point T a steered row heads for: if ca_nav_pref would navigate the row (agent_done == 0, class in 0 .. G-1), T is what
 *     ca_nav_pref heads for -- the centre of the cell reached after `lookahead` pointer steps (x0 + ((float)cx + 0.5f) * cell, as a
 *     double), or the agent's own goal when the walk never moved or ended on CA_NAV_STAY.  Otherwise (class -1, or a done agent
 *     walking to its second goal) T is the agent's own goal (CA_FLD_GOAL_X / _Y).
 *   - For a steered row, the function of the solve kernels (csrc/ca_rules.h action_pref; env.py:371-383):
 *         (pf_x, pf_y) = pref_dir64(pos, T)                       the fp64 unit vector pos -> T (env.py:156-162)
 *         (sn, cs) = sincos64((double)action)
 *         rl_x = pf_x * cs - pf_y * sn;   rl_y = pf_x * sn + pf_y * cs        (fp64)
 *         dir = ((float)pf_x, (float)pf_y);   rot = ((float)rl_x, (float)rl_y)
 *     It writes CA_FLD_PREF_X / _Y = rot, heading_out = dir where given, and dir and rot into a buffer of the handle's ([4, A, N],
 *     allocated on first use, freed by ca_destroy; no ca_field and no state: ca_arena_gather and ca_snapshot_* do not move it).  For
 *     navigated rows only, dist_out follows ca_nav_pref's rule.  The lane of agent 0 notes per arena whether it is steered (1) or
 *     frozen (0) for the kernel behind the step.
 *   Without a navigation, NULL actions or any other flag -> CA_EINVAL.
 *
 * ca_nav_step(env, actions, flags) is, by definition,
 *     1. ca_nav_act(env, actions, NULL, NULL, flags & CA_F_FREEZE)
 *     2. ca_orca_step(env, flags & (CA_F_STATS | CA_F_AUTORESET | CA_F_FREEZE))
 *     3. one launch of nav_reward_kernel: for every present row of an arena that step 1 noted as steered,
 *            CA_FLD_REWARD = step_reward(reward_scale, (VEL_X, VEL_Y) as step 2 left them, dir, rot)          (csrc/ca_rules.h; env.py:389-400)
 *            = scale * (vel.x * dir.x + vel.y * dir.y) + (1.0f - scale) * (vel.x * rot.x + vel.y * rot.y),  scale = (float)reward_scale, in fp32.
 *        Under CA_F_AUTORESET the velocity survives the respawn, so the step that ends an episode is rewarded like any other.  Rows
 *        of a frozen arena keep their reward.  Under CA_F_STATS the arena's rewards are added into the arena's sum_reward in f64; the
 *        order of that sum is not defined: it agrees with a sequential sum to 1e-9 relative, the tolerance of tiled handles.
 *     4. one observation launch (CA_F_OBS) and one contact launch (CA_F_CONTACT) for the state left, if asked for.
 *   Everything else is what ca_orca_step leaves: the step counter, the done test, arrive_step (counted the ORCA-only way: the counter
 *   is incremented before the done test, so an arrival reads one more than under ca_step), the collision statistics, the PREF field
 *   afterwards (the unit vector from the new position to the goal, not the rotated direction ca_step leaves), and the observation
 *   frame.  With no row navigated, POS, VEL, REWARD, the goals, the done flags and the counters are ca_step's, bit for bit.
 *   CA_F_NODONE or an unknown bit, NULL actions, no navigation -> CA_EINVAL; a refusal advances nothing.  The sticky overflow status
 *   works as in ca_rollout.
 *
 * ca_rollout_nav_actions(env, steps, flags, seq) is the loop of ca_nav_step(env, actions + (t / hold) * A * N, flags); returns and
 * first_done follow exactly the rules of ca_rollout_actions (ret = ret + w * r in two fp32 operations, freezing, absent rows, the
 * sum running across a respawn), and it takes ca_rollout_actions's checks, messages and steps == 0 behaviour; CA_F_OBS / CA_F_CONTACT
 * are one launch behind the last step.  ca_rollout_nav_policy(env, steps, flags, seq) is the loop of ca_rollout_policy's definition
 * with ca_nav_step in place of ca_step: the same records, the same checks.  Both -> CA_EINVAL without a navigation, before anything else
 * is looked at.  Both always take the per-step form, also where ca_rollout is one launch (as ca_rollout_nav and ca_rollout_policy do):
 * per step nav_act_kernel, the launches of the ORCA-only step, and ONE kernel behind them -- nav_reward_kernel takes the return,
 * first_done and the reward / done records as optional arguments, so no second accumulate launch follows.  A held action is re-rotated
 * every step about that step's heading, as ca_step re-derives the goal direction every step.  ca_profile counts both kernels under kind 3. */
int ca_nav_act(ca_env* env, const float* actions, float* heading_out, float* dist_out, uint32_t flags);
int ca_nav_step(ca_env* env, const float* actions, uint32_t flags);
int ca_rollout_nav_actions(ca_env* env, int32_t steps, uint32_t flags, const ca_action_seq* seq);
int ca_rollout_nav_policy(ca_env* env, int32_t steps, uint32_t flags, const ca_policy_seq* seq);

/* Reward terms: collisions, walls, crowding, arrival and time, on the device.  The reward a step writes from actions is the reference's
 * (env.py:389-400): progress along the goal direction and along the commanded direction.  While terms are configured, every such step
 * runs one small kernel in front of its launches (reward_begin_kernel) and one behind them (reward_terms_kernel), and the kernel behind
 * rewrites CA_FLD_REWARD as a weighted sum of the reference's reward r_ref and six per-agent counts, so that everything that reads the
 * field afterwards -- returns, the reward records, row_rewards, advantages and targets of the rollouts, the packed copy of
 * ca_step_packed -- is computed from the shaped reward.  No solve, observation, contact, record or policy kernel knows about it.
 * All arithmetic is fp32, one rounding per operation, never contracted.
 *
 * The terms, CA_REWARD_N_TERMS = 7 with weights w[0 .. 6]; c_k for agent i of arena a, of the state the step leaves:
 *   0 CA_REWARD_BASE       no count: it multiplies the reference reward r_ref that the step wrote
 *   1 CA_REWARD_COLLISION  number of other present agents j with absSq(p_i - p_j) < sqr(r_i + r_j)   (the contact report's `agents`)
 *   2 CA_REWARD_WALL       1 if distSqPointSegment(edge, p_i) < sqr(r_i) for any edge of the arena's table, else 0   (the report's `wall`)
 *   3 CA_REWARD_NEAR       number of other present agents j with absSq(p_i - p_j) < sqr((r_i + r_j) + margin); the touching ones included
 *   4 CA_REWARD_WALL_NEAR  1 if the smallest distSqPointSegment over the edges is < sqr(r_i + margin), else 0
 *   5 CA_REWARD_ARRIVAL    1 if the agent arrived in this step (rule below), else 0
 *   6 CA_REWARD_STEP       1 if the agent was not done in front of the step (agent_done == 0), else 0: the count of a time penalty.
 *                          Under CA_DONE_REGOAL it is always 1.
 * r_i is the agent's own radius under ca_set_agent_params, else ca_config.radius; j = i is left out by index, as in the contact
 * report; no range limit applies; absent rows of ca_set_agent_counts are never a j and are not written.
 *
 * The shaped reward:  r = w0 * r_ref  (one multiply);  then for k = 1 .. 6 ascending, where w_k != 0:  r = r + w_k * (float)c_k  (one
 * multiply and one add, each rounded).  A term whose weight is exactly 0 is skipped, so the weights (1, 0, 0, 0, 0, 0, 0) leave the
 * reward's bits unchanged.
 *
 * Rows that are shaped: every present row of an arena that the step advanced.  Under CA_F_FREEZE an arena whose arena_done was set in
 * front of the step keeps the reward it holds (the kernel in front notes this per arena); such rows, like absent ones, are written
 * neither in CA_FLD_REWARD nor in the parts.
 *
 * Arrival.  The kernel in front saves one word per agent.  CA_DONE_XLESS / CA_DONE_GOAL: agent_done; arrived means saved == 0 and
 * agent_done != 0 behind the step.  CA_DONE_REGOAL: regoal_count; arrived means regoal_count changed.
 *
 * A step that respawned its arena (CA_F_AUTORESET among the step's flags and arena_done[a] != 0 behind the step): the positions are
 * the next episode's, so c1 .. c4 are 0 for that step, as the contact report documents for its own planes.  In modes 0 / 1 the done
 * flags were cleared, and the arrival test reads the arena's last-episode word instead (CA_FLD_ARENA_STATS slot 7, length << 32 |
 * agents that arrived, written by every solve kernel whenever an episode ends): an agent with saved == 0 arrived iff the word's low
 * half equals the arena's agent count.  ONE CASE IS LEFT OUT: at an episode that the step cap ends with some agents still under way,
 * an agent arriving in that very step is not credited.
 *
 * Statistics.  Under CA_F_STATS the kernel adds (double)r - (double)r_ref of the arena's shaped rows into the arena's sum_reward,
 * which afterwards is the sum of the shaped rewards.  The order of that sum is not defined: it agrees with a sequential float64 sum
 * to 1e-9 * sum(|r|) (n * 2^-53 for fewer than 10^6 addends; the tolerance of tiled handles and of ca_nav_step).
 *
 * Parts.  The kernel also leaves a buffer of the handle's, [7, A, N] words, allocated on first use: plane 0 is r_ref (f32), planes
 * 1 .. 6 are c_1 .. c_6 (i32).  No ca_field and no state: ca_arena_gather and ca_snapshot_* do not move it.  A count whose weight is 0
 * in every arena is stored as 0 (the pair scan is not made when no arena weighs term 1 or 3, the wall scan when none weighs 2 or 4).
 * ca_reward_parts recomputes the buffer for the current state in one launch, like ca_contacts: plane 0 is the reward field as it
 * stands, arrival is 0, step is agent_done == 0, every present row is written and the reward is not; CA_EINVAL without terms.
 * ca_get_reward_parts copies the planes out (either pointer may be NULL; CA_ESIZE unless ref_bytes == A * N * 4 and counts_bytes ==
 * 6 * A * N * 4; CA_EINVAL before anything was computed on the handle).  ca_reward_parts_ptr: the zero-copy view (allocates the buffer
 * if needed; valid until ca_destroy).
 *
 * ca_reward_configure: all checks run before anything changes, and a failure leaves the handle as it was.  A NULL argument or per_arena
 * outside 0 / 1 -> CA_EINVAL; weights_bytes not exactly the layout -> CA_ESIZE; a non-finite weight -> CA_ERANGE (ca_last_error names
 * the arena and the term); a margin that is not finite, negative or above CA_MAX_LENGTH -> CA_ERANGE.  It drains the stream; calling it
 * again replaces the terms.  The terms are configuration: they survive ca_reset*, CA_F_AUTORESET, ca_init_scenario and
 * ca_set_obstacles*, and per-arena weights stay with the slot under ca_arena_gather / ca_snapshot_load.  ca_reward_clear removes them;
 * ca_reward_get_weights returns [A, 7] as the kernel uses them (CA_EINVAL without terms).
 *
 * While configured, the terms apply to every call that writes the reward from actions: ca_step, ca_step_host, ca_step_packed (shaped
 * before the packed copy); ca_rollout_actions, ca_rollout_policy, ca_rollout_policy_sample; ca_nav_step, ca_rollout_nav_actions,
 * ca_rollout_nav_policy -- a navigated step then runs nav_reward_kernel in its single-step form, the terms kernel behind it, and for
 * the two rollouts the ordinary accumulate / record launch last (three launches more per step than without terms, two for ca_nav_step).
 * NOT AFFECTED: ORCA-only steps and ca_rollout* without actions, which write no reward, and ca_alan_*, whose fp64 reward lives inside
 * the bandit's kernels.  On a handle whose ca_rollout_actions is one launch per 256 steps, the call takes the per-step form while terms
 * are set -- the terms need the state between steps --; ca_solver_info does not change.  ca_profile counts the two kernels under
 * kind 3; a handle without terms launches nothing new. */
#define CA_REWARD_N_TERMS 7
#define CA_REWARD_BASE 0
#define CA_REWARD_COLLISION 1
#define CA_REWARD_WALL 2
#define CA_REWARD_NEAR 3
#define CA_REWARD_WALL_NEAR 4
#define CA_REWARD_ARRIVAL 5
#define CA_REWARD_STEP 6
typedef struct ca_reward_desc {
    const float* weights;   /* HOST f32 [CA_REWARD_N_TERMS], or [A, CA_REWARD_N_TERMS] with per_arena = 1 */
    size_t  weights_bytes;
    int32_t per_arena;      /* 0 | 1 */
    float   margin;         /* the comfort distance of terms 3 and 4: 0 .. CA_MAX_LENGTH */
} ca_reward_desc;
int ca_reward_configure(ca_env* env, const ca_reward_desc* desc);
int ca_reward_clear(ca_env* env);
int ca_reward_info(ca_env* env, int32_t* configured, int32_t* per_arena, float* margin);
int ca_reward_get_weights(ca_env* env, float* weights, size_t bytes);   /* [A, 7] as the kernel uses them */
int ca_reward_parts(ca_env* env);
int ca_get_reward_parts(ca_env* env, float* ref, int32_t* counts /* [6, A, N] */, size_t ref_bytes, size_t counts_bytes, int32_t dst_is_device);
int ca_reward_parts_ptr(ca_env* env, void** dev_ptr, size_t* bytes);

/* Hash of the kernel sources and compiler flags this library was built from (collision_avoidance_amd/build.py compiles
 * it in): reports and counter profiles quote it, so that they name the code that ran.  No reference counterpart. */
const char* ca_source_sha(void);

#ifdef __cplusplus
}
#endif
#endif
