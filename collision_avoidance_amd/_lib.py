"""ctypes binding of libcaenv.so (the C ABI of include/ca_env.h).

Fails loudly: if the library is missing or a call returns an error code a RuntimeError carrying
ca_last_error() is raised.  There is no CPU fallback of any kind.
"""
import ctypes as C
import os

from . import build as _build

OBS_DIM = 64
MAX_NEIGHBORS, MAX_OBST_NEIGHBORS, MAX_AGENTS = 16, 64, 1024
MAX_AGENTS_LARGE = 16384   # on a tiled handle (ca_create_ex with CREATE_TILED)
CREATE_TILED = 1
CREATE_TILED_GRID = 4   # only together with CREATE_TILED: the uniform-grid neighbour search of the tiled path
CREATE_TILED_PARAMS = 16   # only together with CREATE_TILED: the tiled handle takes ca_set_agent_params
CREATE_TILED_WIDE = 32   # only together with CREATE_TILED, never with CREATE_TILED_PARAMS: max_obst_neighbors up to 64 on the tiled handle
EDGE_GRID_MAX_EDGES, EDGE_GRID_MAX_ENTRIES = 65535, 1 << 22   # per table of the static edge grid (ca_tiled_edge_grid)
DONE_XLESS, DONE_GOAL, DONE_REGOAL = 0, 1, 2
F_OBS, F_STATS, F_AUTORESET, F_NODONE, F_FREEZE = 1, 2, 4, 8, 16
F_CONTACT = 32   # leave the per-agent contact report of the state the call leaves (ca_get_contacts)
TRACE_POS, TRACE_VEL = 1, 2   # channels of a recording rollout (struct ca_trace)
SCN_CROWD, SCN_CIRCLE, SCN_DOORWAY, SCN_CONGESTED, SCN_INCOMING, SCN_BLOCKS, SCN_DEADLOCK, SCN_CROWD_SEPARATED = range(8)

(FLD_POS_X, FLD_POS_Y, FLD_VEL_X, FLD_VEL_Y, FLD_PREF_X, FLD_PREF_Y, FLD_GOAL_X, FLD_GOAL_Y,
 FLD_GOAL2_X, FLD_GOAL2_Y, FLD_REWARD, FLD_AGENT_DONE, FLD_ARRIVE_STEP, FLD_NB_COUNT, FLD_NB_IDX,
 FLD_OBST_COUNT, FLD_OBST_IDX, FLD_OBS, FLD_STEP_COUNT, FLD_ARENA_DONE, FLD_EPISODE,
 FLD_REGOAL_COUNT, FLD_ALAN_WEIGHTS, FLD_ALAN_TIMES, FLD_ALAN_ACTION, FLD_ARENA_STATS) = range(26)

EXPORTS = ("ca_create", "ca_destroy", "ca_last_error", "ca_set_stream", "ca_set_obstacles", "ca_init_scenario", "ca_set",
           "ca_get", "ca_field_ptr", "ca_bind_obs", "ca_reset", "ca_step", "ca_step_host", "ca_orca_step", "ca_observe", "ca_rollout",
           "ca_get_stats", "ca_reset_stats", "ca_sync", "ca_debug_math", "ca_profile", "ca_profile_read", "ca_launch_info",
           "ca_alan_configure", "ca_alan_step", "ca_alan_rollout", "ca_reset_masked", "ca_get_obstacles",
           "ca_set_obstacles_per_arena", "ca_get_obstacles_arena", "ca_solver_info", "ca_source_sha", "ca_host_alloc", "ca_host_free",
           "ca_step_packed", "ca_allow_obstacle_overflow", "ca_alan_configure_per_arena", "ca_alan_actions_arena",
           "ca_set_agent_params", "ca_get_agent_params", "ca_agent_params_info",
           "ca_set_agent_counts", "ca_get_agent_counts", "ca_agent_counts_info", "ca_create_ex", "ca_tiled_info", "ca_tiled_grid_info",
           "ca_rollout_trace", "ca_alan_rollout_trace", "ca_tiled_edge_grid", "ca_tiled_edge_grid_info", "ca_edge_grid_build",
           "ca_contacts", "ca_get_contacts", "ca_contacts_ptr",
           "ca_set_agent_sensing", "ca_get_agent_sensing", "ca_agent_sensing_info", "ca_nbr_seed_info", "ca_lp3_pairs_info",
           "ca_arena_gather", "ca_snapshot_create", "ca_snapshot_save", "ca_snapshot_load", "ca_snapshot_destroy",
           "ca_fork_bytes_per_arena", "ca_rollout_actions",
           "ca_policy_configure", "ca_policy_clear", "ca_policy_info", "ca_policy_actions", "ca_rollout_policy",
           "ca_policy_set_heads", "ca_policy_clear_heads", "ca_policy_heads_info", "ca_policy_evaluate", "ca_rollout_policy_sample", "ca_gae",
           "ca_nav_configure", "ca_nav_clear", "ca_nav_info", "ca_nav_get_field", "ca_nav_pref", "ca_rollout_nav", "ca_nav_mask_build",
           "ca_nav_act", "ca_nav_step", "ca_rollout_nav_actions", "ca_rollout_nav_policy",
           "ca_reward_configure", "ca_reward_clear", "ca_reward_info", "ca_reward_get_weights", "ca_reward_parts", "ca_get_reward_parts",
           "ca_reward_parts_ptr")
POLICY_OUT_IDENTITY, POLICY_OUT_CLIP = 0, 1   # out_mode of a policy (struct ca_policy_desc)
POLICY_MAX_LAYERS, POLICY_MAX_WIDTH = 4, 128
POLICY_LOGSTD_MIN, POLICY_LOGSTD_MAX = -20.0, 2.0   # the clamp of a log-std head (ca_policy_set_heads)
NAV_MAX_CELLS, NAV_MAX_GOALS, NAV_MAX_LOOKAHEAD = 32768, 16, 8   # limits of a navigation (struct ca_nav_desc)
NAV_STAY, NAV_NONE = 8, 9   # `next` of the source cell / of a cell nothing leads out of
REWARD_N_TERMS = 7   # the terms of a shaped reward (struct ca_reward_desc), in the order of their weights:
REWARD_BASE, REWARD_COLLISION, REWARD_WALL, REWARD_NEAR, REWARD_WALL_NEAR, REWARD_ARRIVAL, REWARD_STEP = range(7)
REWARD_TERMS = ("base", "collision", "wall", "near", "wall_near", "arrival", "step")
MAX_LENGTH = 1e3   # CA_MAX_LENGTH: the largest length a handle takes (a reward margin among them)
NAV_OFFSETS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))   # (dx, dy) of pointer k = 0 .. 7


class Config(C.Structure):
    """struct ca_config (include/ca_env.h)."""
    _fields_ = [
        ("n_arenas", C.c_int32), ("n_agents", C.c_int32), ("arena_offset", C.c_int64),
        ("seed", C.c_uint64), ("reward_scale", C.c_double), ("time_step", C.c_float),
        ("neighbor_dist", C.c_float), ("max_neighbors", C.c_int32), ("time_horizon", C.c_float),
        ("time_horizon_obst", C.c_float), ("radius", C.c_float), ("max_speed", C.c_float),
        ("max_obst_neighbors", C.c_int32), ("max_step", C.c_int32), ("done_mode", C.c_int32),
        ("done_x_thresh", C.c_float), ("spawn_x0", C.c_float), ("spawn_x1", C.c_float),
        ("spawn_y0", C.c_float), ("spawn_y1", C.c_float), ("goal_x0", C.c_float),
        ("goal_x1", C.c_float), ("goal_y0", C.c_float), ("goal_y1", C.c_float),
    ]


class Stats(C.Structure):
    """struct ca_stats (include/ca_env.h)."""
    _fields_ = [("agent_steps", C.c_uint64), ("episodes", C.c_uint64), ("collisions", C.c_uint64),
                ("obst_collisions", C.c_uint64), ("goals_reached", C.c_uint64),
                ("obst_overflow", C.c_uint64), ("sum_reward", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Trace(C.Structure):
    """struct ca_trace (include/ca_env.h): the caller's buffers of a recording rollout."""
    _fields_ = [("agents", C.c_void_p), ("agents_bytes", C.c_size_t), ("arenas", C.c_void_p), ("arenas_bytes", C.c_size_t),
                ("every", C.c_int32), ("channels", C.c_uint32)]


class ActionSeq(C.Structure):
    """struct ca_action_seq (include/ca_env.h): the caller's buffers of an action-sequence rollout."""
    _fields_ = [("actions", C.c_void_p), ("actions_bytes", C.c_size_t), ("hold", C.c_int32),
                ("weights", C.c_void_p), ("weights_bytes", C.c_size_t), ("returns", C.c_void_p), ("returns_bytes", C.c_size_t),
                ("first_done", C.c_void_p), ("first_done_bytes", C.c_size_t)]


class PolicyDesc(C.Structure):
    """struct ca_policy_desc (include/ca_env.h): the layers of a policy as ca_policy_configure takes them."""
    _fields_ = [("n_layers", C.c_int32), ("width", C.c_int32 * 5), ("weights", C.c_void_p * 4), ("weights_bytes", C.c_size_t * 4),
                ("bias", C.c_void_p * 4), ("bias_bytes", C.c_size_t * 4), ("src_is_device", C.c_int32), ("n_sets", C.c_int32),
                ("set_of_arena", C.c_void_p), ("set_of_arena_bytes", C.c_size_t), ("out_mode", C.c_int32), ("out_limit", C.c_float)]


class PolicySeq(C.Structure):
    """struct ca_policy_seq (include/ca_env.h): the caller's buffers of a policy rollout."""
    _fields_ = [("hold", C.c_int32), ("noise", C.c_void_p), ("noise_bytes", C.c_size_t), ("weights", C.c_void_p), ("weights_bytes", C.c_size_t),
                ("returns", C.c_void_p), ("returns_bytes", C.c_size_t), ("first_done", C.c_void_p), ("first_done_bytes", C.c_size_t),
                ("obs_out", C.c_void_p), ("obs_out_bytes", C.c_size_t), ("actions_out", C.c_void_p), ("actions_out_bytes", C.c_size_t),
                ("rewards_out", C.c_void_p), ("rewards_out_bytes", C.c_size_t), ("done_out", C.c_void_p), ("done_out_bytes", C.c_size_t)]


class PolicyHeads(C.Structure):
    """struct ca_policy_heads (include/ca_env.h): the value and log-std rows as ca_policy_set_heads takes them."""
    _fields_ = [("value_w", C.c_void_p), ("value_w_bytes", C.c_size_t), ("value_b", C.c_void_p), ("value_b_bytes", C.c_size_t),
                ("logstd_w", C.c_void_p), ("logstd_w_bytes", C.c_size_t), ("logstd_b", C.c_void_p), ("logstd_b_bytes", C.c_size_t)]


class PolicyEval(C.Structure):
    """struct ca_policy_eval (include/ca_env.h): the optional outputs of ca_policy_evaluate."""
    _fields_ = [("actions", C.c_void_p), ("logp", C.c_void_p), ("value", C.c_void_p), ("mean", C.c_void_p), ("log_std", C.c_void_p)]


class PolicySampleSeq(C.Structure):
    """struct ca_policy_sample_seq (include/ca_env.h): the members of ca_policy_seq and the records of a PPO batch."""
    _fields_ = list(PolicySeq._fields_) + \
        [(n + s, t) for n in ("logp_out", "dist_out", "values_out", "row_rewards_out", "row_done_out", "row_valid_out", "advantages_out",
                              "targets_out") for s, t in (("", C.c_void_p), ("_bytes", C.c_size_t))] + \
        [("gamma", C.c_float), ("lambda", C.c_float)]


class GaeDesc(C.Structure):
    """struct ca_gae_desc (include/ca_env.h): the caller's buffers of ca_gae."""
    _fields_ = [(n + s, t) for n in ("rewards", "values", "done", "valid", "advantages", "targets")
                for s, t in (("", C.c_void_p), ("_bytes", C.c_size_t))] + [("gamma", C.c_float), ("lambda", C.c_float)]


class NavDesc(C.Structure):
    """struct ca_nav_desc (include/ca_env.h): the grid, the targets and the agents' classes of a navigation."""
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("cell", C.c_float), ("gx", C.c_int32), ("gy", C.c_int32), ("clearance", C.c_float),
                ("n_goals", C.c_int32), ("per_arena", C.c_int32), ("targets", C.c_void_p), ("targets_bytes", C.c_size_t),
                ("agent_class", C.c_void_p), ("class_bytes", C.c_size_t), ("lookahead", C.c_int32)]


class RewardDesc(C.Structure):
    """struct ca_reward_desc (include/ca_env.h): the weights and the comfort distance of the reward terms."""
    _fields_ = [("weights", C.c_void_p), ("weights_bytes", C.c_size_t), ("per_arena", C.c_int32), ("margin", C.c_float)]


class EdgeGridDesc(C.Structure):
    """struct ca_edge_grid_desc (include/ca_env.h): one table of the static edge grid."""
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("ics_x", C.c_float), ("ics_y", C.c_float),
                ("gx", C.c_int32), ("gy", C.c_int32), ("n_entries", C.c_int32), ("margin", C.c_float)]


_lib = None


def lib_path():
    return _build.LIB_PATH


def load():
    """Load libcaenv.so (must have been built: __graft_entry__.build() / python -m
    collision_avoidance_amd.build).  Raises if it is absent -- nothing else can run the path."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError("libcaenv.so is not built (%s); run `python -m collision_avoidance_amd.build` "
                           "-- the HIP extension is the only implementation of this path" % path)
    L = C.CDLL(path)
    vp, i32, u32, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t
    L.ca_create.argtypes = [C.POINTER(Config), C.c_int, vp, C.POINTER(vp)]
    L.ca_create_ex.argtypes = [C.POINTER(Config), u32, C.c_int, vp, C.POINTER(vp)]
    L.ca_tiled_info.argtypes = [vp] + [C.POINTER(i32)] * 4
    L.ca_tiled_grid_info.argtypes = [vp] + [C.POINTER(i32)] * 3 + [C.POINTER(C.c_float), C.POINTER(i32)]
    L.ca_tiled_edge_grid.argtypes = [vp, i32]
    L.ca_tiled_edge_grid_info.argtypes = [vp, i32] + [C.POINTER(i32)] * 3 + [C.POINTER(C.c_float)] * 2 + [C.POINTER(i32)]
    L.ca_edge_grid_build.argtypes = [vp, i32, C.c_float, C.POINTER(EdgeGridDesc), vp, i32, vp, i32]
    L.ca_destroy.argtypes = [vp]
    L.ca_last_error.argtypes = [vp]
    L.ca_last_error.restype = C.c_char_p
    L.ca_set_stream.argtypes = [vp, vp]
    L.ca_set_obstacles.argtypes = [vp, vp, vp, i32]
    L.ca_init_scenario.argtypes = [vp, i32]
    L.ca_get_obstacles.argtypes = [vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.ca_set_obstacles_per_arena.argtypes = [vp, vp, vp, vp]
    L.ca_get_obstacles_arena.argtypes = [vp, i32, vp, vp, vp, i32, C.POINTER(i32)]
    L.ca_set.argtypes = [vp, i32, vp, sz, i32]
    L.ca_get.argtypes = [vp, i32, vp, sz, i32]
    L.ca_field_ptr.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(sz)]
    L.ca_bind_obs.argtypes = [vp, vp, sz]
    L.ca_reset.argtypes = [vp, vp, vp, i32, u32]
    L.ca_reset_masked.argtypes = [vp, vp, i32, u32]
    L.ca_step.argtypes = [vp, vp, u32]
    L.ca_step_host.argtypes = [vp, vp, u32]
    L.ca_step_packed.argtypes = [vp, vp, u32, vp, sz]
    L.ca_host_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.ca_host_free.argtypes = [vp, vp]
    L.ca_orca_step.argtypes = [vp, u32]
    L.ca_observe.argtypes = [vp]
    L.ca_contacts.argtypes = [vp]
    L.ca_get_contacts.argtypes = [vp, vp, vp, vp, vp, vp, sz, i32]
    L.ca_contacts_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.ca_rollout.argtypes = [vp, i32, u32]
    L.ca_alan_configure.argtypes = [vp, vp, i32, C.c_double, C.c_double, C.c_double]
    L.ca_alan_configure_per_arena.argtypes = [vp, vp, vp, C.c_double, C.c_double, C.c_double]
    L.ca_alan_actions_arena.argtypes = [vp, i32, vp, i32, C.POINTER(i32)]
    L.ca_alan_step.argtypes = [vp, vp, i32, u32]
    L.ca_alan_rollout.argtypes = [vp, i32, u32]
    L.ca_rollout_trace.argtypes = [vp, i32, u32, C.POINTER(Trace)]
    L.ca_alan_rollout_trace.argtypes = [vp, i32, u32, C.POINTER(Trace)]
    L.ca_rollout_actions.argtypes = [vp, i32, u32, C.POINTER(ActionSeq)]
    L.ca_policy_configure.argtypes = [vp, C.POINTER(PolicyDesc)]
    L.ca_policy_clear.argtypes = [vp]
    L.ca_policy_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32 * 5), C.POINTER(i32)]
    L.ca_policy_actions.argtypes = [vp, vp, vp]
    L.ca_rollout_policy.argtypes = [vp, i32, u32, C.POINTER(PolicySeq)]
    L.ca_policy_set_heads.argtypes = [vp, C.POINTER(PolicyHeads)]
    L.ca_policy_clear_heads.argtypes = [vp]
    L.ca_policy_heads_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.ca_policy_evaluate.argtypes = [vp, vp, C.POINTER(PolicyEval)]
    L.ca_rollout_policy_sample.argtypes = [vp, i32, u32, C.POINTER(PolicySampleSeq)]
    L.ca_gae.argtypes = [vp, i32, C.POINTER(GaeDesc)]
    L.ca_nav_configure.argtypes = [vp, C.POINTER(NavDesc)]
    L.ca_nav_clear.argtypes = [vp]
    L.ca_nav_info.argtypes = [vp] + [C.POINTER(i32)] * 6
    L.ca_nav_get_field.argtypes = [vp, i32, i32, vp, vp, vp, i32]
    L.ca_nav_pref.argtypes = [vp, vp, u32]
    L.ca_rollout_nav.argtypes = [vp, i32, u32, C.POINTER(Trace)]
    L.ca_nav_mask_build.argtypes = [vp, i32, C.c_float, C.c_float, C.c_float, i32, i32, C.c_float, vp, i32]
    L.ca_nav_act.argtypes = [vp, vp, vp, vp, u32]
    L.ca_nav_step.argtypes = [vp, vp, u32]
    L.ca_rollout_nav_actions.argtypes = [vp, i32, u32, C.POINTER(ActionSeq)]
    L.ca_rollout_nav_policy.argtypes = [vp, i32, u32, C.POINTER(PolicySeq)]
    L.ca_reward_configure.argtypes = [vp, C.POINTER(RewardDesc)]
    L.ca_reward_clear.argtypes = [vp]
    L.ca_reward_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_float)]
    L.ca_reward_get_weights.argtypes = [vp, vp, sz]
    L.ca_reward_parts.argtypes = [vp]
    L.ca_get_reward_parts.argtypes = [vp, vp, vp, sz, sz, i32]
    L.ca_reward_parts_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.ca_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.ca_reset_stats.argtypes = [vp]
    L.ca_sync.argtypes = [vp]
    L.ca_allow_obstacle_overflow.argtypes = [vp, i32]
    L.ca_debug_math.argtypes = [vp, i32, vp, vp, i32]
    L.ca_profile.argtypes = [vp, i32]
    L.ca_profile_read.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_float)]
    L.ca_launch_info.argtypes = [vp] + [C.POINTER(i32)] * 4
    L.ca_solver_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.ca_set_agent_params.argtypes = [vp, vp, vp, vp, vp, sz, i32]
    L.ca_get_agent_params.argtypes = [vp, vp, vp, vp, vp, sz, i32]
    L.ca_agent_params_info.argtypes = [vp, C.POINTER(i32)]
    L.ca_set_agent_counts.argtypes = [vp, vp, sz, i32]
    L.ca_get_agent_counts.argtypes = [vp, vp, sz, i32]
    L.ca_agent_counts_info.argtypes = [vp, C.POINTER(i32)]
    L.ca_set_agent_sensing.argtypes = [vp, vp, vp, sz, i32]
    L.ca_get_agent_sensing.argtypes = [vp, vp, vp, sz, i32]
    L.ca_agent_sensing_info.argtypes = [vp, C.POINTER(i32)]
    L.ca_nbr_seed_info.argtypes = [vp, C.POINTER(i32)]
    L.ca_lp3_pairs_info.argtypes = [vp, C.POINTER(i32)]
    L.ca_arena_gather.argtypes = [vp, vp, sz, i32, u32]
    L.ca_snapshot_create.argtypes = [vp, C.POINTER(vp)]
    L.ca_snapshot_save.argtypes = [vp, vp]
    L.ca_snapshot_load.argtypes = [vp, vp, vp, sz, i32, u32]
    L.ca_snapshot_destroy.argtypes = [vp, vp]
    L.ca_fork_bytes_per_arena.argtypes = [vp, C.POINTER(sz)]
    L.ca_source_sha.argtypes = []
    L.ca_source_sha.restype = C.c_char_p
    for name in EXPORTS:
        if name not in ("ca_last_error", "ca_source_sha"):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def edge_grid_build(edges_pq, rng):
    """The static edge grid of one table, built on the host (ca_edge_grid_build; no device): edges_pq [n, 4] = (px, py, qx, qy),
    rng the obstacle range.  Returns (EdgeGridDesc, cell_start [gx * gy + 1] uint32, entries [n_entries] uint32); a refusal raises
    RuntimeError with the library's message."""
    import numpy as np
    L = load()
    pq = np.ascontiguousarray(edges_pq, np.float32).reshape(-1, 4)
    d = EdgeGridDesc()
    ptr = pq.ctypes.data_as(C.c_void_p) if len(pq) else None
    check(L, None, L.ca_edge_grid_build(ptr, len(pq), float(rng), C.byref(d), None, 0, None, 0), "ca_edge_grid_build")
    cs, en = np.zeros(d.gx * d.gy + 1, np.uint32), np.zeros(max(1, d.n_entries), np.uint32)
    check(L, None, L.ca_edge_grid_build(ptr, len(pq), float(rng), C.byref(d), cs.ctypes.data_as(C.c_void_p), len(cs),
                                        en.ctypes.data_as(C.c_void_p), len(en)), "ca_edge_grid_build")
    return d, cs, en[:d.n_entries]


def nav_mask_build(edges_pq, x0, y0, cell, gx, gy, clearance):
    """The blocked mask of a navigation grid, built on the host (ca_nav_mask_build; no device): edges_pq [n, 4] = (px, py, qx, qy).
    Returns uint8 [gy, gx], 1 where the cell's centre lies within `clearance` of an edge; a refusal raises RuntimeError."""
    import numpy as np
    L = load()
    pq = np.ascontiguousarray(edges_pq, np.float32).reshape(-1, 4)
    out = np.zeros((max(int(gy), 0), max(int(gx), 0)), np.uint8)
    check(L, None, L.ca_nav_mask_build(pq.ctypes.data_as(C.c_void_p) if len(pq) else None, len(pq), float(x0), float(y0), float(cell),
                                       int(gx), int(gy), float(clearance), out.ctypes.data_as(C.c_void_p), out.size), "ca_nav_mask_build")
    return out


def check(L, handle, rc, what):
    if rc != 0:
        msg = L.ca_last_error(handle)
        raise RuntimeError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
