"""Batched collision-avoidance environment on one MI355X: A independent arenas x N agents.

This is the vectorised form of the reference's Collision_Avoidance_Env (reference
collision_avoidance/envs/collision_avoidence_env.py:23-488): the same reset()/step()/orca_step()
semantics applied to every arena at once by the HIP kernels behind the C ABI of
include/ca_env.h.  PyTorch is used only to hand tensors across (observations out, actions in);
without it the same calls work on numpy arrays through host copies.
"""
import ctypes as C

import numpy as np

from . import _lib, scenarios

try:  # plumbing only
    import torch
except Exception:  # pragma: no cover
    torch = None

_I32_FIELDS = {_lib.FLD_AGENT_DONE, _lib.FLD_ARRIVE_STEP, _lib.FLD_NB_COUNT, _lib.FLD_NB_IDX,
               _lib.FLD_OBST_COUNT, _lib.FLD_OBST_IDX, _lib.FLD_STEP_COUNT, _lib.FLD_ARENA_DONE,
               _lib.FLD_EPISODE, _lib.FLD_REGOAL_COUNT, _lib.FLD_ALAN_ACTION}
_ARENA_FIELDS = {_lib.FLD_STEP_COUNT, _lib.FLD_ARENA_DONE, _lib.FLD_EPISODE}
# VecCollisionAvoidanceEnv's default list capacity is min(this, edges of the world): the reference's own worlds never bring more
# than 16 edges in range, and lists of up to 16 keep the register-line and four-lanes kernels available.  A polyline world that
# needs more asks for it: max_obst_neighbors up to _lib.MAX_OBST_NEIGHBORS (64).
DEFAULT_MAX_OBST_NEIGHBORS = 16
_F64_FIELDS = {_lib.FLD_GOAL_X, _lib.FLD_GOAL_Y, _lib.FLD_GOAL2_X, _lib.FLD_GOAL2_Y, _lib.FLD_ALAN_WEIGHTS,
               _lib.FLD_ALAN_TIMES}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _is_tensor(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _shape_of(x):
    return None if x is None else tuple(x.shape if _is_tensor(x) else np.shape(x))


_TRACE_CHANNELS = {"pos": _lib.TRACE_POS, "vel": _lib.TRACE_VEL}


def _trace_channels(channels):
    """The channel mask of struct ca_trace for ("pos", "vel"), a single name, or a mask."""
    if isinstance(channels, (int, np.integer)):
        mask = int(channels)
    else:
        names = (channels,) if isinstance(channels, str) else tuple(channels)
        unknown = [c for c in names if c not in _TRACE_CHANNELS]
        if unknown:
            raise ValueError("trace: unknown channel %r (known: 'pos', 'vel')" % (unknown[0],))
        mask = 0
        for c in names:
            mask |= _TRACE_CHANNELS[c]
    if mask == 0 or mask & ~(_lib.TRACE_POS | _lib.TRACE_VEL):
        raise ValueError("trace: channels must name 'pos', 'vel' or both, got %r" % (channels,))
    return mask


def trace_shape(steps, every, channels, A, N):
    """Shapes of the two arrays of a recording rollout (rollout(..., trace=...) / alan_rollout(..., trace=...)), without a
    device: ((R, C, A, N), (R, 3, A)) with R = steps // every records and C = 2 planes per channel, in the order pos_x, pos_y,
    vel_x, vel_y; the second is step_count, arena_done, episode per arena."""
    every = int(every)
    if every < 1:
        raise ValueError("trace: every=%d, must be at least 1" % every)
    if int(steps) < 0:
        raise ValueError("trace: steps=%d" % int(steps))
    mask = _trace_channels(channels)
    R, Cn = int(steps) // every, 2 * bin(mask).count("1")
    return (R, Cn, int(A), int(N)), (R, 3, int(A))


def fork_index(src, A, allow_keep=False):
    """The index array of fork() / restore() as the library takes it, without a device: contiguous int32 [A], entry a = the arena
    that arena a takes.  Raises ValueError for what the library would refuse: a length other than A, a dtype that is not an
    integer one (bools included), an entry outside 0 .. A-1 -- with allow_keep (restore): outside -1 .. A-1, where -1 keeps the
    arena.  A torch tensor is judged by its own dtype and shape and comes back as a host array."""
    A = int(A)
    if torch is not None and isinstance(src, torch.Tensor):
        if src.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError("fork_index: src must hold integers, got dtype %s" % (src.dtype,))
        src = src.detach().cpu().numpy()
    a = np.asarray(src)
    if a.dtype.kind not in "iu":
        raise ValueError("fork_index: src must hold integers, got dtype %s" % (a.dtype,))
    if a.shape != (A,):
        raise ValueError("fork_index: src must be an [A] array (A=%d), got shape %s" % (A, a.shape))
    lo = -1 if allow_keep else 0
    bad = np.flatnonzero((a.astype(np.int64) < lo) | (a.astype(np.int64) >= A)) if a.dtype != np.uint64 else np.flatnonzero(a >= np.uint64(A))
    if len(bad):
        raise ValueError("fork_index: arena %d takes arena %d, outside [%d, %d)" % (bad[0], int(a[bad[0]]), lo, A))
    return np.ascontiguousarray(a, np.int32)


def action_seq_shape(actions_shape, A, N, hold=1, steps=None, weights_shape=None):
    """(R, steps) of rollout_actions() for an action tensor of shape `actions_shape`, without a device.  Raises ValueError for what
    the library would refuse or misread: hold < 1, a shape other than [R, A, N], steps < 0 or a row count other than
    ceil(steps / hold), weights of a shape other than [steps].  steps=None: R * hold."""
    hold = int(hold)
    if hold < 1:
        raise ValueError("rollout_actions: hold=%d, must be at least 1" % hold)
    shape = tuple(int(d) for d in actions_shape)
    if len(shape) != 3 or shape[1:] != (int(A), int(N)):
        raise ValueError("rollout_actions: actions must be [R, A=%d, N=%d], got shape %s" % (A, N, shape))
    R = shape[0]
    steps = R * hold if steps is None else int(steps)
    if steps < 0 or (steps + hold - 1) // hold != R:
        raise ValueError("rollout_actions: steps=%d with hold=%d needs %d rows of actions, got %d" %
                         (steps, hold, (max(steps, 0) + hold - 1) // hold, R))
    if weights_shape is not None and tuple(weights_shape) != (steps,):
        raise ValueError("rollout_actions: weights must be [steps=%d], got shape %s" % (steps, tuple(weights_shape)))
    return R, steps


def policy_seq_shape(A, N, steps, hold=1, noise_shape=None, weights_shape=None):
    """The buffers of rollout_policy() without a device: dict(R=, noise=, weights=, returns=, first_done=, obs=, actions=, rewards=,
    dones=) with R = ceil(steps / hold) and the shape of every array the call reads or writes.  Raises ValueError for what the library
    would refuse or misread: hold < 1, steps < 0, noise of a shape other than [R, A, N], weights other than [steps]."""
    hold, steps, A, N = int(hold), int(steps), int(A), int(N)
    if hold < 1:
        raise ValueError("rollout_policy: hold=%d, must be at least 1" % hold)
    if steps < 0:
        raise ValueError("rollout_policy: steps=%d" % steps)
    R = (steps + hold - 1) // hold
    if noise_shape is not None and tuple(int(d) for d in noise_shape) != (R, A, N):
        raise ValueError("rollout_policy: noise must be [R=%d, A=%d, N=%d] (R = ceil(steps / hold)), got shape %s" %
                         (R, A, N, tuple(noise_shape)))
    if weights_shape is not None and tuple(int(d) for d in weights_shape) != (steps,):
        raise ValueError("rollout_policy: weights must be [steps=%d], got shape %s" % (steps, tuple(weights_shape)))
    return dict(R=R, noise=(R, A, N), weights=(steps,), returns=(A, N), first_done=(A,), obs=(R, A, N, _lib.OBS_DIM),
                actions=(R, A, N), rewards=(steps, A, N), dones=(steps, A))


def policy_layers(layers):
    """The layers of set_policy() as the library takes them, without a device: (widths [w0 .. wL], P, [W_l float32 [P, out, in]],
    [b_l float32 [P, out]]), C-contiguous host arrays.  `layers` is a list of (W, b) pairs -- numpy arrays or torch tensors, W
    [out, in] and b [out] (one set) or W [P, out, in] and b [P, out] (P sets) -- or a torch.nn.Sequential of Linear modules with a
    ReLU between every two.  Raises ValueError for what ca_policy_configure would refuse: fewer than 2 or more than 4 layers, a first
    width other than 64, a hidden width that is no multiple of 16 in 16 .. 128, an output width other than 1, layers that do not
    chain, sets of different sizes, a value that is not finite."""
    if torch is not None and isinstance(layers, torch.nn.Module):
        mods = list(layers.children()) if isinstance(layers, torch.nn.Sequential) else None
        if mods is None:
            raise ValueError("set_policy: a module must be a torch.nn.Sequential of Linear and ReLU")
        pairs = []
        for k, m in enumerate(mods):
            if k % 2 == 0 and isinstance(m, torch.nn.Linear) and m.bias is not None:
                pairs.append((m.weight, m.bias))
            elif not (k % 2 == 1 and isinstance(m, torch.nn.ReLU) and k < len(mods) - 1):
                raise ValueError("set_policy: module %d of the Sequential is %s; expected Linear (with bias), ReLU, ..., Linear" %
                                 (k, type(m).__name__))
        layers = pairs
    host = lambda t: t.detach().cpu().numpy() if torch is not None and isinstance(t, torch.Tensor) else t
    layers = [(np.asarray(host(W), np.float32), np.asarray(host(b), np.float32)) for W, b in layers]
    if not 2 <= len(layers) <= _lib.POLICY_MAX_LAYERS:
        raise ValueError("set_policy: %d layers, must be 2 .. %d" % (len(layers), _lib.POLICY_MAX_LAYERS))
    Ws, bs, widths, P = [], [], [], None
    for l, (W, b) in enumerate(layers):
        if W.ndim == 2 and b.ndim == 1:
            W, b = W[None], b[None]
        if W.ndim != 3 or b.ndim != 2 or b.shape != W.shape[:2]:
            raise ValueError("set_policy: layer %d: W %s and b %s are not [out, in] and [out] (or [P, out, in] and [P, out])" %
                             (l, W.shape, b.shape))
        if P is None:
            P, widths = W.shape[0], [W.shape[2]]
        if W.shape[0] != P:
            raise ValueError("set_policy: layer %d holds %d sets, layer 0 holds %d" % (l, W.shape[0], P))
        if W.shape[2] != widths[-1]:
            raise ValueError("set_policy: layer %d reads %d values, the layer before it writes %d" % (l, W.shape[2], widths[-1]))
        if not (np.isfinite(W).all() and np.isfinite(b).all()):
            raise ValueError("set_policy: layer %d holds a value that is not finite" % l)
        widths.append(W.shape[1])
        Ws.append(np.ascontiguousarray(W)); bs.append(np.ascontiguousarray(b))
    if widths[0] != _lib.OBS_DIM:
        raise ValueError("set_policy: the first layer reads %d values, an observation has %d" % (widths[0], _lib.OBS_DIM))
    for l, w in enumerate(widths[1:-1], 1):
        if w % 16 or not 16 <= w <= _lib.POLICY_MAX_WIDTH:
            raise ValueError("set_policy: hidden width %d of layer %d, must be a multiple of 16 in 16 .. %d" % (w, l, _lib.POLICY_MAX_WIDTH))
    if widths[-1] != 1:
        raise ValueError("set_policy: the output layer has %d units, must be 1" % widths[-1])
    return [int(w) for w in widths], int(P), Ws, bs


def policy_heads(width, P, value=None, log_std=None):
    """The heads of set_policy_heads() as the library takes them, without a device: dict(value_w=, value_b=, logstd_w=, logstd_b=) of
    C-contiguous float32 host arrays -- weights [P, width], biases [P] -- or None for what is absent (logstd_w None with logstd_b
    given: a state-independent log-std).  width: the policy's last hidden width, P: its number of weight sets.  value = (w, b) or a
    torch.nn.Linear(width, 1); log_std = (w_or_None, b) or a Linear; w [width], [1, width] or [P, width], b a scalar, [1] or [P].
    Raises ValueError for what ca_policy_set_heads would refuse: no head at all, a shape that does not fit, a value that is not
    finite."""
    width, P = int(width), int(P)
    host = lambda t: t.detach().cpu().numpy() if torch is not None and isinstance(t, torch.Tensor) else t

    def one(name, head):
        if head is None:
            return None, None
        if torch is not None and isinstance(head, torch.nn.Linear):
            if head.bias is None or head.out_features != 1:
                raise ValueError("set_policy_heads: the %s head must be a Linear(%d, 1) with a bias" % (name, width))
            head = (head.weight, head.bias)
        if not isinstance(head, (tuple, list)) or len(head) != 2:
            raise ValueError("set_policy_heads: the %s head must be (w, b) or a torch.nn.Linear" % name)
        w, b = head
        if b is None:
            raise ValueError("set_policy_heads: the %s head has no bias" % name)
        if w is None and name == "value":
            raise ValueError("set_policy_heads: the value head has no weights")
        b = np.asarray(host(b), np.float32).reshape(-1)
        if b.size == 1 and P > 1:
            b = np.repeat(b, P)
        if b.shape != (P,):
            raise ValueError("set_policy_heads: the %s bias must hold one value per weight set (P=%d), got shape %s" % (name, P, b.shape))
        if w is not None:
            w = np.asarray(host(w), np.float32)
            if w.ndim == 1:
                w = w[None]
            if w.ndim != 2 or w.shape[1] != width or w.shape[0] not in (1, P):
                raise ValueError("set_policy_heads: the %s weights must be [%d] or [P=%d, %d] (the last hidden width), got shape %s" %
                                 (name, width, P, width, w.shape))
            w = np.ascontiguousarray(np.broadcast_to(w, (P, width)))
            if not np.isfinite(w).all():
                raise ValueError("set_policy_heads: the %s head holds a weight that is not finite" % name)
        if not np.isfinite(b).all():
            raise ValueError("set_policy_heads: the %s head holds a bias that is not finite" % name)
        return w, np.ascontiguousarray(b)

    vw, vb = one("value", value)
    lw, lb = one("log_std", log_std)
    if vb is None and lb is None:
        raise ValueError("set_policy_heads: at least one head must be given")
    return dict(value_w=vw, value_b=vb, logstd_w=lw, logstd_b=lb)


def policy_sample_shape(A, N, steps, hold=1, noise_shape=None, weights_shape=None):
    """The buffers of rollout_policy_sample() without a device: policy_seq_shape's dict plus logp (R, A, N), dist (R, 2, A, N), values
    (R + 1, A, N), row_rewards (R, A, N), row_dones (R, A), row_valid (R, A), advantages and targets (R, A, N)."""
    sh = policy_seq_shape(A, N, steps, hold, noise_shape, weights_shape)
    R, A, N = sh["R"], int(A), int(N)
    sh.update(logp=(R, A, N), dist=(R, 2, A, N), values=(R + 1, A, N), row_rewards=(R, A, N), row_dones=(R, A), row_valid=(R, A),
              advantages=(R, A, N), targets=(R, A, N))
    return sh


def reward_terms(A, base=1.0, collision=0.0, wall=0.0, near=0.0, wall_near=0.0, arrival=0.0, step=0.0, margin=0.0):
    """The description of a shaped reward as ca_reward_configure takes it, without a device: (weights, per_arena, margin).  Each weight
    is a scalar or [A]; weights is float32 [7] when all are scalars (per_arena 0), else [A, 7] (per_arena 1), in the order of
    _lib.REWARD_TERMS.  Raises ValueError for what the library refuses: a weight that is not a scalar or [A] or is not finite, a
    margin that is not finite, negative or above _lib.MAX_LENGTH."""
    A = int(A)
    vals = []
    for name, v in zip(_lib.REWARD_TERMS, (base, collision, wall, near, wall_near, arrival, step)):
        v = np.asarray(v.detach().cpu().numpy() if torch is not None and isinstance(v, torch.Tensor) else v, np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != A):
            raise ValueError("reward terms: %s must be a scalar or [A=%d], got shape %s" % (name, A, v.shape))
        if not np.isfinite(v).all() or (np.abs(v) > float(np.finfo(np.float32).max)).any():
            raise ValueError("reward terms: %s holds a value that is not finite in float32" % name)
        vals.append(v)
    m = float(margin)
    if not np.isfinite(np.float32(m)) or m < 0.0 or np.float32(m) > np.float32(_lib.MAX_LENGTH):
        raise ValueError("reward terms: margin=%r outside [0, %g]" % (margin, _lib.MAX_LENGTH))
    per_arena = any(v.ndim == 1 for v in vals)
    if per_arena:
        w = np.stack([np.broadcast_to(v, (A,)) for v in vals], 1).astype(np.float32)
    else:
        w = np.array([float(v) for v in vals], np.float32)
    return np.ascontiguousarray(w), int(per_arena), m


class Snapshot:
    """A second set of the state buffers on the environment's device (ca_snapshot_*): made and filled by
    VecCollisionAvoidanceEnv.snapshot(), read by restore().  close() destroys it; the environment's close() invalidates every
    snapshot it still has."""

    def __init__(self, env, handle):
        self._env, self._h = env, handle

    @property
    def closed(self):
        return self._h is None or self._env.h is None or self not in self._env.__dict__.get("_snapshots", ())

    def close(self):
        if not self.closed:
            self._env._snapshots.remove(self)
            self._env._call("ca_snapshot_destroy", self._env.h, self._h)
        self._h = None


class VecCollisionAvoidanceEnv:
    """A arenas x N agents advanced per call.

    scenario: "crowd" | "circle" | "doorway" (scenarios.py) or None to leave the state unset.
    params:   dict of ca_config fields; defaults are the reference env's constants.
    use_torch: hand observations/rewards out as torch tensors on the device (zero-copy for the
               observation) and accept device tensors as actions.  False: numpy in/out.
    allow_obst_overflow: the reference's simulator keeps every obstacle edge in range of an agent (env.py:249, 301-318); the
               lists here hold max_obst_neighbors.  False (default): an agent with more edges in range makes the step
               calls raise (CA_ERANGE, naming arena and agent); True: the nearest max_obst_neighbors are kept and the event is
               only counted (stats()["obst_overflow"]).
    max_obst_neighbors: capacity of the obstacle-neighbour lists, 1 .. 64 (_lib.MAX_OBST_NEIGHBORS); None (default):
               min(16, edges of the world).  Above 16 the handle takes the wide LDS-table solve kernel and the wide observation
               (launch_info()): arenas of at most 128 agents (at 64: 64 agents with any max_neighbors, 128 with max_neighbors <= 10;
               other shapes raise CA_ERANGE at construction).  A world of subdivided walls or many pillars that raises the overflow
               error wants this raised, not allow_obst_overflow.
    agent_params: dict(radius=, max_speed=, time_horizon=, time_horizon_obst=) handed to set_agent_params() once the handle
               exists: ORCA parameters per agent instead of the four constants of `params`.
    agent_sensing: dict(neighbor_dist=, max_neighbors=) handed to set_agent_sensing() once the handle exists: how far every agent
               looks and how many others it attends to, with the two values of `params` as capacities.  On a tiled handle it
               follows the rule of agent_params=: only with tiled_params=True (ValueError).
    reward_terms: dict(base=, collision=, wall=, near=, wall_near=, arrival=, step=, margin=) handed to set_reward_terms() once the
               handle exists: the reward every step from actions writes is shaped on the device.
    agent_counts: [A] ints handed to set_agent_counts() before the scenario is initialised: arena a holds agent_counts[a] of its
               n_agents rows (n_agents becomes a capacity).  Only scenario "doorway" or None goes with it (ValueError otherwise).
    tiled:     True: the tiled solve path (ca_create_ex with CA_CREATE_TILED) -- n_agents up to _lib.MAX_AGENTS_LARGE (16384), an
               arena spread over several workgroups, a step in three launches (tiled_info()); max_obst_neighbors <= 16 (tiled_wide=True: 64), no
               agent_counts, and agent_params only with tiled_params=True (ValueError).  Results are the ordinary handle's bit for bit.  False (default): one
               workgroup per arena, n_agents <= 1024.  "grid": the tiled path with its uniform-grid neighbour search
               (CA_CREATE_TILED | CA_CREATE_TILED_GRID): the arena's agents are sorted by cell in three more launches per step and an
               agent tests the cells its range touches instead of the whole arena (tiled_grid_info()); the same results.
    edge_grid: True (with tiled="grid" only; any other handle raises the library's error): set_edge_grid(True) once the obstacles are
               installed -- the obstacle edges in range and the wall test come from a static grid over the edges instead of a scan
               of the arena's whole table (edge_grid_info()); the same results.  False (default): the scan.
    tiled_params: True (with tiled=True or "grid" only; ValueError otherwise): the tiled handle is made with CA_CREATE_TILED_PARAMS
               and takes agent_params= / set_agent_params() -- a heterogeneous crowd of up to 16384 agents in one world.  Until
               parameters are set it runs the uniform tiled kernels.  agent_counts stays refused.  False (default): a tiled
               handle refuses per-agent parameters.
    tiled_wide: True (with tiled=True or "grid" only, never with tiled_params=True; ValueError otherwise): the tiled handle is made
               with CA_CREATE_TILED_WIDE and takes max_obst_neighbors up to 64 -- a large crowd in a polyline world (a pillar hall)
               without truncated obstacle lists.  With max_obst_neighbors <= 16 it is the handle of tiled= alone; above, the solve
               launch builds the sorted list in the tile's LDS line table, the tile is 64 agents (tiled_info()), and the results
               are the ordinary wide handle's and the oracle's bit for bit.  False (default): a tiled handle refuses
               max_obst_neighbors > 16.
    """

    def __init__(self, n_arenas, n_agents, scenario="crowd", params=None, device=0, seed=0,
                 arena_offset=0, max_obst_neighbors=None, use_torch=None, obstacles="scenario", allow_obst_overflow=False,
                 agent_params=None, agent_counts=None, tiled=False, edge_grid=False, tiled_params=False, tiled_wide=False,
                 agent_sensing=None, reward_terms=None):
        if tiled not in (False, True, "grid", None, 0, 1):
            raise ValueError("tiled=%r: False, True or 'grid'" % (tiled,))
        if tiled_params and not tiled:
            raise ValueError("tiled_params=True without tiled=True or tiled='grid': it selects the tiled path's per-agent-parameter "
                             "kernels (an ordinary handle takes agent_params= as it is)")
        if tiled_wide and not tiled:
            raise ValueError("tiled_wide=True without tiled=True or tiled='grid': it selects the tiled path's wide-obstacle-list "
                             "kernels (an ordinary handle takes max_obst_neighbors up to 64 as it is)")
        if tiled_wide and tiled_params:
            raise ValueError("tiled_wide=True together with tiled_params=True: per-agent parameters go with obstacle lists of up to "
                             "16, as on ordinary handles")
        if agent_sensing is not None and (not isinstance(agent_sensing, dict) or set(agent_sensing) - {"neighbor_dist", "max_neighbors"}):
            raise ValueError("agent_sensing=%r: a dict with the keys neighbor_dist and / or max_neighbors" % (agent_sensing,))
        if tiled and agent_sensing and not tiled_params:
            raise ValueError("tiled=%r: the tiled kernels' per-agent form is chosen at construction (agent_sensing= goes with "
                             "tiled_params=True or with tiled=False)" % (tiled,))
        if tiled and ((agent_params and not tiled_params) or agent_counts is not None):
            raise ValueError("tiled=%r: the tiled kernels have no per-arena-count form, and their per-agent-parameter form is chosen "
                             "at construction (agent_params= goes with tiled_params=True or with tiled=False, agent_counts= with "
                             "tiled=False)" % (tiled,))
        self.tiled = "grid" if tiled == "grid" else bool(tiled)
        self.tiled_params = bool(tiled_params)
        self.tiled_wide = bool(tiled_wide)
        if agent_counts is not None and scenario not in (None, "doorway"):
            raise ValueError("agent_counts: scenario %r lays its agents out as a function of n_agents; only 'doorway' or None "
                             "go with per-arena agent counts" % (scenario,))
        self.L = _lib.load()
        self.A, self.N = int(n_arenas), int(n_agents)
        p = scenarios.env_params()
        if params:
            p.update(params)
        worlds = None   # a world per arena (list of polygon lists) or None: the same polygons for every arena
        if obstacles == "scenario":
            worlds = scenarios.obstacle_worlds(scenario, self.A, n_agents, p["radius"], seed, arena_offset) \
                if scenario is not None else None
            polys = scenarios.obstacles(scenario, n_agents, p["radius"]) if scenario is not None and worlds is None else []
        elif isinstance(obstacles, dict) and "per_arena" in obstacles:
            worlds, polys = list(obstacles["per_arena"]), []
        else:
            polys = list(obstacles or [])
        n_edges = max(sum(len(q) for q in w) for w in worlds) if worlds else sum(len(q) for q in polys)
        if max_obst_neighbors is None:
            max_obst_neighbors = max(1, min(DEFAULT_MAX_OBST_NEIGHBORS, n_edges))
        self.cfg = _lib.Config(n_arenas=self.A, n_agents=self.N, arena_offset=arena_offset, seed=seed,
                               max_obst_neighbors=max_obst_neighbors, **p)
        self.K, self.S = self.cfg.max_neighbors, self.cfg.max_obst_neighbors
        self.device = int(device)
        self.use_torch = (torch is not None and torch.cuda.is_available()) if use_torch is None else bool(use_torch)
        h = C.c_void_p()
        if self.tiled:
            flags = _lib.CREATE_TILED | (_lib.CREATE_TILED_GRID if self.tiled == "grid" else 0) | \
                (_lib.CREATE_TILED_PARAMS if self.tiled_params else 0) | (_lib.CREATE_TILED_WIDE if self.tiled_wide else 0)
            rc = self.L.ca_create_ex(C.byref(self.cfg), flags, self.device, None, C.byref(h))
        else:
            rc = self.L.ca_create(C.byref(self.cfg), self.device, None, C.byref(h))
        _lib.check(self.L, None, rc, "ca_create_ex" if self.tiled else "ca_create")
        self.h = h
        if allow_obst_overflow:
            self._call("ca_allow_obstacle_overflow", self.h, 1)
        if self.use_torch:
            # run on PyTorch's current stream (its handle is 0 for the default stream), so that
            # tensor ops and torch.cuda.Event order naturally with the environment's kernels
            torch.cuda.set_device(self.device)
            self._call("ca_set_stream", self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        self._obs_t = None
        self.n_actions = 0
        if self.use_torch:
            dev = torch.device("cuda", self.device)
            self._obs_t = torch.zeros((self.A, self.N, _lib.OBS_DIM), dtype=torch.float32, device=dev)
            self._call("ca_bind_obs", self.h, C.c_void_p(self._obs_t.data_ptr()), self._obs_t.numel() * 4)
            self._rew_t = self.field_tensor(_lib.FLD_REWARD)        # views of the library's own buffers: no copies
            self._done_t = self.field_tensor(_lib.FLD_ARENA_DONE)
            self._act_t = torch.zeros((self.A, self.N), dtype=torch.float32, device=dev)
        if worlds is not None:
            self.set_obstacles_per_arena(worlds)
        else:
            self.set_obstacles(polys)
        if edge_grid:
            self.set_edge_grid(True)
        if agent_counts is not None:
            self.set_agent_counts(agent_counts)
        if scenario is not None:
            self.init_scenario(scenario)
        if agent_params:
            self.set_agent_params(**agent_params)
        if agent_sensing:
            self.set_agent_sensing(**agent_sensing)
        if reward_terms:
            self.set_reward_terms(**reward_terms)

    # ---- plumbing -------------------------------------------------------------------------------
    def _call(self, name, *args):
        rc = getattr(self.L, name)(*args)
        _lib.check(self.L, self.h, rc, name)

    def close(self):
        self.__dict__.pop("_host_bufs", None); self.__dict__.pop("_packed", None); self.__dict__.pop("_packed_act", None)
        for arr in self.__dict__.pop("_host_arrays", []):     # their memory goes with the handle (see host_array)
            try:
                arr.flags.writeable = False
            except Exception:
                pass
        for snap in self.__dict__.pop("_snapshots", []):     # ca_destroy frees them
            snap._h = None
        if getattr(self, "h", None):
            self.L.ca_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape_dtype(self, field):
        if field == _lib.FLD_ARENA_STATS:
            return (self.A, 8), np.uint64
        dt = np.int32 if field in _I32_FIELDS else (np.float64 if field in _F64_FIELDS else np.float32)
        if field in _ARENA_FIELDS:
            return (self.A,), dt
        if field == _lib.FLD_NB_IDX:
            return (self.A, max(self.K, 1), self.N), dt
        if field == _lib.FLD_OBST_IDX:
            return (self.A, self.S, self.N), dt
        if field == _lib.FLD_OBS:
            return (self.A, self.N, _lib.OBS_DIM), dt
        if field in (_lib.FLD_ALAN_WEIGHTS, _lib.FLD_ALAN_TIMES):
            return (self.A, self.n_actions, self.N), dt      # device layout; get()/set() present [A, N, n_actions]
        return (self.A, self.N), dt

    def get(self, field, out=None):
        """Host copy of a state field (synchronises the stream).  out: a C-contiguous array of the field's device shape and
        dtype to fill instead of a new one (e.g. host_buffer(field): page-locked, so the copy runs at the link's rate)."""
        shape, dt = self._shape_dtype(field)
        if out is not None and field in (_lib.FLD_ALAN_WEIGHTS, _lib.FLD_ALAN_TIMES):
            raise ValueError("get: out= is not supported for the ALAN weights / times (they are returned transposed, [A, N, n_actions])")
        if out is None:
            out = np.empty(shape, dt)
        elif out.shape != tuple(shape) or out.dtype != np.dtype(dt) or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("get: out must be a C-contiguous %s array of shape %s" % (np.dtype(dt).name, tuple(shape)))
        self._call("ca_get", self.h, field, _ptr(out), out.nbytes, 0)
        if field in (_lib.FLD_ALAN_WEIGHTS, _lib.FLD_ALAN_TIMES):
            return np.ascontiguousarray(np.transpose(out, (0, 2, 1)))   # [A, N, n_actions] like ALAN_true.py:75-76
        return out

    def host_array(self, shape, dtype):
        """A numpy array over page-locked, device-visible host memory from the library (ca_host_alloc: no PyTorch involved).
        LIFETIME: the memory belongs to the handle and is released by close() (ca_destroy); the array -- and every view of it,
        which is what host_buffer(), step(copy=False) and step_packed() hand out -- must not be touched after close().
        Copy what has to outlive the environment (np.array(view)); close() marks the arrays it still knows read-only
        as a tripwire for late writers."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = C.c_void_p()
        self._call("ca_host_alloc", self.h, max(n, 1), C.byref(ptr))
        buf = (C.c_char * max(n, 1)).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self.__dict__.setdefault("_host_arrays", []).append(arr)
        return arr

    def host_buffer(self, field):
        """A persistent page-locked host array for a field (a pageable destination takes the 67-MB observation of 4096 x 64
        agents at ~10 GB/s, a pinned one at the PCIe rate).  Owned by the environment and reused by step(copy=False): valid until
        the next call that writes it -- the reference's own ownership rule (env.py:463-466: the same dict objects every call,
        mutated in place)."""
        bufs = self.__dict__.setdefault("_host_bufs", {})
        if field not in bufs:
            shape, dt = self._shape_dtype(field)
            bufs[field] = self.host_array(shape, dt)
        return bufs[field]

    def step_packed(self, actions=None, with_obs=True, stats=False, autoreset=False, no_done=False, contacts=False):
        """One host-side step in one round trip (ca_step_packed): actions [A,N] (None: the ORCA-only step) in, (obs, rewards, dones,
        step_counts) out as views of ONE page-locked buffer owned by the environment, valid until the next call and never after
        close() (host_array: the buffer is freed with the handle).  The form for one
        environment per worker with results on the host every step (run_rllib.py:77, 108).  contacts=True: also leave the contact
        report of the state the step leaves (last_contacts()); the four views and their layout do not change."""
        an, A = self.A * self.N, self.A
        if "_packed" not in self.__dict__:
            words = an * _lib.OBS_DIM + an + 2 * A
            raw = self.host_array((words,), np.float32)
            self._packed = (raw, raw[:an * _lib.OBS_DIM].reshape(A, self.N, _lib.OBS_DIM), raw[an * _lib.OBS_DIM:an * _lib.OBS_DIM + an].reshape(A, self.N),
                            raw[an * _lib.OBS_DIM + an:an * _lib.OBS_DIM + an + A].view(np.int32), raw[an * _lib.OBS_DIM + an + A:].view(np.int32))
            self._packed_act = self.host_array((A, self.N), np.float32)
        raw, obs, rew, done, steps = self._packed
        flags = (_lib.F_OBS if with_obs else 0) | (_lib.F_STATS if stats else 0) | (_lib.F_AUTORESET if autoreset else 0) | \
                (_lib.F_NODONE if no_done else 0) | (_lib.F_CONTACT if contacts else 0)
        act_ptr = None
        if actions is not None:
            if torch is not None and isinstance(actions, torch.Tensor):
                actions = actions.detach().cpu().numpy()
            self._packed_act[...] = np.asarray(actions, np.float32).reshape(A, self.N)
            act_ptr = self._packed_act.ctypes.data
        self._call("ca_step_packed", self.h, act_ptr, flags, raw.ctypes.data, raw.nbytes)
        return obs, rew, done, steps

    def set(self, field, arr):
        shape, dt = self._shape_dtype(field)
        if field in (_lib.FLD_ALAN_WEIGHTS, _lib.FLD_ALAN_TIMES):
            arr = np.transpose(np.asarray(arr, dt).reshape(self.A, self.N, self.n_actions), (0, 2, 1))
        a = np.ascontiguousarray(np.asarray(arr, dt).reshape(shape))
        self._call("ca_set", self.h, field, _ptr(a), a.nbytes, 0)

    # ---- checkpoint / resume -------------------------------------------------------------------------
    _STATE_FIELDS = ("POS_X", "POS_Y", "VEL_X", "VEL_Y", "PREF_X", "PREF_Y", "GOAL_X", "GOAL_Y", "GOAL2_X", "GOAL2_Y",
                     "AGENT_DONE", "ARRIVE_STEP", "NB_COUNT", "NB_IDX", "OBST_COUNT", "OBST_IDX", "STEP_COUNT", "ARENA_DONE",
                     "EPISODE", "REGOAL_COUNT", "REWARD")

    def get_state(self):
        """Everything the next step depends on, as a dict of host arrays: simulator state, targets, the neighbour lists of
        the last doStep (the observation of a reset reads them, env.py:461-488), the counters that key the random draws
        (episode, re-goal count, step count), the last rewards (an arena frozen by CA_F_FREEZE keeps them) and, after alan_configure,
        the bandit's weights, times and last actions.  This is the HOST checkpoint (portable, a dict of numpy arrays);
        fork() / snapshot() / restore() move the same fields between arenas or into a second set of buffers on the device,
        without the round trip.  The reference never
        serialises its environment (checkpoints exist at the trainer's level only); with counter-based
        draws a restored environment continues bit for bit.  Statistics counters are not part of the state."""
        st = {name: self.get(getattr(_lib, "FLD_" + name)) for name in self._STATE_FIELDS}
        if self.n_actions > 0:
            st["ALAN_WEIGHTS"] = self.get(_lib.FLD_ALAN_WEIGHTS)
            st["ALAN_TIMES"] = self.get(_lib.FLD_ALAN_TIMES)
            st["ALAN_ACTION"] = self.get(_lib.FLD_ALAN_ACTION)
        st["_shape"] = np.array([self.A, self.N, self.K, self.S, self.n_actions], np.int64)
        return st

    def set_state(self, st):
        """Restore a get_state() dict into an environment of the same shape and configuration (seed included: it keys the
        draws); the obstacle tables and the ALAN action set are configuration, not state.  The device counterpart, between
        arenas of one environment: fork() / snapshot() / restore()."""
        shape = [int(v) for v in np.asarray(st["_shape"]).reshape(-1)]
        if shape != [self.A, self.N, self.K, self.S, self.n_actions]:
            raise ValueError("set_state: the state is of an environment of shape %s, this one is %s"
                             % (shape, [self.A, self.N, self.K, self.S, self.n_actions]))
        optional = ("REWARD", "ALAN_ACTION")   # joined in round 5: older snapshots restore without them; anything else
        need = [n for n in self._STATE_FIELDS if n not in optional] + (["ALAN_WEIGHTS", "ALAN_TIMES"] if self.n_actions > 0 else [])
        missing = [n for n in need if n not in st]
        if missing:                            # missing is a truncated / corrupt snapshot: nothing is restored
            raise KeyError("set_state: the snapshot lacks %s" % ", ".join(missing))
        for name in self._STATE_FIELDS:
            if name in st:
                self.set(getattr(_lib, "FLD_" + name), st[name])
        if self.n_actions > 0:
            self.set(_lib.FLD_ALAN_WEIGHTS, st["ALAN_WEIGHTS"])
            self.set(_lib.FLD_ALAN_TIMES, st["ALAN_TIMES"])
            if "ALAN_ACTION" in st:
                self.set(_lib.FLD_ALAN_ACTION, st["ALAN_ACTION"])

    # ---- fork / rewind on the device (ca_arena_gather, ca_snapshot_*) --------------------------------
    def _fork_src(self, src, allow_keep):
        """(pointer, is_device, keep-alive) of an index array: a device integer tensor goes by pointer, as int32 on this GPU (the
        library copies it back for its checks), everything else through fork_index on the host."""
        if torch is not None and isinstance(src, torch.Tensor) and src.is_cuda:
            if src.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or tuple(src.shape) != (self.A,):
                raise ValueError("fork: a device src must be an integer tensor of shape [A] (A=%d), got %s %s"
                                 % (self.A, src.dtype, tuple(src.shape)))
            if src.dtype == torch.int64:      # (narrowed on the device: out of range stays out of range for the library's check)
                src = src.clamp(-2 ** 31, 2 ** 31 - 1)
            t, _ = self._on_device(src, torch.int32)
            return C.c_void_p(t.data_ptr()), 1, t
        a = fork_index(src, self.A, allow_keep)
        return _ptr(a), 0, a

    def fork(self, src, obs=False, contacts=False):
        """Arena a becomes a copy of arena src[a] as it was before the call, on the device (ca_arena_gather): src is a list, an
        array or a torch int tensor of A entries in 0 .. A-1 (a device tensor is passed by pointer); src[a] == a leaves
        arena a alone.  What moves is exactly what get_state() lists (get_state / set_state remain the host checkpoint);
        obstacles, per-agent parameters, counts and sensing, ALAN action sets, statistics and the random streams' identity stay with
        the slot, so copies of one arena share a past and draw futures of their own.  With a world per arena the written arenas'
        obstacle lists are emptied, with per-agent sensing their agent lists (the next step rebuilds them).  obs=True: returns the
        observation of the new state as observe() does; contacts=True: also leaves the contact report (last_contacts())."""
        ptr, on_dev, keep = self._fork_src(src, False)
        flags = (_lib.F_OBS if obs else 0) | (_lib.F_CONTACT if contacts else 0)
        self._call("ca_arena_gather", self.h, ptr, self.A * 4, on_dev, flags)
        return self._obs_out() if obs else None

    def snapshot(self, into=None):
        """Save the state of every arena into a Snapshot on the device (ca_snapshot_save: one launch, asynchronous) and return it.
        into: a Snapshot of this environment to overwrite instead of making a new one."""
        if into is None:
            h = C.c_void_p()
            self._call("ca_snapshot_create", self.h, C.byref(h))
            into = Snapshot(self, h)
            self.__dict__.setdefault("_snapshots", []).append(into)
        elif not isinstance(into, Snapshot) or into._env is not self or into.closed:
            raise ValueError("snapshot: into= must be an open Snapshot of this environment")
        self._call("ca_snapshot_save", self.h, into._h)
        return into

    def restore(self, snap, src=None, obs=False, contacts=False):
        """Arena a becomes arena src[a] of the snapshot (ca_snapshot_load); an entry of -1 keeps arena a as it is; src=None: every
        arena returns to its own saved state.  The rules, obs= and contacts= are fork()'s.  The host counterpart is set_state()."""
        if not isinstance(snap, Snapshot) or snap.closed:
            raise ValueError("restore: snap must be an open Snapshot (closed by its close() or by the environment's)")
        flags = (_lib.F_OBS if obs else 0) | (_lib.F_CONTACT if contacts else 0)
        if src is None:
            self._call("ca_snapshot_load", self.h, snap._h, None, 0, 0, flags)
        else:
            ptr, on_dev, keep = self._fork_src(src, True)
            self._call("ca_snapshot_load", self.h, snap._h, ptr, self.A * 4, on_dev, flags)
        return self._obs_out() if obs else None

    def fork_bytes_per_arena(self):
        """Bytes of one arena in the planes that fork() / snapshot() / restore() move (ca_fork_bytes_per_arena)."""
        n = C.c_size_t()
        self._call("ca_fork_bytes_per_arena", self.h, C.byref(n))
        return int(n.value)

    def field_tensor(self, field):
        """Zero-copy torch view of a state field's device buffer (valid until close(); kernels of this handle run on
        torch's current stream, so ordinary stream ordering applies)."""
        if torch is None:
            raise RuntimeError("field_tensor needs PyTorch")
        shape, dt = self._shape_dtype(field)
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._call("ca_field_ptr", self.h, field, C.byref(ptr), C.byref(nbytes))

        class _View(object):   # the CUDA array interface, which torch.as_tensor understands
            pass
        v = _View()
        v.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(dt).str, "data": (int(ptr.value), False),
                                      "version": 2, "strides": None}
        t = torch.as_tensor(v, device=torch.device("cuda", self.device))
        assert t.numel() * t.element_size() == nbytes.value
        return t

    def neighbor_lists(self):
        """(count [A,N], idx [A,N,K]) of the ORCA agent neighbours of the last step, nearest first."""
        return self.get(_lib.FLD_NB_COUNT), np.transpose(self.get(_lib.FLD_NB_IDX), (0, 2, 1))[:, :, :self.K]

    def obstacle_neighbor_lists(self):
        return self.get(_lib.FLD_OBST_COUNT), np.transpose(self.get(_lib.FLD_OBST_IDX), (0, 2, 1))

    def set_obstacles(self, polys):
        polys = [np.asarray(q, np.float32).reshape(-1, 2) for q in polys]
        verts = np.ascontiguousarray(np.concatenate(polys) if polys else np.zeros((0, 2), np.float32))
        sizes = np.asarray([len(q) for q in polys], np.int32)
        self._call("ca_set_obstacles", self.h, _ptr(verts), _ptr(sizes), len(polys))

    def set_obstacles_per_arena(self, worlds):
        """A world of its own for every arena (the reference builds one simulator per environment and draws e.g. the
        blocks of ALAN_true.py:359-372 anew for each): worlds[a] = list of polygons of arena a."""
        if len(worlds) != self.A:
            raise ValueError("set_obstacles_per_arena: %d worlds for %d arenas" % (len(worlds), self.A))
        polys = [np.asarray(q, np.float32).reshape(-1, 2) for w in worlds for q in w]
        verts = np.ascontiguousarray(np.concatenate(polys) if polys else np.zeros((0, 2), np.float32))
        sizes = np.asarray([len(q) for q in polys], np.int32)
        counts = np.asarray([len(w) for w in worlds], np.int32)
        self._call("ca_set_obstacles_per_arena", self.h, _ptr(verts), _ptr(sizes), _ptr(counts))

    def obstacle_table(self, arena=0):
        """The processed vertex table of an arena (after the edge cuts of processObstacles): dict(verts [n,2],
        next [n], convex [n]); edge i = verts[i] -> verts[next[i]], the ids of obstacle_neighbor_lists()."""
        n = C.c_int32()
        self._call("ca_get_obstacles_arena", self.h, int(arena), None, None, None, 0, C.byref(n))
        verts, nxt, cvx = np.zeros((n.value, 2), np.float32), np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        self._call("ca_get_obstacles_arena", self.h, int(arena), _ptr(verts), _ptr(nxt), _ptr(cvx), n.value, C.byref(n))
        return dict(verts=verts, next=nxt, convex=cvx)

    def init_scenario(self, scenario):
        sid = scenarios.SCENARIO_IDS[scenario] if isinstance(scenario, str) else int(scenario)
        self._call("ca_init_scenario", self.h, sid)

    def sync(self):
        self._call("ca_sync", self.h)

    def stats(self):
        s = _lib.Stats()
        self._call("ca_get_stats", self.h, C.byref(s))
        return s.as_dict()

    def reset_stats(self):
        self._call("ca_reset_stats", self.h)

    def profile(self, period=1):
        """Time the kernel launches of every `period`-th step (start / stop events on the dispatch itself; 0 = off)."""
        self._call("ca_profile", self.h, int(period))

    def profile_read(self):
        """{kernel: (launches, mean ms)} since the last read; synchronises."""
        n = (C.c_int32 * 4)()
        ms = (C.c_float * 4)()
        self._call("ca_profile_read", self.h, n, ms)
        return {k: (n[i], ms[i]) for i, k in enumerate(("nbr_kernel", "step_kernel", "obs_kernel", "reset_kernels"))}

    def launch_info(self):
        v = [C.c_int32() for _ in range(4)]
        self._call("ca_launch_info", self.h, *[C.byref(x) for x in v])
        lanes, roll = C.c_int32(), C.c_int32()
        self._call("ca_solver_info", self.h, C.byref(lanes), C.byref(roll))
        per, cnt, sen = C.c_int32(), C.c_int32(), C.c_int32()
        self._call("ca_agent_params_info", self.h, C.byref(per))
        self._call("ca_agent_counts_info", self.h, C.byref(cnt))
        self._call("ca_agent_sensing_info", self.h, C.byref(sen))
        return dict(block=v[0].value, grid=v[1].value, lds_bytes=v[2].value, obs_grid=v[3].value,
                    lanes_per_agent=lanes.value, rollout_one_launch=roll.value, agent_params=bool(per.value),
                    agent_counts=bool(cnt.value), agent_sensing=bool(sen.value))

    def nbr_seed_info(self):
        """True if a plain step of this handle launches a SeededScan solve kernel: the agent-neighbour scan of arenas of at most 64
        agents seeded with last step's lists (ca_nbr_seed_info; CA_NBR_SEED=0 in the environment at construction switches it off)."""
        v = C.c_int32()
        self._call("ca_nbr_seed_info", self.h, C.byref(v))
        return bool(v.value)

    def lp3_pairs_info(self):
        """True if a plain step of this handle launches a PairedLp3 solve kernel: a wave with 17 to 32 infeasible agents solves
        them in one LP3 round, two lanes per agent (ca_lp3_pairs_info; CA_LP3_PAIRS=0 / 1 in the environment at construction
        selects the kernel without / with the tag)."""
        v = C.c_int32()
        self._call("ca_lp3_pairs_info", self.h, C.byref(v))
        return bool(v.value)

    def tiled_info(self):
        """dict(tiled, tile_agents, tiles_per_arena, launches_per_step) of the tiled solve path (ca_tiled_info); zeros on an
        ordinary handle."""
        v = [C.c_int32() for _ in range(4)]
        self._call("ca_tiled_info", self.h, *[C.byref(x) for x in v])
        return dict(tiled=bool(v[0].value), tile_agents=v[1].value, tiles_per_arena=v[2].value, launches_per_step=v[3].value)

    def tiled_grid_info(self):
        """dict(grid, cells_x, cells_y, cell_size, sort_launches) of the uniform grid of a tiled="grid" handle (ca_tiled_grid_info):
        the wrapped cell table's sides, the width of a cell, the launches in front of the solve launch; zeros on every other handle."""
        v = [C.c_int32() for _ in range(3)] + [C.c_float(), C.c_int32()]
        self._call("ca_tiled_grid_info", self.h, *[C.byref(x) for x in v])
        return dict(grid=bool(v[0].value), cells_x=v[1].value, cells_y=v[2].value, cell_size=v[3].value, sort_launches=v[4].value)

    def set_edge_grid(self, on=True):
        """The static edge grid of a tiled="grid" handle on or off (ca_tiled_edge_grid): a uniform grid over the obstacle edges of each
        installed table, built once on the host and rebuilt by set_obstacles() / set_obstacles_per_arena() while on.  Configuration
        like the obstacles: it survives reset() and init_scenario() and is no part of get_state().  Results do not change.  Raises
        on any other handle, and for a world of more than 65535 edges or of walls so long that the table passes its cap (subdivide
        them); the handle then keeps scanning."""
        self._call("ca_tiled_edge_grid", self.h, 1 if on else 0)

    def edge_grid_info(self, arena=0):
        """dict(on, cells_x, cells_y, cell_size_x, cell_size_y, entries) of the static edge grid of `arena` (ca_tiled_edge_grid_info);
        zeros while off and on every other handle."""
        v = [C.c_int32() for _ in range(3)] + [C.c_float(), C.c_float(), C.c_int32()]
        self._call("ca_tiled_edge_grid_info", self.h, int(arena), *[C.byref(x) for x in v])
        return dict(on=v[0].value, cells_x=v[1].value, cells_y=v[2].value, cell_size_x=v[3].value, cell_size_y=v[4].value,
                    entries=v[5].value)

    # ---- per-agent ORCA parameters (sim.addAgent's per-agent arguments, env.py:126-133) ---------------
    _AGENT_PARAMS = ("radius", "max_speed", "time_horizon", "time_horizon_obst")

    def set_agent_params(self, radius=None, max_speed=None, time_horizon=None, time_horizon_obst=None):
        """radius, max_speed, time_horizon and time_horizon_obst per agent (ca_set_agent_params): each a numpy array or torch
        tensor of shape [A,N] -- a scalar or an [A] array (one value per arena) is broadcast --, or None: every agent keeps the
        value of `params`.  Configuration like the obstacles: it survives reset() and init_scenario() and is not part of
        get_state().  The handle then runs the per-agent kernels (launch_info()["agent_params"]); all four None returns it to
        uniform parameters, like clear_agent_params().  neighbor_dist and max_neighbors per agent: set_agent_sensing()."""
        keep, ptrs = [], []
        for name, v in zip(self._AGENT_PARAMS, (radius, max_speed, time_horizon, time_horizon_obst)):
            if v is None:
                ptrs.append(None)
                continue
            if torch is not None and isinstance(v, torch.Tensor):   # a configuration call: the library checks every value on the host anyway
                v = v.detach().cpu().numpy()
            a = np.asarray(v, np.float32)
            if a.ndim == 1 and a.shape[0] == self.A:   # one value per arena (also where A == N)
                a = a[:, None]
            try:
                full = np.ascontiguousarray(np.broadcast_to(a, (self.A, self.N)), np.float32)
            except ValueError:
                raise ValueError("set_agent_params: %s must be a scalar, an [A] array or an [A,N] array (A=%d, N=%d), got shape %s"
                                 % (name, self.A, self.N, a.shape))
            keep.append(full)
            ptrs.append(_ptr(full))
        self._call("ca_set_agent_params", self.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], self.A * self.N * 4, 0)

    def clear_agent_params(self):
        """Back to the uniform parameters of `params` and to the kernels the handle used with them."""
        self._call("ca_set_agent_params", self.h, None, None, None, None, 0, 0)

    def agent_params(self):
        """dict(radius, max_speed, time_horizon, time_horizon_obst) of [A,N] float32 arrays: what the kernels use (the value of
        `params` everywhere on a handle with uniform parameters)."""
        out = {k: np.empty((self.A, self.N), np.float32) for k in self._AGENT_PARAMS}
        self._call("ca_get_agent_params", self.h, *[_ptr(out[k]) for k in self._AGENT_PARAMS], self.A * self.N * 4, 0)
        return out

    # ---- per-agent sensing (sim.addAgent's neighborDist and maxNeighbors, env.py:126-133) ---------------
    def _broadcast_an(self, who, name, v, dtype):
        """v as a contiguous [A,N] array of dtype: a scalar, an [A] array (one value per arena) or an [A,N] array."""
        if torch is not None and isinstance(v, torch.Tensor):   # a configuration call: the library checks every value on the host anyway
            v = v.detach().cpu().numpy()
        a = np.asarray(v)
        if dtype == np.int32:
            if a.dtype.kind not in "iu":
                if a.dtype.kind != "f" or not np.all(np.isfinite(a)) or np.any(a != np.floor(a)):
                    raise ValueError("%s: %s must hold whole numbers, got dtype %s" % (who, name, a.dtype))
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError("%s: %s does not fit 32 bits" % (who, name))
        a = a.astype(dtype)
        if a.ndim == 1 and a.shape[0] == self.A:   # one value per arena (also where A == N)
            a = a[:, None]
        try:
            return np.ascontiguousarray(np.broadcast_to(a, (self.A, self.N)), dtype)
        except ValueError:
            raise ValueError("%s: %s must be a scalar, an [A] array or an [A,N] array (A=%d, N=%d), got shape %s"
                             % (who, name, self.A, self.N, a.shape))

    def set_agent_sensing(self, neighbor_dist=None, max_neighbors=None):
        """neighbor_dist (float) and max_neighbors (int) per agent (ca_set_agent_sensing): each a numpy array or torch tensor of
        shape [A,N] -- a scalar or an [A] array (one value per arena) is broadcast --, or None: every agent keeps the value of
        `params`.  The values of `params` are capacities: neighbor_dist_i in [1e-3, params neighbor_dist], max_neighbors_i in
        [0, params max_neighbors]; the library raises otherwise.  Agent i's list is its max_neighbors_i nearest within
        neighbor_dist_i; the observation's laser range stays the handle's.  Configuration like the obstacles: it survives reset()
        and init_scenario() and is not part of get_state().  The handle then runs the per-agent kernels
        (launch_info()["agent_sensing"]); both None returns it to what it ran before, like clear_agent_sensing()."""
        nd = None if neighbor_dist is None else self._broadcast_an("set_agent_sensing", "neighbor_dist", neighbor_dist, np.float32)
        mk = None if max_neighbors is None else self._broadcast_an("set_agent_sensing", "max_neighbors", max_neighbors, np.int32)
        self._call("ca_set_agent_sensing", self.h, None if nd is None else _ptr(nd), None if mk is None else _ptr(mk),
                   self.A * self.N * 4, 0)

    def clear_agent_sensing(self):
        """Back to the handle's neighbor_dist and max_neighbors for every agent and to the kernels it used with them."""
        self._call("ca_set_agent_sensing", self.h, None, None, 0, 0)

    def agent_sensing(self):
        """dict(neighbor_dist [A,N] float32, max_neighbors [A,N] int32): what the kernels use (the values of `params` everywhere
        on a handle without per-agent sensing)."""
        out = dict(neighbor_dist=np.empty((self.A, self.N), np.float32), max_neighbors=np.empty((self.A, self.N), np.int32))
        self._call("ca_get_agent_sensing", self.h, _ptr(out["neighbor_dist"]), _ptr(out["max_neighbors"]), self.A * self.N * 4, 0)
        return out

    # ---- agents per arena (the reference's constructor argument numAgents, env.py:23-60, per arena) ---
    def set_agent_counts(self, counts):
        """Arena a holds counts[a] agents, rows 0 .. counts[a]-1 of its N (ca_set_agent_counts): an [A] int array or torch
        tensor, every entry in [1, N].  Shapes stay [A,N,...]; absent rows show a zero observation and reward and are left alone
        otherwise (agent_mask()).  Configuration like the obstacles: it survives reset() and init_scenario("doorway") and is
        not part of get_state().  Clears the neighbour lists of every arena.  The handle then runs the per-arena-count kernels
        (launch_info()["agent_counts"]); the other scenario generators and the ALAN calls raise while counts are set."""
        if torch is not None and isinstance(counts, torch.Tensor):   # a configuration call: the library checks every value on the host
            counts = counts.detach().cpu().numpy()
        c = np.asarray(counts)
        if c.shape != (self.A,) or c.dtype.kind not in "iu":
            raise ValueError("set_agent_counts: counts must be an [A] integer array (A=%d), got shape %s, dtype %s" % (self.A, c.shape, c.dtype))
        c = np.ascontiguousarray(np.clip(c, -2 ** 31, 2 ** 31 - 1), np.int32)   # (out of range stays out of range for the library's check)
        self._call("ca_set_agent_counts", self.h, _ptr(c), c.nbytes, 0)

    def clear_agent_counts(self):
        """Every arena holds N agents again; back to the kernels the handle used before."""
        self._call("ca_set_agent_counts", self.h, None, 0, 0)

    def agent_counts(self):
        """int32 [A]: the agents of every arena (N everywhere on a handle without counts)."""
        out = np.empty(self.A, np.int32)
        self._call("ca_get_agent_counts", self.h, _ptr(out), out.nbytes, 0)
        return out

    def agent_mask(self):
        """bool [A,N]: True for the rows that are agents of their arena."""
        return np.arange(self.N)[None, :] < self.agent_counts()[:, None]

    # ---- the environment API ----------------------------------------------------------------------
    def _on_device(self, t, dtype):
        """A torch tensor as (contiguous tensor on this handle's GPU, True) or, for a CPU tensor, as
        (numpy array, False): the library dereferences a device pointer as device memory, so a CPU tensor
        must take the host path and a tensor of another GPU is moved here first."""
        if not t.is_cuda:
            return t.detach().to(dtype=dtype).contiguous().numpy(), False
        dev = torch.device("cuda", self.device)
        t = t.detach().to(device=dev, dtype=dtype).contiguous()
        if not self.use_torch:   # the handle runs on a stream of its own: torch's producer must be finished
            torch.cuda.current_stream(self.device).synchronize()
        return t, True

    def _obs_out(self):
        return self._obs_t if self.use_torch else self.get(_lib.FLD_OBS)

    def reset(self, pos_x=None, pos_y=None, with_obs=True, contacts=False):
        """reference reset() (env.py:461-488) for every arena.  pos_x/pos_y [A,N]: explicit new
        positions (numpy or device tensor); default: drawn from the spawn box.  contacts=True: also leave the contact report of
        the new state (last_contacts())."""
        flags = (_lib.F_OBS if with_obs else 0) | (_lib.F_CONTACT if contacts else 0)
        if pos_x is None:
            self._call("ca_reset", self.h, None, None, 0, flags)
        elif torch is not None and isinstance(pos_x, torch.Tensor) and pos_x.is_cuda and \
                isinstance(pos_y, torch.Tensor) and pos_y.is_cuda:
            px, _ = self._on_device(pos_x, torch.float32)
            py, _ = self._on_device(pos_y, torch.float32)
            if px.numel() != self.A * self.N or py.numel() != self.A * self.N:
                raise ValueError("reset: pos_x / pos_y must hold %d x %d values" % (self.A, self.N))
            self._call("ca_reset", self.h, C.c_void_p(px.data_ptr()), C.c_void_p(py.data_ptr()), 1, flags)
            self.sync()
        else:
            if torch is not None and isinstance(pos_x, torch.Tensor):
                pos_x = pos_x.detach().cpu().numpy()
            if torch is not None and isinstance(pos_y, torch.Tensor):
                pos_y = pos_y.detach().cpu().numpy()
            px = np.ascontiguousarray(np.asarray(pos_x, np.float32).reshape(self.A, self.N))
            py = np.ascontiguousarray(np.asarray(pos_y, np.float32).reshape(self.A, self.N))
            self._call("ca_reset", self.h, _ptr(px), _ptr(py), 0, flags)
        return self._obs_out() if with_obs else None

    def reset_masked(self, mask, with_obs=True, contacts=False):
        """reset() for the arenas with mask[a] != 0 only (numpy or device int32 tensor [A]).  contacts: as for reset()."""
        flags = (_lib.F_OBS if with_obs else 0) | (_lib.F_CONTACT if contacts else 0)
        on_dev = False
        if torch is not None and isinstance(mask, torch.Tensor):
            mask, on_dev = self._on_device(mask, torch.int32)
        if on_dev:
            if mask.numel() != self.A:
                raise ValueError("reset_masked: mask must hold %d values" % self.A)
            self._call("ca_reset_masked", self.h, C.c_void_p(mask.data_ptr()), 1, flags)
            self.sync()
        else:
            m = np.ascontiguousarray(np.asarray(mask, np.int32).reshape(self.A))
            self._call("ca_reset_masked", self.h, _ptr(m), 0, flags)
        return self._obs_out() if with_obs else None

    def arena_stats(self):
        """Per-arena counters as a dict of [A] arrays (synchronises)."""
        r = self.get(_lib.FLD_ARENA_STATS)
        return dict(episodes=r[:, 0], collisions=r[:, 1], obst_collisions=r[:, 2], goals_reached=r[:, 3],
                    obst_overflow=r[:, 4], sum_reward=r[:, 5].copy().view(np.float64), frozen_steps=r[:, 6],
                    last_episode_steps=(r[:, 7] >> np.uint64(32)).astype(np.int64),
                    last_episode_arrived=(r[:, 7] & np.uint64(0xFFFFFFFF)).astype(np.int64))

    def step(self, actions, with_obs=True, stats=False, autoreset=False, copy=True, contacts=False):
        """reference step(action) (env.py:367-416) for every arena.
        actions [A,N] heading offsets (rad).  Returns (obs [A,N,64], rewards [A,N], dones [A], {}).
        contacts=True: the infos are {"contacts": <the report of the state this step leaves, as last_contacts() returns it>}
        instead of {} -- who touches whom, the nearest neighbour, the walls, per agent (CA_F_CONTACT: one small launch behind
        the step; with autoreset an arena that was reset reports its respawned state, like the observation).
        copy=False (numpy mode): the results land in the environment's own page-locked host buffers (host_buffer) and are
        valid until the next step / reset -- no allocation per step and the device -> host copy at the link's rate."""
        flags = (_lib.F_OBS if with_obs else 0) | (_lib.F_STATS if stats else 0) | \
                (_lib.F_AUTORESET if autoreset else 0) | (_lib.F_CONTACT if contacts else 0)
        if self.use_torch:
            if not isinstance(actions, torch.Tensor):
                actions = torch.as_tensor(np.asarray(actions, np.float32).reshape(self.A, self.N))
            if actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous() and \
                    actions.numel() == self.A * self.N and actions.device.index == self.device:
                src = actions                      # already where and what the kernel reads: no staging copy
            else:
                self._act_t.copy_(actions.reshape(self.A, self.N), non_blocking=True)
                src = self._act_t
            self._call("ca_step", self.h, C.c_void_p(src.data_ptr()), flags)
            return (self._obs_t if with_obs else None), self._rew_t, self._done_t, \
                ({"contacts": self.last_contacts()} if contacts else {})
        a = np.ascontiguousarray(np.asarray(actions, np.float32).reshape(self.A, self.N))
        self._call("ca_step_host", self.h, _ptr(a), flags)
        infos = {"contacts": self.last_contacts()} if contacts else {}
        if not copy:
            return (self.get(_lib.FLD_OBS, self.host_buffer(_lib.FLD_OBS)) if with_obs else None), \
                self.get(_lib.FLD_REWARD, self.host_buffer(_lib.FLD_REWARD)), \
                self.get(_lib.FLD_ARENA_DONE, self.host_buffer(_lib.FLD_ARENA_DONE)), infos
        return (self.get(_lib.FLD_OBS) if with_obs else None), self.get(_lib.FLD_REWARD), \
            self.get(_lib.FLD_ARENA_DONE), infos

    def orca_step(self, with_obs=False, stats=False, no_done=False, autoreset=False, freeze=False, contacts=False):
        """reference orca_step (env.py:447-458 with no_done=True; ALAN_true.py:631-636 + done test).
        freeze: arenas whose episode is over are no longer advanced.  contacts=True: also leave the contact report of the state
        the step leaves (last_contacts())."""
        flags = (_lib.F_OBS if with_obs else 0) | (_lib.F_STATS if stats else 0) | \
                (_lib.F_NODONE if no_done else 0) | (_lib.F_AUTORESET if autoreset else 0) | \
                (_lib.F_FREEZE if freeze else 0) | (_lib.F_CONTACT if contacts else 0)
        self._call("ca_orca_step", self.h, flags)
        return self._obs_out() if with_obs else None

    def observe(self):
        """reference _get_obs() (env.py:231-277) on the current state."""
        self._call("ca_observe", self.h)
        return self._obs_out()

    # ---- the per-agent contact report (ca_contacts / CA_F_CONTACT) ------------------------------------
    _CONTACT_PLANES = (("agents", np.int32), ("wall", np.int32), ("nearest", np.int32), ("nearest_d2", np.float32),
                       ("wall_d2", np.float32))

    def contacts(self):
        """The contact report of the current state (ca_contacts), a dict of five [A,N] arrays:
          agents      int32    other agents of the arena this agent overlaps: |p_i - p_j|^2 < (r_i + r_j)^2
          wall        int32    1 if the agent lies within its radius of an obstacle edge of its arena
          nearest     int32    index of the nearest other agent of the arena (ties: the smaller index), -1 in an arena of one
          nearest_d2  float32  the squared distance to it, inf when there is none
          wall_d2     float32  the squared distance to the nearest obstacle edge, inf in a world without obstacles
        Radii are the agents' own under set_agent_params(); absent rows (set_agent_counts) read 0, 0, -1, inf, inf.  Over an
        arena `agents` sums to twice the pairs and `wall` to the wall hits that stats=True counts for the same state.
        With use_torch the arrays are tensor views of the handle's one device buffer (valid until close(), rewritten by the next
        report); else host copies."""
        self._call("ca_contacts", self.h)
        return self.last_contacts()

    def last_contacts(self):
        """The last contact report computed -- by contacts() or by a call with contacts=True -- without recomputing it.  Raises
        if the handle has computed none yet."""
        if self.use_torch:
            planes = self.__dict__.get("_contact_t")
            if planes is None:
                ptr, nbytes = C.c_void_p(), C.c_size_t()
                self._call("ca_contacts_ptr", self.h, C.byref(ptr), C.byref(nbytes))

                class _View(object):   # the CUDA array interface, as in field_tensor
                    pass
                v = _View()
                v.__cuda_array_interface__ = {"shape": (5, self.A, self.N), "typestr": np.dtype(np.float32).str,
                                              "data": (int(ptr.value), False), "version": 2, "strides": None}
                t = torch.as_tensor(v, device=torch.device("cuda", self.device))
                assert t.numel() * 4 == nbytes.value
                planes = self._contact_t = {name: (t[k].view(torch.int32) if dt is np.int32 else t[k])
                                            for k, (name, dt) in enumerate(self._CONTACT_PLANES)}
            # (the library refuses a read before the first report: asked for here, without a copy)
            self._call("ca_get_contacts", self.h, None, None, None, None, None, self.A * self.N * 4, 1)
            return dict(planes)
        out = {name: np.empty((self.A, self.N), dt) for name, dt in self._CONTACT_PLANES}
        self._call("ca_get_contacts", self.h, *[_ptr(out[name]) for name, _ in self._CONTACT_PLANES], self.A * self.N * 4, 0)
        return out

    def _trace_bufs(self, steps, trace):
        """(agents, arenas, struct ca_trace or None) for trace=dict(...): torch tensors on the handle's device; None when `steps`
        holds no record (an empty tensor has no address to hand over)."""
        if torch is None or not torch.cuda.is_available():
            raise RuntimeError("trace= needs PyTorch with a device: the records are written into device tensors")
        unknown = set(trace) - {"every", "channels", "arenas"}
        if unknown:
            raise ValueError("trace: unknown key %r (known: every, channels, arenas)" % sorted(unknown)[0])
        every, channels = int(trace.get("every", 1)), trace.get("channels", ("pos", "vel"))
        ag_shape, ar_shape = trace_shape(steps, every, channels, self.A, self.N)
        dev = torch.device("cuda", self.device)
        agents = torch.empty(ag_shape, dtype=torch.float32, device=dev)
        arenas = torch.empty(ar_shape, dtype=torch.int32, device=dev) if trace.get("arenas", True) else None
        if ag_shape[0] == 0:
            return agents, arenas, None
        return agents, arenas, _lib.Trace(agents=agents.data_ptr(), agents_bytes=agents.numel() * 4,
                                          arenas=arenas.data_ptr() if arenas is not None else None,
                                          arenas_bytes=arenas.numel() * 4 if arenas is not None else 0,
                                          every=every, channels=_trace_channels(channels))

    def _traced(self, name, steps, flags, trace):
        """ca_rollout_trace / ca_alan_rollout_trace into torch tensors on the handle's device; returns dict(agents, arenas)."""
        agents, arenas, tr = self._trace_bufs(steps, trace)
        if tr is None:   # fewer steps than `every`: no record
            self._call(name[:-len("_trace")], self.h, int(steps), flags)
        else:
            self._call(name, self.h, int(steps), flags, C.byref(tr))
        if not self.use_torch:   # the handle runs on a stream of its own: the records are complete before torch's stream reads them
            self.sync()
        return dict(agents=agents, arenas=arenas)

    def rollout(self, steps, with_obs=False, stats=False, autoreset=False, freeze=False, trace=None, contacts=False):
        """`steps` ORCA-only steps without returning to the host (ca_rollout).  trace=dict(every=1, channels=("pos", "vel"),
        arenas=True): also record the state after every `every`-th step (ca_rollout_trace) and return
        dict(agents=[R, C, A, N] float32, arenas=[R, 3, A] int32 or None) of torch tensors on the handle's device (shapes:
        trace_shape); record r is the state after (r + 1) * every steps.  The tensors are filled on the handle's stream (torch's
        current stream of construction with use_torch=True; else the call waits for them).  contacts=True: also leave the contact
        report of the final state (last_contacts()): one launch behind the last step, not one per step."""
        flags = (_lib.F_OBS if with_obs else 0) | (_lib.F_STATS if stats else 0) | \
                (_lib.F_AUTORESET if autoreset else 0) | (_lib.F_FREEZE if freeze else 0) | (_lib.F_CONTACT if contacts else 0)
        if trace is not None:
            return self._traced("ca_rollout_trace", steps, flags, trace)
        self._call("ca_rollout", self.h, int(steps), flags)

    # ---- action-sequence rollouts (ca_rollout_actions) ------------------------------------------------
    def _actseq_host(self, name, shape, dtype):
        """A page-locked, device-visible array of the handle's for the numpy form of rollout_actions(), kept per name and shape."""
        bufs = self.__dict__.setdefault("_actseq_bufs", {})
        key = (name, tuple(shape))
        if key not in bufs:
            bufs[key] = self.host_array(shape, dtype)
        return bufs[key]

    @staticmethod
    def _seq_flags(with_obs, stats, autoreset, freeze, contacts):
        """The flag word of a sequence call."""
        return (_lib.F_OBS if with_obs else 0) | (_lib.F_STATS if stats else 0) | (_lib.F_AUTORESET if autoreset else 0) | \
               (_lib.F_FREEZE if freeze else 0) | (_lib.F_CONTACT if contacts else 0)

    def _seq_in(self, name, x, rows, tail=(), dtype=np.float32):
        """The input x [rows, *tail] of a sequence call where the library reads it: a contiguous device tensor (use_torch), or the
        handle's page-locked array `name` -- of at least one row -- with x in its first rows.  None stays None."""
        if x is None:
            return None
        if self.use_torch:
            return torch.as_tensor(x).detach().to(device=torch.device("cuda", self.device),
                                                  dtype=torch.float32 if dtype is np.float32 else torch.int32).contiguous()
        a = self._actseq_host(name, (max(rows, 1),) + tuple(tail), dtype)
        a[:rows] = np.asarray(x.detach().cpu().numpy() if _is_tensor(x) else x, dtype)
        return a

    def _seq_ptr(self):
        """The address of what _seq_in / _policy_bufs returned (an empty tensor has no address to hand over: None, as for None)."""
        if self.use_torch:
            return lambda t: t.data_ptr() if t is not None and t.numel() else None
        return lambda a: a.ctypes.data if a is not None else None

    def rollout_actions(self, actions, hold=1, weights=None, returns=True, first_done=False, with_obs=False, stats=False,
                        autoreset=False, freeze=False, contacts=False, steps=None, _entry="ca_rollout_actions"):
        """`steps` step() calls under the action tensor `actions` [R, A, N] without returning to the host (ca_rollout_actions): row
        t // hold drives step t, so every row is held for `hold` steps (frame skip) and steps = R * hold; steps= gives a shorter
        last row (R == ceil(steps / hold)).  The state, fields and statistics left are those of the step() calls, bit for bit.
        weights [steps] float32 (a planner's gamma ** t) or None: 1.  Returns dict(returns=, first_done=, obs=):
          returns     [A, N] float32: ret = ret + weights[t] * reward_t over the steps that advanced the agent's arena, in step
                      order, each operation rounded to float32 (returns_reference in tests/actseq_scenes.py restates the rule); a
                      frozen arena (freeze=True) adds nothing, an absent row (set_agent_counts) stays 0, and with autoreset the
                      sum runs across the respawn.  None with returns=False.
          first_done  [A] int32: the first step of the call that left the arena's done flag set, -1 if none (and for an arena
                      already frozen at entry).  None with first_done=False.
          obs         the observation of the state the call leaves (with_obs=True), else None.
        With use_torch a contiguous float32 tensor on the handle's device is read where it lies and the outputs are device
        tensors, filled on the handle's stream; otherwise numpy goes in and out and the call synchronises.  contacts=True: also
        leave the contact report of the final state (last_contacts())."""
        on_torch = self.use_torch
        if not _is_tensor(actions):
            actions = np.asarray(actions, np.float32)
        if weights is not None and not _is_tensor(weights):
            weights = np.asarray(weights, np.float32)
        hold = int(hold)
        R, steps = action_seq_shape(tuple(actions.shape), self.A, self.N, hold, steps,
                                    None if weights is None else tuple(weights.shape))
        flags = self._seq_flags(with_obs, stats, autoreset, freeze, contacts)
        act, w, ptr = self._seq_in("actions", actions, R, (self.A, self.N)), self._seq_in("weights", weights, steps), self._seq_ptr()
        if on_torch:
            dev = torch.device("cuda", self.device)
            if R == 0:   # (an empty tensor has no address to hand over)
                act = torch.zeros((1, self.A, self.N), dtype=torch.float32, device=dev)
            ret = torch.empty((self.A, self.N), dtype=torch.float32, device=dev) if returns else None
            fd = torch.empty((self.A,), dtype=torch.int32, device=dev) if first_done else None
            if not act.is_cuda:
                raise RuntimeError("rollout_actions: use_torch=True needs a device")
        else:
            ret = self._actseq_host("returns", (self.A, self.N), np.float32) if returns else None
            fd = self._actseq_host("first_done", (self.A,), np.int32) if first_done else None
        nbytes = lambda t, n: 0 if t is None else n * 4
        seq = _lib.ActionSeq(actions=ptr(act), actions_bytes=R * self.A * self.N * 4, hold=hold,
                             weights=ptr(w) if steps else None, weights_bytes=nbytes(w, steps),
                             returns=ptr(ret), returns_bytes=nbytes(ret, self.A * self.N),
                             first_done=ptr(fd), first_done_bytes=nbytes(fd, self.A))
        self._call(_entry, self.h, steps, flags, C.byref(seq))
        if not on_torch:
            self.sync()
            ret = None if ret is None else np.array(ret)
            fd = None if fd is None else np.array(fd)
        return dict(returns=ret, first_done=fd, obs=self._obs_out() if with_obs else None)

    def step_repeat(self, actions, k, with_obs=True, stats=False, autoreset=False):
        """step(actions) k times in one call (frame skip; rollout_actions with one row held for k steps).  Returns (obs,
        summed_rewards [A,N], dones [A], {"first_done": [A]}): the rewards of the k steps added up in float32 in step order,
        dones[a] true if an episode of arena a ended inside the k steps, first_done the step at which it did (-1: none)."""
        k = int(k)
        if k < 1:
            raise ValueError("step_repeat: k=%d, must be at least 1" % k)
        if self.use_torch and isinstance(actions, torch.Tensor):
            a = actions.reshape(1, self.A, self.N)
        else:
            a = np.asarray(actions, np.float32).reshape(1, self.A, self.N)
        out = self.rollout_actions(a, hold=k, returns=True, first_done=True, with_obs=with_obs, stats=stats, autoreset=autoreset)
        return out["obs"], out["returns"], out["first_done"] >= 0, {"first_done": out["first_done"]}

    # ---- the policy on the device (ca_policy_*, ca_rollout_policy) ---------------------------------------
    def set_policy(self, layers, sets=None, out="identity", limit=np.pi):
        """Install a ReLU MLP policy over the 64-float observation with one output per agent, the heading offset step() takes
        (ca_policy_configure).  layers: a list of (W, b) -- W [out, in], b [out], numpy or torch; with a leading P axis: P weight
        sets -- or a torch.nn.Sequential of Linear and ReLU; 2 .. 4 layers, hidden widths multiples of 16 in 16 .. 128 (policy_layers
        above).  sets [A] int: the set arena a plays (required with P > 1), so a population is evaluated side by side.  out="clip"
        clamps the action to [-limit, limit].  The result is defined bit for bit (include/ca_env.h); calling it again replaces the
        policy.  Configuration: it survives resets and stays with the slot under fork() / restore()."""
        if out not in ("identity", "clip"):
            raise ValueError("set_policy: out=%r, must be 'identity' or 'clip'" % (out,))
        widths, P, Ws, bs = policy_layers(layers)
        d = _lib.PolicyDesc(n_layers=len(Ws), src_is_device=0, n_sets=P, out_mode=_lib.POLICY_OUT_CLIP if out == "clip" else _lib.POLICY_OUT_IDENTITY,
                            out_limit=float(limit))
        for l, (W, b) in enumerate(zip(Ws, bs)):
            d.width[l] = widths[l]
            d.weights[l], d.weights_bytes[l] = W.ctypes.data, W.nbytes
            d.bias[l], d.bias_bytes[l] = b.ctypes.data, b.nbytes
        d.width[len(Ws)] = widths[-1]
        if sets is not None:
            if torch is not None and isinstance(sets, torch.Tensor):
                sets = sets.detach().cpu().numpy()
            s = np.asarray(sets)
            if s.dtype.kind not in "iu" or s.shape != (self.A,):
                raise ValueError("set_policy: sets must be an integer [A=%d] array, got %s %s" % (self.A, s.dtype, s.shape))
            s = np.ascontiguousarray(s, np.int32)
            d.set_of_arena, d.set_of_arena_bytes = s.ctypes.data, s.nbytes
        elif P > 1:
            raise ValueError("set_policy: %d weight sets need sets=[A] (the set every arena plays)" % P)
        self._call("ca_policy_configure", self.h, C.byref(d))

    def clear_policy(self):
        self._call("ca_policy_clear", self.h)

    def policy_info(self):
        """dict(configured=, n_layers=, widths=[w0 .. wL], n_sets=) of the installed policy (ca_policy_info)."""
        on, L, P, w = C.c_int32(0), C.c_int32(0), C.c_int32(0), (C.c_int32 * 5)()
        self._call("ca_policy_info", self.h, C.byref(on), C.byref(L), C.byref(w), C.byref(P))
        return dict(configured=bool(on.value), n_layers=L.value, widths=list(w)[:L.value + 1] if on.value else [], n_sets=P.value)

    def _policy_bufs(self, specs, on_torch):
        """{name: array} for the (name, shape, dtype) of specs: device tensors, or the handle's page-locked host arrays"""
        if on_torch:
            dev = torch.device("cuda", self.device)
            tdt = {np.float32: torch.float32, np.int32: torch.int32}
            return {n: torch.empty(tuple(max(int(d), 0) for d in shape), dtype=tdt[dt], device=dev) for n, shape, dt in specs}
        return {n: self._actseq_host("policy_" + n, tuple(max(int(d), 1) if k == 0 else int(d) for k, d in enumerate(shape)), dt)
                for n, shape, dt in specs}

    def _noise1(self, who, noise):
        """The [A, N] noise of a single policy launch where the library reads it (_seq_in), or None."""
        if noise is None:
            return None
        if not self.use_torch:
            noise = np.asarray(noise.detach().cpu().numpy() if _is_tensor(noise) else noise, np.float32).reshape(self.A, self.N)
        nz = self._seq_in("policy_noise1", noise, self.A, (self.N,))
        if tuple(nz.shape) != (self.A, self.N):
            raise ValueError("%s: noise must be [A=%d, N=%d], got %s" % (who, self.A, self.N, tuple(nz.shape)))
        return nz

    def policy_actions(self, noise=None):
        """The policy's actions [A, N] for the observation buffer as it stands (ca_policy_actions: one launch; observe() or a step
        with_obs=True fills the buffer).  noise [A, N] float32 or None is added to the mean before the output mode."""
        ptr = self._seq_ptr()
        out = self._policy_bufs([("act1", (self.A, self.N), np.float32)], self.use_torch)["act1"]
        self._call("ca_policy_actions", self.h, ptr(self._noise1("policy_actions", noise)), ptr(out))
        if self.use_torch:
            return out
        self.sync()
        return np.array(out)

    def _policy_seq_in(self, sh, noise, weights):
        """(noise, weights, ptr, size) of a policy rollout of the shapes sh: the two inputs where the library reads them, the address
        of an array and the bytes of the array of a name."""
        return (self._seq_in("policy_noise", noise, sh["R"], (self.A, self.N)), self._seq_in("policy_weights", weights, sh["weights"][0]),
                self._seq_ptr(), lambda n: int(np.prod(sh[n])) * 4)

    def _policy_seq_out(self, bufs, sh, names, with_obs):
        """What a policy rollout returns: the arrays of `names` (None: not asked for) -- under numpy, after the call has finished,
        copies of the rows the call filled -- and obs_last."""
        if not self.use_torch:
            self.sync()
            bufs = {n: np.array(a) if n in ("returns", "first_done") else np.array(a[:sh[n][0]]) for n, a in bufs.items()}
        out = {n: bufs.get(n) for n in names}
        out["obs_last"] = self._obs_out() if with_obs else None
        return out

    def rollout_policy(self, steps, hold=1, noise=None, weights=None, record=("obs", "actions", "rewards", "dones"), returns=True,
                       first_done=False, with_obs=False, stats=False, autoreset=False, freeze=False, contacts=False,
                       _entry="ca_rollout_policy"):
        """`steps` steps under the installed policy without returning to the host (ca_rollout_policy): at every hold-th step
        observe(), the policy on that observation (plus noise[t // hold] where given), then step() under the action for `hold`
        steps.  The state, fields and statistics left are those of that loop, bit for bit.  noise [R, A, N] (R = ceil(steps /
        hold)): exploration noise the caller drew; weights [steps]: as for rollout_actions().  record: which of the trajectory
        records to write -- "obs" [R, A, N, 64] and "actions" [R, A, N], what the policy read and emitted per row; "rewards"
        [steps, A, N] and "dones" [steps, A] (int32, the arenas' done flags) per step.  Returns a dict with those, returns [A, N],
        first_done [A] and obs_last (with_obs=True: the observation of the final state); what was not asked for is None.  With
        use_torch the arrays are device tensors filled on the handle's stream, else numpy arrays (the call synchronises).  Shapes:
        policy_seq_shape."""
        on_torch = self.use_torch
        record = (record,) if isinstance(record, str) else tuple(record or ())
        for r in record:
            if r not in ("obs", "actions", "rewards", "dones"):
                raise ValueError("rollout_policy: record holds %r; it may hold 'obs', 'actions', 'rewards', 'dones'" % (r,))
        sh = policy_seq_shape(self.A, self.N, steps, hold, _shape_of(noise), _shape_of(weights))
        steps, hold, R = int(steps), int(hold), sh["R"]
        flags = self._seq_flags(with_obs, stats, autoreset, freeze, contacts)
        specs = [(n, sh[n], np.int32 if n in ("first_done", "dones") else np.float32)
                 for n, want in (("returns", returns), ("first_done", first_done), ("obs", "obs" in record), ("actions", "actions" in record),
                                 ("rewards", "rewards" in record), ("dones", "dones" in record)) if want]
        bufs = self._policy_bufs(specs, on_torch)
        nz, w, ptr, size = self._policy_seq_in(sh, noise, weights)
        b = bufs.get
        seq = _lib.PolicySeq(hold=hold, noise=ptr(nz) if R else None, noise_bytes=size("noise") if nz is not None else 0,
                             weights=ptr(w) if steps else None, weights_bytes=size("weights") if w is not None else 0,
                             returns=ptr(b("returns")), returns_bytes=size("returns") if returns else 0,
                             first_done=ptr(b("first_done")), first_done_bytes=size("first_done") if first_done else 0,
                             obs_out=ptr(b("obs")) if R else None, obs_out_bytes=size("obs") if "obs" in bufs else 0,
                             actions_out=ptr(b("actions")) if R else None, actions_out_bytes=size("actions") if "actions" in bufs else 0,
                             rewards_out=ptr(b("rewards")) if steps else None, rewards_out_bytes=size("rewards") if "rewards" in bufs else 0,
                             done_out=ptr(b("dones")) if steps else None, done_out_bytes=size("dones") if "dones" in bufs else 0)
        self._call(_entry, self.h, steps, flags, C.byref(seq))
        return self._policy_seq_out(bufs, sh, ("returns", "first_done", "obs", "actions", "rewards", "dones"), with_obs)

    # ---- PPO sample collection (ca_policy_set_heads, ca_policy_evaluate, ca_rollout_policy_sample, ca_gae) ---------
    def set_policy_heads(self, value=None, log_std=None):
        """Install a value head and / or a log-std head on the installed policy (ca_policy_set_heads): two extra rows of the output
        layer, read from the last hidden layer.  value=(w, b), log_std=(w_or_None, b) -- numpy or torch, per weight set or shared
        -- or torch.nn.Linear modules (policy_heads above).  log-std is clamped to [-20, 2]; w None: a state-independent log-std.
        Configuration like the policy; set_policy() and clear_policy() drop the heads."""
        info = self.policy_info()
        if not info["configured"]:
            raise RuntimeError("set_policy_heads: call set_policy first")
        h = policy_heads(info["widths"][-2], info["n_sets"], value, log_std)
        d = _lib.PolicyHeads()
        for n, a in h.items():
            if a is not None:
                setattr(d, n, a.ctypes.data)
                setattr(d, n + "_bytes", a.nbytes)
        self._call("ca_policy_set_heads", self.h, C.byref(d))

    def clear_policy_heads(self):
        self._call("ca_policy_clear_heads", self.h)

    def policy_heads_info(self):
        """dict(value=, log_std=): which heads are installed (ca_policy_heads_info)."""
        v, s = C.c_int32(0), C.c_int32(0)
        self._call("ca_policy_heads_info", self.h, C.byref(v), C.byref(s))
        return dict(value=bool(v.value), log_std=bool(s.value))

    def policy_evaluate(self, noise=None):
        """The policy with its heads on the observation buffer as it stands (ca_policy_evaluate: one launch): dict(actions=, logp=,
        value=, mean=, log_std=), each [A, N] float32.  noise [A, N] is eps: action = out(mean + exp(log_std) * eps), logp the
        log-density of the unclipped sample (include/ca_env.h has the definition, bit for bit)."""
        names = ("actions", "logp", "value", "mean", "log_std")
        ptr = self._seq_ptr()
        bufs = self._policy_bufs([("eval_" + n, (self.A, self.N), np.float32) for n in names], self.use_torch)
        o = _lib.PolicyEval(**{n: ptr(bufs["eval_" + n]) for n in names})
        self._call("ca_policy_evaluate", self.h, ptr(self._noise1("policy_evaluate", noise)), C.byref(o))
        if self.use_torch:
            return {n: bufs["eval_" + n] for n in names}
        self.sync()
        return {n: np.array(bufs["eval_" + n]) for n in names}

    _SAMPLE_RECORDS = ("obs", "actions", "rewards", "dones", "logp", "dist", "values", "row_rewards", "row_dones", "row_valid",
                       "advantages", "targets")

    def rollout_policy_sample(self, steps, hold=1, noise=None, gamma=0.95, lam=1.0, weights=None,
                              record=("obs", "actions", "logp", "dist", "values", "row_rewards", "row_dones", "row_valid", "advantages", "targets"),
                              returns=True, first_done=False, with_obs=False, stats=False, autoreset=False, freeze=False, contacts=False):
        """rollout_policy() under the policy with its heads, handing back a PPO batch (ca_rollout_policy_sample).  noise [R, A, N]
        is eps (R = ceil(steps / hold)).  record: rollout_policy's four records and "logp" [R, A, N], "dist" [R, 2, A, N] (mean,
        clamped log-std), "values" [R + 1, A, N] (row R: the bootstrap value of the state the call leaves), "row_rewards"
        [R, A, N] (the rewards of a row's steps added up), "row_dones" / "row_valid" [R, A] int32, "advantages" / "targets"
        [R, A, N] (GAE under gamma and lam; they need "values").  Returns a dict as rollout_policy()'s; conventions as there.
        Shapes: policy_sample_shape."""
        on_torch = self.use_torch
        record = (record,) if isinstance(record, str) else tuple(record or ())
        for r in record:
            if r not in self._SAMPLE_RECORDS:
                raise ValueError("rollout_policy_sample: record holds %r; it may hold %s" % (r, ", ".join(repr(n) for n in self._SAMPLE_RECORDS)))
        if ("advantages" in record or "targets" in record) and "values" not in record:
            raise ValueError("rollout_policy_sample: 'advantages' and 'targets' need 'values' among the records")
        sh = policy_sample_shape(self.A, self.N, steps, hold, _shape_of(noise), _shape_of(weights))
        steps, hold, R = int(steps), int(hold), sh["R"]
        flags = self._seq_flags(with_obs, stats, autoreset, freeze, contacts)
        ints = ("first_done", "dones", "row_dones", "row_valid")
        wanted = [n for n, want in (("returns", returns), ("first_done", first_done)) if want] + [n for n in self._SAMPLE_RECORDS if n in record]
        bufs = self._policy_bufs([("sample_" + n, sh[n], np.int32 if n in ints else np.float32) for n in wanted], on_torch)
        bufs = {n[len("sample_"):]: a for n, a in bufs.items()}
        nz, w, ptr, size = self._policy_seq_in(sh, noise, weights)
        kw = dict(hold=hold, noise=ptr(nz) if R else None, noise_bytes=size("noise") if nz is not None else 0,
                  weights=ptr(w) if steps else None, weights_bytes=size("weights") if w is not None else 0,
                  gamma=float(gamma))
        kw["lambda"] = float(lam)
        member = dict(returns="returns", first_done="first_done", obs="obs_out", actions="actions_out", rewards="rewards_out", dones="done_out",
                      logp="logp_out", dist="dist_out", values="values_out", row_rewards="row_rewards_out", row_dones="row_done_out",
                      row_valid="row_valid_out", advantages="advantages_out", targets="targets_out")
        for n, a in bufs.items():
            empty = n != "values" and n not in ("returns", "first_done") and (steps == 0)
            kw[member[n]] = None if empty else ptr(a)
            kw[member[n] + "_bytes"] = size(n)
        seq = _lib.PolicySampleSeq(**kw)
        self._call("ca_rollout_policy_sample", self.h, steps, flags, C.byref(seq))
        return self._policy_seq_out(bufs, sh, ("returns", "first_done") + self._SAMPLE_RECORDS, with_obs)

    def gae(self, rewards, values, done, valid=None, gamma=0.95, lam=1.0):
        """Generalised advantage estimation on the device (ca_gae): rewards [R, A, N], values [R + 1, A, N], done [R, A], valid
        [R, A] or None (all 1).  Returns (advantages, targets), each [R, A, N] float32; include/ca_env.h has the definition, bit for
        bit.  Device tensors in and out under use_torch, else numpy (the call synchronises)."""
        on_torch = self.use_torch
        R = int(_shape_of(rewards)[0])
        want = dict(rewards=(R, self.A, self.N), values=(R + 1, self.A, self.N), done=(R, self.A), valid=(R, self.A))
        given = dict(rewards=rewards, values=values, done=done, valid=valid)
        for n, x in given.items():
            if x is not None and _shape_of(x) != want[n]:
                raise ValueError("gae: %s must be %s, got shape %s" % (n, list(want[n]), _shape_of(x)))
        out = self._policy_bufs([("gae_advantages", want["rewards"], np.float32), ("gae_targets", want["rewards"], np.float32)], on_torch)
        ins = {n: self._seq_in("gae_" + n, x, want[n][0], want[n][1:], np.float32 if n in ("rewards", "values") else np.int32)
               for n, x in given.items() if x is not None}
        ptr = self._seq_ptr()
        kw = dict(gamma=float(gamma))
        kw["lambda"] = float(lam)
        for n in ins:
            kw[n], kw[n + "_bytes"] = ptr(ins[n]), int(np.prod(want[n])) * 4
        for n in ("advantages", "targets"):
            kw[n], kw[n + "_bytes"] = ptr(out["gae_" + n]), int(np.prod(want["rewards"])) * 4
        if R:
            self._call("ca_gae", self.h, R, C.byref(_lib.GaeDesc(**kw)))
        if on_torch:
            return out["gae_advantages"], out["gae_targets"]
        self.sync()
        return np.array(out["gae_advantages"][:R]), np.array(out["gae_targets"][:R])

    # ---- reward terms (ca_reward_*) ---------------------------------------------------------------------
    def set_reward_terms(self, base=1.0, collision=0.0, wall=0.0, near=0.0, wall_near=0.0, arrival=0.0, step=0.0, margin=0.0):
        """Shape the reward on the device (ca_reward_configure; include/ca_env.h has the definition, bit for bit): while set, every
        call that writes the reward from actions -- step, step_packed, rollout_actions, rollout_policy, rollout_policy_sample, step_nav
        and the navigated rollouts -- leaves
            r = base * r_ref + collision * (agents touched) + wall * (on a wall) + near * (agents within the radii + margin)
                + wall_near * (a wall within the radius + margin) + arrival * (arrived in this step) + step * (was not done)
        in the reward, so that returns, records, advantages and targets are computed from it.  A penalty is a negative weight.  Each
        weight is a scalar or [A] (a curriculum over arenas); margin is the comfort distance of near / wall_near.  Configuration: it
        survives resets and scenarios and stays with the slot under fork() / restore().  orca_step, rollout and alan_* are not
        affected."""
        w, per_arena, m = reward_terms(self.A, base, collision, wall, near, wall_near, arrival, step, margin)
        d = _lib.RewardDesc(weights=_ptr(w), weights_bytes=w.nbytes, per_arena=per_arena, margin=m)
        self._call("ca_reward_configure", self.h, C.byref(d))

    def clear_reward_terms(self):
        self._call("ca_reward_clear", self.h)

    def reward_terms_info(self):
        """dict(configured=, per_arena=, margin=, weights=) of the installed terms (ca_reward_info, ca_reward_get_weights): weights
        float32 [A, 7] as the kernel uses them, None while nothing is configured."""
        c, pa, m = C.c_int32(0), C.c_int32(0), C.c_float(0.0)
        self._call("ca_reward_info", self.h, C.byref(c), C.byref(pa), C.byref(m))
        w = None
        if c.value:
            w = np.empty((self.A, _lib.REWARD_N_TERMS), np.float32)
            self._call("ca_reward_get_weights", self.h, _ptr(w), w.nbytes)
        return dict(configured=bool(c.value), per_arena=bool(pa.value), margin=float(m.value), weights=w)

    def reward_parts(self):
        """The parts of a shaped reward for the current state (ca_reward_parts), a dict of seven [A,N] arrays: ref float32 -- the
        reward field as it stands -- and collision, wall, near, wall_near, arrival (0 here), step (agent_done == 0) int32.  A count
        that no arena has a weight for reads 0.  The reward is not written.  With use_torch the arrays are views of the handle's one
        device buffer (rewritten by every step under terms); else host copies."""
        self._call("ca_reward_parts", self.h)
        return self.last_reward_parts()

    def last_reward_parts(self):
        """The parts last computed -- by reward_parts() or by a step under terms -- without recomputing them.  Raises if the handle
        has computed none yet."""
        names = ("ref",) + _lib.REWARD_TERMS[1:]
        if self.use_torch:
            planes = self.__dict__.get("_reward_parts_t")
            if planes is None:
                ptr, nbytes = C.c_void_p(), C.c_size_t()
                self._call("ca_reward_parts_ptr", self.h, C.byref(ptr), C.byref(nbytes))

                class _View(object):   # the CUDA array interface, as in field_tensor
                    pass
                v = _View()
                v.__cuda_array_interface__ = {"shape": (_lib.REWARD_N_TERMS, self.A, self.N), "typestr": np.dtype(np.float32).str,
                                              "data": (int(ptr.value), False), "version": 2, "strides": None}
                t = torch.as_tensor(v, device=torch.device("cuda", self.device))
                assert t.numel() * 4 == nbytes.value
                planes = self._reward_parts_t = {name: (t[k] if k == 0 else t[k].view(torch.int32)) for k, name in enumerate(names)}
            # (the library refuses a read before the first computation: asked for here, without a copy)
            self._call("ca_get_reward_parts", self.h, None, None, 0, 0, 1)
            return dict(planes)
        ref = np.empty((self.A, self.N), np.float32)
        cnt = np.empty((_lib.REWARD_N_TERMS - 1, self.A, self.N), np.int32)
        self._call("ca_get_reward_parts", self.h, _ptr(ref), _ptr(cnt), ref.nbytes, cnt.nbytes, 0)
        out = {"ref": ref}
        out.update({name: cnt[k] for k, name in enumerate(names[1:])})
        return out

    # ---- navigation fields (ca_nav_*) ------------------------------------------------------------------
    def set_navigation(self, targets, agent_class, cell, origin=None, shape=None, clearance=None, lookahead=2):
        """Shortest-path fields towards a few shared targets, to steer agents round obstacles (ca_nav_configure; include/ca_env.h has
        the definition, bit for bit).  targets [G, 2]: one set of fields for all arenas (needs one common obstacle table), or
        [A, G, 2]: a set per arena, relaxed round the arena's own table.  agent_class int [A, N] (or a scalar / [N], broadcast): the
        target an agent walks to, -1: not navigated.  cell: the grid's cell size; origin (x0, y0) and shape (gx, gy) default to the
        bounding box of the obstacle table(s); clearance (how near an edge a cell centre may lie) to the radius; lookahead: pointer
        steps per nav_pref().  Configuration: it survives resets and scenarios and stays with the slot under fork() / restore();
        set_obstacles*() clears it."""
        t = np.ascontiguousarray(np.asarray(targets.detach().cpu().numpy() if torch is not None and isinstance(targets, torch.Tensor) else targets,
                                            np.float32))
        if t.ndim not in (2, 3) or t.shape[-1] != 2 or (t.ndim == 3 and t.shape[0] != self.A):
            raise ValueError("set_navigation: targets must be [G, 2] or [A=%d, G, 2], got %s" % (self.A, t.shape))
        cls = np.ascontiguousarray(np.broadcast_to(np.asarray(agent_class, np.int32), (self.A, self.N)))
        cell = float(cell)
        if origin is None or shape is None:
            tabs = [self.obstacle_table(a)["verts"] for a in (range(self.A) if t.ndim == 3 else (0,))]
            v = np.concatenate(tabs) if tabs else np.zeros((0, 2), np.float32)
            if len(v) == 0:
                raise ValueError("set_navigation: no obstacle table to take the grid's box from: give origin= and shape=")
            lo, hi = v.min(axis=0), v.max(axis=0)
            if origin is None:
                origin = (float(lo[0]), float(lo[1]))
            if shape is None:
                shape = tuple(max(1, int(np.ceil((float(hi[k]) - float(origin[k])) / cell))) for k in (0, 1))
        d = _lib.NavDesc(x0=float(origin[0]), y0=float(origin[1]), cell=cell, gx=int(shape[0]), gy=int(shape[1]),
                         clearance=float(self.cfg.radius if clearance is None else clearance), n_goals=int(t.shape[-2]),
                         per_arena=1 if t.ndim == 3 else 0, targets=_ptr(t), targets_bytes=t.nbytes, agent_class=_ptr(cls),
                         class_bytes=cls.nbytes, lookahead=int(lookahead))
        self._call("ca_nav_configure", self.h, C.byref(d))

    def clear_navigation(self):
        self._call("ca_nav_clear", self.h)

    def navigation_info(self):
        """dict(configured=, gx=, gy=, n_goals=, n_sets=, sweeps_max=) of the installed navigation (ca_nav_info)."""
        v = [C.c_int32(0) for _ in range(6)]
        self._call("ca_nav_info", self.h, *[C.byref(x) for x in v])
        return dict(configured=bool(v[0].value), gx=v[1].value, gy=v[2].value, n_goals=v[3].value, n_sets=v[4].value, sweeps_max=v[5].value)

    def nav_field(self, arena=0, goal=0):
        """(dist float32 [gy, gx], next uint8, blocked uint8) of one field, as host arrays (ca_nav_get_field): the distance to the
        target (inf: blocked or unreachable), the pointer per cell (_lib.NAV_OFFSETS[k], _lib.NAV_STAY, _lib.NAV_NONE) and the mask."""
        i = self.navigation_info()
        gx, gy = max(i["gx"], 1), max(i["gy"], 1)
        dist, nxt, blk = np.empty((gy, gx), np.float32), np.empty((gy, gx), np.uint8), np.empty((gy, gx), np.uint8)
        self._call("ca_nav_get_field", self.h, int(arena), int(goal), _ptr(dist), _ptr(nxt), _ptr(blk), gx * gy)
        return dist, nxt, blk

    def _nav_dist_buf(self, dist):
        """(buffer the kernel writes, its address) for dist=True or an [A, N] array / tensor whose rows that are not navigated keep
        their values: a device tensor with use_torch, else the handle's page-locked array."""
        given = dist is not True
        if self.use_torch:
            dev = torch.device("cuda", self.device)
            if given:
                buf = torch.as_tensor(dist).detach().to(device=dev, dtype=torch.float32).reshape(self.A, self.N).contiguous()
            else:
                buf = torch.full((self.A, self.N), float("inf"), dtype=torch.float32, device=dev)
            return buf, buf.data_ptr()
        buf = self._actseq_host("nav_dist", (self.A, self.N), np.float32)
        buf[...] = np.asarray(dist.detach().cpu().numpy() if torch is not None and isinstance(dist, torch.Tensor) else dist,
                              np.float32).reshape(self.A, self.N) if given else np.inf
        return buf, buf.ctypes.data

    def nav_pref(self, dist=False, freeze=False):
        """Write the preferred velocities (PREF_X / PREF_Y) of the navigated agents from the fields (ca_nav_pref: one launch); the
        next orca_step() steers by them.  freeze: the agents of arenas whose episode is over are not written.  dist=True: returns
        the distance to go [A, N] (inf in a blocked cell and for rows that are not navigated); dist=an [A, N] array: the same with
        that array's values kept for rows that are not navigated.  A device tensor with use_torch, else a numpy array."""
        if dist is False or dist is None:
            self._call("ca_nav_pref", self.h, None, _lib.F_FREEZE if freeze else 0)
            return None
        buf, addr = self._nav_dist_buf(dist)
        self._call("ca_nav_pref", self.h, C.c_void_p(addr), _lib.F_FREEZE if freeze else 0)
        if self.use_torch:
            return buf
        self.sync()
        return np.array(buf)

    def rollout_nav(self, steps, with_obs=False, stats=False, autoreset=False, freeze=False, trace=None, contacts=False, dist=False):
        """`steps` navigated ORCA-only steps without returning to the host (ca_rollout_nav): per step nav_pref(freeze=freeze), then
        orca_step(...) -- the state, fields and statistics left are those of that loop, bit for bit.  with_obs / contacts: one
        launch behind the last step.  trace=dict(...): as for rollout(); returns its dict.  dist=True (not together with trace): the
        last step is made as nav_pref(dist=True) + orca_step(), the same launches, and the distances to go seen in front of it are
        returned."""
        steps = int(steps)
        flags = (_lib.F_OBS if with_obs else 0) | (_lib.F_STATS if stats else 0) | \
                (_lib.F_AUTORESET if autoreset else 0) | (_lib.F_FREEZE if freeze else 0) | (_lib.F_CONTACT if contacts else 0)
        if trace is not None:
            if dist:
                raise ValueError("rollout_nav: dist=True does not go together with trace=")
            agents, arenas, tr = self._trace_bufs(steps, trace)
            self._call("ca_rollout_nav", self.h, steps, flags, C.byref(tr) if tr is not None else None)
            if not self.use_torch:
                self.sync()
            return dict(agents=agents, arenas=arenas)
        if dist and steps > 0:
            self._call("ca_rollout_nav", self.h, steps - 1, flags & ~(_lib.F_OBS | _lib.F_CONTACT), None)
            out = self.nav_pref(dist=True, freeze=freeze)
            self._call("ca_orca_step", self.h, flags)
            return out
        self._call("ca_rollout_nav", self.h, steps, flags, None)

    # ---- action steps steered by the navigation fields (ca_nav_act, ca_nav_step, ca_rollout_nav_*) -------------------
    def nav_act(self, actions, heading=False, dist=False, freeze=False):
        """Write the preferred velocities (PREF_X / PREF_Y) of every present agent as the navigation heading rotated by actions [A, N]
        (ca_nav_act: one launch): the heading is nav_pref()'s for a navigated agent and the direction to its own goal for every
        other one (class -1, or arrived and walking on).  The next orca_step() steers by them.  freeze: the agents of arenas whose
        episode is over are not written.  Returns None, or a dict of what was asked for: heading [2, A, N] (the unrotated
        direction; heading=True: zeros for rows that were not written, heading=an array: that array's values) and dist [A, N] as
        nav_pref(dist=...) gives it (navigated rows only).  Device tensors with use_torch, else numpy arrays."""
        flags = _lib.F_FREEZE if freeze else 0
        want_dist = not (dist is False or dist is None)
        head_given = None if heading is True or heading is False or heading is None else heading
        heading = heading is True or head_given is not None
        if head_given is not None and torch is not None and isinstance(head_given, torch.Tensor) and not self.use_torch:
            head_given = head_given.detach().cpu().numpy()
        if self.use_torch:
            dev = torch.device("cuda", self.device)
            act = torch.as_tensor(actions).detach().to(device=dev, dtype=torch.float32).reshape(self.A, self.N).contiguous()
            head = torch.zeros((2, self.A, self.N), dtype=torch.float32, device=dev) if heading else None
            if head_given is not None:
                head.copy_(torch.as_tensor(head_given).to(device=dev, dtype=torch.float32).reshape(2, self.A, self.N))
            a_addr, h_addr = act.data_ptr(), head.data_ptr() if heading else None
        else:
            if torch is not None and isinstance(actions, torch.Tensor):
                actions = actions.detach().cpu().numpy()
            act = self._actseq_host("nav_actions", (self.A, self.N), np.float32)
            act[...] = np.asarray(actions, np.float32).reshape(self.A, self.N)
            head = None
            if heading:
                head = self._actseq_host("nav_heading", (2, self.A, self.N), np.float32)
                head[...] = 0.0 if head_given is None else np.asarray(head_given, np.float32).reshape(2, self.A, self.N)
            a_addr, h_addr = act.ctypes.data, head.ctypes.data if heading else None
        dbuf, d_addr = self._nav_dist_buf(dist) if want_dist else (None, None)
        self._call("ca_nav_act", self.h, C.c_void_p(a_addr), C.c_void_p(h_addr) if heading else None,
                   C.c_void_p(d_addr) if want_dist else None, flags)
        if not (heading or want_dist):
            if not self.use_torch:
                self.sync()       # (the action buffer is the handle's own: the next call may overwrite it)
            return None
        if not self.use_torch:
            self.sync()
            head, dbuf = (None if head is None else np.array(head)), (None if dbuf is None else np.array(dbuf))
        return dict(heading=head, dist=dbuf)

    def step_nav(self, actions, with_obs=True, stats=False, autoreset=False, freeze=False, copy=True, contacts=False):
        """step(actions) with the actions taken as offsets from the navigation heading (ca_nav_step): nav_act(actions), the
        launches of orca_step(), and a small kernel that writes the reference's reward from the velocity the step left and the two
        directions nav_act kept -- progress along the navigation heading and along the rotated one.  Returns what step() returns.
        An agent that is not navigated steps exactly as under step(); arrive_step counts the ORCA-only way and PREF afterwards is
        the direction to the goal (include/ca_env.h).  Needs set_navigation()."""
        flags = (_lib.F_OBS if with_obs else 0) | (_lib.F_STATS if stats else 0) | (_lib.F_AUTORESET if autoreset else 0) | \
                (_lib.F_FREEZE if freeze else 0) | (_lib.F_CONTACT if contacts else 0)
        if self.use_torch:
            if not isinstance(actions, torch.Tensor):
                actions = torch.as_tensor(np.asarray(actions, np.float32).reshape(self.A, self.N))
            if actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous() and \
                    actions.numel() == self.A * self.N and actions.device.index == self.device:
                src = actions
            else:
                self._act_t.copy_(actions.reshape(self.A, self.N), non_blocking=True)
                src = self._act_t
            self._call("ca_nav_step", self.h, C.c_void_p(src.data_ptr()), flags)
            return (self._obs_t if with_obs else None), self._rew_t, self._done_t, \
                ({"contacts": self.last_contacts()} if contacts else {})
        if torch is not None and isinstance(actions, torch.Tensor):
            actions = actions.detach().cpu().numpy()
        a = self._actseq_host("nav_actions", (self.A, self.N), np.float32)   # page-locked and device-visible: read where it lies
        a[...] = np.asarray(actions, np.float32).reshape(self.A, self.N)
        self._call("ca_nav_step", self.h, C.c_void_p(a.ctypes.data), flags)
        infos = {"contacts": self.last_contacts()} if contacts else {}
        if not copy:
            return (self.get(_lib.FLD_OBS, self.host_buffer(_lib.FLD_OBS)) if with_obs else None), \
                self.get(_lib.FLD_REWARD, self.host_buffer(_lib.FLD_REWARD)), \
                self.get(_lib.FLD_ARENA_DONE, self.host_buffer(_lib.FLD_ARENA_DONE)), infos
        return (self.get(_lib.FLD_OBS) if with_obs else None), self.get(_lib.FLD_REWARD), \
            self.get(_lib.FLD_ARENA_DONE), infos

    def rollout_nav_actions(self, actions, hold=1, weights=None, returns=True, first_done=False, with_obs=False, stats=False,
                            autoreset=False, freeze=False, contacts=False, steps=None):
        """rollout_actions() with step_nav() in place of step() (ca_rollout_nav_actions): the same arguments, the same dict."""
        return self.rollout_actions(actions, hold, weights, returns, first_done, with_obs, stats, autoreset, freeze, contacts, steps,
                                    _entry="ca_rollout_nav_actions")

    def rollout_nav_policy(self, steps, hold=1, noise=None, weights=None, record=("obs", "actions", "rewards", "dones"), returns=True,
                           first_done=False, with_obs=False, stats=False, autoreset=False, freeze=False, contacts=False):
        """rollout_policy() with step_nav() in place of step() (ca_rollout_nav_policy): the same arguments, the same dict."""
        return self.rollout_policy(steps, hold, noise, weights, record, returns, first_done, with_obs, stats, autoreset, freeze, contacts,
                                   _entry="ca_rollout_nav_policy")

    # ---- ALAN online learning (ALAN_true.py:569-628) -----------------------------------------------
    def alan_configure(self, actions, temp=0.2, timewindow=2.0, time_step=1 / 60.):
        """Bandit state of the reference's constructor (ALAN_true.py:31-38, 47-49, 73-76): `actions`
        [n, 2] vectors, weights and times zeroed."""
        a = np.ascontiguousarray(np.asarray(actions, np.float64).reshape(-1, 2))
        self._call("ca_alan_configure", self.h, _ptr(a), a.shape[0], float(temp), float(timewindow), float(time_step))
        self.n_actions = a.shape[0]

    def alan_configure_per_arena(self, action_sets, temp=0.2, timewindow=2.0, time_step=1 / 60.):
        """An action set per arena (ca_alan_configure_per_arena): `action_sets` is a list of A lists of (x, y), each of
        1..32 actions; weights and times zeroed.  n_actions becomes the largest set (the stride of the weights / times,
        whose rows beyond an arena's own set stay zero), so get_state / set_state work unchanged."""
        if len(action_sets) != self.A:
            raise ValueError("alan_configure_per_arena: %d action sets for %d arenas" % (len(action_sets), self.A))
        sets = [np.asarray(acts, np.float64).reshape(-1, 2) for acts in action_sets]
        n = np.ascontiguousarray([s.shape[0] for s in sets], np.int32)
        xy = np.ascontiguousarray(np.concatenate(sets, 0) if n.sum() else np.zeros((0, 2)), np.float64)
        self._call("ca_alan_configure_per_arena", self.h, _ptr(xy), _ptr(n), float(temp), float(timewindow), float(time_step))
        self.n_actions = int(n.max())

    def alan_actions(self, arena):
        """The action set of `arena` as the kernels use it (ca_alan_actions_arena): [n, 2] unit (cos, sin) pairs."""
        cnt = C.c_int32(0)
        self._call("ca_alan_actions_arena", self.h, int(arena), None, 0, C.byref(cnt))
        out = np.zeros((max(cnt.value, 1), 2), np.float64)
        self._call("ca_alan_actions_arena", self.h, int(arena), _ptr(out), cnt.value, C.byref(cnt))
        return out[:cnt.value]

    def alan_step(self, u=None, with_obs=False, stats=False, freeze=False, contacts=False):
        """reference online_step (ALAN_true.py:569-628) + step counter + goal test (ALAN:118-121).
        u [A,N] float64: the uniforms behind np.random.choice, one per agent (numpy or device tensor);
        None: the handle's counter-based RNG.  contacts=True: also leave the contact report of the state the step leaves
        (last_contacts())."""
        flags = (_lib.F_OBS if with_obs else 0) | (_lib.F_STATS if stats else 0) | (_lib.F_FREEZE if freeze else 0) | \
                (_lib.F_CONTACT if contacts else 0)
        if u is None:
            self._call("ca_alan_step", self.h, None, 0, flags)
        elif torch is not None and isinstance(u, torch.Tensor) and u.is_cuda:
            ud, _ = self._on_device(u, torch.float64)
            if ud.numel() != self.A * self.N:
                raise ValueError("alan_step: u must hold %d x %d values" % (self.A, self.N))
            self._call("ca_alan_step", self.h, C.c_void_p(ud.data_ptr()), 1, flags)
            self.sync()
        else:
            if torch is not None and isinstance(u, torch.Tensor):
                u = u.detach().numpy()
            uh = np.ascontiguousarray(np.asarray(u, np.float64).reshape(self.A, self.N))
            self._call("ca_alan_step", self.h, _ptr(uh), 0, flags)
        return self._obs_out() if with_obs else None

    def alan_rollout(self, steps, stats=False, freeze=True, trace=None, contacts=False):
        """run_sim(mode=1) (ALAN_true.py:106-123) for every arena at once: each arena stops at the end of
        its own episode (freeze) or after `steps` steps.  trace, contacts: as for rollout() (ca_alan_rollout_trace)."""
        flags = (_lib.F_STATS if stats else 0) | (_lib.F_FREEZE if freeze else 0) | (_lib.F_CONTACT if contacts else 0)
        if trace is not None:
            return self._traced("ca_alan_rollout_trace", steps, flags, trace)
        self._call("ca_alan_rollout", self.h, int(steps), flags)

    def state(self):
        names = dict(pos_x=_lib.FLD_POS_X, pos_y=_lib.FLD_POS_Y, vel_x=_lib.FLD_VEL_X, vel_y=_lib.FLD_VEL_Y,
                     pref_x=_lib.FLD_PREF_X, pref_y=_lib.FLD_PREF_Y, goal_x=_lib.FLD_GOAL_X,
                     goal_y=_lib.FLD_GOAL_Y, agent_done=_lib.FLD_AGENT_DONE,
                     step_count=_lib.FLD_STEP_COUNT, arena_done=_lib.FLD_ARENA_DONE)
        return {k: self.get(v) for k, v in names.items()}
