"""Scenes for the paired LP3 round of the one-wave register-line solve kernels (csrc/ca_lp.h lp3_pair_lds, CA_LP3_PAIRS): one arena
of 64 agents in the crowd world (its border: four edges, obstacle lists of 4), range 5, K = 10 or 5, built so that a wave's count of
agents infeasible after LP2 crosses the two thresholds of the pool round (16 four-lane slots, 32 two-lane slots):

  clump    all agents in a small disc, heading for its centre: the count starts near zero, climbs through 16 | 17 and past 32;
  corner   the same clump pressed into the corner (0, 0) of the border, so that infeasible agents hold obstacle lines;
  mirror   rows along x that are bit-exact mirror images about their middle agent: triples d apart (the middle agent overlapped
           from both sides: LP3 meets a parallel line of the opposite direction) and rows of five (a resting agent 1.25 away on
           each side, a fast one 0.5 behind it heading inward: the far line is the violated one and the near line before it is parallel
           with the SAME direction).

tests/test_lp3_pairs_cpu.py checks on the oracle alone that the scenes reach these cases; tests/test_gpu_lp3_pairs.py runs them on the
kernels.  Every figure below is exact in fp32 where the mirror symmetry needs it."""
import numpy as np

from oracle import oracle as o
from tests import helpers as H

F = np.float32
N = 64
RANGE = 5.0
STEPS = 48          # steps of every scene (the GPU test's 40 .. 60)
E = 16.0            # side of the crowd world of 64 agents (scenarios.crowd_envsize)


def params(K):
    return H.scenario_params("crowd", N, neighbor_dist=RANGE, max_neighbors=K)


def _disc(cx, cy, rad, seed, lo=None):
    """64 points of a sunflower spiral in the disc, jittered by a seeded draw; lo: keep this far inside the border's corner"""
    rng = np.random.RandomState(seed)
    k = np.arange(N) + 0.5
    r = rad * np.sqrt(k / N)
    t = k * 2.399963229728653 + rng.uniform(0, 0.3, N)
    x, y = cx + r * np.cos(t), cy + r * np.sin(t)
    if lo is not None:
        x, y = np.maximum(x, lo), np.maximum(y, lo)
    return x.astype(F), y.astype(F)


def clump(seed=1, rad=7.0):
    px, py = _disc(E / 2, E / 2, rad, seed)
    z = np.zeros(N, F)
    return dict(px=px, py=py, vx=z, vy=z, gx=np.full(N, E / 2), gy=np.full(N, E / 2))


def corner(seed=2, rad=6.5):
    px, py = _disc(3.0, 3.0, rad, seed, lo=0.75)
    z = np.zeros(N, F)
    return dict(px=px, py=py, vx=z, vy=z, gx=np.full(N, 0.5), gy=np.full(N, 0.5))


def mirror():
    """15 triples (45 agents) and 3 rows of five (15 agents), 4 agents parked apart; rows 2.0 apart in y, groups 5.5 apart in x"""
    px, py, vx, vy = [], [], [], []
    def put(x, y, u=0.0):
        px.append(x); py.append(y); vx.append(u); vy.append(0.0)
    for g in range(15):                       # triples: 0.75 apart (each end overlaps the middle agent, not the other end)
        cx, cy = 1.5 + 3.25 * (g % 4), 1.0 + 2.0 * (g // 4)
        for dx in (-0.75, 0.0, 0.75):
            put(cx + dx, cy)
    for g in range(3):                        # rows of five: resting at +-1.25, inward at full speed from +-1.75
        cx, cy = 3.0 + 5.5 * g, 10.0 + 1.5 * g
        put(cx, cy); put(cx + 1.25, cy); put(cx - 1.25, cy); put(cx + 1.75, cy, -1.0); put(cx - 1.75, cy, 1.0)
    for k in range(N - len(px)):
        put(1.0 + 4.0 * k, 15.0)
    px, py = np.asarray(px, F), np.asarray(py, F)
    return dict(px=px, py=py, vx=np.asarray(vx, F), vy=np.asarray(vy, F), gx=px.astype(np.float64), gy=py.astype(np.float64))


SCENES = {"clump": clump, "corner": corner, "mirror": mirror}


def apply(env, fld, sc, arena=None):
    """the scene into every arena of a handle or an oracle env (arena: into that one only); fld: the module that names its fields"""
    def put(name, v):
        cur = env.get(getattr(fld, "FLD_" + name))
        new = np.broadcast_to(np.asarray(v)[None, :], cur.shape).astype(cur.dtype)
        if arena is not None:
            row, new = new[arena], cur.copy()
            new[arena] = row
        env.set(getattr(fld, "FLD_" + name), np.ascontiguousarray(new))
    put("POS_X", sc["px"]); put("POS_Y", sc["py"]); put("VEL_X", sc["vx"]); put("VEL_Y", sc["vy"])
    put("GOAL_X", sc["gx"]); put("GOAL_Y", sc["gy"])


def actions(step, A=1):
    """the action of every agent at a step: straight for the goal, a seeded wobble every fourth step"""
    if step % 4:
        return np.zeros((A, N), F)
    return np.random.RandomState(100 + step).uniform(-0.2, 0.2, (A, N)).astype(F)


def oracle_env(name, K):
    env = H.make_oracle(1, N, "crowd", params(K), seed=5)
    apply(env, o, SCENES[name]())
    return env


def infeasible_per_step(name, K, steps=STEPS):
    """[(LP3_ENTERED, LP3_ENTERED_WITH_OBST_LINES, LP3_PARALLEL_OPPOSITE, LP3_PARALLEL_SAME_DIR)] of every serial step of the arena"""
    env = oracle_env(name, K)
    out = []
    for s in range(steps):
        o.branch_counts(reset=True)
        env.step(actions(s), flags=o.F_OBS | o.F_STATS)
        br = o.branch_counts(reset=True)
        out.append((br["LP3_ENTERED"], br["LP3_ENTERED_WITH_OBST_LINES"], br["LP3_PARALLEL_OPPOSITE"], br["LP3_PARALLEL_SAME_DIR"]))
    return out


# ---- the batch of tests/test_gpu_lp3_pairs.py: arena 0 the scene, arena 1 the scene under other actions, arena 2 the handle's own crowd ----
BATCH = 3
SEED = 5


def batch_actions(step):
    a = np.concatenate([actions(step), actions(step + 1), actions(step + 2)], axis=0)
    a[1] += F(0.05)
    return np.ascontiguousarray(a, dtype=F)


def batch_infeasible(name, K, steps=STEPS):
    """[steps][BATCH] LP3_ENTERED of each arena of that batch: every arena stepped as an oracle env of its own (the crowd of arena a
    is the one a handle of one arena draws at arena_offset = a), so that the thread's branch counters can be read per arena"""
    envs = [H.make_oracle(1, N, "crowd", params(K), seed=SEED, arena_offset=a) for a in range(BATCH)]
    for a in (0, 1):
        apply(envs[a], o, SCENES[name]())
    out = []
    for s in range(steps):
        act, row = batch_actions(s), []
        for a, env in enumerate(envs):
            o.branch_counts(reset=True)
            env.step(act[a:a + 1], flags=o.F_OBS | o.F_STATS)
            row.append(o.branch_counts(reset=True)["LP3_ENTERED"])
        out.append(row)
    return out
