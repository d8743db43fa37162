"""Phase A of the observation kernel sends only the chord a ray ENTERS a neighbour's octagon by through the reference's arithmetic
wherever that decides the pair (csrc/ca_obs_chord.h, CA_OBS_ENTRY_CHORD): the agent outside the neighbour's circle, no vertex within
the filter's tolerance of the ray's line.  Every check here is the CPU oracle's observation bit for bit at the same state, at the
smallest shape that reaches each instantiation of obs_kernel, on hand-placed scenes around the rule's two conditions.

A scene is placed through ca_set, one ORCA step makes the neighbour lists, and ca_reset then puts the agents back on the crafted
positions -- new positions, the frame from position and goal, the observation from the lists of the last step (env.py:461-488).
The observer stands at the origin with its goal on the +x axis, so its frame is the world's and a neighbour's offset of 1e-8 from
a ray's line is a number fp32 holds."""
import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from oracle import oracle as o
from tests import agent_count_scenes as CS
from tests import helpers as H

pytestmark = pytest.mark.gpu

FLAGS = o.F_OBS | o.F_STATS
BOX = [[(-100.0, -100.0), (-100.0, 100.0), (100.0, 100.0), (100.0, -100.0)]]   # walls out of everybody's range
DELTAS = (1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 2e-4, 1e-3, 1e-2)   # the filter's tolerance is 7e-4 / |ray| = 1.4e-4 of distance at R = 0.5


def _parked(n):
    """agents that take no part: a grid of pitch 3, more than the range away from the scene"""
    k = np.arange(n)
    return np.stack([20.0 + 3.0 * (k % 20), -30.0 + 3.0 * (k // 20)], axis=1)


def _graze(R, d):
    """Ten agents around the observer 0 at the origin.  1: on ray 0, vertices 0 and 4 at d beside its line.  2, 3, 4: on rays 4, 8
    and 12, one vertex d INSIDE the ray's line (d > 0: a corner cut) or d beyond it (d < 0: the line misses the octagon)."""
    return np.array([(0.0, 0.0), (2.0, d), (R - d, -2.2), (-2.4, R - d), (-(R - d), 2.6),
                     (3.0, 3.0), (-3.0, 3.1), (-3.2, -3.0), (3.1, -3.3), (4.2, 1.7)])


def _overlap(R, turn):
    """1-2, 3-4, 5-6: a neighbour's centre at 0.9 R, 1.0 R and 1.03 R from the agent.  7: a neighbour whose octagon holds the end of
    the observer's ray 8 (centre at range - 0.6 R).  8, 9: two neighbours on ONE spot just inside the range -- the observer's ray 4
    ends inside both, at equal distances, which the first segment index wins."""
    u = lambda t: np.array([np.cos(t + turn), np.sin(t + turn)])
    a1, a3, a5 = np.array([3.0, 0.4]), np.array([0.5, 3.0]), np.array([-3.0, -2.0])
    return np.array([(0.0, 0.0), a1, a1 + 0.9 * R * u(0.3), a3, a3 + 1.0 * R * u(2.0), a5, a5 + 1.03 * R * u(4.0),
                     (-(5.0 - 0.6 * R), 0.0), (0.0, -4.999), (0.0, -4.999)])


def _base_overlap(R):
    """the overlap scene pulled apart for the ORCA step that makes the lists"""
    b = _overlap(R, 0.0)
    b[2], b[4], b[6], b[9] = b[1] + (1.3, 0.4), b[3] + (0.2, 1.4), b[5] + (-0.3, -1.4), b[8] + (1.5, 0.0)
    return b


def _scene(A, N, ten):
    """[A,N,2] positions: the ten scene agents in front, the rest parked; every arena the same"""
    pos = np.concatenate([ten, _parked(N - 10)]).astype(np.float32)
    return np.broadcast_to(pos, (A, N, 2)).copy()


def _state(A, N, pos):
    goal = pos.astype(np.float64) + (6.0, 0.0)            # straight along +x: every frame is the world's ...
    goal[:, 1::2] = pos[:, 1::2].astype(np.float64) * 0.5 + (1.0, -2.0)   # ... but every other agent's, which looks somewhere else
    return dict(pos=pos, vel=np.zeros((A, N, 2), np.float32), goal=goal, goal2=goal.copy())


class _Uniform(object):
    """a HIP env and ONE oracle of the same batch"""

    def __init__(self, A, N, **kw):
        self.p = scenarios.bench_params(N, 5.0, 10)
        self.g = H.make_gpu(A, N, "crowd", self.p, seed=4, polys=BOX, **kw)
        self.e = H.make_oracle(A, N, "crowd", self.p, seed=4, polys=BOX, **kw)
        self.R = [self.p["radius"]] * A

    def set_state(self, sc):
        CS.set_state(self.g, _lib, sc); CS.set_state(self.e, o, sc)

    def orca_step(self):
        self.g.orca_step(with_obs=True, stats=True); self.e.orca_step(flags=FLAGS)

    def reset(self, pos):
        self.g.reset(pos[..., 0], pos[..., 1]); self.e.reset(pos[..., 0], pos[..., 1], flags=o.F_OBS)

    def same(self, what):
        H.assert_state_equal(self.g, self.e, what, obs=True)

    def oracle_obs(self):
        return self.e.get(o.FLD_OBS)


class _Radii(_Uniform):
    """a HIP env with a radius per arena (ca_set_agent_params) and an oracle per arena"""

    def __init__(self, A, N):
        self.p = scenarios.bench_params(N, 5.0, 10)
        self.R = [0.3, 0.7, 0.45][:A]
        consts = dict(radius=np.asarray(self.R, np.float32))
        self.g = H.make_gpu(A, N, None, self.p, seed=4, polys=BOX)
        self.g.set_agent_params(**consts)
        self.rag = CS.RaggedOracleVec(N, (N,) * A, self.p, BOX, 4, S_cap=self.g.S, consts=consts)
        li = self.g.launch_info()
        assert li["agent_params"] and not li["agent_counts"], li

    def set_state(self, sc):
        CS.set_state(self.g, _lib, sc); self.rag.set_scene(sc)

    def orca_step(self):
        self.g.orca_step(with_obs=True, stats=True); self.rag.orca_step(FLAGS)

    def reset(self, pos):
        self.g.reset(pos[..., 0], pos[..., 1])
        for a, e in enumerate(self.rag.orc):
            e.reset(pos[a:a + 1, :, 0], pos[a:a + 1, :, 1], flags=o.F_OBS)

    def same(self, what):
        CS.same(self.g, self.rag, what, obs=True, reward=False)

    def oracle_obs(self):
        return self.rag.get(_lib.FLD_OBS)


def _make(kind):
    if kind == "headline":
        w = _Uniform(2, 16)
        assert w.g.launch_info()["obs_grid"] == 2                       # obs_kernel<256, false, false>: a workgroup per arena
    elif kind == "dense":
        w = _Uniform(3, 10)
        assert w.g.launch_info()["obs_grid"] == 2                       # DENSE: 30 agents of three arenas in two workgroups
    elif kind == "gather":
        w = _Uniform(1, 272)
        assert w.g.launch_info()["obs_grid"] == 17                      # 16-bit ids: the neighbours are gathered
    elif kind == "radii":
        w = _Radii(2, 16)
    else:
        w = _Uniform(2, 16, max_obst_neighbors=24)                      # WideObstLists
        assert w.g.S == 24
    return w


def _scene_of(w, A, N, fn):
    pos = np.stack([_scene(1, N, fn(w.R[a]))[0] for a in range(A)])
    return pos


KINDS = ["headline", "dense", "gather", "radii", "wide"]


@pytest.mark.parametrize("kind", KINDS)
def test_vertex_beside_a_rays_line_and_corner_cuts(kind):
    w = _make(kind)
    A, N = w.g.A, w.g.N
    w.set_state(_state(A, N, _scene_of(w, A, N, lambda R: _graze(R, 0.3))))
    w.orca_step()
    w.same("%s graze lists" % kind)
    cut = missed = 0
    for d in DELTAS:
        for sign in (1.0, -1.0):
            pos = _scene_of(w, A, N, lambda R: _graze(R, sign * d))
            w.reset(pos)
            w.same("%s vertex %g beside the line" % (kind, sign * d))
            obs = w.oracle_obs().reshape(A, N, 16, 4)[:, 0]              # the observer's rays
            assert (obs[:, 0, 0] > 1.0).all() and (np.abs(obs[:, 0, 0] - (2.0 - np.asarray(w.R))) < 0.05).all(), obs[:, 0]   # ray 0 meets 1
            hit = (obs[:, [4, 8, 12], :2] != 0).any(axis=2)              # rays 4, 8, 12: a corner cut, or nothing
            cut += hit.sum(); missed += (~hit).sum()
    assert cut > 0 and missed > 0, (cut, missed)
    w.g.close()


@pytest.mark.parametrize("kind", KINDS)
def test_agent_at_the_circle_ray_ends_inside_and_equal_distances(kind):
    w = _make(kind)
    A, N = w.g.A, w.g.N
    w.set_state(_state(A, N, _scene_of(w, A, N, _base_overlap)))
    w.orca_step()
    w.same("%s overlap lists" % kind)
    for turn in (0.0, np.pi / 8, 1.0):
        pos = _scene_of(w, A, N, lambda R: _overlap(R, turn))
        w.reset(pos)
        w.same("%s overlap, turned by %g" % (kind, turn))
        obs = w.oracle_obs().reshape(A, N, 16, 4)
        far = 5.0 - 1.6 * np.asarray(w.R)                                  # ray 8 meets 7's near side, and ends inside it
        assert (np.abs(obs[:, 0, 8, 0] + far) < 0.1).all() and (obs[:, 0, 4, 1] < -4.0).all(), (obs[:, 0, 8], obs[:, 0, 4])
        for k in (2, 4, 6):                                                # whoever stands inside an octagon sees it on every ray
            inside = np.hypot(*(pos[:, k] - pos[:, k - 1]).T) < 0.92 * np.asarray(w.R)
            assert ((np.abs(obs[:, k, :, :2]).max(axis=2) > 0).all(axis=1) | ~inside).all(), k
    w.g.close()


def test_overlapping_crowd_of_64_for_200_steps_with_automatic_reset():
    """uniform starts overlap; a cap of 70 steps ends every episode twice, and the new one starts on top of each other again"""
    A, N = 2, 64
    p = dict(scenarios.alan_params(N, "crowd"), max_step=70)
    g, e = H.make_gpu(A, N, "crowd", p, seed=0), H.make_oracle(A, N, "crowd", p, seed=0)
    assert g.launch_info()["obs_grid"] == A * 4
    rng = np.random.RandomState(3)
    for s in range(200):
        act = rng.uniform(-0.5, 0.5, (A, N)).astype(np.float32)
        g.step(act, stats=True, autoreset=True); e.step(act, flags=FLAGS | o.F_AUTORESET)
        H.assert_state_equal(g, e, "crowd step %d" % s, obs=True)
    assert e.stats()["episodes"] >= 2 * A, e.stats()
    g.close()
