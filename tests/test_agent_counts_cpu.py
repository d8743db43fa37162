"""The input guard of tests/test_gpu_agent_counts.py on the CPU oracle alone, and the parts of per-arena agent counts
(ca_set_agent_counts) that need no GPU: the scenes of tests/agent_count_scenes.py are not trivial -- full and short neighbour lists,
collisions, a new goal, arenas that end by arrival at steps of their own and one that the cap cuts --, the adapters present a
vector env with counts as the issue of heterogeneous crowds asks, and the header and the binding declare the calls."""
import inspect
import os
import re

import numpy as np
import pytest

from collision_avoidance_amd import _lib, scenarios
from oracle import oracle as o
from tests import agent_count_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(S.BOXES))
def test_box_scenes_fill_and_leave_lists_collide_and_regoal(name):
    A, N, counts, p, polys, sc, steps = S.box_scene(name)
    rag = S.RaggedOracleVec(N, counts, p, polys, S.BOXES[name][3])
    rag.set_scene(sc)
    rng = np.random.RandomState(S.BOX_ACTION_SEED)
    full = np.zeros(A, bool)
    short = np.zeros(A, bool)
    for s in range(steps):
        rag.step(rng.uniform(-1, 1, (A, N)).astype(np.float32), stats=True)
        nc = rag.get(_lib.FLD_NB_COUNT)
        for a, n in enumerate(counts):
            full[a] |= bool((nc[a, :n] == p["max_neighbors"]).any())
            short[a] |= bool((nc[a, :n] < p["max_neighbors"]).any())
            assert (nc[a, :n] <= n - 1).all()
    st = rag.arena_stats()
    print(name, "full lists", full, "short lists", short, "collisions", st["collisions"], "regoals", rag.get(_lib.FLD_REGOAL_COUNT).sum(axis=1))
    assert full.any() and short.all(), (full, short)                  # both kinds of list occur
    assert not full[np.asarray(counts) <= p["max_neighbors"]].any()   # an arena of n agents has lists of at most n - 1
    assert st["collisions"].sum() > 0 and rag.get(_lib.FLD_REGOAL_COUNT).sum() > 0
    assert st["obst_overflow"].sum() == 0


def test_arrival_scene_ends_arenas_at_steps_of_their_own():
    rag, p, px, py = S.arrival_oracles()
    counts = rag.agent_counts()
    end = np.full(rag.A, -1)
    for s in range(1, S.ARRIVAL_CAP + 1):
        for a, e in enumerate(rag.orc):
            if end[a] < 0:
                e.orca_step(flags=o.F_STATS)
                if e.get(o.FLD_ARENA_DONE)[0]:
                    end[a] = s
    st = rag.arena_stats()
    arrived = st["last_episode_arrived"]
    print("arenas end at", end, "with", arrived, "arrivals of", counts)
    assert (end > 0).all() and np.array_equal(st["last_episode_steps"], end)
    by_arrival = (end < S.ARRIVAL_CAP) & (arrived == counts)
    assert by_arrival.sum() >= 2 and len(set(end[by_arrival])) >= 2, (end, arrived)
    assert ((end == S.ARRIVAL_CAP) & (arrived < counts)).any(), (end, arrived)


def _adapter_vec():
    return S.RaggedOracleVec(S.ADAPTER_N, S.ADAPTER_COUNTS, S.adapter_params(), scenarios.obstacles("doorway", S.ADAPTER_N), S.ADAPTER_SEED,
                             scenario="doorway")


def test_multi_agent_adapter_holds_the_arenas_own_agents():
    S.check_multi_agent_adapter(_adapter_vec())


def test_agent_vector_adapter_marks_absent_slots():
    S.check_agent_vector_adapter(_adapter_vec())


def test_adapters_without_counts_are_what_they_were():
    """A vector env that knows nothing of counts (tests/helpers.py::OracleVec has no agent_counts()): every slot is active and
    truncated is arrived < N."""
    from collision_avoidance_amd.adapters import AgentVectorEnv
    from tests import helpers as H
    env = AgentVectorEnv(H.OracleVec(2, 4, "doorway", S.adapter_params(), seed=1))
    env.reset()
    for s in range(S.ADAPTER_CAP):
        _, _, _, infos = env.step(np.zeros(8, np.float32))
    assert infos["agent_active"].all() and len(infos["episode"]["arena"]) == 2
    assert np.array_equal(infos["episode"]["truncated"], infos["episode"]["arrived"] < 4)


def test_header_declares_the_calls_and_their_limits():
    h = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    for name in ("ca_set_agent_counts", "ca_get_agent_counts", "ca_agent_counts_info"):
        assert re.search(r"\bint %s\(ca_env\* env," % name, h) and name in _lib.EXPORTS, name
    doc = h[h.index("Arenas of different crowd sizes in one batch"):h.index("int ca_set_agent_counts")]
    for word in ("CA_ESIZE", "CA_ERANGE", "CA_EINVAL", "CA_SCN_DOORWAY", "ca_alan_step", "ca_set_agent_params", "agent_steps",
                 "rollout_one_launch = 0", "not a ca_field"):
        assert word in doc, word
    fields = h[h.index("enum ca_field {"):h.index("CA_FLD__COUNT")]
    assert len(re.findall(r"\bCA_FLD_\w+", fields)) == 26 and "COUNTS" not in fields      # configuration, not state


def test_vec_env_has_the_interface():
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv as V
    for name in ("set_agent_counts", "clear_agent_counts", "agent_counts", "agent_mask"):
        assert callable(getattr(V, name)), name
    assert "agent_counts" in inspect.signature(V.__init__).parameters
    with pytest.raises(ValueError):          # raised before the library is touched: the crowd's geometry is a function of n_agents
        V(2, 4, scenario="crowd", agent_counts=[1, 2])
