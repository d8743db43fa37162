"""The per-agent contact report without a device: (a) the numpy fp32 restatement that the GPU tests compare the kernel with
(tests/contact_scenes.py) against the unchanged CPU oracle's per-arena collision totals; (b) the header, the ctypes binding and the
Python interface; (c) the compiled kernel's resources."""
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from collision_avoidance_amd import _lib, adapters, build as B
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
from oracle import oracle as o
from tests import contact_scenes as CS
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ca_env.h")


# ---- (a) the restatement against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N,min_touch,min_wall", [(3, 64, 1000, 100), (7, 10, 100, 100)], ids=["doorway3x64", "doorway7x10"])
def test_restatement_sums_to_the_oracles_per_arena_totals(A, N, min_touch, min_wall):
    """Every step of 30, every arena: sum_i agents[a, i] == 2 x the pairs and sum_i wall[a, i] == the wall hits that the oracle's
    arena_collisions counted for that state (CA_F_STATS).  The floors keep the test from passing on an empty scene."""
    p = H.scenario_params("doorway", N)
    orc = H.make_oracle(A, N, "doorway", p, seed=3)
    tabs = CS.tables_of(orc, A)
    prev = orc.get(o.FLD_ARENA_STATS).copy()
    touches = walls = 0
    for s, act in CS.doorway_actions(A, N, 3, 30):
        orc.step(act, flags=o.F_STATS)
        px, py = orc.get(o.FLD_POS_X), orc.get(o.FLD_POS_Y)
        st = orc.get(o.FLD_ARENA_STATS).copy()
        rep = CS.reference(px, py, p["radius"], tabs)
        np.testing.assert_array_equal(rep["agents"].sum(1), 2 * (st[:, 1] - prev[:, 1]).astype(np.int64), "step %d: pairs" % s)
        np.testing.assert_array_equal(rep["wall"].sum(1), (st[:, 2] - prev[:, 2]).astype(np.int64), "step %d: walls" % s)
        # the planes agree with each other: an agent that touches somebody has its nearest neighbour within 2 R
        hit = rep["agents"] > 0
        assert (rep["nearest_d2"][hit] < np.float32(2 * p["radius"]) ** 2).all()
        assert ((rep["wall_d2"] < np.float32(p["radius"]) ** 2) == (rep["wall"] != 0)).all()
        touches += int(rep["agents"].sum()); walls += int(rep["wall"].sum())
        prev = st
    print("doorway %d x %d: %d touches, %d wall touches" % (A, N, touches, walls))
    assert touches >= min_touch and walls >= min_wall, (touches, walls)


def test_restatement_on_hand_made_states():
    """what the hand-made scenes of the GPU tests are meant to show, stated as numbers"""
    px, py = CS.boundary_pairs(0.5)
    r = CS.reference(px, py, 0.5, np.zeros((0, 4), np.float32))
    assert r["agents"][0].tolist() == [0, 0, 1, 1, 0, 0, 2, 2, 2]            # at: no; one ulp inside: yes; outside: no; coincident
    assert r["nearest"][0].tolist() == [1, 0, 3, 2, 5, 4, 7, 6, 6] and (r["nearest_d2"][0, 6:] == 0).all()
    assert (r["wall"] == 0).all() and np.isinf(r["wall_d2"]).all()
    px, py, rad = CS.nearest_cases()
    r = CS.reference(px, py, rad, np.zeros((0, 4), np.float32))
    assert r["nearest"][0, 0] == 1 and r["nearest_d2"][0, 0] == np.float32(1.8125)   # tie with agent 2
    assert r["nearest"][0, 3] == 4 and r["agents"][0].tolist() == [0, 0, 0, 1, 0, 1]  # 3 touches 5, its nearest is 4
    px, py = CS.wall_cases(0.5)
    tab = CS.table_edges(dict(verts=np.float32([[0, 0], [4, 0], [10, 0], [10, 4]]), next=[1, 0, 3, 2]))
    r = CS.reference(px, py, 0.5, tab)
    assert r["wall"][0].tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0]
    one = CS.reference(np.float32([[1.0]]), np.float32([[2.0]]), 0.5, tab)
    assert one["nearest"][0, 0] == -1 and np.isinf(one["nearest_d2"][0, 0]) and one["agents"][0, 0] == 0
    # absent rows on top of present agents: counted by nobody, and they report the empty row
    px, py = np.zeros((1, 4), np.float32), np.zeros((1, 4), np.float32)
    r = CS.reference(px, py, 0.5, tab, counts=[2])
    assert r["agents"][0].tolist() == [1, 1, 0, 0] and r["nearest"][0].tolist() == [1, 0, -1, -1]
    assert r["wall"][0].tolist() == [1, 1, 0, 0] and np.isinf(r["wall_d2"][0, 2:]).all() and np.isinf(r["nearest_d2"][0, 2:]).all()


# ---- (b) header, binding, interface -----------------------------------------------------------------------------------------------
def test_header_declares_the_contact_calls():
    text = open(HEADER).read()
    assert re.search(r"^#define CA_F_CONTACT 32u\b", text, re.M)
    flat = " ".join(text.split())
    assert "int ca_contacts(ca_env* env);" in flat
    assert ("int ca_get_contacts(ca_env* env, int32_t* agents, int32_t* wall, int32_t* nearest, float* nearest_d2, float* wall_d2, "
            "size_t bytes_each, int32_t dst_is_device);") in flat
    assert "int ca_contacts_ptr(ca_env* env, void** dev_ptr, size_t* bytes);" in flat
    block = text[text.index("enum ca_field {"):text.index("CA_FLD__COUNT")]
    assert len(re.findall(r"\bCA_FLD_\w+", block)) == 26 and "contact" not in block.lower()   # the report is no field


def test_binding_names_the_contact_calls():
    assert _lib.F_CONTACT == 32
    assert {"ca_contacts", "ca_get_contacts", "ca_contacts_ptr"} <= set(_lib.EXPORTS)
    assert os.path.join(os.path.dirname(B.LIB_PATH), "csrc", "ca_contact.h") in B.SOURCES   # the source hash covers the kernel
    src = inspect.getsource(_lib.load)
    for name in ("ca_contacts", "ca_get_contacts", "ca_contacts_ptr"):
        assert "L.%s.argtypes" % name in src


def test_interface_keywords_default_off():
    V = VecCollisionAvoidanceEnv
    for name in ("step", "orca_step", "rollout", "alan_step", "alan_rollout", "reset", "reset_masked", "step_packed"):
        par = inspect.signature(getattr(V, name)).parameters
        assert "contacts" in par and par["contacts"].default is False, name
    assert callable(V.contacts) and callable(V.last_contacts)
    assert "contacts" not in V._STATE_FIELDS and not any("CONTACT" in n for n in V._STATE_FIELDS)   # the report is not state
    from collision_avoidance_amd import envs
    for cls in (adapters.AgentVectorEnv, adapters.MultiAgentVectorEnv, envs.Collision_Avoidance_Env):
        par = inspect.signature(cls.__init__).parameters
        assert "contacts" in par and par["contacts"].default is False, cls


class _ContactVec(H.OracleVec):
    """OracleVec whose step() takes contacts=True and returns a hand-made report as its infos"""

    def __init__(self, *a, **kw):
        H.OracleVec.__init__(self, *a, **kw)
        self.report, self.asked = None, []

    def step(self, actions, with_obs=True, stats=False, autoreset=False, contacts=False):
        out = H.OracleVec.step(self, actions, with_obs=with_obs, stats=stats, autoreset=autoreset)
        self.asked.append(contacts)
        return out[:3] + (({"contacts": self.report} if contacts else {}),)


def _hand_made(A, N):
    rep = dict(agents=np.zeros((A, N), np.int32), wall=np.zeros((A, N), np.int32), nearest=np.full((A, N), -1, np.int32),
               nearest_d2=np.full((A, N), np.inf, np.float32), wall_d2=np.full((A, N), np.inf, np.float32))
    rep["agents"][0, 1], rep["nearest"][0, 1], rep["nearest_d2"][0, 1] = 2, 0, 0.25
    rep["wall"][1, 2], rep["nearest"][1, 2], rep["nearest_d2"][1, 2] = 1, 0, 9.0
    return rep


def test_adapter_infos_carry_the_report():
    A, N = 2, 3
    p = H.scenario_params("doorway", N, max_step=40)
    vec = _ContactVec(A, N, "doorway", p, seed=1)
    vec.report = _hand_made(A, N)
    env = adapters.AgentVectorEnv(vec, contacts=True)
    env.reset()
    _, _, _, info = env.step(np.zeros((A * N, 1), np.float32))
    assert vec.asked == [True]
    assert info["agent_contact"].dtype == bool and info["agent_contact"].tolist() == [False, True, False, False, False, True]
    assert info["agent_touching"].tolist() == [0, 2, 0, 0, 0, 0]
    assert info["agent_nearest_d2"].shape == (A * N,) and info["agent_nearest_d2"][1] == np.float32(0.25)
    assert np.isinf(info["agent_nearest_d2"][[0, 2, 3, 4]]).all()            # absent / lone slots read inf
    # default: the keyword is not passed on and the infos are the old ones
    plain_vec = H.OracleVec(A, N, "doorway", p, seed=1)
    plain = adapters.AgentVectorEnv(plain_vec)
    plain.reset()
    _, _, _, info0 = plain.step(np.zeros((A * N, 1), np.float32))
    assert not any(k in info0 for k in ("agent_contact", "agent_touching", "agent_nearest_d2"))

    vec2 = _ContactVec(A, N, "doorway", p, seed=1)
    vec2.report = _hand_made(A, N)
    menv = adapters.MultiAgentVectorEnv(vec2, contacts=True)
    obs = menv.vector_reset()
    _, _, _, infos = menv.vector_step([{aid: [0.0] for aid in ob} for ob in obs])
    assert infos[0]["agent_1"] == dict(contact=True, nearest_d2=0.25) and infos[0]["agent_0"]["contact"] is False
    assert infos[1]["agent_2"] == dict(contact=True, nearest_d2=9.0) and infos[1]["agent_0"]["nearest_d2"] == float("inf")
    assert "__common__" in infos[0]
    menv0 = adapters.MultiAgentVectorEnv(H.OracleVec(A, N, "doorway", p, seed=1))
    obs = menv0.vector_reset()
    _, _, _, infos0 = menv0.vector_step([{aid: [0.0] for aid in ob} for ob in obs])
    assert infos0[0]["agent_0"] == {}


# ---- (c) the compiled kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_contact_kernel_uses_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    KR.ensure_asm()
    rows = [r for r in KR.parse() if "contact_kernel" in r["name"]]
    assert len(rows) == 1, [r["name"] for r in rows]           # one kernel text for all handles
    r = rows[0]
    print("contact_kernel: %d VGPRs, %d SGPRs, %d B LDS, %d B code" % (r["vgpr"], r["sgpr"], r["lds"], r["code_bytes"]))
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == 3 * 256 * 4, r
