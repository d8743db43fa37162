"""The programmes whose answer leaves the speed disc, by value.

In the run recorded at the bench's shape (tests/golden/env_n64_k10.npz: 64 agents in the 5 x 10 spawn box, ~100 overlapping
pairs per step, every list full) the ORCA solver returns speeds above maxSpeed + 1e-4 on 0.9 % of the agent-steps, up to
1.2073; the same run with its reset() taken 50 steps earlier (tests/golden/overspeed_n64_k10.npz keeps the agent-steps after
it) meets a programme whose answer is 31.99.  Every such agent-step is rebuilt here as a one-agent scene (the focus agent, its
ten nearest within 5.0, the doorway polygons, the previous step's positions and velocities, this step's preferred velocity) and

  * the oracle's simulator reproduces the recorded velocity bit for bit from that scene;
  * the programme is infeasible and at least one neighbour overlaps the focus agent (tests/orca_geometry.py): a feasible
    programme, or one without overlap, above maxSpeed + 1e-4 is a defect and fails;
  * LP1 / LP2 / LP3 in the operation order of SURVEY App. A.5, restated in numpy fp64 (tests/orca_lp.py) and run on the fp32 half-planes the
    oracle captured, stays on the disc (1e-9) and meets the optimum of tests/orca_geometry.solve_minimal_penetration (1e-5,
    the by-value test's limit): the algorithm is right and the overshoot is fp32 rounding of that operation order.  Where:
    LP3 intersects line i with every earlier line j; two nearly parallel lines of overlapping neighbours (|point| up to 30)
    meet up to 1e5 from the origin, and LP1's discriminant dp^2 + r^2 - |point|^2 then cancels to a value whose fp32 error
    (an ulp of 1e10 is 1024) exceeds r^2, so the "circle" it cuts the line with is tens of units wide.  The table
    (CA_OVERSPEED_TABLE=<path>, committed as profiles/r07_overspeed_states.txt) lists per state the speed next to the
    largest |point| among LP3's projected lines;
  * each fp32 answer is held to what that cancellation can account for at ITS OWN `far` (tests/orca_lp.py fp32_limits:
    |v|^2 <= r^2 + 14 * 2^-24 * far^2, i.e. 2.0 for the 1.2073 of fixture A and 67 for the 31.99 of run B); the seeded
    dense-overlap scenes of tests/test_oracle_orca_definition.py are held to the same function.

RVO2 does not clamp the result, and neither does this project."""
import os

import numpy as np

from collision_avoidance_amd import scenarios
from tests import orca_geometry as G
from tests import orca_scenes as S
from tests.orca_lp import fp32_limits, solve_published_f64

HEADLINE = "env_n64_k10.npz"
EXTRA = "overspeed_n64_k10.npz"


def _one_agent_scene(pos, vel, pref, i, nd, K, polys):
    """the neighbours doStep listed for agent i: the nearest K strictly within nd, ties by index"""
    d = pos - pos[i]                                                  # fp32, as the simulator measures it
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    d2[i] = np.inf
    idx = [i] + [int(j) for j in np.argsort(d2, kind="stable") if d2[j] < np.float32(nd) * np.float32(nd)][:K]
    return S._scene("recorded", polys, pos[idx], vel[idx], pref[idx])


def recorded_states(golden_dir):
    """(label, scene, recorded velocity) of every recorded agent-step with |v| > maxSpeed + 1e-4.  A scene is what doStep saw:
    positions and velocities left by the step before (the start state before step 0, reset()'s positions in the step that
    follows it), the preferred velocity step() set before doStep (an orca_step runs on the one left by the step before)."""
    g = np.load(os.path.join(golden_dir, HEADLINE))
    polys = scenarios.obstacles("doorway", int(g["n_agents"]))
    nd, K = float(g["neighbor_dist"]), int(g["max_neighbors"])
    resets = {int(t): k for k, t in enumerate(g["reset_steps"])}
    speed = np.hypot(g["vel"][..., 0].astype(np.float64), g["vel"][..., 1].astype(np.float64))
    out = []
    for s, i in np.argwhere(speed > S.VMAX + 1e-4):
        pos = g["reset_pos"][resets[s]] if s in resets else (g["pos0"] if s == 0 else g["pos"][s - 1])
        vel = g["vel0"] if s == 0 else g["vel"][s - 1]
        pref = g["pref"][s] if g["kind"][s] == 0 else (g["pref0"] if s == 0 else g["pref"][s - 1])
        out.append(("%s %3d %2d" % ("A", s, i), _one_agent_scene(pos, vel, pref, int(i), nd, K, polys), g["vel"][s, i]))
    n_a, total = len(out), speed.size
    h = np.load(os.path.join(golden_dir, EXTRA))       # the same run with its reset() at step 150: states after it
    for k in range(len(h["step"])):
        sc = _one_agent_scene(h["pos"][k], h["vel"][k], h["pref"][k], int(h["agent"][k]), float(h["neighbor_dist"]),
                              int(h["max_neighbors"]), polys)
        out.append(("%s %3d %2d" % ("B", h["step"][k], h["agent"][k]), sc, h["new_vel"][k]))
    return out, n_a, total, speed


def _planes(cap):
    """captured lines -> (hard, soft) half-planes (point, inward normal) in fp64"""
    L = cap["lines"].astype(np.float64)
    hp = [(l[:2], np.array([-l[3], l[2]])) for l in L]
    return hp[:cap["n_obst_lines"]], hp[cap["n_obst_lines"]:]


def examine(sc, got32):
    """One programme by value -> dict(kinds, feasible, speed32, speed64, rel32, rel64, far, z)."""
    f = sc["focus"]
    got_v, cap, sim = S.run_oracle_sim(sc)
    assert (got_v.astype(np.float32) == got32).all() if got32 is not None else True, (got_v, got32)
    P, V = sc["pos"].astype(np.float64), sc["vel"].astype(np.float64)
    order = sorted((j for j in range(len(P)) if j != f), key=lambda j: (float(np.sum((P[j] - P[f]) ** 2)), j))
    kinds = [G.agent_halfplane(P[f], V[f], P[j], V[j], S.R, S.R, S.TAU, S.DT)[1] for j in order]
    hard, soft = _planes(cap)
    pref = sc["pref"][f].astype(np.float64)
    out = dict(kinds=kinds, feasible=G.solve_feasible(hard + soft, pref, S.VMAX) is not None, speed32=float(np.linalg.norm(got_v)),
               v32=got_v, n_lines=len(hard) + len(soft))
    v64, infeasible, far = solve_published_f64(cap["lines"], cap["n_obst_lines"], pref, S.VMAX)
    far = max(far, float(np.hypot(cap["lines"][:, 0], cap["lines"][:, 1]).max()))      # ... and among the captured lines themselves
    out.update(speed64=float(np.linalg.norm(v64)), far=far, infeasible64=infeasible)
    if not out["feasible"] and soft:
        z = G.solve_minimal_penetration(hard, soft, S.VMAX)[0]
        pen = lambda v: max(float(-(v - x0) @ nn) for x0, nn in soft)
        out.update(z=z, rel32=(pen(got_v) - z) / max(1.0, abs(z)), rel64=(pen(v64) - z) / max(1.0, abs(z)),
                   hard32=min([float((got_v - x0) @ nn) for x0, nn in hard] + [1.0]),
                   hard64=min([float((v64 - x0) @ nn) for x0, nn in hard] + [1.0]))
    return out


def test_recorded_overspeed_programmes_by_value(golden_dir):
    states, n_a, total, speed = recorded_states(golden_dir)
    assert n_a >= 100 and len(states) - n_a >= 10, (n_a, len(states))       # the recordings reach the regime
    n_a_over_1pc = int((speed > 1.01 * S.VMAX).sum())
    rows, worst = [], dict(over=0.0, below=0.0, above=0.0, over64=0.0, rel64=0.0, hard=0.0)
    for label, sc, recorded in states:
        r = examine(sc, recorded)                   # (asserts that the scene reproduces the recorded velocity bit for bit)
        n_coll = sum(k == "collision" for k in r["kinds"])
        # the condition: only an infeasible programme with an overlapping neighbour may leave the disc
        assert not r["feasible"] and n_coll >= 1, (label, r)
        # the reference of this item: the same operations in fp64 stay on the disc and meet the optimum
        assert r["infeasible64"] and r["speed64"] <= S.VMAX + 1e-9, (label, r)
        assert abs(r["rel64"]) <= 1e-5 and r["hard64"] >= -1e-9, (label, r)
        # fp32: what rounding of that order can account for at this programme's `far` (tests/orca_lp.py), not more
        lim_over, lim_below, lim_above = fp32_limits(r["far"], r["z"], S.VMAX)
        assert r["speed32"] - S.VMAX <= lim_over and -lim_below <= r["rel32"] <= lim_above and r["hard32"] >= -1e-5 - 4 * 2.0 ** -24 * r["far"], (
            label, r, lim_over, lim_below, lim_above)
        worst["over"] = max(worst["over"], r["speed32"] - S.VMAX)
        worst["below"] = max(worst["below"], -r["rel32"]); worst["above"] = max(worst["above"], r["rel32"])
        worst["over64"] = max(worst["over64"], r["speed64"] - S.VMAX); worst["rel64"] = max(worst["rel64"], abs(r["rel64"]))
        worst["hard"] = max(worst["hard"], -r["hard32"])
        rows.append("%-8s %9d %9d  %12.6f  %12.6f  %12.3e  %12.3e  %12.3e  %12.3e" % (
            label, n_coll, r["n_lines"], r["speed32"], S.VMAX + lim_over, r["far"], r["rel32"], r["speed64"] - S.VMAX, r["rel64"]))
    head = ["# agent-steps with |v| > maxSpeed + 1e-4.  A: tests/golden/env_n64_k10.npz, %d of %d (%.2f %%); above 1.001: %d, above 1.02: %d." % (
                n_a, total, 100.0 * n_a / total, int((speed > 1.001).sum()), int((speed > 1.02).sum())),
            "# B: tests/golden/overspeed_n64_k10.npz (the same run with its reset() at step 150; the steps after it), %d." % (len(states) - n_a),
            "# Written by tests/test_oracle_overspeed.py::test_recorded_overspeed_programmes_by_value.  Every one is an infeasible programme with",
            "# overlapping neighbours, reproduced bit for bit as a one-agent scene.  fp32 = the oracle (= the kernels); fp64 = LP1 / LP2 / LP3 in",
            "# the same operation order in numpy fp64 on the oracle's fp32 half-planes.  far = largest |point| among LP3's projected lines;",
            "# rel = (largest penetration - fp64 optimum) / max(1, optimum): negative = less penetration than any point of the disc allows.",
            "# worst: fp32 |v| - maxSpeed %.6g, fp32 rel %.3g below / %.3g above, fp32 hard-constraint violation %.3g; fp64 |v| - maxSpeed %.3g, fp64 |rel| %.3g" % (
                worst["over"], worst["below"], worst["above"], worst["hard"], worst["over64"], worst["rel64"]),
            "# limit = maxSpeed + what the fp32 roundings of LP1's discriminant at |point| = far can add (tests/orca_lp.py fp32_limits).",
            "run step agent  overlaps  lines   fp32 |v|      limit         far           fp32 rel      fp64 |v|-max  fp64 rel"]
    table = "\n".join(head + rows) + "\n"
    print(table)
    if os.environ.get("CA_OVERSPEED_TABLE"):
        with open(os.environ["CA_OVERSPEED_TABLE"], "w") as fh:
            fh.write(table)
    assert worst["over"] > 30.0 and n_a_over_1pc >= 3, (worst, n_a_over_1pc)      # the recordings hold the regime they are kept for
