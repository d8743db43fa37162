#!/usr/bin/env python3
"""What the policy kernels give at the edges of fp32: the scenes of tests/policy_edge_scenes.py -- the ones
tests/test_gpu_policy_edges.py asserts on -- through policy_kernel<false> (policy_actions, noise off and on) and policy_kernel<true>
(policy_evaluate, its five outputs, eps off and on), out = identity, against the numpy restatement.  One line per class and kernel:
values compared, values whose bits differ, and, where the definition gives NaNs, places where only one side has one (a NaN's payload
and sign are not defined and not counted).

  python tools/policy_edges_report.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collision_avoidance_amd import _lib, build as b, scenarios  # noqa: E402
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv  # noqa: E402
from tests import policy_edge_scenes as E  # noqa: E402
from tests import policy_scenes as PS  # noqa: E402
from tests import ppo_scenes as PP  # noqa: E402

OUTS = ("actions", "logp", "value", "mean", "log_std")


def count(got, want):
    """(compared, bits differ outside NaNs, NaN on one side only)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    both = ~gn & ~wn
    return got.size, int((got.view(np.uint32) != want.view(np.uint32))[both].sum()), int((gn != wn).sum())


def run(name):
    sc, _ = E.SCENES[name][0]()
    A, N = sc.obs.shape[:2]
    g = VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.alan_params(N, "crowd"), seed=1, use_torch=False)
    g.set(_lib.FLD_OBS, sc.obs)
    Ws, bs = E.restated(sc)
    value, log_std = sc.heads
    g.set_policy(sc.layers, sets=sc.sets)
    plain, heads = np.zeros(3, np.int64), np.zeros(3, np.int64)
    with np.errstate(all="ignore"):
        for nz in (None, sc.eps):
            plain += count(g.policy_actions(nz), PS.actions_reference(sc.obs, Ws, bs, sc.sets, nz))
        g.set_policy_heads(value=value, log_std=log_std)
        for nz in (None, sc.eps):
            got, want = g.policy_evaluate(nz), PP.evaluate_reference(sc.obs, Ws, bs, sc.sets, value, log_std, nz)
            for n in OUTS:
                heads += count(got[n], want[n])
    g.close()
    return plain, heads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = ["policy kernels against the restatement at the edges of fp32 (tools/policy_edges_report.py)",
             "library source sha %s (loaded %s)" % (b.source_sha(), b.loaded_sha()),
             "%-14s %-22s %10s %10s %14s" % ("class", "kernel", "compared", "differ", "NaN one side")]
    for name in E.SCENES:
        plain, heads = run(name)
        for kernel, c in (("policy_kernel<false>", plain), ("policy_kernel<true>", heads)):
            lines.append("%-14s %-22s %10d %10d %14d" % (name, kernel, c[0], c[1], c[2]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
