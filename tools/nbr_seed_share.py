#!/usr/bin/env python3
"""Diagnostic: for how many candidates does a wave of the seeded neighbour scan (csrc/ca_nbr.h, CA_NBR_SEED) still run the insertion
network?  Builds the CA_STAMPS variant of the library into variants/ (never the product build; `build` as the only argument stops
there), runs the bench workload's crowd and reads the two counts every solve wave leaves in the row behind the launch's time stamps
(ca_debug_stamps): candidate trips, and trips that ran the network.  Three states: the first step of a fresh handle (every seed
empty), a young crowd (step 20), the settled crowd the bench times.  Usage (GPU box): python tools/nbr_seed_share.py [C3|C2]"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from collision_avoidance_amd import build as b

out = os.path.join(ROOT, "variants", "libcaenv_stamps1.so")
os.makedirs(os.path.dirname(out), exist_ok=True)
if not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in b.SOURCES):
    subprocess.check_call([b.hipcc()] + b.HIPCC_FLAGS + ["-DCA_STAMPS=1", "-o", out, b.SOURCES[0]])
if len(sys.argv) > 1 and sys.argv[1] == "build":
    raise SystemExit(0)
b.LIB_PATH = out  # the loader reads this
from collision_avoidance_amd import scenarios
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv

wl = sys.argv[1] if len(sys.argv) > 1 else "C3"
w = scenarios.BENCH_CONFIGS[wl]
A, N = w["n_arenas"], w["n_agents"]
env = VecCollisionAvoidanceEnv(A, N, "crowd", scenarios.bench_params(N, w["neighbor_dist"], w["max_neighbors"]), use_torch=False)
if env.launch_info()["lanes_per_agent"] != 1 or env.launch_info()["block"] != 64:
    raise SystemExit("%s does not run the one-wave solve kernel: %s" % (wl, env.launch_info()))
env.L.ca_debug_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
rng = np.random.RandomState(0)
done = 0
for upto, what in ((0, "first step of a fresh handle"), (20, "young crowd (step 21)"),
                   (int(os.environ.get("CA_STAMPS_WARM", "3000")), "settled crowd")):
    if upto > done:
        env.rollout(upto - done, stats=True)
        done = upto
    env.step(rng.uniform(-0.5, 0.5, (A, N)).astype(np.float32), with_obs=False, stats=True)
    done += 1
    nw = C.c_int32()
    buf = np.zeros((2 * env.launch_info()["grid"], 16), np.uint64)   # (one wave per workgroup: rows [0, grid) are the time stamps)
    env._call("ca_debug_stamps", env.h, buf.ctypes.data, buf.shape[0], C.byref(nw))
    assert 2 * nw.value == buf.shape[0], (nw.value, buf.shape)
    trips, ran = buf[nw.value:, 0].astype(np.int64), buf[nw.value:, 1].astype(np.int64)
    print("%s %s: %d waves, %d candidate trips; the network ran in %d (%.2f %%): per wave mean %.2f, p50 %d, p90 %d, max %d of %d"
          % (wl, what, nw.value, trips.sum(), ran.sum(), 100.0 * ran.sum() / max(trips.sum(), 1), ran.mean(),
             np.percentile(ran, 50), np.percentile(ran, 90), ran.max(), trips.max()))
