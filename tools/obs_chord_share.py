#!/usr/bin/env python3
"""Diagnostic: in how many of phase A's pair trips does a whole wave of obs_kernel take the entry-chord path (csrc/ca_obs_chord.h)?
Builds the CA_STAMPS variant of the library into variants/ (never the product build; `build` as the only argument stops there),
settles the bench workload's crowd and reads the three counts every wave leaves behind its time stamps (ca_obs.h): pair trips,
trips whose lanes all qualify, trips that ran the two-chord block.  Usage (GPU box): python tools/obs_chord_share.py [C3|C2|C5]"""
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
env.L.ca_debug_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
rng = np.random.RandomState(0)
for settle, what in ((0, "young crowd (after the first step)"), (int(os.environ.get("CA_STAMPS_WARM", "3000")), "settled crowd")):
    if settle:
        env.rollout(settle, stats=True)
    env.step(rng.uniform(-0.5, 0.5, (A, N)).astype(np.float32), with_obs=True, stats=True)
    nw = C.c_int32()
    buf = np.zeros((A * ((N + 15) // 16 + 16) * 4, 16), np.uint64)
    env._call("ca_debug_stamps", env.h, buf.ctypes.data, -buf.shape[0], C.byref(nw))
    trips, fast, two = (int(buf[:nw.value, k].sum()) for k in (9, 10, 11))
    print("%s %s: %d waves, %d pair trips; every lane on the entry-chord path in %d (%.1f %%); the two-chord block ran in %d (%.1f %%)"
          % (wl, what, nw.value, trips, fast, 100.0 * fast / max(trips, 1), two, 100.0 * two / max(trips, 1)))
