#!/usr/bin/env python3
"""Diagnostic: how many LP3 pool rounds does a wave of the one-wave register-line solve kernel take, and what do they cost?  The
direct check of the premise of the paired LP3 round (csrc/ca_lp.h lp3_pair_lds, CA_LP3_PAIRS): a second four-lane round costs a wave
nearly as much as the first.  Builds the CA_STAMPS variant of the library into variants/ (never the product build; `build` as the only
argument stops there), settles the bench workload's crowd on a handle made with CA_LP3_PAIRS=0 (the kernel without the tag: before)
and on one made with CA_LP3_PAIRS=1 (the twin: after), and reads from the last steps' stamps (ca_debug_stamps) the cycles between
the stamps around "LP3+integrate" and, in slot 2 of the wave's row behind the stamps, the round counts (csrc/ca_step.h): loop trips of
the four-lane rounds including the closing one, paired rounds << 16, waiting lanes summed over the trips << 32.
Usage (GPU box): python tools/lp3_rounds.py [C3]"""
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
WARM = int(os.environ.get("CA_STAMPS_WARM", "3000"))
SAMPLES = 8   # timed steps read, one launch each


def run(pairs):
    os.environ["CA_LP3_PAIRS"] = pairs
    env = VecCollisionAvoidanceEnv(A, N, "crowd", scenarios.bench_params(N, w["neighbor_dist"], w["max_neighbors"]), use_torch=False)
    del os.environ["CA_LP3_PAIRS"]
    info = env.launch_info()
    if info["lanes_per_agent"] != 1 or info["block"] != 64:
        raise SystemExit("%s does not run the one-wave solve kernel: %s" % (wl, info))
    has = hasattr(env, "lp3_pairs_info") and env.lp3_pairs_info()
    env.L.ca_debug_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    rng = np.random.RandomState(0)
    env.rollout(WARM, stats=True)
    four, paired, lp3, whole = [], [], [], []
    for _ in range(SAMPLES):
        env.step(rng.uniform(-0.5, 0.5, (A, N)).astype(np.float32), with_obs=False, stats=True)
        nw = C.c_int32()
        buf = np.zeros((2 * info["grid"], 16), np.uint64)   # (one wave per workgroup: rows [0, grid) are the time stamps)
        env._call("ca_debug_stamps", env.h, buf.ctypes.data, buf.shape[0], C.byref(nw))
        assert 2 * nw.value == buf.shape[0], (nw.value, buf.shape)
        t = buf[:nw.value, :12].astype(np.int64)
        cnt = buf[nw.value:, 2]
        four.append((cnt & np.uint64(0xFFFF)).astype(np.int64) - 1)        # (the closing trip is no round)
        paired.append(((cnt >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64))
        lp3.append(t[:, 7] - t[:, 6])
        whole.append(t[:, 11] - t[:, 0])
    env.close()
    four, paired, lp3, whole = (np.concatenate(x) for x in (four, paired, lp3, whole))
    print("%s settled crowd (step %d ..), CA_LP3_PAIRS=%s, a PairedLp3 kernel: %s; %d waves x %d steps" % (wl, WARM + 1, pairs, has, A, SAMPLES))
    print("  %-28s %9s %8s | LP3+integrate cycles: %8s %8s %8s | stamps 0..11: %8s" % ("rounds (four-lane + paired)", "waves", "share", "mean", "p50", "p95", "mean"))
    keys = sorted(set(zip(four.tolist(), paired.tolist())))
    for f4, pr in keys:
        sel = (four == f4) & (paired == pr)
        print("  %-28s %9d %7.2f%% | %30.0f %8.0f %8.0f | %21.0f" % ("%d + %d" % (f4, pr), sel.sum(), 100.0 * sel.mean(), lp3[sel].mean(),
                                                                  np.percentile(lp3[sel], 50), np.percentile(lp3[sel], 95), whole[sel].mean()))
    print("  %-28s %9d %7.2f%% | %30.0f %8.0f %8.0f | %21.0f" % ("all", len(lp3), 100.0, lp3.mean(), np.percentile(lp3, 50), np.percentile(lp3, 95), whole.mean()))


for pairs in ("0", "1"):
    run(pairs)
