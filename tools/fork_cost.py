#!/usr/bin/env python3
"""What forking and rewinding arenas costs (ca_arena_gather / ca_snapshot_*): fork() -- a broadcast of arena 0 and a
random permutation --, snapshot() and restore() on the device, against the same moves done through the host (get_state() -> numpy
permutation of the arena axis -> set_state()), and against the byte model at the HBM rate.

  python tools/fork_cost.py [--shapes 4096x64,16384x10,1024x16] [--repeat 7] [--calls 20] [--out FILE]

Per shape and move: the wall time of a call (the stream drained at both ends of `--calls` calls; the median of `--repeat` rounds, min
.. max) and the time of the copy kernel alone (ca_profile, kind 3: start / stop events on its own dispatch; a fork is two launches and
shows their sum).  The bytes are what the plane descriptors say (ca_fork_bytes_per_arena): a save or a load reads and writes every
byte of a written arena once, a fork does both; the model is that traffic at 6.3 TB/s, the measured float4-copy rate of the chip.
The host route is timed --host-repeat times (it takes long enough to need no averaging).  Shapes: 4096 x 64 is the headline shape
(crowd, K = 10), 16384 x 10 the reference env's own (doorway, K = 5, 8-bit ids, 50-byte rows: the element path), 1024 x 16 a small
batch (crowd, K = 10)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collision_avoidance_amd import build as b, scenarios  # noqa: E402
from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv  # noqa: E402

HBM = 6.3e12   # bytes/s


def make(A, N):
    if N == 10:
        return VecCollisionAvoidanceEnv(A, N, scenario="doorway", params=scenarios.env_params(), use_torch=False), "doorway, K = 5"
    return VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, 5.0, 10), use_torch=False), "crowd, K = 10"


def wall(g, call, calls, repeat):
    call(); g.sync()
    out = []
    for _ in range(repeat):
        g.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        g.sync()
        out.append((time.perf_counter() - t0) / calls)
    return sorted(out)


def kernel_ms(g, call, launches):
    """the copy kernel's own time per call: the mean of its launches (kind 3) times the launches of a call"""
    g.profile(1); g.profile_read()
    for _ in range(10):
        call()
    n, ms = g.profile_read()["reset_kernels"]
    g.profile(0)
    assert n == 10 * launches, (n, launches)
    return ms * launches


def host_move(g, src):
    st = g.get_state()
    g.set_state({k: (v if k == "_shape" else np.ascontiguousarray(v[src])) for k, v in st.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x64,16384x10,1024x16")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["sources %s; device route: per call, median of %d rounds of %d calls (min .. max); kernel: ca_profile kind 3; host route: "
             "get_state -> numpy -> set_state, best of %d" % (b.source_sha(), a.repeat, a.calls, a.host_repeat),
             "model: bytes read + bytes written at %.1f TB/s" % (HBM / 1e12)]
    for shape in a.shapes.split(","):
        A, N = (int(v) for v in shape.split("x"))
        g, what = make(A, N)
        g.rollout(20)
        per = g.fork_bytes_per_arena()
        rng = np.random.RandomState(0)
        perm = rng.permutation(A).astype(np.int32)
        bcast = np.zeros(A, np.int32)
        snap = g.snapshot()
        lines += ["", "%d x %d agents (%s): %d bytes per arena, %.2f MB per set of the state buffers" % (A, N, what, per, per * A / 1e6)]
        lines.append("%-34s %10s %22s %12s %10s %10s %12s" % ("move", "wall us", "(min .. max)", "kernel us", "model us", "GB/s", "host route ms"))
        moves = [("fork(broadcast of arena 0)", lambda: g.fork(bcast), 2, 2 * per * A + 2 * per * (A - 1), bcast),
                 ("fork(random permutation)", lambda: g.fork(perm), 2, 2 * per * A + 2 * per * int((perm != np.arange(A)).sum()), perm),
                 ("snapshot(into=snap)", lambda: g.snapshot(into=snap), 1, 2 * per * A, None),
                 ("restore(snap)", lambda: g.restore(snap), 1, 2 * per * A, np.arange(A))]
        for name, call, launches, traffic, src in moves:
            w = wall(g, call, a.calls, a.repeat)
            k = kernel_ms(g, call, launches) * 1e3
            host = ""
            if src is not None:
                ts = []
                for _ in range(a.host_repeat):
                    g.sync()
                    t0 = time.perf_counter()
                    host_move(g, src)
                    g.sync()
                    ts.append(time.perf_counter() - t0)
                host = "%.1f (x %.0f)" % (min(ts) * 1e3, min(ts) / w[len(w) // 2])
            lines.append("%-34s %10.1f %22s %12.1f %10.1f %10.0f %12s"
                         % (name, w[len(w) // 2] * 1e6, "(%.1f .. %.1f)" % (w[0] * 1e6, w[-1] * 1e6), k, traffic / HBM * 1e6, traffic / (k * 1e-6) / 1e9, host))
        g.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
