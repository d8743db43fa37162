#!/usr/bin/env python3
"""What recording a rollout costs (ca_rollout_trace): agent-steps/s of the one-launch rollout with and without a
trace, of the loop a caller had to write before (ca_orca_step plus a device-side copy of the four fields per step), and of the
same rollout in other builds of the library -- all in ONE process, the variants alternated, every timed run at least --seconds
long, --repeat runs of each.

  python tools/trace_cost.py [--shapes 1024x16,64x64] [--repeat 5] [--seconds 1.0] [--lib NAME=PATH ...] [--tiled 16384] [--out FILE]

--lib NAME=PATH adds another build of libcaenv.so: its plain rollout is timed, and its recording rollout if it exports one.  The
committed table names three: `parent` (the commit before the recording rollouts: the plain rollout must not have moved), and the
two other ways for the four-lanes kernel to store a record, built with -DCA_TRACE_STORE=1 (lane 0 of a quad stores the four
planes) and -DCA_TRACE_STORE=2 (lane q stores plane q, non-temporal); the library itself is CA_TRACE_STORE=0 (lane q stores plane
q, plain stores).  The workload is bench.py's crowd (bench_params: a new goal whenever one is reached), T = 256 steps per call,
the trace buffers allocated once and rewritten by every call.  --tiled N adds one tiled handle of 1 x N agents with the grid,
every = 1, against the same rollout without a trace (there a rollout is six launches per step plus the record kernel).
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collision_avoidance_amd import _lib, build as b, scenarios  # noqa: E402

T = 256
FIELDS = (_lib.FLD_POS_X, _lib.FLD_POS_Y, _lib.FLD_VEL_X, _lib.FLD_VEL_Y)


def open_lib(path):
    """A build of the library with the prototypes this tool calls (the package binds one library per process)."""
    L = C.CDLL(path)
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    L.ca_create_ex.argtypes = [C.POINTER(_lib.Config), u32, C.c_int, vp, C.POINTER(vp)]
    L.ca_set_obstacles.argtypes = [vp, vp, vp, i32]
    L.ca_init_scenario.argtypes = [vp, i32]
    L.ca_rollout.argtypes = [vp, i32, u32]
    L.ca_orca_step.argtypes = [vp, u32]
    L.ca_sync.argtypes = [vp]
    L.ca_destroy.argtypes = [vp]
    L.ca_field_ptr.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.ca_solver_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.ca_last_error.argtypes = [vp]
    L.ca_last_error.restype = C.c_char_p
    if hasattr(L, "ca_rollout_trace"):
        L.ca_rollout_trace.argtypes = [vp, i32, u32, C.POINTER(_lib.Trace)]
    return L


class Handle(object):
    """The crowd of bench.py on one build of the library, on the torch stream `stream`."""

    def __init__(self, L, A, N, nd, K, stream, create_flags=0):
        self.L, self.A, self.N = L, A, N
        p = scenarios.bench_params(N, nd, K)
        polys = [np.asarray(q, np.float32).reshape(-1, 2) for q in scenarios.obstacles("crowd", N, p["radius"])]
        cfg = _lib.Config(n_arenas=A, n_agents=N, arena_offset=0, seed=0, max_obst_neighbors=max(1, min(16, sum(len(q) for q in polys))), **p)
        h = C.c_void_p()
        self.h = None
        self.ok(L.ca_create_ex(C.byref(cfg), create_flags, 0, C.c_void_p(stream.cuda_stream), C.byref(h)), "ca_create_ex")
        self.h = h
        verts = np.ascontiguousarray(np.concatenate(polys))
        sizes = np.asarray([len(q) for q in polys], np.int32)
        self.ok(L.ca_set_obstacles(h, verts.ctypes.data, sizes.ctypes.data, len(polys)), "ca_set_obstacles")
        self.ok(L.ca_init_scenario(h, _lib.SCN_CROWD), "ca_init_scenario")
        lanes, one = C.c_int32(), C.c_int32()
        self.ok(L.ca_solver_info(h, C.byref(lanes), C.byref(one)), "ca_solver_info")
        self.one_launch = bool(one.value)

    def ok(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, (self.L.ca_last_error(self.h) or b"?").decode()))

    def field(self, f):
        ptr, n = C.c_void_p(), C.c_size_t()
        self.ok(self.L.ca_field_ptr(self.h, f, C.byref(ptr), C.byref(n)), "ca_field_ptr")

        class V(object):
            pass
        v = V()
        v.__cuda_array_interface__ = {"shape": (self.A, self.N), "typestr": "<f4", "data": (int(ptr.value), False), "version": 2, "strides": None}
        return torch.as_tensor(v, device="cuda")

    def rollout(self):
        self.ok(self.L.ca_rollout(self.h, T, 0), "ca_rollout")

    def traced(self, every, channels):
        C_ = 2 * bin(channels).count("1")
        ag = torch.empty((T // every, C_, self.A, self.N), dtype=torch.float32, device="cuda")
        ar = torch.empty((T // every, 3, self.A), dtype=torch.int32, device="cuda")
        tr = _lib.Trace(agents=ag.data_ptr(), agents_bytes=ag.numel() * 4, arenas=ar.data_ptr(), arenas_bytes=ar.numel() * 4, every=every,
                        channels=channels)
        keep = (ag, ar, tr)

        def call():
            keep[0].data_ptr()
            self.ok(self.L.ca_rollout_trace(self.h, T, 0, C.byref(tr)), "ca_rollout_trace")
        return call

    def step_and_copy(self):
        views = [self.field(f) for f in FIELDS]
        buf = torch.empty((T, 4, self.A, self.N), dtype=torch.float32, device="cuda")

        def call():
            for s in range(T):
                self.ok(self.L.ca_orca_step(self.h, 0), "ca_orca_step")
                for c, v in enumerate(views):
                    buf[s, c].copy_(v, non_blocking=True)
        return call

    def sync(self):
        self.ok(self.L.ca_sync(self.h), "ca_sync")

    def close(self):
        self.L.ca_destroy(self.h)


def timed(h, call, seconds):
    """calls of `call` until `seconds` have passed (the stream drained at both ends) -> agent-steps/s"""
    h.sync()
    n, t0 = 0, time.perf_counter()
    while True:
        call()
        n += 1
        if n % 4 == 0 or not h.one_launch:
            h.sync()
            if time.perf_counter() - t0 >= seconds:
                break
    h.sync()
    return h.A * h.N * T * n / (time.perf_counter() - t0)


def fmt(name, runs):
    r = sorted(runs)
    return "%-58s %9.4f  %9.4f .. %-9.4f  %s" % (name, r[len(r) // 2] / 1e9, r[0] / 1e9, r[-1] / 1e9, " ".join("%.4f" % (v / 1e9) for v in runs))


def measure(variants, repeat, seconds):
    res = {name: [] for name, _, _ in variants}
    for name, h, call in variants:      # warm-up: one call each
        call(); h.sync()
    for _ in range(repeat):             # alternated: one run of every variant per round
        for name, h, call in variants:
            res[name].append(timed(h, call, seconds))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x16,64x64")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--lib", action="append", default=[])
    ap.add_argument("--tiled", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    libs = [("this", open_lib(b.LIB_PATH))] + [(s.split("=", 1)[0], open_lib(s.split("=", 1)[1])) for s in a.lib]
    stream = torch.cuda.Stream()
    lines = ["sources %s; T = %d steps per call, %d alternated repeats of at least %.1f s each; G agent-steps/s: median, min .. max, every repeat"
             % (b.source_sha(), T, a.repeat, a.seconds)]
    with torch.cuda.stream(stream):
        for shape in a.shapes.split(","):
            A, N = (int(v) for v in shape.split("x"))
            nd, K = (1.5, 5) if N <= 16 else (5.0, 10)
            hs = {name: Handle(L, A, N, nd, K, stream) for name, L in libs}
            assert all(h.one_launch for h in hs.values()), "the shape does not take the one-launch rollout"
            variants = [("rollout(T), library `%s`" % name, h, h.rollout) for name, h in hs.items() if name == "parent"]
            variants.append(("rollout(T), library `this`", hs["this"], hs["this"].rollout))
            for name, h in hs.items():
                if name == "parent" or not hasattr(h.L, "ca_rollout_trace"):
                    continue
                for every in (1, 10):
                    for ch, cn in ((1, "pos"), (3, "pos+vel")):
                        variants.append(("rollout(T, trace every=%d %s), library `%s`" % (every, cn, name), h, h.traced(every, ch)))
            variants.append(("orca_step() + 4 device copies per step, library `this`", hs["this"], hs["this"].step_and_copy()))
            res = measure(variants, a.repeat, a.seconds)
            lines.append("")
            lines.append("%d x %d agents (neighbor_dist %.1f, max_neighbors %d)" % (A, N, nd, K))
            lines += [fmt(name, res[name]) for name, _, _ in variants]
            for h in hs.values():
                h.close()
        if a.tiled:
            h0, h1 = (Handle(libs[0][1], 1, a.tiled, 5.0, 10, stream, _lib.CREATE_TILED | _lib.CREATE_TILED_GRID) for _ in range(2))
            variants = [("tiled grid 1 x %d: rollout(T)" % a.tiled, h0, h0.rollout),
                        ("tiled grid 1 x %d: rollout(T, trace every=1 pos+vel)" % a.tiled, h1, h1.traced(1, 3))]
            res = measure(variants, a.repeat, a.seconds)
            lines.append("")
            lines.append("tiled handle with the grid, 1 x %d agents: six launches per step, plus the record kernel" % a.tiled)
            lines += [fmt(name, res[name]) for name, _, _ in variants]
            h0.close(); h1.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
