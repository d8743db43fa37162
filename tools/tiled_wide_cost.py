#!/usr/bin/env python3
"""What obstacle lists of up to 64 edges cost on a tiled grid handle (CA_CREATE_TILED_WIDE; csrc/ca_tiled.h's WideObstLists
instantiations), and which tile serves them: a report, no threshold.

  python tools/tiled_wide_cost.py [--steps 100] [--warmup 20] [--repeats 5] [--out profiles/tiled_wide_cost.txt]

One crowd of 1 x 16384 agents with the parameters of bench.py (scenarios.bench_params: range 5, K = 10, a new goal whenever one is
reached, walls), the same seed on every handle, the handles of a case alternated block by block in this one call:
  (a) create flags 5 with lists of 16 next to flags 37 with lists of 64, in the crowd's own world (its border: 4 edges).  No list
      holds more than a few edges, so the two run the same simulation bit for bit and the difference is the price of the wide path:
      the list in LDS instead of registers, a tile of 64 instead of 128, K + 64 lines of LDS per lane instead of K + 16.
  (b) flags 37 with lists of 64 and the static edge grid on, in scenarios.pillar_hall(16384, 127, 1.0): the largest hall of that
      pitch that the 16-bit edge ids hold (16129 pillars, 64520 edges, a quarter of the arena; the lists there reach into the
      thirties) -- the world the flag is for.  Overflow is allowed and reported.
  (c) the handle of (b) with CA_TILE=128 next to the default tile of 64.
Per handle: us per ORCA-only step with statistics (ca_rollout: the six launches) and per full step (ca_step with CA_F_OBS |
CA_F_STATS on device actions), every block and the median; and ca_profile's kernel time per ORCA step (mean per launch x launches:
it does not tell the launches apart, but the two handles of a case differ in the solve launch alone, so the difference of the two
sums is the solve launch's).  Needs a GPU and PyTorch (for the device action pool and the synchronisation only).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

A, N = 1, 16384
HALL = (N, 127, 1.0)


def make(polys, S, wide, edge_grid=False, tile=None):
    from collision_avoidance_amd import scenarios
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    if tile is None:
        os.environ.pop("CA_TILE", None)
    else:
        os.environ["CA_TILE"] = str(tile)     # (read once, by ca_create_ex)
    try:
        return VecCollisionAvoidanceEnv(A, N, scenario="crowd", params=scenarios.bench_params(N, 5.0, 10), seed=0, use_torch=True,
                                        tiled="grid", tiled_wide=wide, obstacles=polys, max_obst_neighbors=S, allow_obst_overflow=True,
                                        edge_grid=edge_grid)
    finally:
        os.environ.pop("CA_TILE", None)


def main():
    import torch  # noqa: F401  (before the library is loaded: PyTorch brings a HIP runtime of its own)
    import tiled_cost as tc
    from collision_avoidance_amd import _lib, scenarios
    from collision_avoidance_amd import build as b
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text=""):
        lines.append(text)
        print(text, flush=True)

    def case(title, envs, base):
        """envs: name -> handle, alternated; base: the name the others are compared with"""
        say(title)
        pool = tc.pool_for(A, N)
        for k, e in envs.items():
            ti = e.tiled_info()
            say("%5d x %-6d %-14s create flags %d, lists of %d, tile %d (%d B of LDS per workgroup), edge grid %s, %d launches per step"
                % (A, N, k, 37 if e.tiled_wide else 5, e.S, ti["tile_agents"], ti["tile_agents"] * ((e.K + e.S) * 16 + 8),
                   "on" if e.edge_grid_info()["on"] else "off", ti["launches_per_step"]))
        med = {}
        for mode in ("ORCA only", "full step"):
            full = mode == "full step"
            for e in envs.values():
                (tc.block(e, pool, args.warmup, 0) if full else tc.orca_block(e, args.warmup))
            times = {k: [] for k in envs}
            for r in range(args.repeats):
                for k, e in envs.items():
                    sec = tc.block(e, pool, args.steps, args.warmup + r * args.steps) if full else tc.orca_block(e, args.steps)
                    times[k].append(sec * 1e6)
            med[mode] = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            for k in envs:
                say("%5d x %-6d %-10s %-14s %s   median %10.1f us/step" % (A, N, mode, k, " ".join("%10.1f" % t for t in times[k]), med[mode][k]))
            for k in envs:
                if k != base:
                    say("%5d x %-6d %-10s %s / %s = %.3f   (difference %.1f us, spread of %s's repeats %.1f us)"
                        % (A, N, mode, k, base, med[mode][k] / med[mode][base], med[mode][k] - med[mode][base], base,
                           max(times[base]) - min(times[base])))
        kern = {}
        for k, e in envs.items():
            e.profile(1)
            tc.orca_block(e, 20)
            n, ms = e.profile_read()["step_kernel"]
            e.profile(0)
            kern[k] = ms * 1e3 * e.tiled_info()["launches_per_step"]
            say("%5d x %-6d ca_profile, ORCA only, %-14s mean %.1f us per launch, %.1f us of kernels per step" % (A, N, k, ms * 1e3, kern[k]))
        for k in envs:
            if k != base:
                say("%5d x %-6d ca_profile: the solve launch of %s takes %.1f us more than that of %s (the other launches are the same kernels)"
                    % (A, N, k, kern[k] - kern[base], base))
        for k, e in envs.items():
            e.sync()
            st = e.stats()
            say("%5d x %-6d %-14s largest obstacle list after the run %d, lists that overflowed %d" % (A, N, k, int(e.get(_lib.FLD_OBST_COUNT).max()),
                                                                                                 st["obst_overflow"]))
        names = list(envs)
        same = all((envs[names[0]].get(f) == envs[k].get(f)).all() for k in names[1:] for f in (0, 1, 2, 3))
        say("%5d x %-6d positions and velocities of the handles after the run: %s" % (A, N, "equal" if same else "DIFFERENT"))
        for e in envs.values():
            e.close()
        say()

    say("# tools/tiled_wide_cost.py, sources %s: tiled grid handles with obstacle lists of 16 and of 64, alternated block by block, %d blocks "
        "of %d steps each; us per step, every block, then the median" % (b.loaded_sha(), args.repeats, args.steps))
    e = scenarios.envsize("crowd", N)
    border = [[(0.0, 0.0), (0.0, e), (e, e), (e, 0.0)]]
    case("(a) the crowd's border only: flags 5 with lists of 16 next to flags 37 with lists of 64 (the same simulation)",
         {"lists of 16": make(border, 16, False), "lists of 64": make(border, 64, True)}, "lists of 16")
    hall = scenarios.pillar_hall(*HALL)
    say("pillar_hall%r: %d polygons, %d edges" % (HALL, len(hall), sum(len(q) for q in hall)))
    case("(b), (c) the pillar hall, flags 37 with lists of 64, edge grid on: the default tile of 64 next to CA_TILE=128",
         {"tile 64": make(hall, 64, True, edge_grid=True), "tile 128": make(hall, 64, True, edge_grid=True, tile=128)}, "tile 64")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
