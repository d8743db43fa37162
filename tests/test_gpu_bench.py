"""bench.py --dump-outputs: the same arguments give the same outputs.  The warm-up keeps the clocks busy for
CA_BENCH_MIN_WARM seconds with steps that run from a snapshot of the state (get_state / set_state) and are discarded, so
whether that branch ran must not change what the timed steps compute.  Each run is a fresh child process."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTLE, WARM, STEPS = 300, 50, 50       # multiples of the 50-step launches of --mode orca / alan


def _bench(out_dir, min_warm, extra):
    env = dict(os.environ, CA_BENCH_MIN_WARM=min_warm, CA_BENCH_SETTLE_STEPS=str(SETTLE))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "C2", "--arenas", "64", "--steps", str(STEPS),
           "--warmup", str(WARM), "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    arrays = {os.path.basename(f): np.load(f) for f in sorted(glob.glob(os.path.join(str(out_dir), "*.npy")))}
    return json.loads(lines[0]), arrays


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "orca", "alan"])
def test_dumped_outputs_do_not_depend_on_the_clock_warm_up(tmp_path, mode):
    plain, a = _bench(tmp_path / "plain", "0", ["--mode", mode])
    # the steps before the snapshot (at most 250 of 64 small arenas) take far less than 2 s: clock-only steps run from it;
    # the oracle replays every step the state really went through
    warmed, b = _bench(tmp_path / "warmed", "2", ["--mode", mode, "--verify", "4"])
    assert plain["warmup_steps_run"] == warmed["warmup_steps_run"] == SETTLE
    assert plain["warmup_clock_steps"] == 0 and warmed["warmup_clock_steps"] > 0, warmed["warmup_clock_steps"]
    assert warmed["verified"]["bit_exact"] and warmed["verified"]["steps"] == SETTLE + STEPS, warmed["verified"]
    assert plain["stats"] == warmed["stats"]
    expected = {"pos_x", "pos_y", "vel_x", "vel_y", "agent_done", "arena_done"} | \
        ({"reward", "obs"} if mode == "step" else {"alan_action", "alan_weights"} if mode == "alan" else set())
    assert sorted(a) == sorted(b) == sorted(n + ".npy" for n in expected)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64) and a[name].shape[0] == 64, (name, a[name].dtype, a[name].shape)
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, name
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name
