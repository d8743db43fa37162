"""The input guard of tests/test_gpu_lp3_pairs.py, on the CPU oracle alone: the scenes of tests/lp3_pair_scenes.py really put a wave
of the solve kernel on every side of the pool round's two thresholds -- at most 16 agents infeasible after LP2 (the four-lane round),
17 to 32 (the paired round), more than 32 (both) -- with obstacle lines among the infeasible agents and with the parallel lines that
the paired solver marks instead of compacting.  The counts are the oracle's branch counters around serial steps of the one arena:
LP3_ENTERED of a step is the number of lanes that wait for the pool in that step's wave.  A scene that stops reaching its case fails
here; nothing skips.  Plus what needs no GPU: the twins' resources from the compiler's metadata, the declaration and the binding."""
import os
import re
import shutil
import sys

import pytest

from collision_avoidance_amd import _lib
from tests import lp3_pair_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_RUNS = {}


def _run(name, K):
    if (name, K) not in _RUNS:
        _RUNS[(name, K)] = S.infeasible_per_step(name, K)
    return _RUNS[(name, K)]


@pytest.mark.parametrize("K", [10, 5])
def test_scenes_reach_both_sides_of_both_thresholds(K):
    runs = {name: _run(name, K) for name in S.SCENES}
    for name, r in runs.items():
        print(name, K, "LP3_ENTERED per step", [x[0] for x in r])
    entered = [x[0] for r in runs.values() for x in r]
    assert any(17 <= n <= 32 for n in entered)
    assert any(n > 32 for n in entered)
    assert any(0 < n <= 16 for n in entered)
    # the boundary pair 16 | 17, in consecutive steps of the clump
    c = [x[0] for x in runs["clump"]]
    assert any(a == 16 and b == 17 for a, b in zip(c, c[1:])), c
    # every scene runs the paired round and the four-lane round itself
    for name, r in runs.items():
        n = [x[0] for x in r]
        assert any(v > 16 for v in n) and any(0 < v <= 16 or v > 32 for v in n), (name, n)


@pytest.mark.parametrize("K", [10, 5])
def test_obstacle_lines_and_parallel_lines_in_waves_that_take_the_paired_round(K):
    corner, mirror = _run("corner", K), _run("mirror", K)
    assert any(n > 16 and with_obst > 0 for n, with_obst, _, _ in corner), corner
    # the mirror rows: opposite (the triples' middle agents) and same-direction (the rows of five) parallel lines, in a step whose
    # wave has more than 16 waiting lanes
    assert any(n > 16 and opp > 0 for n, _, opp, _ in mirror), mirror
    assert any(n > 16 and same > 0 for n, _, _, same in mirror), mirror


@pytest.mark.parametrize("K", [10, 5])
@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_the_gpu_batch_mixes_both_rounds_in_one_launch(name, K):
    """the three arenas of tests/test_gpu_lp3_pairs.py, each as an oracle env of its own: in some step one arena has 1 .. 16 infeasible
    agents (the four-lane round) while another has more than 16 (the paired round)"""
    rows = S.batch_infeasible(name, K)
    print(name, K, rows)
    assert any(any(0 < n <= 16 for n in r) and any(n > 16 for n in r) for r in rows), rows


def test_twins_exist_without_scratch_within_128_registers():
    """tools/kernel_resources.py: step_kernel<K, 64, 4, 4, false, SeededScan, PairedLp3> for both K classes -- no scratch memory, no
    spilled vector register, at most 128 VGPRs (four waves per SIMD: all 4096 arenas of the headline shape resident), static LDS as
    the kernel without the tag.  Compiles the device assembly once per source change."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    kr.ensure_asm()
    rows = {r["name"]: r for r in kr.parse()}
    for K in (5, 10):
        twin = rows["step_kernel<%d, 64, 4, 4, false, SeededScan, PairedLp3>" % K]
        plain = rows["step_kernel<%d, 64, 4, 4, false, SeededScan>" % K]
        assert twin["scratch"] == 0 and twin["vgpr_spill"] == 0 and twin["vgpr"] <= 128, twin
        assert twin["lds"] == plain["lds"], (twin, plain)
    assert not [n for n in rows if "PairedLp3" in n and not re.match(r"step_kernel<(5|10), 64, 4, 4, false, SeededScan, PairedLp3>$", n)]


def test_declaration_and_binding():
    text = open(os.path.join(ROOT, "include", "ca_env.h")).read()
    assert re.search(r"int ca_lp3_pairs_info\(ca_env\* env, int32_t\* paired\);", text)
    assert "ca_lp3_pairs_info" in _lib.EXPORTS
    from collision_avoidance_amd.vec_env import VecCollisionAvoidanceEnv
    assert callable(VecCollisionAvoidanceEnv.lp3_pairs_info)
