"""The rule of an action-sequence rollout (ca_rollout_actions, include/ca_env.h), restated in numpy float32 for the tests: which row
drives a step, which steps advance an arena, what the returns and first_done are given the reward and the arena_done flag every step
leaves.  No device and no library: tests/test_actseq_cpu.py checks it on hand-made tables, tests/test_gpu_actseq.py feeds it what a
twin handle's single steps left."""
import numpy as np


def rows(steps, hold):
    """(R, [row of step t]): R = ceil(steps / hold), step t is driven by row t // hold"""
    return (steps + hold - 1) // hold, [t // hold for t in range(steps)]


def advanced_reference(done_entry, done_after, freeze):
    """[T, A] bool: step t advanced arena a.  done_entry [A]: arena_done before the call; done_after [T, A]: after each step.  Without
    CA_F_FREEZE every step advances every arena; with it, a step advances the arenas whose flag was clear before it."""
    done_after = np.asarray(done_after).reshape(-1, len(done_entry))
    T = done_after.shape[0]
    if not freeze:
        return np.ones((T, len(done_entry)), bool)
    before = np.concatenate([np.asarray(done_entry)[None], done_after[:-1]], 0) if T else done_after
    return before == 0


def returns_reference(rewards, advanced, weights=None, present=None):
    """[A, N] float32: +0.0, then for every step in order ret = ret + w[t] * r_t -- a float32 product and a float32 sum -- or
    ret = ret + r_t without weights, for the agents of the arenas the step advanced; absent rows (present [A, N] False) stay 0.
    rewards [T, A, N]: what step t left in the reward field."""
    rewards = np.asarray(rewards, np.float32)
    assert rewards.ndim == 3
    T, A, N = rewards.shape
    ret = np.zeros((A, N), np.float32)
    present = np.ones((A, N), bool) if present is None else np.asarray(present, bool)
    for t in range(T):
        term = rewards[t] if weights is None else (np.float32(weights[t]) * rewards[t]).astype(np.float32)
        with np.errstate(all="ignore"):
            new = (ret + term).astype(np.float32)
        ret = np.where(np.asarray(advanced[t], bool)[:, None] & present, new, ret)
    return ret


def first_done_reference(done_after, advanced):
    """[A] int32: the first step that advanced the arena and left its flag set, -1 if none (an arena frozen at entry: -1)"""
    advanced = np.asarray(advanced, bool)
    done_after = np.asarray(done_after).reshape(advanced.shape)
    hit = advanced & (done_after != 0)
    return np.where(hit.any(0), hit.argmax(0), -1).astype(np.int32) if hit.shape[0] else np.full(hit.shape[1], -1, np.int32)
