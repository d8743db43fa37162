"""The rule of the seeded neighbour scan (csrc/ca_nbr.h, CA_NBR_SEED) as a numpy model of one wave, against a brute-force
K smallest.

The model states what the kernel does for an arena of at most 64 agents, one lane per agent, every decision that the kernel
takes wave-wide taken over all lanes at once:
  * the list is KMAX + 1 composite keys ((image of dsq) << logP | index), right-aligned behind zeros, and an insertion is the
    median-of-three network  new[k] = med3(old[k - 1], old[k], c);
  * the seed -- a count and K ids that may hold anything -- is sanitised (count clamped to K; a member only if it is a present
    row, not the lane itself, not taken before) and its members are inserted first, with their current distances;
  * the scan in index order runs the network for candidate j only if SOME lane wants it: bits(dsq) <= the lane's threshold
    (the K-th key taken back to fp32 bits, the (K + 1)-th for K = 1, capped at the range) and j not yet taken by that lane;
    then every lane inserts it through its own exact pass test, or all ones.
Compared with: the K smallest composite keys of the passing candidates (and, for K = 1, the second smallest, which decides the
fall-back to the exact scan), and -- wherever no lane holds two clamped keys -- App. A.2 itself, the K smallest (dsq, index)."""
import numpy as np
import pytest

F = np.float32
ONES = 0xFFFFFFFF


def _dsq(px, py):
    dx = px[:, None] - px[None, :]
    dy = py[:, None] - py[None, :]
    d = dx * dx + dy * dy          # fp32 elementwise: fl(fl(dx^2) + fl(dy^2))
    assert d.dtype == F
    return d


def _image_consts(nd, logP):
    r2 = F(F(nd) * F(nd))
    top = int(np.array(r2, F).view(np.uint32))
    span = ONES >> logP
    u0 = top - span + 1 if top >= span else 0
    return r2, top, span, u0


def _med3(a, b, c):
    return np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))


def seeded_scan(px, py, n_a, K, KMAX, nd, seed_cnt, seed_ids, forced=()):
    """One wave.  px, py [N] fp32; rows >= n_a are absent.  seed_cnt [N], seed_ids [N, K]: any integers 0 .. 255.
    forced: candidates whose network runs whether a lane wants them or not (another arena of the same wave wanted them).
    Returns (ck [N, KMAX + 1] uint64, number of candidates whose network ran)."""
    N = len(px)
    P, logP = 1, 0
    while P < N:
        P, logP = P << 1, logP + 1
    r2, top, span, u0 = _image_consts(nd, logP)
    d = _dsq(px, py)
    U = d.view(np.uint32).astype(np.int64)
    lanes = np.arange(N)
    active = lanes < n_a
    kofs = KMAX - K
    ck = np.full((N, KMAX + 1), ONES, np.int64)
    ck[:, :kofs] = 0
    vis = np.ones((N, 64), bool)                      # an idle lane: every bit
    vis[active, :n_a] = False
    vis[lanes[active], lanes[active]] = True          # the lane itself

    def insert(jj, dsq, u, take):
        ok = take & (dsq < r2)
        key = ((np.maximum(u, u0) - u0) << logP) | jj
        assert (key[ok] < ONES).all()
        c = np.where(ok, key, ONES)
        for k in range(KMAX, 0, -1):
            ck[:, k] = _med3(ck[:, k - 1], ck[:, k], c)
        ck[:, 0] = np.minimum(ck[:, 0], c)

    def threshold():
        kth = ck[:, KMAX - 1] if K >= 2 else ck[:, KMAX]
        return np.minimum(u0 + (kth >> logP), top)

    sn = np.minimum(np.asarray(seed_cnt, np.int64), K)
    for k in range(K):
        m = np.asarray(seed_ids[:, k], np.int64)
        ok = (k < sn) & (m < n_a) & active
        mm = np.where(ok, m, 0)
        ok &= ~vis[lanes, mm]
        if ok.any():
            vis[lanes[ok], mm[ok]] = True
            src = np.where(ok, mm, lanes)             # (no position is read through an unchecked index)
            insert(mm, d[lanes, src], U[lanes, src], ok)
    thr = threshold()
    ran = 0
    for j in range(N):
        want = (U[:, j] <= thr) & ~vis[:, j]
        if want.any() or j in forced:
            insert(np.full(N, j, np.int64), d[:, j], U[:, j], ~vis[:, j])
            thr = threshold()
            ran += 1
    return ck, ran


def brute(px, py, n_a, K, nd):
    """Per lane: the sorted composite keys of every passing candidate (all of them), and App. A.2's (dsq, index) order."""
    N = len(px)
    logP = int(np.ceil(np.log2(N))) if N > 1 else 0
    r2, top, span, u0 = _image_consts(nd, logP)
    d = _dsq(px, py)
    U = d.view(np.uint32).astype(np.int64)
    keys, exact = [], []
    for i in range(N):
        js = np.array([j for j in range(n_a) if j != i and i < n_a and d[i, j] < r2], np.int64)
        kk = ((np.maximum(U[i, js], u0) - u0) << logP) | js
        keys.append(np.sort(kk))
        exact.append(js[np.lexsort((js, d[i, js]))] if js.size else js)
    return keys, exact, (1 << logP) - 1


def check(px, py, n_a, K, KMAX, nd, seed_cnt, seed_ids, forced=()):
    ck, ran = seeded_scan(px, py, n_a, K, KMAX, nd, seed_cnt, seed_ids, forced)
    keys, exact, lowmask = brute(px, py, n_a, K, nd)
    kofs = KMAX - K
    diffs = 0
    any_clamped_pair = any(len(k) >= 2 and k[1] <= lowmask for k in keys)
    for i in range(len(px)):
        want = np.full(K, ONES, np.int64)
        want[:min(K, len(keys[i]))] = keys[i][:K]
        diffs += int((ck[i, kofs:KMAX] != want).sum())
        if K == 1:                                    # the second smallest key: clamped_pair reads it
            second = keys[i][1] if len(keys[i]) >= 2 else ONES
            diffs += int(ck[i, KMAX] != second)
        if not any_clamped_pair:                      # the wave keeps the composite lists: they are App. A.2's
            got = [int(c & lowmask) for c in ck[i, kofs:KMAX] if c != ONES]
            diffs += int(got != [int(j) for j in exact[i][:K]])
    return diffs, ran


def _positions(rng, kind, N):
    if kind == "random":
        s = 0.9 * np.sqrt(N)
        return rng.uniform(-s, s, N).astype(F), rng.uniform(-s, s, N).astype(F)
    if kind == "lattice":                             # many bit-identical dsq: tie groups of 4 and 8, more than K for small K
        side = int(np.ceil(np.sqrt(N)))
        perm = rng.permutation(side * side)[:N]
        return (perm % side).astype(F) * F(1.25), (perm // side).astype(F) * F(1.25)
    if kind == "overlap":                             # deep overlaps and coincident agents: clamped keys, the fall-back flag
        x, y = rng.uniform(-2, 2, N).astype(F), rng.uniform(-2, 2, N).astype(F)
        for k in range(1, N, 3):
            x[k], y[k] = x[k - 1] + F(rng.choice([0.0, 0.01, 0.2])), y[k - 1]
        return x, y
    raise ValueError(kind)


def _seeds(rng, kind, px, py, n_a, K, nd):
    N = len(px)
    cnt = np.zeros(N, np.int64)
    ids = np.zeros((N, K), np.int64)
    if kind == "empty":
        return cnt, ids
    if kind == "previous":                            # the true lists of slightly different positions
        qx = (px + rng.uniform(-0.02, 0.02, N).astype(F)).astype(F)
        qy = (py + rng.uniform(-0.02, 0.02, N).astype(F)).astype(F)
        _, exact, _ = brute(qx, qy, n_a, K, nd)
        for i in range(N):
            e = exact[i][:K]
            cnt[i] = len(e)
            ids[i, :len(e)] = e
            ids[i, len(e):] = 255                     # (an empty slot reads -1 as a byte)
        return cnt, ids
    if kind == "stale":                               # real candidates, but somebody else's
        return rng.randint(0, K + 1, N), rng.randint(0, N, (N, K))
    if kind == "duplicated":
        return np.full(N, K), np.repeat(rng.randint(0, N, (N, 1)), K, axis=1)
    if kind == "out_of_range":
        return rng.randint(0, 256, N), rng.randint(0, 256, (N, K))
    if kind == "self":
        return np.full(N, 255), np.repeat(np.arange(N)[:, None], K, axis=1)
    raise ValueError(kind)


SEED_KINDS = ("empty", "previous", "stale", "duplicated", "out_of_range", "self")


@pytest.mark.parametrize("K", [1, 2, 10])
@pytest.mark.parametrize("N", [2, 3, 11, 64])
def test_seeded_scan_is_the_k_smallest(N, K):
    rng = np.random.RandomState(1000 * N + K)
    diffs = cases = 0
    for pos_kind in ("random", "lattice", "overlap"):
        for seed_kind in SEED_KINDS:
            for nd in (5.0, 1.3):
                px, py = _positions(rng, pos_kind, N)
                n_a = N if rng.rand() < 0.6 else rng.randint(0, N + 1)       # (unequal arena counts: absent rows)
                cnt, ids = _seeds(rng, seed_kind, px, py, n_a, K, nd)
                forced = set(rng.randint(0, N, rng.randint(0, 3)).tolist())
                for KMAX in sorted({K, 10}):
                    d, _ = check(px, py, n_a, K, KMAX, nd, cnt, ids, forced)
                    diffs += d
                    cases += 1
    assert cases >= 36
    assert diffs == 0


def test_a_true_seed_skips_nearly_every_network():
    """What the change is for: seeded with the lists of positions a step earlier, a full wave runs the network for a few
    candidates, not for all 64 (unseeded, every candidate in range of some lane runs it)."""
    rng = np.random.RandomState(5)
    px, py = _positions(rng, "random", 64)
    K, nd = 10, 5.0
    cnt, ids = _seeds(rng, "previous", px, py, 64, K, nd)
    d_seeded, ran_seeded = check(px, py, 64, K, K, nd, cnt, ids)
    d_empty, ran_empty = check(px, py, 64, K, K, nd, np.zeros(64, np.int64), np.zeros((64, K), np.int64))
    assert d_seeded == 0 and d_empty == 0
    assert ran_empty == 64
    assert ran_seeded < ran_empty // 2, ran_seeded
