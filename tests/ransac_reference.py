"""A numpy restatement of the RANSAC contract of include/teaser_hip.h ("RANSAC registration on correspondences"): the
splitmix64 draws, the edge-length and distance checkers, Umeyama on the samples, the score with its stated summation
order, and Open3D's loop as one thread runs it.  Everything but the estimate is meant bit for bit (numpy's elementwise
float64 operations are IEEE and never fused; cumsum adds in order); the estimate goes through numpy's SVD and is only as
good as float64.  The stop rule uses math.log and math.pow, the C library's, with the IEEE special cases Python turns
into exceptions put back.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

BLOCK = 256
FLAG_EDGE, FLAG_DIST, FLAG_SCORED = 1, 2, 4
M64 = (1 << 64) - 1


def draw(seed, m):
    """z(seed, m): splitmix64's output for the state seed + m 0x9E3779B97F4A7C15 (Python integers)."""
    z = (seed + m * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def samples(seed, ransac_n, ncorr, first, n):
    """[n, ransac_n] int32: c_k = z(seed, ransac_n i + k + 1) mod ncorr for the trials first .. first + n - 1."""
    out = np.empty((n, ransac_n), dtype=np.int32)
    for q in range(n):
        for k in range(ransac_n):
            out[q, k] = draw(seed, (ransac_n * (first + q) + k + 1) & M64) % ncorr
    return out


def records_of(P, Q, corr):
    """[ncorr, 6]: the pair records {P[i], Q[j]}."""
    corr = np.asarray(corr).reshape(-1, 2)
    return np.concatenate([np.asarray(P, dtype=np.float64)[corr[:, 0]], np.asarray(Q, dtype=np.float64)[corr[:, 1]]], 1)


def _length(a, b):
    d = a - b
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def edge_pass(rec, smp, s):
    """[n] bool: the edge-length test of every trial (all True when s == 0: off)."""
    ok = np.ones(len(smp), dtype=bool)
    if not s > 0:
        return ok
    n = smp.shape[1]
    for a in range(n):
        for b in range(a + 1, n):
            ra, rb = rec[smp[:, a]], rec[smp[:, b]]
            ls, lt = _length(ra[:, :3], rb[:, :3]), _length(ra[:, 3:], rb[:, 3:])
            ok &= ~((ls < lt * s) | (lt < ls * s))
    return ok


def cross_covariance(rec, smp_row):
    """mu_P, mu_Q, H of one trial in the contract's order."""
    n = len(smp_row)
    mp, mq = np.zeros(3), np.zeros(3)
    for k in smp_row:
        mp = mp + rec[k, :3]
        mq = mq + rec[k, 3:]
    mp, mq = mp / float(n), mq / float(n)
    H = np.zeros((3, 3))
    for k in smp_row:
        H = H + np.outer(rec[k, :3] - mp, rec[k, 3:] - mq)
    return mp, mq, H


def estimate(rec, smp_row):
    """T (4 x 4) of one trial: Umeyama without scaling through numpy's SVD."""
    mp, mq, H = cross_covariance(rec, smp_row)
    U, _, Vt = np.linalg.svd(H)
    D = np.eye(3)
    D[2, 2] = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mq - R @ mp
    return T


def d2_of(T, rec):
    """[m, c]: d2 of apply(T[m], p) to q for records rec [c, 6] (or [m, c, 6]), nothing fused."""
    T = np.asarray(T).reshape(-1, 4, 4)[:, None]
    p, q = rec[..., :3], rec[..., 3:]
    x = [((T[..., r, 0] * p[..., 0] + T[..., r, 1] * p[..., 1]) + T[..., r, 2] * p[..., 2]) + T[..., r, 3] for r in range(3)]
    dx, dy, dz = x[0] - q[..., 0], x[1] - q[..., 1], x[2] - q[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def distance_pass(T, rec, smp, d):
    """[n] bool: the distance test of every trial under its own T (all True when d == 0: off)."""
    if not d > 0:
        return np.ones(len(smp), dtype=bool)
    return ~(np.sqrt(d2_of(T, rec[smp])) > d).any(axis=1)  # rec[smp]: [n, ransac_n, 6], one T per row


def score(T, rec, r):
    """count [m] and sum d2 [m] over the inliers (d2 < r r) in the stated order: blocks of 256 consecutive pairs, each
    added in ascending position from 0, the block sums added in ascending block order from 0."""
    d2 = d2_of(T, rec)
    inl = d2 < r * r
    total = np.zeros(len(d2))
    for c0 in range(0, rec.shape[0], BLOCK):
        part = np.where(inl[:, c0:c0 + BLOCK], d2[:, c0:c0 + BLOCK], 0.0)
        total = total + np.cumsum(part, axis=1)[:, -1]
    return inl.sum(axis=1).astype(np.int32), total, inl


def trial_records(P, Q, corr, r, first, n, ransac_n=3, s=0.0, d=0.0, seed=1, T=None):
    """The stage call's records for the trials first .. first + n - 1: samples, flags, transformation, count, sum_d2.
    T given ([n, 4, 4], e.g. the device's): the distance flags and the scores are evaluated on it instead of on the
    restatement's own estimate."""
    corr = np.asarray(corr).reshape(-1, 2)
    ncorr = len(corr)
    if ncorr < ransac_n:
        return dict(samples=np.full((n, ransac_n), -1, np.int32), flags=np.zeros(n, np.uint8),
                    transformation=np.tile(np.eye(4), (n, 1, 1)), count=np.zeros(n, np.int32), sum_d2=np.zeros(n))
    rec = records_of(P, Q, corr)
    smp = samples(seed, ransac_n, ncorr, first, n)
    e_ok = edge_pass(rec, smp, s)
    if T is None:
        T = np.tile(np.eye(4), (n, 1, 1))
        for q in np.nonzero(e_ok)[0]:
            T[q] = estimate(rec, smp[q])
    d_ok = e_ok & distance_pass(T, rec, smp, d)
    flags = (e_ok * FLAG_EDGE + d_ok * (FLAG_DIST | FLAG_SCORED)).astype(np.uint8)
    count, total = np.zeros(n, np.int32), np.zeros(n)
    if d_ok.any():
        c, t, _ = score(T[d_ok], rec, r)
        count[d_ok], total[d_ok] = c, t
    return dict(samples=smp, flags=flags, transformation=np.asarray(T), count=count, sum_d2=total)


def _log(x):
    if x != x:
        return x
    return -math.inf if x == 0.0 else math.log(x)


def _div(a, b):
    if a != a or b != b:
        return math.nan
    if math.isinf(a) and math.isinf(b):
        return math.nan
    if b == 0.0:
        if a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    if math.isinf(b):
        return math.copysign(0.0, a) * math.copysign(1.0, b)
    return a / b


def stop_k(confidence, count, ncorr, ransac_n):
    """k = log(1 - confidence) / log(1 - pow(count / ncorr, ransac_n)) with IEEE's special cases."""
    return _div(_log(1.0 - confidence), _log(1.0 - math.pow(count / ncorr, float(ransac_n))))


def rmse_of(count, total):
    return math.sqrt(total / count) if count > 0 else 0.0


def loop(fetch, ncorr, ransac_n, max_iteration, confidence, chunk=256):
    """Open3D's loop as one thread runs it, over per-trial records fetch(first, n) -> dict(flags, count, sum_d2,
    transformation), asked for `chunk` trials at a time (which must not matter)."""
    best = dict(transformation=np.eye(4), count=0, rmse=0.0, sum_d2=0.0, best_trial=-1)
    trials = valid = 0
    if ncorr < ransac_n or max_iteration == 0:
        return dict(best, trials=0, valid_trials=0, fitness=0.0, inlier_rmse=0.0)
    est_k = float(max_iteration)
    i = 0
    rec, rec_first = None, 0
    while i < max_iteration and i < est_k:
        if rec is None or i >= rec_first + len(rec["flags"]):
            rec_first = i
            rec = fetch(i, int(min(chunk, max_iteration - i)))
        q = i - rec_first
        trials += 1
        if rec["flags"][q] & FLAG_SCORED:
            valid += 1
            count, total = int(rec["count"][q]), float(rec["sum_d2"][q])
            rmse = rmse_of(count, total)
            if count > best["count"] or (count == best["count"] and rmse < best["rmse"]):
                best = dict(transformation=np.array(rec["transformation"][q]), count=count, rmse=rmse, sum_d2=total,
                            best_trial=i)
                k = stop_k(confidence, count, ncorr, ransac_n)
                if k < est_k:
                    est_k = math.ceil(k) if math.isfinite(k) else k
        i += 1
    return dict(best, trials=trials, valid_trials=valid, fitness=best["count"] / ncorr if best["count"] else 0.0,
                inlier_rmse=best["rmse"])


def ransac(P, Q, corr, r, ransac_n=3, max_iteration=100000, confidence=0.999, seed=1, s=0.0, d=0.0, chunk=256):
    """The full call by the restatement alone (its own estimates)."""
    corr = np.asarray(corr).reshape(-1, 2)
    out = loop(lambda first, n: trial_records(P, Q, corr, r, first, n, ransac_n, s, d, seed), len(corr), ransac_n,
               max_iteration, confidence, chunk)
    if out["best_trial"] >= 0:
        out["inliers"] = corr[score(out["transformation"][None], records_of(P, Q, corr), r)[2][0]]
    else:
        out["inliers"] = np.zeros((0, 2), dtype=np.int32)
    return out


# ---- the batch tests/test_gpu_wide_batches.py and tests/test_wide_batch_cases.py share ----
WIDE_BATCH = 320
WIDE_CHUNKS = (4096, 3072, 2048, 1024)  # chunk_trials values of the wide test: 1, 2, 3 and 4 chunks in a group
WIDE_STAGE = 130  # trials of the wide test's stage call: past two tiles of 64


def group_chunks(chunk, batch):
    """The chunks the full call enqueues between two synchronisations: min(4, 2^21 / (chunk batch)), at least 1."""
    return max(1, min(4, (1 << 21) // (chunk * max(batch, 1))))


def wide_batch():
    """320 problems of 20 .. 40 pairs: dict(P, Q, corr, r, ransac_n, s, max_iteration, confidence, seed), one entry per
    problem.  Every 80th runs to its max_iteration (confidence 1) of 5 000, 7 000 or 13 000, every 16th after it has a
    quarter to a third of its pairs planted and stops after some hundreds of trials, the others stop after some tens; one problem
    has fewer pairs than ransac_n and one is empty.  What the wide test rests on is asserted from the sizes alone."""
    b = WIDE_BATCH
    out = dict(P=[], Q=[], corr=[], r=[], ransac_n=[], s=[], max_iteration=[], confidence=[], seed=[])
    long_runs = (5000, 7000, 13000)
    for i in range(b):
        rng = np.random.default_rng(7000 + i)
        ncorr = (20, 40, 33, 27)[i % 4]
        if i == 100:
            ncorr = 2
        if i == 200:
            ncorr = 0
        if i % 80 == 0:
            ratio, max_iteration, confidence = 0.5, long_runs[(i // 80) % 3], 1.0
        elif i % 16 == 1:
            ratio, max_iteration, confidence = (0.25, 0.3, 0.35)[(i // 16) % 3], 13000, 0.999
        else:
            ratio, max_iteration, confidence = (0.6, 0.7, 0.8)[(i // 4) % 3], 3000, 0.999
        n_s, n_t = (ncorr + 5, ncorr + 9) if ncorr else (0, 0)
        P = rng.uniform(-1.0, 1.0, (n_s, 3))
        Q = rng.uniform(-1.0, 1.0, (n_t, 3))
        a = rng.uniform(0.2, 1.0)
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        src, dst = rng.permutation(n_s)[:ncorr], rng.permutation(n_t)[:ncorr]
        n_in = int(round(ratio * ncorr))
        Q[dst[:n_in]] = P[src[:n_in]] @ R.T + np.array([0.1, -0.2, 0.3]) + rng.normal(0.0, 0.002, (n_in, 3))
        corr = np.stack([src, dst], axis=1)[rng.permutation(ncorr)] if ncorr else np.zeros((0, 2))
        for k, v in zip(out, (P, Q, np.ascontiguousarray(corr, dtype=np.int32), 0.02, (3, 4)[i % 2],
                              (0.0, 0.9)[i % 3 == 0], max_iteration, confidence, 9000 + i)):
            out[k].append(v)
    assert b > 256
    assert [group_chunks(c, b) for c in WIDE_CHUNKS] == [1, 2, 3, 4]
    full = [m for m, c in zip(out["max_iteration"], out["confidence"]) if c == 1.0]
    # at every chunk size some problem that never stops early is done within two groups of chunks, another needs a third
    assert all(min(full) <= 2 * group_chunks(c, b) * c < max(full) for c in WIDE_CHUNKS)
    assert all(sorted(full)[-2] > group_chunks(c, b) * c for c in WIDE_CHUNKS)
    assert out["confidence"][0] == 1.0 and out["confidence"][257] == 0.999 and out["max_iteration"][257] == 13000
    assert sum(len(c) < n for c, n in zip(out["corr"], out["ransac_n"])) == 2
    return out
