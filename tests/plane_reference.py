"""A numpy restatement of the plane-segmentation contract of include/teaser_hip.h ("Plane segmentation"), statement for
statement: the splitmix64 draws, both models, plane_from_points, the score in position order, Open3D's loop as one
thread runs it, and the finish.  Everything is meant bit for bit: numpy's elementwise float64 operations are IEEE and
never fused, and every contract sum is taken with cumsum (np.add.accumulate adds in order; np.sum is pairwise and is not
used).  A position that contributes nothing is given the term +0.0: a running sum that starts at +0.0 is never -0.0, so
adding +0.0 leaves its bits alone, which is the contract's "adds nothing".  The stop rule uses math.log and math.pow,
the C library's, with the IEEE special cases Python turns into exceptions put back.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

from ransac_reference import M64, draw

BLOCK, GROUP = 256, 64
FLAG_VALID = 1
SLAB = 128  # trials scored at a time (memory only)


def samples(seed, ransac_n, n, first, cnt):
    """[cnt, ransac_n] int32: c_k = z(seed, ransac_n i + k + 1) mod n for the trials first .. first + cnt - 1."""
    out = np.empty((cnt, ransac_n), dtype=np.int32)
    for q in range(cnt):
        for k in range(ransac_n):
            out[q, k] = draw(seed, (ransac_n * (first + q) + k + 1) & M64) % n
    return out


def _seq(terms):
    """The sum along the last axis in ascending order starting from 0.0."""
    z = np.zeros(terms.shape[:-1] + (1,))
    return np.cumsum(np.concatenate([z, terms], axis=-1), axis=-1)[..., -1]


def _pad(a, m):
    """The last axis of `a` padded with +0.0 to a multiple of m and cut into rows of m."""
    n = a.shape[-1]
    k = (n + m - 1) // m
    out = np.zeros(a.shape[:-1] + (k * m,))
    out[..., :n] = a
    return out.reshape(a.shape[:-1] + (k, m))


def position_sum(terms):
    """[..., n] -> [...]: the contract's position order (blocks of 256, groups of 64 blocks, groups)."""
    if terms.shape[-1] == 0:
        return np.zeros(terms.shape[:-1])
    blocks = _seq(_pad(terms, BLOCK))
    groups = _seq(_pad(blocks, GROUP))
    return _seq(groups)


def normalise(abc, anchor):
    """normalise(abc, anchor) per row: ([T, 4] planes, [T] bool not-zero-plane)."""
    a, b, c = abc[:, 0], abc[:, 1], abc[:, 2]
    with np.errstate(all="ignore"):
        ln = np.sqrt((a * a + b * b) + c * c)
        ok = (ln > 0.0) & np.isfinite(ln)
        a, b, c = a / ln, b / ln, c / ln
        s = (a * anchor[:, 0] + b * anchor[:, 1]) + c * anchor[:, 2]
        planes = np.stack([a, b, c, -s], axis=1)
    planes[~ok] = 0.0
    return planes, ok


def from_sums(cen, S):
    """Steps 3 .. 6 of plane_from_points per row: cen [T, 3], S [T, 6] = xx, xy, xz, yy, yz, zz."""
    xx, xy, xz, yy, yz, zz = (S[:, k] for k in range(6))
    with np.errstate(all="ignore"):
        det_x, det_y, det_z = yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy
        axis = np.zeros(len(S), dtype=np.int64)
        det_max = det_x.copy()
        pick = det_y > det_max
        axis[pick] = 1
        det_max[pick] = det_y[pick]
        axis[det_z > det_max] = 2
        cand = [np.stack([det_x, xz * yz - xy * zz, xy * yz - xz * yy], 1),
                np.stack([xz * yz - xy * zz, det_y, xy * xz - yz * xx], 1),
                np.stack([xy * yz - xz * yy, xy * xz - yz * xx, det_z], 1)]
    abc = np.where(axis[:, None] == 0, cand[0], np.where(axis[:, None] == 1, cand[1], cand[2]))
    return normalise(abc, cen)


def _products(r):
    x, y, z = r[..., 0], r[..., 1], r[..., 2]
    return [x * x, x * y, x * z, y * y, y * z, z * z]


def plane_from_samples(pts):
    """plane_from_points over pts [T, m, 3] in sample order, every sum sequential from 0.0."""
    m = pts.shape[1]
    cen = np.stack([_seq(pts[:, :, k]) for k in range(3)], 1) / float(m)
    S = np.stack([_seq(t) for t in _products(pts - cen[:, None, :])], 1)
    return from_sums(cen, S)


def plane_from_inliers(P, mask):
    """plane_from_points over the inliers of one cloud, all nine sums in position order."""
    P, mask = np.asarray(P, dtype=np.float64), np.asarray(mask, dtype=bool)
    m = int(mask.sum())
    if m == 0:
        return np.zeros(4)
    cen = np.array([position_sum(np.where(mask, P[:, k], 0.0)) for k in range(3)]) / float(m)
    S = np.array([position_sum(np.where(mask, t, 0.0)) for t in _products(P - cen[None, :])])
    return from_sums(cen[None, :], S[None, :])[0][0]


def models(P, smp):
    """([T, 4] planes, [T] uint8 flags) of the trials whose samples are the rows of smp."""
    P = np.asarray(P, dtype=np.float64)
    if smp.shape[1] == 3:
        p0, p1, p2 = P[smp[:, 0]], P[smp[:, 1]], P[smp[:, 2]]
        u, v = p1 - p0, p2 - p0
        abc = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                        u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        planes, ok = normalise(abc, p0)
    else:
        planes, ok = plane_from_samples(P[smp])
    return planes, ok.astype(np.uint8) * FLAG_VALID


def distances(P, planes):
    """[T, n]: dist = |((a x + b y) + c z) + d4|."""
    a, b, c, d4 = (planes[:, k, None] for k in range(4))
    return np.abs(((a * P[None, :, 0] + b * P[None, :, 1]) + c * P[None, :, 2]) + d4)


def score(P, planes, flags, d):
    """([T] int32 count, [T] E): over all points in position order; 0 where the trial is degenerate."""
    P = np.asarray(P, dtype=np.float64)
    count, E = np.zeros(len(planes), dtype=np.int32), np.zeros(len(planes))
    for lo in range(0, len(planes), SLAB):
        sl = slice(lo, lo + SLAB)
        dist = distances(P, planes[sl])
        inl = dist < d
        count[sl] = inl.sum(axis=1)
        E[sl] = position_sum(np.where(inl, dist, 0.0))
    dead = (flags & FLAG_VALID) == 0
    count[dead], E[dead] = 0, 0.0
    return count, E


def trials(P, d, ransac_n, seed, first, cnt):
    """What the stage call returns for one problem: samples, flags, plane, count, E."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    if n < ransac_n:
        return dict(samples=np.full((cnt, ransac_n), -1, dtype=np.int32), flags=np.zeros(cnt, dtype=np.uint8),
                    plane=np.zeros((cnt, 4)), count=np.zeros(cnt, dtype=np.int32), E=np.zeros(cnt))
    smp = samples(seed, ransac_n, n, first, cnt)
    planes, flags = models(P, smp)
    count, E = score(P, planes, flags, d)
    return dict(samples=smp, flags=flags, plane=planes, count=count, E=E)


def rmse_of(count, E):
    return float(E) / math.sqrt(float(count)) if count > 0 else 0.0


def _log(x):
    return -math.inf if x == 0.0 else math.log(x)


def stop_bound(count, n, probability, ransac_n, num_iterations):
    """k after a replacement: 0 when count == n, else min(log(1 - p) / log(1 - pow(fitness, ransac_n)), num_iterations)
    with min(a, b) = a < b ? a : b, the quotient first; IEEE division."""
    if count == n:
        return 0.0
    fitness = float(count) / float(n)
    num, den = _log(1.0 - probability), _log(1.0 - math.pow(fitness, float(ransac_n)))
    with np.errstate(all="ignore"):
        q = float(np.float64(num) / np.float64(den))
    cap = float(num_iterations)
    return q if q < cap else cap


def segment(P, d, ransac_n=3, num_iterations=100, probability=0.99999999, seed=1, slab=64):
    """The full call for one problem: plane, inliers, mask, fitness, inlier_rmse, best_trial, trials, valid_trials."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    best_count, best_rmse, best_trial, best_plane = 0, 0.0, -1, np.zeros(4)
    k, counted, visited = math.inf, 0, 0
    rec, rec_first = None, 0
    if n >= ransac_n:
        for i in range(num_iterations):
            if counted > k:
                break
            visited = i + 1
            if rec is None or i >= rec_first + slab:
                rec_first = i
                rec = trials(P, d, ransac_n, seed, i, min(slab, num_iterations - i))
            q = i - rec_first
            if not rec["flags"][q] & FLAG_VALID:
                continue
            count, rmse = int(rec["count"][q]), rmse_of(int(rec["count"][q]), rec["E"][q])
            if count > best_count or (count == best_count and rmse < best_rmse):
                best_count, best_rmse, best_trial, best_plane = count, rmse, i, rec["plane"][q].copy()
                k = stop_bound(count, n, probability, ransac_n, num_iterations)
            counted += 1
    out = dict(plane=np.zeros(4), inliers=np.zeros(0, dtype=np.int32), mask=np.zeros(n, dtype=np.uint8), fitness=0.0,
               inlier_rmse=0.0, best_trial=best_trial, trials=visited, valid_trials=counted)
    if best_trial < 0:
        return out
    mask = distances(P, best_plane[None, :])[0] < d
    out.update(plane=plane_from_inliers(P, mask), inliers=np.nonzero(mask)[0].astype(np.int32),
               mask=mask.astype(np.uint8), fitness=float(best_count) / float(n), inlier_rmse=best_rmse,
               winning_plane=best_plane)
    return out


# ---- the batch tests/test_gpu_wide_batches.py and tests/test_wide_batch_cases.py share ----
WIDE_CHUNK = 64  # chunk_trials of the wide test: one 64-hypothesis tile per chunk


def wide_batch():
    """320 clouds of 0 .. 65 points (normals_reference's sizes, half of each cloud planted on a plane), 70 trials each:
    dict(clouds, d, ransac_n, num_iterations, probability, seed), one entry per problem, with what the wide test rests
    on asserted from the sizes alone."""
    import normals_reference as RN
    import plane_scenes as SC
    b = RN.WIDE_BATCH
    n = [RN.WIDE_CYCLE[(i + RN.WIDE_ROTATE) % len(RN.WIDE_CYCLE)] for i in range(b)]
    ransac_n = [(3, 5, 4)[i % 3] for i in range(b)]
    num_iterations = [70] * b
    probability = [(1.0, 0.99)[(i // 3) % 2] for i in range(b)]  # 1.0: the loop never stops early
    assert b > 256  # plane_winner_kernel, plane_fin_total_kernel: a fifth 64-lane tile; blockIdx.y / .z past 255
    assert min(num_iterations) > WIDE_CHUNK  # a second chunk of trials, a partial one
    runs = [k >= r for k, r in zip(n, ransac_n)]
    assert any(runs) and not all(runs)  # "no plane" (n < ransac_n) and trials that run
    assert all(runs[i] for i in (0, 63, 64, 65, 255, 256, 257, b - 1)) and not runs[260]
    return dict(clouds=[SC.planted(n[i], 0.5, 2000 + i) for i in range(b)], d=[(0.01, 0.05)[i % 2] for i in range(b)],
                ransac_n=ransac_n, num_iterations=num_iterations, probability=probability,
                seed=[3000 + i for i in range(b)])
