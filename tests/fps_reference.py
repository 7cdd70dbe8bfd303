"""The numpy restatement of farthest-point down-sampling (include/teaser_hip.h, "Farthest-point down-sampling"):
Open3D's PointCloud.farthest_point_down_sample loop vectorised per round, a literal transcription of the scalar loop to
check the vectorised form against, brute-force forms of the two distance outputs, and the scenes the tests share.
numpy contracts nothing, so d2 = ((dx dx + dy dy) + dz dz) is the contract's expression bit for bit."""
import numpy as np


def fps(P, K, start=0):
    """(index int32 [K], sel_dist float64 [K], final_dist float64 [n]) of the contract."""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    assert 0 <= K <= n and (K == 0 or 0 <= start < n)
    index = np.zeros(K, dtype=np.int32)
    sel = np.zeros(K, dtype=np.float64)
    d = np.full(n, np.inf)
    cur = int(start)
    x, y, z = P[:, 0].copy(), P[:, 1].copy(), P[:, 2].copy()
    with np.errstate(over="ignore"):
        for k in range(K):
            index[k] = cur
            sel[k] = d[cur]
            dx, dy, dz = x - x[cur], y - y[cur], z - z[cur]
            v = (dx * dx + dy * dy) + dz * dz
            d = np.where(v < d, v, d)
            m = int(np.argmax(d))  # the first of the largest: the smallest index
            if d[m] > 0:
                cur = m
    return index, sel, d


def fps_literal(P, K, start=0):
    """The scalar loop, statement for statement: Open3D's max_dist = 0 with its strict > (which keeps the first of equal
    distances and keeps the current sample when every distance is 0)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    index, sel = [], []
    d = [np.inf] * n
    cur = int(start)
    with np.errstate(over="ignore"):
        for _ in range(K):
            index.append(cur)
            sel.append(d[cur])
            c = P[cur]
            max_dist, nxt = 0.0, cur
            for j in range(n):
                dx, dy, dz = P[j, 0] - c[0], P[j, 1] - c[1], P[j, 2] - c[2]
                v = (dx * dx + dy * dy) + dz * dz
                if v < d[j]:
                    d[j] = v
                if d[j] > max_dist:
                    max_dist, nxt = d[j], j
            cur = nxt
    return np.array(index, dtype=np.int32), np.array(sel, dtype=np.float64), np.array(d, dtype=np.float64)


def d2_matrix(A, B):
    """d2 of the contract between every point of A and every point of B (differences A minus B)."""
    e = A[:, None, :] - B[None, :, :]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def brute_sel_dist(P, index):
    """sel_dist from its meaning: +inf, then the smallest d2 of sample k to the samples before it."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    S = P[index]
    out = np.full(len(index), np.inf)
    for k in range(1, len(index)):
        out[k] = d2_matrix(S[k:k + 1], S[:k]).min()
    return out


def brute_final_dist(P, index):
    """final_dist from its meaning: the smallest d2 of every point to the sample set."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    if len(index) == 0:
        return np.full(len(P), np.inf)
    return d2_matrix(P, P[index]).min(axis=1)


# ---- scenes --------------------------------------------------------------------------------------------------------------
def lattice(rng, n, side=6):
    """n points with integer coordinates 0 .. side - 1: every d2 exact, ties and repeated positions everywhere."""
    return rng.integers(0, side, size=(n, 3)).astype(np.float64)


def planted(n, at, seed=0):
    """A lattice cloud in [0, 5]^3 whose point `at` lies far outside: from start_index != at it is the unique farthest
    point of the first round."""
    P = lattice(np.random.default_rng(1000 + seed), n)
    P[at] = (40.0, 50.0, 60.0)
    return P


def gaussian(rng, n):
    """N(0, 1) + 1 000: products and sums round, so a fused d2 would show."""
    return rng.standard_normal((n, 3)) + 1000.0


def identical(n=513):
    return np.full((n, 3), 2.5)


def three_positions(n=600):
    """n points on 3 distinct positions, interleaved."""
    pos = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 5.0, 1.0]])
    return pos[np.arange(n) % 3]


WIDE_CAPACITY = 10240  # the default of "fps_resident_max" (kFpsResidentCap): the largest cloud the resident route serves
WIDE_LARGE = (0, 256, 257, 319)  # where the clouds above it stand in the wide batch


def wide_batch():
    """normals_reference.wide_batch()'s 320 clouds of 0 .. 65 points, four of them replaced by clouds of
    WIDE_CAPACITY + 1 points, with the sample counts 0, 1, n and min(n, 7) and the start indices 0, n - 1 and n / 2 in
    turn: (clouds, K, start).  What the wide test rests on is asserted from the sizes alone."""
    import normals_reference as RN
    clouds = RN.wide_batch()
    b = len(clouds)
    rng = np.random.default_rng(41)
    for i in WIDE_LARGE:
        clouds[i] = gaussian(rng, WIDE_CAPACITY + 1)
    n = [len(P) for P in clouds]
    K = [(0, 1, n[i], min(n[i], 7))[i % 4] for i in range(b)]
    for i, k in zip(WIDE_LARGE, (5, 17, 1, 33)):
        K[i] = k
    start = [0 if n[i] == 0 else (0, n[i] - 1, n[i] // 2)[i % 3] for i in range(b)]
    assert b > 256 and WIDE_LARGE[-1] == b - 1
    streamed = [i for i in range(b) if n[i] > WIDE_CAPACITY]
    resident = [i for i in range(b) if 0 < n[i] <= WIDE_CAPACITY and K[i] > 0]
    # the resident map: a workgroup per resident cloud, past 128 of them; the block map of the others: past 128 blocks
    assert tuple(streamed) == WIDE_LARGE and len(resident) > 128 and sum((n[i] + 255) // 256 for i in streamed) > 128
    assert all(K[i] > 0 for i in WIDE_LARGE) and any(K[i] == n[i] > 1 for i in range(b)) and any(k == 0 for k in K)
    return clouds, K, start
