"""numpy restatement of the voxel down-sampling contract (include/teaser_hip.h, "Voxel down-sampling"), the yardstick
of tests/test_gpu_voxel.py.  Open3D's arithmetic: lo = min_bound - v/2, i = floor((p - lo) / v) in FP64; each occupied
voxel's output is (0 + p_0 + p_1 + ...) / count with its points added one at a time in input order; voxels in
ascending (i_x, i_y, i_z) order.  The sums are written out step by step (step t adds every voxel's t-th point), so
nothing depends on the order in which a numpy reduction happens to add."""
import numpy as np

INT_MAX = 2 ** 31 - 1


def check_args(points, voxel_size):
    """The refusal rule: raises ValueError naming the argument, as the library answers BAD_ARG."""
    v = float(voxel_size)
    if not np.isfinite(v) or not v > 0:
        raise ValueError("voxel_size must be finite and > 0")
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if len(p) == 0:
        return
    if not np.all(np.isfinite(p)):
        raise ValueError("points has a non-finite coordinate")
    lo = p.min(0) - 0.5 * v
    hi = p.max(0) + 0.5 * v
    if v * INT_MAX < np.max(hi - lo):
        raise ValueError("voxel_size is too small for 32-bit voxel indices")


def voxel_indices(points, voxel_size):
    """n x 3 int64 voxel indices floor((p - (min_bound - v/2)) / v)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    v = float(voxel_size)
    lo = p.min(0) - 0.5 * v
    return np.floor((p - lo) / v).astype(np.int64)


def voxel_down_sample(points, voxel_size):
    """Returns (means n_out x 3 float64, counts n_out int32, trace n int32) -- trace[i] = output voxel of point i."""
    check_args(points, voxel_size)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if n == 0:
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    idx = voxel_indices(p, voxel_size)
    # stable LSD sort: by i_z, then i_y, then i_x -- points of one voxel keep their input order
    order = np.argsort(idx[:, 2], kind="stable")
    for a in (1, 0):
        order = order[np.argsort(idx[order, a], kind="stable")]
    sidx = idx[order]
    head = np.ones(n, dtype=bool)
    head[1:] = np.any(sidx[1:] != sidx[:-1], axis=1)
    start = np.flatnonzero(head)
    count = np.diff(np.append(start, n))
    # step t adds the t-th point of every voxel that has one (longest voxels first, so the active ones are a prefix)
    by_len = np.argsort(-count, kind="stable")
    s_start, s_count = start[by_len], count[by_len]
    sp = p[order]
    sums = np.zeros((len(start), 3))
    for t in range(int(s_count[0])):
        m = int(np.searchsorted(-s_count, -t, side="left"))  # voxels with count > t
        sums[:m] += sp[s_start[:m] + t]
    acc = np.empty_like(sums)
    acc[by_len] = sums
    means = acc / count[:, None].astype(np.float64)
    trace = np.empty(n, dtype=np.int32)
    trace[order] = (np.cumsum(head) - 1).astype(np.int32)
    return means, count.astype(np.int32), trace


def bits_for(v):
    """Number of bits that hold every value in [0, v]."""
    return int(v).bit_length()


def key_bits(clouds, sizes):
    """The sort key the library lays out for this call (voxel.hip, "key layout"): (bits, shifts, prob_shift).  Per
    non-empty cloud the fields i_z, i_y, i_x from bit 0 up, each bits_for(the axis' largest voxel index) wide: shifts[b]
    = (shift of i_x, of i_y, of i_z), None for an empty cloud.  The problem index sits above the widest cloud, at
    prob_shift, and is bits_for(batch - 1) wide; bits is the whole width, at least 1.  Up to 64 bits the sort is one
    pass over the low word; above, a second pass sorts the bits - 64 bits of the high word."""
    sizes = np.broadcast_to(np.asarray(sizes, dtype=np.float64), (len(clouds),))
    shifts, widest = [], 0
    for c, v in zip(clouds, sizes):
        p = np.asarray(c, dtype=np.float64).reshape(-1, 3)
        if len(p) == 0:
            shifts.append(None)
            continue
        bx, by, bz = (bits_for(m) for m in voxel_indices(p, v).max(0))
        shifts.append((by + bz, bz, 0))
        widest = max(widest, bx + by + bz)
    return max(1, widest + bits_for(max(len(clouds) - 1, 0))), shifts, widest


def corner_cloud(a, b, c, seed, n=300):
    """v = 1: the origin and the corner (2^a - 1, 2^b - 1, 2^c - 1) fix the largest voxel indices, hence a, b and c key
    bits; between them n random points, a third of them on exact faces (x = k + 1/2), and a copy of the first 100
    moved by 1/4, most of which share their voxel with the original."""
    rng = np.random.default_rng(seed)
    corner = np.array([2.0 ** a - 1, 2.0 ** b - 1, 2.0 ** c - 1])
    p = rng.uniform(0, corner - 2, size=(n, 3))
    p[: n // 3] = np.floor(p[: n // 3]) + 0.5
    p = np.concatenate([[[0.0, 0.0, 0.0]], p, p[:100] + 0.25, [corner]])
    return p[rng.permutation(len(p))]


def line_of_runs(lengths, seed):
    """Voxel j of a line along x (v = 1) holds exactly lengths[j] points, uniform inside it, the cloud shuffled."""
    rng = np.random.default_rng(seed)
    j = np.repeat(np.arange(len(lengths)), lengths)
    p = rng.uniform(0, 0.5, size=(len(j), 3))  # min_bound 0 (set below) -> lo = -1/2: voxel j is [j - 1/2, j + 1/2)
    p[0] = 0.0
    p[:, 0] += j
    return p[rng.permutation(len(p))]


def many_runs(runs, length, tail, seed):
    """`runs` voxels of exactly `length` points each and `tail` voxels of one point, on a 128-wide sheet of voxels
    (v = 1), the points uniform inside their voxel, the cloud shuffled."""
    rng = np.random.default_rng(seed)
    cell = np.arange(runs + tail)
    cell = np.stack([cell // 128, cell % 128, np.zeros_like(cell)], 1).astype(np.float64)
    p = np.concatenate([np.repeat(cell[:runs], length, axis=0), cell[runs:]])
    p += rng.uniform(0, 0.5, size=p.shape)
    p[0] = 0.0  # min_bound 0 -> lo = -1/2
    return p[rng.permutation(len(p))]


def scan_like(seed=5, n=313395, offset=0.0):
    """A room-sized scan: noisy planes (floor, walls, a table) and a few blobs, float32 like a PLY."""
    rng = np.random.default_rng(seed)
    parts = []
    k = n // 6
    u = rng.uniform(0, 1, size=(5, k, 2))
    parts.append(np.stack([3 * u[0, :, 0], 2.5 * u[0, :, 1], 0.005 * rng.standard_normal(k)], 1))       # floor
    parts.append(np.stack([3 * u[1, :, 0], 0.005 * rng.standard_normal(k), 2.4 * u[1, :, 1]], 1))       # wall
    parts.append(np.stack([0.005 * rng.standard_normal(k), 2.5 * u[2, :, 0], 2.4 * u[2, :, 1]], 1))     # wall
    parts.append(np.stack([1 + 0.8 * u[3, :, 0], 1 + 0.6 * u[3, :, 1], 0.75 + 0.003 * rng.standard_normal(k)], 1))
    parts.append(np.stack([2 + 0.3 * u[4, :, 0], 0.5 + 0.3 * u[4, :, 1], 2 * u[4, :, 0] * u[4, :, 1]], 1))
    rest = n - 5 * k
    parts.append(rng.normal([1.5, 1.2, 1.0], 0.2, size=(rest, 3)))
    p = np.concatenate(parts)[rng.permutation(n)]
    return (p + offset).astype(np.float32).astype(np.float64)
