"""Numpy restatement of the ISS keypoint contract of include/teaser_hip.h ("ISS keypoints"), built on the pieces the
earlier contracts are pinned with: outlier_reference.self_knn / block_sum / squared_distances, icp_gicp_reference.jacobi3
and normals_reference.ascending3.  It adds what is new: the resolution and the "both radii replaced" rule, the cell
coordinates of the handle's grid (icp_cell / set_grid of csrc/icp_internal.h and icp_host.h, restated in FP64), the
uncapped neighbourhood summed in ascending (c_x, c_y, c_z, j), the population covariance, the two ratio tests and the
non-maximum suppression with its strict comparison."""
import numpy as np

import icp_gicp_reference as RG
import normals_reference as RN
import outlier_reference as RO


def resolution(P):
    """Open3D's ComputeModelResolution: the mean distance to the nearest other point (slot 1 of self k-NN, k = 2),
    summed by the 256-block rule; 0 when n < 2."""
    n = len(P)
    if n < 2:
        return np.float64(0.0)
    _, d2 = RO.self_knn(P, 2)
    return RO.block_sum(np.sqrt(d2[:, 1]), np.ones(n, dtype=bool)) / np.float64(n)


def radii(P, salient_radius, non_max_radius):
    """(res or NaN, r_s, r_n): both radii are replaced when either is 0."""
    rs, rn = np.float64(salient_radius), np.float64(non_max_radius)
    if rs == 0.0 or rn == 0.0:
        res = resolution(P)
        return res, np.float64(6.0) * res, np.float64(4.0) * res
    return np.float64(np.nan), rs, rn


def cells(P, r):
    """n x 3 int64: icp_cell per axis with the cell edge and origin set_grid computes from r and the bounding box."""
    lo, hi = P.min(axis=0), P.max(axis=0)
    mag = np.float64(max(np.abs(lo).max(), np.abs(hi).max()))
    edge = np.float64(r) * np.float64(1 + 1e-6) + np.float64(1e-12) * mag
    inv_h = np.float64(1.0) / edge
    v = np.floor((P - lo[None, :]) * inv_h)
    return np.clip(v, -2.0, 1099511627776.0).astype(np.int64)


def bits_for(v):
    """Number of bits that hold every value in [0, v]."""
    return int(v).bit_length()


def key_bits(clouds, r_s, r_n, details=False):
    """The width of the call's cell keys (icp_keypoints.hip, "descriptors, grids and the key layout"): per cloud with
    neighbours to find (n > 0, both radii squared > 0) each grid needs the sum over the axes of bits_for(its largest
    cell coordinate); the cell field is as wide as the wider grid of the widest cloud, and the grid id above it
    (cloud b: b for r_s, batch + b for r_n) is bits_for(2 batch - 1) wide.  r_s, r_n: one value for all clouds or one
    per cloud, 0 meaning automatic as in iss_keypoints.  details=True: (bits, cell bits, id bits, [(w_s, w_n) per
    cloud]).  A call is served up to 63 bits."""
    b = len(clouds)
    r_s = np.broadcast_to(np.asarray(r_s, dtype=np.float64), (b,))
    r_n = np.broadcast_to(np.asarray(r_n, dtype=np.float64), (b,))
    widths = []
    for c, rs, rn in zip(clouds, r_s, r_n):
        P = np.asarray(c, dtype=np.float64).reshape(-1, 3)
        _, rs, rn = radii(P, rs, rn)
        if len(P) == 0 or not rs * rs > 0 or not rn * rn > 0:
            widths.append((0, 0))
            continue
        widths.append(tuple(sum(bits_for(m) for m in cells(P, r).max(axis=0)) for r in (rs, rn)))
    cell_bits = max([max(w) for w in widths], default=0)
    id_bits = bits_for(2 * b - 1) if b else 0
    if details:
        return cell_bits + id_bits, cell_bits, id_bits, widths
    return cell_bits + id_bits


def refused_for_width(clouds, r_s, r_n):
    """None when the call's keys fit in 63 bits, else (cloud, "salient_radius" or "non_max_radius"): the first cloud
    whose wider grid is the call's widest, and r_s when its r_s grid is that wide -- what the refusal names."""
    bits, cell_bits, _, widths = key_bits(clouds, r_s, r_n, details=True)
    if bits <= 63:
        return None
    for c, (ws, wn) in enumerate(widths):
        if max(ws, wn) == cell_bits:
            return c, "salient_radius" if ws == cell_bits else "non_max_radius"


def population_covariance(P, i, js):
    """The six upper entries (00 01 02 11 12 22) of (S2 - S1 S1^T / m) / m, the sums added one neighbour at a time in
    the order of js from 0."""
    o = P[js] - P[i]
    m = np.float64(len(js))
    s1 = RG._seq(o)
    prod = np.stack([o[:, 0] * o[:, 0], o[:, 0] * o[:, 1], o[:, 0] * o[:, 2], o[:, 1] * o[:, 1], o[:, 1] * o[:, 2],
                     o[:, 2] * o[:, 2]], 1)
    s2 = RG._seq(prod)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    with np.errstate(all="ignore"):
        return np.array([(s2[k] - (s1[a] * s1[b]) / m) / m for k, (a, b) in enumerate(pairs)])


def saliency_of(a6, gamma_21, gamma_32):
    """e3 when e2 / e1 < gamma_21 and e3 / e2 < gamma_32, else 0 (a NaN ratio fails its test)."""
    diag, _ = RG.jacobi3(a6)
    e3, e2, e1 = RN.ascending3(diag[0], diag[1], diag[2])
    with np.errstate(all="ignore"):
        ok = np.float64(e2) / np.float64(e1) < gamma_21 and np.float64(e3) / np.float64(e2) < gamma_32
    return np.float64(e3) if ok else np.float64(0.0)


def iss_keypoints(points, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5,
                  order=None):
    """dict(keep uint8 n, saliency n, count n x 2 int32 (m, cnt), radii (res or NaN, r_s, r_n)).  order: None, or a
    function js -> js that reorders a neighbour list before the sums (the order experiment of the tests)."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    res, rs, rn = radii(P, salient_radius, non_max_radius)
    out = dict(keep=np.zeros(n, dtype=np.uint8), saliency=np.zeros(n), count=np.zeros((n, 2), dtype=np.int32),
               radii=np.array([res, rs, rn]))
    rs2, rn2 = rs * rs, rn * rn
    if n == 0 or not (rs2 > 0) or not (rn2 > 0):  # no j has d2 < 0: no neighbours, no keypoints, no grid
        return out
    g21, g32 = np.float64(gamma_21), np.float64(gamma_32)
    c = cells(P, rs)
    sal = out["saliency"]
    near = []
    for i in range(n):
        D = RO.squared_distances(P, [i])[0]
        js = np.flatnonzero(D < rs2)
        js = js[np.lexsort((js, c[js, 2], c[js, 1], c[js, 0]))]
        out["count"][i, 0] = len(js)
        near.append(np.flatnonzero(D < rn2))
        out["count"][i, 1] = len(near[i])
        if len(js) >= min_neighbors:
            sal[i] = saliency_of(population_covariance(P, i, js if order is None else order(js)), g21, g32)
    for i in range(n):
        if sal[i] > 0 and len(near[i]) >= min_neighbors and not (sal[near[i]] > sal[i]).any():
            out["keep"][i] = 1
    return out


def dyadic_cloud(n=150, seed=11):
    """Coordinates k / 16, k in [0, 64): every offset, product and sum of a neighbourhood is exact in FP64, so a
    covariance does not depend on the order of its sums."""
    return np.random.default_rng(seed).integers(0, 64, size=(n, 3)).astype(np.float64) / 16.0


def corner_clusters(sx, sy, sz):
    """Eight tight clusters of 40 points (half-unit cubes) at the corners of a box: keypoints exist inside the
    clusters, while the cell coordinates span side / cell edge per axis."""
    return np.concatenate([RN.cube(40, 60 + k) * 0.5 + np.array([sx * (k & 1), sy * (k >> 1 & 1), sz * (k >> 2 & 1)])
                           for k in range(8)])


def wide_batch_params(b):
    """Per cloud of normals_reference.wide_batch() the ISS parameters that differ from the defaults: odd clouds keep
    the automatic radii, min_neighbors cycles, every third cloud passes both ratio tests."""
    params = []
    for i in range(b):
        p = dict(min_neighbors=(0, 3, 5)[i % 3])
        if i % 2 == 0:
            p.update(salient_radius=0.4, non_max_radius=0.3)
        if i % 3 == 0:
            p.update(gamma_21=2.0, gamma_32=2.0)
        params.append(p)
    return params
