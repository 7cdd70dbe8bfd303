"""Pins tests/keypoints_reference.py, the numpy restatement of the ISS keypoint contract the GPU is compared with bit
for bit: against straight Python loops on small clouds; on a cloud of small dyadic rationals, where every sum is exact,
the result does not depend on the sum order and permutes with the cloud; automatic radii follow the "both replaced"
rule; a 0 / 0 ratio fails its test; tied maxima survive together."""
import math

import numpy as np

import icp_gicp_reference as RG
import keypoints_reference as RK
import normals_reference as RN
import outlier_reference as RO


def loops(P, rs, rn, g21, g32, mn):
    """The contract in straight loops over Python floats (radii given and > 0)."""
    P = [[float(v) for v in p] for p in P]
    n = len(P)
    lo = [min(p[a] for p in P) for a in range(3)]
    hi = [max(p[a] for p in P) for a in range(3)]
    mag = max(max(abs(v) for v in lo), max(abs(v) for v in hi))
    inv_h = 1.0 / (rs * (1 + 1e-6) + 1e-12 * mag)
    cell = [tuple(int(min(max(math.floor((p[a] - lo[a]) * inv_h), -2.0), 1099511627776.0)) for a in range(3)) for p in P]

    def d2(i, j):
        dx, dy, dz = P[i][0] - P[j][0], P[i][1] - P[j][1], P[i][2] - P[j][2]
        return (dx * dx + dy * dy) + dz * dz

    sal, m_of, cnt = [0.0] * n, [0] * n, [0] * n
    for i in range(n):
        js = sorted((j for j in range(n) if d2(i, j) < rs * rs), key=lambda j: cell[j] + (j,))
        m_of[i] = m = len(js)
        cnt[i] = sum(1 for j in range(n) if d2(i, j) < rn * rn)
        if m < mn:
            continue
        s1, s2 = [0.0] * 3, [0.0] * 6
        for j in js:
            o = [P[j][a] - P[i][a] for a in range(3)]
            for a in range(3):
                s1[a] += o[a]
            for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                s2[k] += o[a] * o[b]
        cov = [(s2[k] - (s1[a] * s1[b]) / m) / m for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))]
        e3, e2, e1 = sorted(float(v) for v in RG.jacobi3(np.array(cov))[0])
        if e1 != 0 and e2 != 0 and e2 / e1 < g21 and e3 / e2 < g32:
            sal[i] = e3
    keep = [int(sal[i] > 0 and cnt[i] >= mn and not any(d2(i, j) < rn * rn and sal[j] > sal[i] for j in range(n)))
            for i in range(n)]
    return keep, sal, m_of, cnt


def test_against_straight_loops():
    kept = 0
    for P, rs, rn, g21, g32, mn in ((RN.cube(90, 1), 0.4, 0.3, 0.975, 0.975, 5), (RN.cube(70, 2), 0.3, 0.5, 0.9, 0.95, 3),
                                    (RN.planar(60), 0.35, 0.2, 0.975, 0.975, 5), (RN.tied_lattice(), 0.55, 0.3, 2.0, 2.0, 5),
                                    (RN.cube(50, 3) + 1e4, 0.5, 0.1, 2.0, 2.0, 0)):
        ref = RK.iss_keypoints(P, rs, rn, g21, g32, mn)
        keep, sal, m_of, cnt = loops(P, rs, rn, g21, g32, mn)
        assert ref["keep"].tolist() == keep and ref["count"][:, 0].tolist() == m_of and ref["count"][:, 1].tolist() == cnt
        assert ref["saliency"].tobytes() == np.array(sal).tobytes()
        assert np.isnan(ref["radii"][0]) and ref["radii"][1] == rs and ref["radii"][2] == rn
        kept += sum(keep)
    assert kept > 10


def test_exact_sums_do_not_depend_on_the_order_and_permute_with_the_cloud():
    P = RK.dyadic_cloud()
    rng = np.random.default_rng(2)
    ref = RK.iss_keypoints(P, 1.0, 0.75)
    shuffled = RK.iss_keypoints(P, 1.0, 0.75, order=lambda js: rng.permutation(js))
    assert ref["keep"].sum() > 0 and (ref["count"][:, 0] >= 5).mean() > 0.8  # sums of several terms
    assert shuffled["saliency"].tobytes() == ref["saliency"].tobytes() and np.array_equal(shuffled["keep"], ref["keep"])
    perm = rng.permutation(len(P))
    moved = RK.iss_keypoints(P[perm], 1.0, 0.75)
    assert moved["saliency"].tobytes() == ref["saliency"][perm].tobytes()
    assert np.array_equal(moved["keep"], ref["keep"][perm]) and np.array_equal(moved["count"], ref["count"][perm])
    # on a cloud whose sums round, the order does show: the contract has to name one
    Q = RN.cube(200, 8)
    a = RK.iss_keypoints(Q, 0.3, 0.2, 2.0, 2.0)
    b = RK.iss_keypoints(Q, 0.3, 0.2, 2.0, 2.0, order=lambda js: js[::-1])
    assert a["saliency"].tobytes() != b["saliency"].tobytes() and np.allclose(a["saliency"], b["saliency"], rtol=1e-9)


def test_automatic_radii_replace_both():
    P = RN.cube(300, 4)
    res = RK.resolution(P)
    d = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(d, np.inf)
    assert abs(res - d.min(axis=1).mean()) < 1e-12
    for rs, rn in ((0.0, 0.0), (0.0, 0.2), (0.3, 0.0)):
        got = RK.iss_keypoints(P, rs, rn)["radii"]
        assert got[0] == res and got[1] == 6.0 * res and got[2] == 4.0 * res
    given = RK.iss_keypoints(P, 0.3, 0.2)["radii"]
    assert np.isnan(given[0]) and given[1] == 0.3 and given[2] == 0.2
    for Q in (np.zeros((0, 3)), RN.cube(1), RN.identical()):  # a resolution of 0: no neighbours, no keypoints
        out = RK.iss_keypoints(Q)
        assert out["radii"].tolist() == [0.0, 0.0, 0.0] and not out["keep"].any() and not out["count"].any()
        assert not out["saliency"].any()


def test_a_nan_ratio_fails_its_test():
    P = RN.identical()  # every covariance is the zero matrix: e2 / e1 = 0 / 0
    out = RK.iss_keypoints(P, 0.1, 0.1, 2.0, 2.0, 0)
    assert (out["count"] == len(P)).all() and not out["saliency"].any() and not out["keep"].any()
    assert RK.saliency_of(np.zeros(6), 2.0, 2.0) == 0.0
    line = RK.iss_keypoints(RN.collinear(), 0.6, 0.4, 2.0, 2.0, 2)  # e3 = e2 = 0 up to rounding: never a positive saliency above e2
    assert (line["saliency"] >= 0).all()


def test_tied_maxima_survive_together():
    X = RN.tied_lattice()
    rn = 0.6
    out = RK.iss_keypoints(X, 0.3, rn, 2.0, 2.0, 5)
    kept = np.flatnonzero(out["keep"])
    D = RO.squared_distances(X, kept)[:, kept]
    s = out["saliency"][kept]
    tied = [(a, b) for a in range(len(kept)) for b in range(a + 1, len(kept)) if D[a, b] < rn * rn and s[a] == s[b]]
    assert len(kept) > 1 and len(tied) > 10  # keypoints inside each other's suppression ball with equal saliency bits
    assert (s > 0).all()


def test_key_bits_on_hand_computed_cases():
    one = np.array([[3.0, -2.0, 7.5]])
    two_cells = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]])  # r = 0.3: c_x in {0, 1}, one bit; r = 0.2: {0, 2}, two
    assert RK.key_bits([one], 0.4, 0.3, details=True) == (1, 0, 1, [(0, 0)])  # ids 0 and 1: one bit
    assert RK.key_bits([two_cells], 0.6, 0.3, details=True) == (2, 1, 1, [(0, 1)])
    assert RK.key_bits([two_cells], 0.3, 0.2, details=True) == (3, 2, 1, [(1, 2)])
    assert RK.key_bits([two_cells, one], 0.3, 0.2) == 2 + 2          # ids 0 .. 3
    assert RK.key_bits([two_cells] + [one] * 256, 0.3, 0.2) == 2 + 10  # batch 257: ids 0 .. 513
    assert RK.key_bits([two_cells] + [one] * 255, 0.3, 0.2) == 2 + 9   # batch 256: ids 0 .. 511
    # a cloud without neighbours to find has no grid: empty, or a resolution of 0
    assert RK.key_bits([np.zeros((0, 3)), RN.identical()], [0.3, 0.0], [0.2, 0.0], details=True)[1] == 0
    box = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.25]])
    assert [int(v) for v in RK.cells(box, 0.1).max(axis=0)] == [9, 4, 2]
    assert RK.key_bits([box], 0.1, 0.1, details=True) == (4 + 3 + 2 + 1, 9, 1, [(9, 9)])
    assert RK.refused_for_width([box], 0.1, 0.1) is None


def test_key_bits_of_the_clouds_at_the_63_bit_boundary():
    """The clouds and radii of tests/test_gpu_keypoints.py's key-width tests and of tests/test_gpu_batch_width.py."""
    others = [RN.cube(65, 65), None, np.zeros((0, 3)), RN.cube(129, 129)]

    def batched(X):
        return RK.key_bits([X if c is None else c for c in others], 0.4, 0.3, details=True)

    a = RK.corner_clusters(512.0, 512.0, 512.0)
    assert RK.key_bits([a], 0.4, 0.3, details=True) == (34, 33, 1, [(33, 33)]) and batched(a)[:3] == (36, 33, 3)
    b = RK.corner_clusters(393216.0, 393216.0, 196608.0)
    assert RK.key_bits([b], 0.4, 0.3, details=True) == (63, 62, 1, [(59, 62)])
    b4 = RK.corner_clusters(196608.0, 196608.0, 196608.0)
    assert batched(b4)[:3] == (63, 60, 3) and RK.refused_for_width([b4], 0.4, 0.3) is None
    c = RK.corner_clusters(393216.0, 393216.0, 393216.0)
    assert RK.key_bits([c], 0.4, 0.3, details=True) == (64, 63, 1, [(60, 63)])
    assert RK.refused_for_width([c], 0.4, 0.3) == (0, "non_max_radius")
    assert RK.key_bits([c], 0.3, 0.45, details=True) == (64, 63, 1, [(63, 60)])
    assert RK.refused_for_width([c], 0.3, 0.45) == (0, "salient_radius")
    assert RK.refused_for_width([RN.cube(65, 5), c], [0.4, 0.4], [0.3, 0.3]) == (1, "non_max_radius")
    assert RK.refused_for_width([RN.cube(65, 5), c], [0.4, 0.3], [0.3, 0.45]) == (1, "salient_radius")
    wide = RN.wide_batch()
    p = RK.wide_batch_params(len(wide))
    bits, cell_bits, id_bits, widths = RK.key_bits(wide, [q.get("salient_radius", 0.0) for q in p],
                                                   [q.get("non_max_radius", 0.0) for q in p], details=True)
    assert len(wide) == 320 and id_bits == 10 and bits == cell_bits + 10 <= 63
    assert widths[260] == (0, 0) and max(widths[256]) > 0
