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
