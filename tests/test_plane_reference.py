"""The numpy restatement of the plane-segmentation contract (tests/plane_reference.py) alone, without a GPU, against
facts it does not compute itself: an exact integer-grid plane, a planted plane under clutter, plane_from_points in
exact rational arithmetic, the stop rule's special cases as IEEE lets them fall, the draws of the RANSAC restatement,
and the behaviours of the chosen seeds that the GPU tests rely on."""
import math
from fractions import Fraction

import numpy as np

import plane_reference as PR
import plane_scenes as SC
import ransac_reference as RR


def test_draws_are_the_ransac_restatements():
    for seed, n, m, first in ((0x5EED, 3, 7, 2), (99, 5, 1000, (1 << 32) + 3), (2 ** 64 - 1, 8, 257, 0)):
        assert np.array_equal(PR.samples(seed, n, m, first, 6), RR.samples(seed, n, m, first, 6))
    assert PR.samples(7, 3, 11, 4, 1).tolist() == [[RR.draw(7, 3 * 4 + k + 1) % 11 for k in range(3)]]


def test_exact_grid_plane_is_found_by_the_first_trial():
    for ransac_n, seed in ((3, 5), (5, 6)):
        P = SC.grid_plane(300)
        r = PR.segment(P, 1e-9, ransac_n, 1000, 0.99999999, seed)
        assert r["trials"] == 1 and r["valid_trials"] == 1 and r["best_trial"] == 0
        assert len(r["inliers"]) == 300 and r["fitness"] == 1.0 and r["mask"].all()
        sign = 1.0 if r["plane"][0] > 0 else -1.0
        assert np.abs(sign * r["plane"] - SC.GRID_PLANE).max() < 1e-12


def test_planted_plane_under_half_clutter_is_recovered():
    P = SC.planted(2000, 0.5, 21)
    d = 0.01
    r = PR.segment(P, d, 3, 1000, 0.99999999, 77)
    assert 0 < r["trials"] < 1000 and r["best_trial"] >= 0
    w = r["plane"] * (1.0 if r["plane"][2] > 0 else -1.0)
    assert np.abs(w - SC.PLANTED_NORMAL).max() < d
    truth = np.abs(P @ SC.PLANTED_NORMAL[:3] + SC.PLANTED_NORMAL[3]) < 0.004
    assert (r["mask"].astype(bool) & truth).sum() > 0.9 * truth.sum()
    assert r["fitness"] == len(r["inliers"]) / 2000.0 and 0.4 < r["fitness"] < 0.62


def _fraction_plane(pts):
    """plane_from_points up to the normalisation, in exact arithmetic: (axis, abc, centroid)."""
    m = len(pts)
    cen = [sum(Fraction(int(p[k])) for p in pts) / m for k in range(3)]
    r = [[Fraction(int(p[k])) - cen[k] for k in range(3)] for p in pts]
    s = lambda a, b: sum(q[a] * q[b] for q in r)  # noqa: E731
    xx, xy, xz, yy, yz, zz = s(0, 0), s(0, 1), s(0, 2), s(1, 1), s(1, 2), s(2, 2)
    dets = [yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy]
    axis = 0
    if dets[1] > dets[axis]:
        axis = 1
    if dets[2] > dets[axis]:
        axis = 2
    abc = [[dets[0], xz * yz - xy * zz, xy * yz - xz * yy], [xz * yz - xy * zz, dets[1], xy * xz - yz * xx],
           [xy * yz - xz * yy, xy * xz - yz * xx, dets[2]]][axis]
    return axis, abc, cen


def test_plane_from_points_agrees_with_exact_rational_arithmetic():
    rng = np.random.default_rng(3)
    for m in (4, 5, 8, 300, 700):
        pts = rng.integers(-50, 50, size=(m, 3)).astype(np.float64)
        axis, abc, cen = _fraction_plane(pts)
        ln = math.sqrt(float(sum(c * c for c in abc)))
        want = np.array([float(c) / ln for c in abc] + [-float(sum(c * q for c, q in zip(abc, cen))) / ln])
        assert abs(want[axis]) == max(abs(want[:3]))
        if m <= 8:
            got, ok = PR.plane_from_samples(pts[None, :, :])
            assert ok[0] and np.abs(got[0] - want).max() < 1e-12
        got = PR.plane_from_inliers(pts, np.ones(m, dtype=bool))
        assert np.abs(got - want).max() < 1e-11
        mask = rng.uniform(size=m) < 0.5
        mask[:4] = True
        axis, abc, cen = _fraction_plane(pts[mask])
        ln = math.sqrt(float(sum(c * c for c in abc)))
        want = np.array([float(c) / ln for c in abc] + [-float(sum(c * q for c, q in zip(abc, cen))) / ln])
        assert np.abs(PR.plane_from_inliers(pts, mask) - want).max() < 1e-11
    # the determinant tie (the corners of a cube: all three are 4): the first axis wins; a line gives the zero plane
    cube = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])
    got, ok = PR.plane_from_samples(cube[None])
    assert ok[0] and got[0].tolist() == [1.0, 0.0, 0.0, -0.5]
    got, ok = PR.plane_from_samples(SC.collinear(8)[None])
    assert not ok[0] and not got.any()
    assert not PR.plane_from_inliers(SC.collinear(40), np.ones(40, dtype=bool)).any()


def test_position_sum_is_blocks_then_groups_then_total():
    rng = np.random.default_rng(4)
    for n in (1, 255, 256, 257, 16384, 16385, 2 * 16384 + 1):
        t = rng.uniform(0, 1, size=n)
        total = 0.0
        for g0 in range(0, n, 256 * 64):
            gs = 0.0
            for b0 in range(g0, min(n, g0 + 256 * 64), 256):
                bs = 0.0
                for x in t[b0:b0 + 256]:
                    bs += x
                gs += bs
            total += gs
        assert PR.position_sum(t[None, :])[0] == total
    assert PR.position_sum(np.zeros((2, 0))).tolist() == [0.0, 0.0]


def test_stop_rule_special_cases():
    assert PR.stop_bound(10, 10, 0.99, 3, 100) == 0.0                  # count = n
    assert PR.stop_bound(5, 10, 1.0, 3, 100) == 100.0                   # probability = 1: +inf, capped
    assert PR.stop_bound(1, 10 ** 7, 0.99, 3, 100) == -math.inf         # 1 - pow(..) rounds to 1: -x / 0
    assert math.pow(1e-7, 3.0) < 2.0 ** -54
    assert PR.stop_bound(1, 10 ** 7, 1.0, 3, 100) == -math.inf          # ... also with probability = 1: -inf / 0
    k = PR.stop_bound(5, 10, 0.99999999, 3, 1000)
    assert k == math.log(1.0 - 0.99999999) / math.log(1.0 - math.pow(0.5, 3.0)) and 137 < k < 139
    P = SC.planted(400, 0.5, 8)
    never = PR.segment(P, 0.01, 3, 300, 1.0, 9)
    assert never["trials"] == 300
    early = PR.segment(P, 0.01, 3, 300, 0.99, 9)
    assert early["trials"] < 300 and early["valid_trials"] <= early["trials"]
    none = PR.segment(P[:2], 0.01, 3, 300, 0.99, 9)
    assert none["trials"] == 0 and none["best_trial"] == -1 and not none["plane"].any()
    assert PR.segment(P, 0.01, 3, 0, 0.99, 9)["trials"] == 0


def test_chosen_seeds_behave_as_the_gpu_tests_need():
    """n = 3, ransac_n = 3: only the 6 orderings of three distinct indices span a plane; collinear: none does."""
    P3 = np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])
    t = PR.trials(P3, 0.1, 3, 41, 0, 256)
    dead = int((t["flags"] == 0).sum())
    assert 0 < dead < 256
    distinct = np.array([len(set(row)) == 3 for row in t["samples"].tolist()])
    assert np.array_equal(distinct, t["flags"] == 1) and (t["count"][distinct] == 3).all()
    c = PR.trials(SC.collinear(50), 0.1, 3, 42, 0, 64)
    assert not c["flags"].any() and not c["plane"].any() and not c["count"].any()
    r = PR.segment(SC.collinear(50), 0.1, 3, 64, 0.99, 42)
    assert r["best_trial"] == -1 and r["trials"] == 64 and r["valid_trials"] == 0 and not r["plane"].any()
    # the segment loop does not depend on how its trials are asked for
    P = SC.planted(600, 0.4, 10)
    a, b = PR.segment(P, 0.01, 4, 200, 0.999, 5, slab=64), PR.segment(P, 0.01, 4, 200, 0.999, 5, slab=7)
    assert a["trials"] == b["trials"] and np.array_equal(a["plane"], b["plane"]) and np.array_equal(a["mask"], b["mask"])
