"""Boundary points on the MI355X (include/teaser_hip.h, "Boundary points") against the numpy restatement
(tests/boundary_reference.py) with EQUALITY: the mask, the list lengths, n_boundary and the raw bytes of max_gap.  The
contract uses only IEEE operations in a stated order and max_gap does not depend on how the sort orders equal angles, so
there is no tolerance.  The case list is the host driver's (tests/test_boundary_host.py)."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import boundary_reference as R

tp = importlib.import_module("teaser-plusplus_amd")
pytestmark = pytest.mark.gpu

Hybrid, KNN = tp.KDTreeSearchParamHybrid, tp.KDTreeSearchParamKNN


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def param(search, radius, max_nn):
    return ("hybrid", radius, max_nn) if search == R.HYBRID else ("knn", max_nn)


@functools.lru_cache(maxsize=None)
def cases():
    """The shared cases with the restatement's (mask, max_gap, m), computed once."""
    out = []
    for name, P, N, search, radius, max_nn, thr in R.case_list():
        mask, gap, m = R.boundary_points(P, N, search, radius, max_nn, thr)
        out.append((name, P, N, param(search, radius, max_nn), thr, mask, gap, m))
    return out


def index(name):
    return [c[0] for c in cases()].index(name)


def run(sel, **kw):
    cs = [cases()[k] for k in sel]
    return tp.compute_boundary_points_batch([c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs], [c[4] for c in cs],
                                            return_max_gap=True, return_counts=True, **kw)


def check(sel, got, what):
    for k, r in zip(sel, got):
        name, _, _, _, _, mask, gap, m = cases()[k]
        assert np.array_equal(r.counts, m), "%s: list lengths of %s" % (what, name)
        assert r.max_gap.tobytes() == gap.tobytes(), "%s: max_gap of %s" % (what, name)
        assert np.array_equal(r.mask, mask), "%s: mask of %s" % (what, name)
        assert r.n_boundary == int(mask.sum()), "%s: n_boundary of %s" % (what, name)


def test_the_case_list_in_one_batch_alone_and_reversed():
    """The lattices (both frame branches), the sphere and the hemisphere, 257 random points with max_nn 10 and with
    every list full (99 angles: both slots of every lane that has one), k-NN with max_nn 2, 33, 64, 65 (the lane-slot
    edges), clouds of 0, 1, 2, 63, 64, 65 points, coincident points, a zero normal and the other frame edges, isolated
    points, the thresholds 0 and 360, a shifted cloud: one batch, every cloud alone, the batch reversed."""
    sel = list(range(len(cases())))
    assert (cases()[index("n257_full")][7] == 100).all() and (cases()[index("isolated")][7] == 1).all()
    assert np.isnan(cases()[index("frames")][6][3]) and {c[3][0] for c in cases()} == {"hybrid", "knn"}
    lat = cases()[index("lattice_z")]
    assert np.array_equal(lat[5], R.lattice_perimeter(9)) and np.array_equal(cases()[index("lattice_x")][5], lat[5])
    assert not cases()[index("sphere")][5].any() and cases()[index("hemisphere")][5].any()
    check(sel, run(sel), "one batch")
    for k in sel:
        check([k], run([k]), "alone")
    check(sel[::-1], run(sel[::-1]), "reversed")


def test_a_cloud_gives_the_same_bytes_at_any_batch_position():
    k = index("n257")
    a, b, c = index("n63"), index("n0"), index("n65")
    got = run([k, a, b, k, c])
    alone = run([k])[0]
    for r in (got[0], got[3]):
        assert r.max_gap.tobytes() == alone.max_gap.tobytes() and np.array_equal(r.mask, alone.mask)
        assert np.array_equal(r.counts, alone.counts) and r.n_boundary == alone.n_boundary
    check([k, a, b, k, c], got, "two positions")


def test_a_small_list_bound_changes_no_bit():
    """fpfh_list_bytes so small that the 257-point cloud (max_nn 10: 120 bytes of lists per point, pieces of 64 points)
    runs in five pieces and five passes; then 1."""
    default = tp.get_icp_option("fpfh_list_bytes")
    sel = list(range(len(cases())))
    k257 = index("n257")
    try:
        tp.set_icp_option("fpfh_list_bytes", 64 * 10 * 12)
        check([k257], run([k257]), "small bound, alone")
        check(sel, run(sel), "small bound, one batch")
        tp.set_icp_option("fpfh_list_bytes", 1)
        check(sel, run(sel), "bound 1, one batch")
    finally:
        tp.set_icp_option("fpfh_list_bytes", default)
    assert tp.get_icp_option("fpfh_list_bytes") == default


def test_knn_records_do_not_depend_on_the_ring_cap():
    sel = [k for k, c in enumerate(cases()) if c[3][0] == "knn"]
    assert len(sel) >= 6
    cap = tp.get_icp_option("knn_ring_cap")
    try:
        tp.set_icp_option("knn_ring_cap", 0)
        check(sel, run(sel), "knn_ring_cap 0")
    finally:
        tp.set_icp_option("knn_ring_cap", cap)
    check(sel, run(sel), "knn_ring_cap default")


def test_normals_inside_the_call_equal_the_two_calls():
    rng = np.random.default_rng(21)
    clouds = [rng.random((n, 3)) for n in (257, 0, 64, 5)]
    nsp = [Hybrid(0.2, 30), KNN(10), KNN(12), Hybrid(0.5, 3)]
    sps = [Hybrid(0.3, 40), KNN(5), ("knn", 2), KNN(30)]
    normals = tp.estimate_normals_batch(clouds, nsp)
    kw = dict(return_max_gap=True, return_counts=True)
    two = tp.compute_boundary_points_batch(clouds, normals, sps, 75.0, **kw)
    one = tp.compute_boundary_points_batch(clouds, None, sps, 75.0, normal_search=nsp, return_normals=True, **kw)
    for a, b, N in zip(one, two, normals):
        assert a.normals.tobytes() == N.tobytes() and a.max_gap.tobytes() == b.max_gap.tobytes()
        assert np.array_equal(a.mask, b.mask) and np.array_equal(a.counts, b.counts) and a.n_boundary == b.n_boundary
    assert two[0].mask.any() and not two[0].mask.all()
    # given and estimated normals in one call
    mixed = tp.compute_boundary_points_batch(clouds, [normals[0], None, None, normals[3]], sps, 75.0,
                                             normal_search=[None, nsp[1], nsp[2], None], **kw)
    for a, b in zip(mixed, two):
        assert a.max_gap.tobytes() == b.max_gap.tobytes() and np.array_equal(a.mask, b.mask)


def test_python_front():
    """compute_boundary_points returns the points the mask selects; tuple and class search parameters and the
    radius / max_nn form give the same result; boundary_mask returns the gaps and the counts on request."""
    _, P, N, _, _, mask, gap, m = cases()[index("hemisphere")]
    pts, got = tp.compute_boundary_points(P, N, radius=0.35, max_nn=30, angle_threshold=90.0)
    assert got.dtype == bool and np.array_equal(got, mask) and np.array_equal(pts, P[mask])
    for sp in (Hybrid(0.35, 30), ("hybrid", 0.35, 30)):
        pts2, got2 = tp.compute_boundary_points(P, N, search_param=sp)
        assert np.array_equal(got2, mask) and np.array_equal(pts2, pts)
    k1 = tp.boundary_mask(P, N, search_param=KNN(12), angle_threshold=60.0, return_max_gap=True, return_counts=True)
    k2 = tp.boundary_mask(P, N, search_param=("knn", 12), angle_threshold=60.0, return_max_gap=True, return_counts=True)
    ref = R.boundary_points(P, N, R.KNN, 0.0, 12, 60.0)
    for got3 in (k1, k2):
        assert np.array_equal(got3[0], ref[0]) and got3[1].tobytes() == ref[1].tobytes() and np.array_equal(got3[2], ref[2])
    assert np.array_equal(tp.boundary_mask(P, N, 0.35), mask)
    # normals estimated inside the call
    ns = Hybrid(0.35, 30)
    pts3, got3 = tp.compute_boundary_points(P, None, radius=0.35, normal_search=ns)
    assert np.array_equal(got3, tp.boundary_mask(P, tp.estimate_normals(P, ns), 0.35)) and np.array_equal(pts3, P[got3])
    with pytest.raises(ValueError, match="KDTreeSearchParamRadius"):
        tp.compute_boundary_points(P, N, search_param=tp.KDTreeSearchParamRadius(0.3))
    with pytest.raises(ValueError, match="angle_threshold"):
        tp.compute_boundary_points(P, N, radius=0.3, angle_threshold=361.0)
    with pytest.raises(ValueError, match="neither normals"):
        tp.compute_boundary_points(P, None, radius=0.3)
    with pytest.raises(ValueError, match="radius"):
        tp.compute_boundary_points(P, N)


def test_every_refusal_names_its_argument_and_cloud_and_the_handle_goes_on():
    _, P, N, _, _, mask, gap, m = cases()[index("n257")]
    n_pts = len(P)
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    Rec = tp.icp.IcpNormalSearchC
    ok = (0, 10, 0.3, 0, 0)
    out = [np.zeros(n_pts, dtype=np.uint8) for _ in range(2)]
    nb = np.zeros(2, dtype=np.int32)

    def call(points=(P, P), normals=(N, N), n=(n_pts, n_pts), recs=(ok, ok), nrecs=None, thr=(90.0, 90.0), masks=out):
        arr = lambda xs, t: None if xs is None else (t * 2)(*[None if x is None else x.ctypes.data_as(t) for x in xs])  # noqa: E731
        rec = lambda r: Rec(r[0], r[1], r[2], r[3], r[4], (C.c_double * 3)())  # noqa: E731
        t = None if thr is None else np.array(thr, dtype=np.float64)
        cnt = np.array(n, dtype=np.int32)
        tp.icp._handle(-1).call(tp.lib().teaser_hip_icp_boundary_points_batch, 2, arr(points, dp), arr(normals, dp),
                                cnt.ctypes.data_as(ip), (Rec * 2)(*[rec(r) for r in recs]),
                                None if nrecs is None else (Rec * 2)(*[rec(r) for r in nrecs]),
                                None if t is None else t.ctypes.data_as(dp), arr(masks, bp), nb.ctypes.data_as(ip),
                                None, None, None)

    def refused(words, **kw):
        with pytest.raises(tp.TeaserHipError) as e:
            call(**kw)
        assert "BAD_ARG" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)

    bad_p, bad_n = P.copy(), N.copy()
    bad_p[1, 1], bad_n[2, 1] = np.nan, np.inf
    refused(("points has a non-finite", "problem 1"), points=(P, bad_p))
    refused(("normals has a non-finite", "problem 0"), normals=(bad_n, N))
    refused(("n must be", "problem 1"), n=(n_pts, -1))
    refused(("points is NULL", "problem 0"), points=(None, P))
    refused(("radius-only", "problem 1"), recs=(ok, (2, 10, 0.3, 0, 0)))
    refused(("search must be 0 or 1", "problem 0"), recs=((3, 10, 0.3, 0, 0), ok))
    refused(("max_nn must lie in [2, 100]", "problem 1"), recs=(ok, (0, 1, 0.3, 0, 0)))
    refused(("max_nn must lie", "problem 0"), recs=((1, 101, 0.3, 0, 0), ok))
    refused(("orient must be 0", "problem 1"), recs=(ok, (0, 10, 0.3, 1, 0)))
    refused(("reserved", "problem 0"), recs=((0, 10, 0.3, 0, 3), ok))
    for r in (0.0, -1.0, np.nan, np.inf, 1e200):
        refused(("radius", "problem 1"), recs=(ok, (0, 10, r, 0, 0)))
    for t in (-1e-9, 360.0000001, np.nan, np.inf):
        refused(("angle_threshold", "problem 1"), thr=(90.0, t))
    refused(("normals is NULL and normal_search", "problem 1"), normals=(N, None))
    refused(("normals is NULL and normal_search", "problem 0"), normals=None, nrecs=((0, 0, 0.0, 0, 0), (0, 0, 0.0, 0, 0)))
    refused(("normal_search", "problem 1"), normals=(N, None), nrecs=((0, 0, 0.0, 0, 0), (0, 2, 0.2, 0, 0)))
    refused(("mask_out is NULL", "problem 1"), masks=(out[0], None))
    refused(("angle_threshold must not be NULL",), thr=None)
    # the handle serves a good call afterwards: both copies give the restatement's mask
    call(recs=((0, 10, 0.3, 0, 0),) * 2)
    assert np.array_equal(out[0].astype(bool), mask) and np.array_equal(out[1].astype(bool), mask)
    assert nb.tolist() == [int(mask.sum())] * 2
