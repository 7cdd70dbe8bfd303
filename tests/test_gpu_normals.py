"""Batched normal estimation and the point-to-plane entry that estimates its own target normals, on the MI355X against
the numpy restatement (tests/normals_reference.py): raw covariances and eigenvalues bit for bit; normals at the
per-point bar tests/test_gpu_icp_gicp.py uses for covariances, 512 2^-52 lambda2 / (lambda1 - lambda0) on |dn| (the
reason is given there: |dn| <= |dcov| / (lambda1 - lambda0), |dcov| <= (m + the Jacobi's few tens) ulps of lambda2),
the points whose bar exceeds 1e-6 excluded, counted, and asserted to be at most 1 % of a cloud
(tests/test_normals_reference.py checks on the CPU that the restatement itself stays inside that).

The scan kernel's wave merge is reached only through knn_ring_cap (0, and 4 on a far-outlier cloud).  The exclusion
count is asserted everywhere but on the clouds with exact ties by construction (planar, collinear, identical points,
the tied lattice)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import icp_plane_reference as RP
import icp_reference as R
import normals_reference as RN
import outlier_reference as RO

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")
Hybrid, KNN = tp.KDTreeSearchParamHybrid, tp.KDTreeSearchParamKNN
Plane = tp.TransformationEstimationPointToPlane


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def reference(X, sp):
    return RN.estimate_normals(X, sp.search, sp.radius, sp.max_nn, sp.orient, sp.ref)


def check(got, ref, what, ties=False):
    """got = (normals, covariances, eigenvalues) of the GPU, ref = the restatement's 4-tuple."""
    N, Cv, E = got
    Nr, Cr, Er, M = ref
    assert RO.bits_equal(Cv, Cr), what + ": covariances"
    assert RO.bits_equal(E, Er), what + ": eigenvalues"
    few = M < 3
    assert N[few].tobytes() == Nr[few].tobytes(), what + ": filled-in normals"
    bar = RN.normal_bar(Er)
    use = ~few & (bar <= 1e-6)
    excluded = int((~few & ~use).sum())
    err = np.linalg.norm(N - Nr, axis=1)
    exact = int((N[use].view(np.uint64) == Nr[use].view(np.uint64)).all(axis=1).sum()) if use.any() else 0
    print("%s: n %d, below three %d, excluded %d, max err / bar %.3g, normals bit-equal %d of %d" % (
        what, len(N), few.sum(), excluded, (err[use] / bar[use]).max() if use.any() else 0.0, exact, use.sum()))
    if not ties:
        assert excluded <= 0.01 * len(N), what
    assert (err[use] <= bar[use]).all(), what
    assert np.allclose(np.linalg.norm(N[~few], axis=1), 1.0, atol=1e-12)


def run(clouds, sps):
    return tp.estimate_normals_batch(clouds, sps, covariances=True, eigenvalues=True)


SIZES = (1, 2, 3, 63, 64, 65, 129, 513)


@pytest.mark.parametrize("max_nn", [3, 32, 33, 100])
def test_every_size_and_capacity_against_the_restatement(max_nn):
    clouds = [RN.cube(n, seed=n) for n in SIZES[:4]] + [np.zeros((0, 3))] + [RN.cube(n, seed=n) for n in SIZES[4:]]
    for sp in (KNN(max_nn), Hybrid(0.17, max_nn)):  # the radius leaves points of every cloud below three neighbours
        got = run(clouds, sp)
        below = 0
        for X, g in zip(clouds, got):
            ref = reference(X, sp)
            below += int((ref[3] < 3).sum())
            check(g, ref, "%s n %d" % (sp, len(X)))
    assert below > 10


def test_two_capacities_in_one_call_and_orientation_per_cloud():
    X, Y = RN.cube(257, 1), RN.cube(300, 2)
    sps = [KNN(20).towards([0.5, 0.5, 5.0]), KNN(40), Hybrid(0.3, 40).along([0, 0, 1]), Hybrid(0.3, 20)]
    clouds = [X, Y, X, Y]
    got = run(clouds, sps)
    for X_, sp, g in zip(clouds, sps, got):
        check(g, reference(X_, sp), repr(sp))
        alone = tp.estimate_normals(X_, sp, covariances=True, eigenvalues=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(alone, g))


def test_degenerate_clouds():
    for name, X in (("planar", RN.planar()), ("collinear", RN.collinear()), ("identical", RN.identical())):
        for sp in (KNN(12), Hybrid(0.6, 12)):
            check(run([X], sp)[0], reference(X, sp), "%s %s" % (name, sp), ties=True)


def test_tied_lattice_permutes_with_the_cloud():
    X = RN.tied_lattice()
    perm = np.random.default_rng(6).permutation(len(X))
    for sp in (Hybrid(0.25 * np.sqrt(2.5), 100), KNN(100)):  # not binding / binding: the index order breaks the ties
        a, b = run([X, X[perm]], sp)
        check(a, reference(X, sp), "lattice", ties=True)
        check(b, reference(X[perm], sp), "lattice permuted", ties=True)
    a, b = run([X, X[perm]], Hybrid(0.25 * np.sqrt(2.5), 100))  # every sum is exact: the same set gives the same bits
    assert all(u[perm].tobytes() == v.tobytes() for u, v in zip(a, b))


def test_far_from_the_origin():
    """A cloud moved by s = (1e5, -2e5, 3e4) against the un-shifted one: normals do not move with a translation.  Bars
    as in the far-from-origin test of tests/test_gpu_icp_gicp.py: ten times the difference MEASURED ON THE CPU with the
    restatement before any GPU run, shifted against un-shifted (sign-aligned, since the sign without an orientation
    carries no meaning): max |dn| 1.68e-9 with k-NN search (k = 30), 7.11e-10 with hybrid search (0.2, 30); every
    neighbour count equal, no point excluded by the 1e-6 rule.  (The coordinates' own rounding at 2e5, 2.9e-11, over
    neighbour offsets of about 0.1, amplified by lambda2 / (lambda1 - lambda0), is what these figures are.)  Each run
    is also compared with the restatement on its own cloud, the exclusion count asserted."""
    X = RN.cube(513, 9)
    s = np.array([1e5, -2e5, 3e4])
    for sp, bar in ((KNN(30), 1.68e-8), (Hybrid(0.2, 30), 7.11e-9)):
        near, far = run([X, X + s], sp)
        ref_near, ref_far = reference(X, sp), reference(X + s, sp)
        check(near, ref_near, "un-shifted %s" % sp)
        check(far, ref_far, "shifted %s" % sp)
        assert np.array_equal(ref_near[3], ref_far[3])
        has = ref_near[3] >= 3
        err = np.minimum(np.linalg.norm(far[0] - near[0], axis=1), np.linalg.norm(far[0] + near[0], axis=1))
        print("shifted against un-shifted, %s: max |dn| %.3g (bar %.3g)" % (sp, err[has].max(), bar))
        assert (err[has] < bar).all()
        assert far[0][~has].tobytes() == near[0][~has].tobytes()


def test_knn_search_does_not_depend_on_the_ring_cap():
    """k = 10 on the planted cloud: the box is 13 wide, the grid has 606 / 5 = 121 cells of edge 2.63, five per axis.
    The outermost planted points sit in cells 4 of every axis, so rings 0 .. 3 do not cover the grid from there, and
    their tenth neighbour (six planted points exist) is a point of the unit cube more than 13 away, beyond 3 edges:
    they must reach the worklist.  (At k >= 20 the cells are wide enough for ring 3 to cover the whole grid from
    every cell, and no query of this cloud falls back: the contract's search, not a fault.)"""
    P, _ = RO.planted_cloud()
    clouds = [P, RN.cube(129, 3), RN.planar()]
    try:
        tp.set_icp_option("knn_ring_cap", 4)
        a = run(clouds, KNN(10))
        fell = tp.get_icp_option("knn_fallbacks")
        print("fallbacks at ring cap 4, k = 10:", fell)
        assert 0 < fell < len(P)  # the far points of the planted cloud
        a30 = run(clouds, KNN(30))
        tp.set_icp_option("knn_ring_cap", 0)
        b = run(clouds, KNN(10))
        assert tp.get_icp_option("knn_fallbacks") == sum(len(c) for c in clouds)
        b30 = run(clouds, KNN(30))
    finally:
        tp.set_icp_option("knn_ring_cap", 4)
    for x, y in list(zip(a, b)) + list(zip(a30, b30)):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
    check(a[0], reference(P, KNN(10)), "planted")
    check(a30[0], reference(P, KNN(30)), "planted, k = 30")
    run(clouds[1:], Hybrid(0.3, 30))
    assert tp.get_icp_option("knn_fallbacks") == 0


@pytest.fixture(scope="module")
def config5():
    P, Q, r, init = R.config5_problem()
    return P, Q, r, init


def test_orientation_on_the_config5_target(config5):
    _, Q, r, _ = config5
    centre = 0.5 * (Q.min(axis=0) + Q.max(axis=0)) + np.array([0.0, 0.0, 10.0])
    sp = Hybrid(2 * r, 30)
    n0, n1, n2 = tp.estimate_normals_batch([Q, Q, Q], [sp, sp.towards(centre), sp.along([0, 0, 1])])
    V = centre - Q
    assert (((n1[:, 0] * V[:, 0] + n1[:, 1] * V[:, 1]) + n1[:, 2] * V[:, 2]) >= 0).all()
    assert (n2[:, 2] >= 0).all()
    same, flipped = (n1 == n0).all(axis=1), (n1 == -n0).all(axis=1)
    M = RN.estimate_normals(Q, 0, 2 * r, 30)[3]
    assert (same | flipped | (M < 3)).all() and flipped.any() and same.any()
    assert np.array_equal(tp.estimate_normals(Q, sp, along=[0, 0, 1]), n2)
    check(tp.estimate_normals(Q, sp, towards=centre, covariances=True, eigenvalues=True),
          RN.estimate_normals(Q, 0, 2 * r, 30, 1, centre), "config-5 target")


def test_batch_independence_next_to_other_calls():
    rng = np.random.default_rng(12)
    clouds = [rng.random((n, 3)) for n in (40, 0, 129, 513, 64, 3, 200, 65, 300)]
    sps = [KNN(10), Hybrid(0.2, 30), Hybrid(0.3, 50).along([1, 0, 0]), KNN(64), KNN(3), Hybrid(5.0, 3), KNN(33),
           Hybrid(0.4, 32).towards([0, 0, 9]), KNN(100)]
    first = run(clouds, sps)
    tp.estimate_covariances(clouds[3], 0.3, 20)
    tp.remove_statistical_outlier(clouds[8], 20, 2.0)
    again = run(clouds, sps)
    for k in range(len(clouds)):
        alone = tp.estimate_normals(clouds[k], sps[k], covariances=True, eigenvalues=True)
        for u, v, w in zip(first[k], again[k], alone):
            assert u.tobytes() == v.tobytes() == w.tobytes()


def same_bits(a, b):
    return (a.transformation.tobytes() == b.transformation.tobytes() and a.fitness == b.fitness and
            a.inlier_rmse == b.inlier_rmse and a.iterations == b.iterations and
            np.array_equal(a.correspondence_set, b.correspondence_set))


@pytest.mark.parametrize("kernel", [None, tp.HuberLoss(0.05), tp.CauchyLoss(0.05), tp.GMLoss(0.05), tp.TukeyLoss(0.1)])
def test_self_estimated_normals_equal_the_two_call_form(config5, kernel):
    P, Q, r, init = config5
    sp = Hybrid(2 * r, 30).along([0, 0, 1])
    auto = tp.registration_icp(P, Q, r, init, Plane(kernel), target_normals=sp)
    N = tp.estimate_normals(Q, sp)
    two = tp.registration_icp(P, Q, r, init, Plane(kernel), target_normals=N)  # teaser_hip_icp_batch_ex on the array
    assert same_bits(auto, two) and auto.iterations >= 2 and auto.fitness > 0.3
    knn = tp.registration_icp(P, Q, r, init, Plane(kernel), target_normals=KNN(30))
    assert same_bits(knn, tp.registration_icp(P, Q, r, init, Plane(kernel),
                                              target_normals=tp.estimate_normals(Q, KNN(30))))


def test_mixed_batch_equals_single_runs_and_old_entries_keep_their_bits(config5):
    P, Q, r, init = config5
    given = RP.config5_normals()
    Cs, Ct = tp.estimate_covariances_batch([P, Q], 2 * r, 20)
    sp, kn = Hybrid(2 * r, 30).towards([0, 0, 0]), KNN(25)
    G = tp.TransformationEstimationForGeneralizedICP()
    ests = [Plane(), Plane(), None, G, Plane(tp.TukeyLoss(0.1)), Plane()]
    normals = [given, sp, None, None, kn, sp]
    srcs = [P, P, P, P, P[:700], np.zeros((0, 3))]
    dsts = [Q, Q, Q, Q, Q[:2000], Q[:100]]
    kw = dict(estimation_methods=ests, target_normals=normals, source_covariances=[None, None, None, Cs, None, None],
              target_covariances=[None, None, None, Ct, None, None])
    batch = tp.registration_icp_batch(srcs, dsts, r, inits=init, **kw)
    again = tp.registration_icp_batch(srcs, dsts, r, inits=init, **kw)
    for k in range(len(srcs)):
        alone = tp.registration_icp(srcs[k], dsts[k], r, init, ests[k], target_normals=normals[k],
                                    source_covariances=kw["source_covariances"][k],
                                    target_covariances=kw["target_covariances"][k])
        assert same_bits(batch[k], alone) and same_bits(batch[k], again[k]), k
    # the same problems without a search object go through the older entries: the same bits as inside the mixed batch
    assert same_bits(batch[0], tp.registration_icp_batch([P], [Q], r, inits=init, estimation_methods=[Plane()],
                                                         target_normals=[given])[0])
    assert same_bits(batch[2], tp.registration_icp(P, Q, r, init))
    assert same_bits(batch[3], tp.registration_icp(P, Q, r, init, G, source_covariances=Cs, target_covariances=Ct))


def raw_normals(clouds, recs, want=(True, False, False)):
    """teaser_hip_icp_normals_batch through ctypes with records built by hand: (rc, message)."""
    from importlib import import_module
    icp = import_module("teaser-plusplus_amd.icp")
    L = tp.lib()
    b = len(clouds)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    pts = [np.ascontiguousarray(c, dtype=np.float64) for c in clouds]
    n = np.array([len(p) for p in pts], dtype=np.int32)
    outs = [[np.zeros((len(p), w)) for p in pts] if use else None for use, w in zip(want, (3, 9, 3))]
    ptrs = lambda a: None if a is None else (dp * b)(*[x.ctypes.data_as(dp) for x in a])  # noqa: E731
    h = icp._handle(-1)
    try:
        h.call(L.teaser_hip_icp_normals_batch, b, ptrs(pts), n.ctypes.data_as(ip),
               (icp.IcpNormalSearchC * b)(*recs), ptrs(outs[0]), ptrs(outs[1]), ptrs(outs[2]))
    except tp.TeaserHipError as e:
        return str(e)
    return ""


def test_refusals_name_the_argument_and_the_cloud_and_leave_the_handle_usable(config5):
    from importlib import import_module
    Rec = import_module("teaser-plusplus_amd.icp").IcpNormalSearchC
    X = RN.cube(50)
    ok = lambda **kw: Rec(**dict(dict(search=0, max_nn=30, radius=0.3, orient=0, reserved=0), **kw))  # noqa: E731
    ref3 = lambda *v: (C.c_double * 3)(*v)  # noqa: E731
    bad = X.copy()
    bad[7, 1] = np.inf
    cases = [([X, bad], [ok(), ok()], "points"), ([X, X], [ok(), ok(search=2)], "search"),
             ([X, X], [ok(), ok(orient=3)], "orient"), ([X, X], [ok(), ok(reserved=1)], "reserved"),
             ([X, X], [ok(), ok(max_nn=2)], "max_nn"), ([X, X], [ok(), ok(max_nn=101)], "max_nn"),
             ([X, X], [ok(), ok(radius=0.0)], "radius"), ([X, X], [ok(), ok(radius=np.nan)], "radius"),
             ([X, X], [ok(), ok(radius=1e200)], "radius"),
             ([X, X], [ok(), ok(orient=1, ref=ref3(0, np.nan, 0))], "ref")]
    for clouds, recs, word in cases:
        msg = raw_normals(clouds, recs)
        assert "BAD_ARG" in msg and word in msg and "problem 1" in msg, (word, msg)
    assert "normals_out" in raw_normals([X], [ok()], want=(False, False, False))
    L, icp = tp.lib(), import_module("teaser-plusplus_amd.icp")
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    n2 = np.array([50, 50], dtype=np.int32)
    out = [np.zeros((50, 3)), np.zeros((50, 3))]
    po = (dp * 2)(*[o.ctypes.data_as(dp) for o in out])
    recs = (Rec * 2)(ok(), ok())
    h = icp._handle(-1)
    for pts, where in ((None, "problem 0"), ((dp * 2)(X.ctypes.data_as(dp), None), "problem 1")):  # NULL where n > 0
        with pytest.raises(tp.TeaserHipError, match="points is NULL.*" + where):
            h.call(L.teaser_hip_icp_normals_batch, 2, pts, n2.ctypes.data_as(ip), recs, po, None, None)
    # teaser_hip_icp_batch_auto itself: a point-to-plane problem with neither normals nor a record, refused by name
    P, Q, r, init = config5
    src = (dp * 1)(P.ctypes.data_as(dp))
    dst = (dp * 1)(Q.ctypes.data_as(dp))
    ns, nt = np.array([len(P)], dtype=np.int32), np.array([len(Q)], dtype=np.int32)
    prm = (icp.IcpParamsC * 1)(icp.IcpParamsC(r, 30, 1e-6, 1e-6))
    est = (icp.IcpEstimationC * 1)(icp.IcpEstimationC(1, 0, 1.0))
    res = (icp.IcpResultC * 1)()
    for rec in (None, (Rec * 1)(Rec())):  # no records at all, and a record with max_nn = 0
        with pytest.raises(tp.TeaserHipError, match="dst_normals is NULL.*problem 0"):
            h.call(L.teaser_hip_icp_batch_auto, 1, src, ns.ctypes.data_as(ip), dst, nt.ctypes.data_as(ip), None, prm,
                   res, None, None, est, None, None, rec)
    with pytest.raises(tp.TeaserHipError, match="dst_normal_search: radius.*problem 0"):
        h.call(L.teaser_hip_icp_batch_auto, 1, src, ns.ctypes.data_as(ip), dst, nt.ctypes.data_as(ip), None, prm, res,
               None, None, est, None, None, (Rec * 1)(ok(radius=-1.0)))
    h.call(L.teaser_hip_icp_batch_auto, 1, src, ns.ctypes.data_as(ip), dst, nt.ctypes.data_as(ip),
           np.ascontiguousarray(init).ctypes.data_as(dp), prm, res, None, None, est, None, None, (Rec * 1)(ok(radius=2 * r)))
    assert res[0].iterations >= 2  # the handle works afterwards
    assert raw_normals([X, X], [ok(search=1, radius=np.nan), ok(ref=ref3(np.nan, 0, 0))]) == ""  # both ignored
    with pytest.raises(ValueError, match="target_normals"):
        tp.registration_icp(P, Q, r, init, Plane())
    assert len(tp.estimate_normals(X, KNN(5))) == 50
