"""Neighbour search between two clouds on the MI355X (k-NN, hybrid, uncapped radius) against the numpy restatement of the
contract (tests/search_reference.py): indices, counts, row splits and d2 bits are EQUAL -- the contract leaves no order
of evaluation open, so there is no tolerance.  Shapes: the smallest at which each path is taken -- both list capacities
(k <= 32 and k > 32), one and several blocks of 64 and of 256 queries, k below, at and above n_data, queries inside the
data's box, just outside it (served by the grid) and far from it (served by the scan of the whole cloud), and every k-NN
case again with "knn_ring_cap" = 0, where the scan serves every query."""
import ctypes as C
import importlib

import numpy as np
import pytest

import outlier_reference as R
import search_reference as S

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")
icp = importlib.import_module("teaser-plusplus_amd.icp")
_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_ref_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


@pytest.fixture(params=[4, 0], ids=["rings", "scan"])
def ring_cap(request):
    """Runs a k-NN test with the default ring cap and with 0 (every query takes the whole-cloud route); restores it."""
    before = tp.get_icp_option("knn_ring_cap")
    tp.set_icp_option("knn_ring_cap", request.param)
    yield request.param
    tp.set_icp_option("knn_ring_cap", before)
    assert tp.get_icp_option("knn_ring_cap") == before == 4


def ref_knn(key, P, Q, k):
    """The restatement's answer, computed once per problem (both ring caps compare with the same one)."""
    if key not in _ref_cache:
        _ref_cache[key] = S.knn_search(P, Q, k)
    return _ref_cache[key]


def assert_knn(got, ref, what=""):
    idx, d2 = got
    ridx, rd2 = ref
    assert idx.shape == ridx.shape and idx.dtype == np.int32
    bad = np.flatnonzero((idx != ridx).any(axis=1))
    assert len(bad) == 0, "%s: %d rows differ, first %d: %s vs %s" % (what, len(bad), bad[0], idx[bad[0]], ridx[bad[0]])
    assert R.bits_equal(d2, rd2), what


def assert_radius(got, P, Q, radius):
    idx, d2, splits = got
    ridx, rd2, rsplits = S.radius_search(P, Q, radius)
    assert splits.dtype == np.int64 and np.array_equal(splits, rsplits)
    assert idx.dtype == np.int32 and np.array_equal(idx, ridx) and R.bits_equal(d2, rd2)
    return rsplits


def assert_hybrid(got, P, Q, radius, max_nn):
    idx, d2, cnt = got
    ridx, rd2, rcnt = S.hybrid_search(P, Q, radius, max_nn)
    assert np.array_equal(cnt, rcnt) and np.array_equal(idx, ridx) and R.bits_equal(d2, rd2)
    return rcnt


def fallbacks():
    return tp.get_icp_option("knn_fallbacks")


# ---- k-NN ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 32, 33, 100])
def test_knn_block_edge_sizes_with_k_below_at_and_above_n_data(k, ring_cap):
    rng = np.random.default_rng(200)
    data = {n: rng.random((n, 3)) for n in (1, 2, 63, 64, 65, 257, 513)}
    query = {n: rng.random((n, 3)) * 1.5 - 0.25 for n in (1, 64, 65, 130)}  # a good part outside the data's box
    pairs = [(nd, nq) for nd in data for nq in query]
    got = tp.knn_search_batch([data[nd] for nd, _ in pairs], [query[nq] for _, nq in pairs], k)
    fell = fallbacks()
    total = sum(nq for _, nq in pairs)
    assert fell == total if ring_cap == 0 else 0 <= fell < total
    for (nd, nq), g in zip(pairs, got):
        assert g[0].shape == (nq, k)
        assert_knn(g, ref_knn(("sizes", nd, nq, k), data[nd], query[nq], k), "n_data %d n_query %d k %d" % (nd, nq, k))
        assert ((g[0] >= 0).sum(axis=1) == min(k, nd)).all()


def test_knn_lattice_ties_go_to_the_smaller_index(ring_cap):
    P = S.lattice()  # 343 points, dyadic spacing: every d2 exact, massive ties
    centres = S.lattice_centres()  # eight nearest points tie
    perm = np.random.default_rng(3).permutation(len(P))
    ks = [1, 8, 27, 100]
    for Q, name in ((P, "points"), (centres, "centres")):
        got = tp.knn_search_batch([P] * len(ks), [Q] * len(ks), ks)
        assert fallbacks() == (len(ks) * len(Q) if ring_cap == 0 else 0)  # a dense lattice needs no scan
        for k, g in zip(ks, got):
            assert_knn(g, ref_knn(("lattice", name, k), P, Q, k), "lattice %s k %d" % (name, k))
        # the permuted data cloud: the same distances in the same order, the tie classes in the new numbering
        for k, g, g0 in zip(ks, tp.knn_search_batch([P[perm]] * len(ks), [Q] * len(ks), ks), got):
            assert_knn(g, ref_knn(("lattice perm", name, k), P[perm], Q, k))
            assert R.bits_equal(g[1], g0[1])
    g = tp.knn_search(P, centres[:1], 8)
    assert g[0][0].tolist() == [0, 1, 7, 8, 49, 50, 56, 57] and (g[1] == 3 * 0.125 ** 2).all()


def test_knn_with_query_equal_to_data_is_self_knn(ring_cap):
    rng = np.random.default_rng(12)
    for P, k in ((rng.random((513, 3)), 20), (S.lattice(5), 33), (np.tile([[0.5, 1.5, -2.0]], (70, 1)), 5)):
        idx, d2 = tp.knn_search(P, P, k)
        sidx, sd2 = tp.self_knn(P, k, return_distance=True)
        assert np.array_equal(idx, sidx) and d2.tobytes() == sd2.tobytes()


def test_knn_queries_outside_the_box_near_and_far(ring_cap):
    rng = np.random.default_rng(21)
    P = rng.random((600, 3))
    near = np.concatenate([rng.random((100, 3)) * [0.2, 1, 1] + [1.0, 0, 0],      # a slab beyond the x = 1 face
                           rng.random((100, 3)) * [1, 0.3, 1] + [0, -0.3, 0],     # and one below y = 0
                           [[-0.05, -0.05, 1.05], [0.5, 0.5, 1.4], [1.0, 1.0, 1.0]]])
    # the first and the last lie more than kIcpSearchR0Max cells outside whatever the cell edge: they take the scan; the
    # middle one's clamped cell is two cells outside, its rings end on the worklist or when they have covered the grid
    far = np.array([[1e6, 0.5, 0.5], [-40.0, -40.0, -40.0], [0.5, 0.5, 3e9]])
    for k in (5, 40):
        assert_knn(tp.knn_search(P, near, k), ref_knn(("near", k), P, near, k), "near k %d" % k)
        fell_near = fallbacks()
        assert_knn(tp.knn_search(P, far, k), ref_knn(("far", k), P, far, k), "far k %d" % k)
        assert fallbacks() == len(far) if ring_cap == 0 else 2 <= fallbacks() <= len(far)
        if ring_cap:
            assert fell_near < len(near)  # just outside the box: the grid serves queries there
    # the lattice's interior is served by the grid alone, a far query by the scan
    L = S.lattice()
    inner = rng.random((130, 3)) * 1.0 + 0.25
    assert_knn(tp.knn_search(L, inner, 8), ref_knn(("inner", 8), L, inner, 8))
    assert fallbacks() == (len(inner) if ring_cap == 0 else 0)
    both = np.concatenate([inner, far])
    assert_knn(tp.knn_search(L, both, 8), ref_knn(("both", 8), L, both, 8))
    assert fallbacks() == len(both) if ring_cap == 0 else 2 <= fallbacks() <= len(far)


def test_knn_of_a_cloud_far_from_the_origin(ring_cap):
    rng = np.random.default_rng(33)
    P = rng.random((300, 3)) + 1e6
    Q = rng.random((130, 3)) * 1.25 + (1e6 - 0.125)
    for k in (3, 33):
        assert_knn(tp.knn_search(P, Q, k), ref_knn(("1e6", k), P, Q, k))
    d = tp.compute_point_cloud_distance(Q, P)
    assert R.bits_equal(d, np.sqrt(ref_knn(("1e6", 1), P, Q, 1)[1][:, 0]))


def test_degenerate_data(ring_cap):
    rng = np.random.default_rng(8)
    same = np.tile([[0.3, -1.25, 7.0]], (300, 1))
    line = np.outer(rng.random(400), [1.0, 2.0, -0.5]) + [3.0, 0.0, 1.0]
    plane = np.stack([rng.random(500), rng.random(500), np.full(500, 0.75)], 1)
    for name, P in (("same", same), ("line", line), ("plane", plane)):
        Q = P[:65] + rng.normal(size=(65, 3)) * 0.05
        for k in (5, 40):
            assert_knn(tp.knn_search(P, Q, k), ref_knn((name, k), P, Q, k), name)


# ---- hybrid -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_nn", [1, 32, 33, 100])
def test_hybrid_rows_with_more_fewer_and_no_neighbours(max_nn):
    rng = np.random.default_rng(50)
    P = rng.random((513, 3))
    Q = np.concatenate([rng.random((100, 3)), rng.random((29, 3)) + [1.3, 0, 0], [[9.0, 9.0, 9.0]]])  # 130 queries
    seen = set()
    for radius in (0.08, 0.45):
        cnt = assert_hybrid(tp.hybrid_search(P, Q, radius, max_nn), P, Q, radius, max_nn)
        assert fallbacks() == 0
        full = np.diff(S.radius_search(P, Q, radius)[2])
        seen |= {"zero"} if (full == 0).any() else set()
        seen |= {"fewer"} if ((full > 0) & (full < max_nn)).any() else set()
        seen |= {"more"} if (full > max_nn).any() else set()
        assert np.array_equal(cnt, np.minimum(full, max_nn))
    assert seen == {"zero", "more"} | ({"fewer"} if max_nn > 1 else set())


def test_hybrid_boundary_is_strict_and_rows_are_prefixes_of_the_radius_rows():
    P = S.lattice()
    idx, d2, cnt = tp.hybrid_search(P, P, 0.25, 8)  # the six axis neighbours sit at exactly the radius: excluded
    assert (cnt == 1).all() and np.array_equal(idx[:, 0], np.arange(len(P))) and (idx[:, 1:] == -1).all()
    assert (d2[:, 0] == 0).all() and np.isinf(d2[:, 1:]).all()
    Q = np.concatenate([S.lattice_centres(), P[::5] + 0.03125])
    for radius, max_nn in ((0.25 * 1.0001, 5), (0.5, 33), (0.6, 100)):
        hidx, hd2, hcnt = tp.hybrid_search(P, Q, radius, max_nn)
        assert_hybrid((hidx, hd2, hcnt), P, Q, radius, max_nn)
        ridx, rd2, splits = tp.radius_search(P, Q, radius)
        for i in range(len(Q)):
            m = min(max_nn, int(splits[i + 1] - splits[i]))
            assert hcnt[i] == m and np.array_equal(hidx[i, :m], ridx[splits[i]:splits[i] + m])
            assert hd2[i, :m].tobytes() == rd2[splits[i]:splits[i] + m].tobytes()


def test_hybrid_and_radius_with_colliding_buckets_and_empty_sides():
    rng = np.random.default_rng(14)
    five = rng.random((5, 3)) * 0.2  # 16 buckets for up to 27 cells: offsets share buckets
    Q = rng.random((65, 3)) * 0.4 - 0.1
    for radius in (0.05, 0.12, 0.2, 0.26, 2.0):
        assert_hybrid(tp.hybrid_search(five, Q, radius, 3), five, Q, radius, 3)
        assert_radius(tp.radius_search(five, Q, radius), five, Q, radius)
    none = np.zeros((0, 3))
    idx, d2, cnt = tp.hybrid_search(none, Q, 0.1, 4)
    assert (idx == -1).all() and np.isinf(d2).all() and (cnt == 0).all()
    assert tp.hybrid_search(five, none, 0.1, 4)[0].shape == (0, 4)
    idx, d2 = tp.knn_search(none, Q, 3)
    assert (idx == -1).all() and np.isinf(d2).all() and fallbacks() == 0
    assert tp.knn_search(five, none, 3)[0].shape == (0, 3)
    idx, d2, splits = tp.radius_search(none, Q, 0.1)
    assert len(idx) == 0 and len(d2) == 0 and not splits.any() and len(splits) == len(Q) + 1
    assert tp.radius_search(five, none, 0.1)[2].tolist() == [0]


# ---- radius -------------------------------------------------------------------------------------------------------
def test_radius_counts_equal_radius_outlier_removal_when_query_is_data():
    rng = np.random.default_rng(61)
    for P, radius in ((rng.random((513, 3)), 0.15), (S.lattice(5), 0.25), (rng.random((257, 3)) + 1e6, 0.2)):
        splits = assert_radius(tp.radius_search(P, P, radius), P, P, radius)
        counts = tp.remove_radius_outlier(P, 1, radius, return_counts=True)[2]
        assert np.array_equal(np.diff(splits), counts)
        assert fallbacks() == 0


def test_radius_that_covers_the_whole_cloud_and_one_that_reaches_nothing():
    P = np.concatenate([S.lattice(8), [[0.03125, 0.0625, 0.09375]]])  # 513 points, exact d2, ties by index
    Q = P[::8]  # 65 queries
    idx, d2, splits = tp.radius_search(P, Q, 4.0)
    assert_radius((idx, d2, splits), P, Q, 4.0)
    assert (np.diff(splits) == 513).all()
    rows_d, rows_j = d2.reshape(len(Q), 513), idx.reshape(len(Q), 513)
    assert (np.diff(rows_d, axis=1) >= 0).all()
    assert ((np.diff(rows_d, axis=1) > 0) | (np.diff(rows_j, axis=1) > 0)).all()  # ties in index order
    assert (np.sort(rows_j, axis=1) == np.arange(513)).all()
    idx, d2, splits = tp.radius_search(P, Q + 100.0, 0.5)
    assert len(idx) == 0 and len(d2) == 0 and not splits.any()


def raw_radius(problems, radius, capacity, arrays=True, fill=-77):
    """teaser_hip_icp_radius_search_batch as given: (counts, totals, idx arrays, d2 arrays), the arrays of capacity + 1
    entries preset to `fill`."""
    b = len(problems)
    dat = [np.ascontiguousarray(P, dtype=np.float64) for P, _ in problems]
    qry = [np.ascontiguousarray(Q, dtype=np.float64) for _, Q in problems]
    ptr = lambda arrs, t: (t * b)(*[a.ctypes.data_as(t) if a.size else None for a in arrs])  # noqa: E731
    nd = np.array([len(a) for a in dat], dtype=np.int32)
    nq = np.array([len(a) for a in qry], dtype=np.int32)
    cnt = [np.full(max(len(a), 1), -5, dtype=np.int32) for a in qry]
    cap = np.asarray(capacity, dtype=np.int64)
    idx = [np.full(int(c) + 1, fill, dtype=np.int32) for c in cap]
    d2 = [np.full(int(c) + 1, float(fill)) for c in cap]
    total = np.full(b, -1, dtype=np.int64)
    rs = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (b,)))
    icp._handle(-1).call(tp.lib().teaser_hip_icp_radius_search_batch, b, ptr(dat, _dp), nd.ctypes.data_as(_ip),
                         ptr(qry, _dp), nq.ctypes.data_as(_ip), rs.ctypes.data_as(_dp),
                         cap.ctypes.data_as(_lp) if arrays else None, ptr(cnt, _ip), ptr(idx, _ip) if arrays else None,
                         ptr(d2, _dp) if arrays else None, total.ctypes.data_as(_lp))
    return [c[:len(q)] for c, q in zip(cnt, qry)], total, idx, d2


def test_radius_count_then_fill_halves_and_row_splits_across_problems():
    rng = np.random.default_rng(71)
    problems = [(rng.random((257, 3)), rng.random((130, 3))), (rng.random((64, 3)), rng.random((300, 3)) * 2 - 0.5),
                (np.zeros((0, 3)), rng.random((7, 3))), (S.lattice(4), S.lattice_centres(4))]
    radius = [0.2, 0.3, 0.1, 0.25]
    refs = [S.radius_search(P, Q, r) for (P, Q), r in zip(problems, radius)]
    totals = [len(r[0]) for r in refs]
    assert totals[0] > 0 and totals[1] > 0 and totals[2] == 0 and totals[3] == 27 * 8
    # the count half: no arrays at all
    cnt, total, _, _ = raw_radius(problems, radius, [0] * 4, arrays=False)
    assert total.tolist() == totals
    for c, r in zip(cnt, refs):
        assert np.array_equal(c, np.diff(r[2]))
    # one entry short where there are entries: counts and totals only, the arrays are not touched
    cnt, total, idx, d2 = raw_radius(problems, radius, [max(t - 1, 0) for t in totals])
    assert total.tolist() == totals
    for c, r, i, d in zip(cnt, refs, idx, d2):
        assert np.array_equal(c, np.diff(r[2])) and (i == -77).all() and (d == -77.0).all()
    # exact, and mixed: problem 0 short, problem 1 with room to spare, the others exact
    for caps in (totals, [totals[0] - 1, totals[1] + 9, 0, totals[3]]):
        cnt, total, idx, d2 = raw_radius(problems, radius, caps)
        assert total.tolist() == totals
        for p, (c, r, i, d) in enumerate(zip(cnt, refs, idx, d2)):
            assert np.array_equal(c, np.diff(r[2]))
            t = totals[p] if caps[p] >= totals[p] else 0
            assert np.array_equal(i[:t], r[0][:t]) and R.bits_equal(d[:t], r[1][:t])
            assert (i[t:] == -77).all() and (d[t:] == -77.0).all()  # nothing beyond the rows, nothing when short
    # the Python call: count then fill, or one call with a hint; a hint that is too small costs the second call
    for hint in (None, max(totals), 3):
        for got, (P, Q), r in zip(tp.radius_search_batch([p[0] for p in problems], [p[1] for p in problems], radius,
                                                         max_total=hint), problems, radius):
            assert_radius(got, P, Q, r)


# ---- batch --------------------------------------------------------------------------------------------------------
def test_mixed_batch_gives_each_problem_its_own_bits_in_both_orders_and_leaves_the_handle_clean():
    from test_gpu_outlier import fresh_handle_covariances
    rng = np.random.default_rng(31)
    sizes = [(0, 40), (300, 0), (1000, 700), (40, 257), (257, 64), (1, 65), (600, 130), (64, 1), (343, 216)]
    data = [rng.random((nd, 3)) * rng.uniform(0.5, 3.0, size=3) for nd, _ in sizes]
    query = [rng.random((nq, 3)) * 1.2 - 0.1 for _, nq in sizes]
    query[6][5] = [5e5, 50.0, 50.0]  # the far-query problem
    data[8], query[8] = S.lattice(), S.lattice_centres()
    ks = [5, 3, 20, 100, 33, 7, 64, 32, 8]  # both list capacities
    radii = [0.1, 0.1, 0.12, 0.6, 0.3, 0.5, 0.2, 0.5, 0.25]
    cov_in = data[2][:800]
    cov_ref = fresh_handle_covariances(cov_in, 0.3, 20)  # a handle no search has ever touched
    self_ref = tp.self_knn(data[6], 20, return_distance=True)
    order = list(range(9))
    rev = order[::-1]
    pick = lambda seq, o: [seq[c] for c in o]  # noqa: E731
    knn = tp.knn_search_batch(data, query, ks)
    assert fallbacks() >= 1
    self_mid = tp.self_knn(data[6], 20, return_distance=True)
    hyb = tp.hybrid_search_batch(data, query, radii, ks)
    cov_mid = tp.estimate_covariances(cov_in, 0.3, 20)
    rad = tp.radius_search_batch(data, query, radii)
    knn_r = tp.knn_search_batch(pick(data, rev), pick(query, rev), pick(ks, rev))[::-1]
    hyb_r = tp.hybrid_search_batch(pick(data, rev), pick(query, rev), pick(radii, rev), pick(ks, rev))[::-1]
    rad_r = tp.radius_search_batch(pick(data, rev), pick(query, rev), pick(radii, rev))[::-1]
    cov_end = tp.estimate_covariances(cov_in, 0.3, 20)
    self_end = tp.self_knn(data[6], 20, return_distance=True)
    assert cov_ref.tobytes() == cov_mid.tobytes() == cov_end.tobytes()
    assert cov_ref.tobytes() == fresh_handle_covariances(cov_in, 0.3, 20).tobytes()
    for g in (self_mid, self_end):
        assert np.array_equal(g[0], self_ref[0]) and g[1].tobytes() == self_ref[1].tobytes()
    same = lambda a, b: all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()  # noqa: E731
                            for x, y in zip(a, b))
    for c in order:
        P, Q, k, r = data[c], query[c], ks[c], radii[c]
        k1 = tp.knn_search(P, Q, k)
        assert c != 6 or fallbacks() >= 1  # the far query
        h1 = tp.hybrid_search(P, Q, r, k)
        r1 = tp.radius_search(P, Q, r)
        assert same(knn[c], k1) and same(knn_r[c], k1)
        assert same(hyb[c], h1) and same(hyb_r[c], h1)
        assert same(rad[c], r1) and same(rad_r[c], r1)
        assert_knn(k1, S.knn_search(P, Q, k), "problem %d" % c)
        assert_hybrid(h1, P, Q, r, k)
        assert_radius(r1, P, Q, r)


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_by_name_and_the_handle_survives():
    L = tp.lib()
    h = C.c_void_p()
    assert L.teaser_hip_icp_create(0, C.byref(h)) == 0
    try:
        rng = np.random.default_rng(2)
        A, B = np.ascontiguousarray(rng.random((50, 3))), np.ascontiguousarray(rng.random((60, 3)))
        QA, QB = np.ascontiguousarray(rng.random((20, 3))), np.ascontiguousarray(rng.random((30, 3)))
        bad, qbad = B.copy(), QA.copy()
        bad[7, 1] = np.nan
        qbad[3, 2] = np.inf

        def ptrs(*arrs):
            return (_dp * len(arrs))(*[a.ctypes.data_as(_dp) if a is not None else None for a in arrs])

        i32 = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(_ip)  # noqa: E731
        f64 = lambda *v: np.array(v, dtype=np.float64).ctypes.data_as(_dp)  # noqa: E731
        i64 = lambda *v: np.array(v, dtype=np.int64).ctypes.data_as(_lp)  # noqa: E731
        nd, nq = i32(50, 60), i32(20, 30)
        idx = [np.zeros((20, 100), dtype=np.int32), np.zeros((30, 100), dtype=np.int32)]
        ip = (_ip * 2)(*[a.ctypes.data_as(_ip) for a in idx])
        ip_half = (_ip * 2)(idx[0].ctypes.data_as(_ip), None)
        cnt = [np.zeros(20, dtype=np.int32), np.zeros(30, dtype=np.int32)]
        cp = (_ip * 2)(*[a.ctypes.data_as(_ip) for a in cnt])
        total = np.zeros(2, dtype=np.int64)
        tq = total.ctypes.data_as(_lp)

        def refused(rc, *words):
            msg = L.teaser_hip_icp_last_error(h).decode()
            assert rc == 1, (rc, msg)  # TEASER_HIP_ERR_BAD_ARG
            for w in words:
                assert w in msg, msg

        knn, hyb, rad = (L.teaser_hip_icp_knn_search_batch, L.teaser_hip_icp_hybrid_search_batch,
                         L.teaser_hip_icp_radius_search_batch)
        refused(knn(h, 2, ptrs(A, bad), nd, ptrs(QA, QB), nq, i32(5, 5), ip, None), "data", "non-finite", "problem 1")
        refused(knn(h, 2, ptrs(A, B), nd, ptrs(qbad, QB), nq, i32(5, 5), ip, None), "query", "non-finite", "problem 0")
        refused(knn(h, 2, ptrs(A, None), nd, ptrs(QA, QB), nq, i32(5, 5), ip, None), "data is NULL", "problem 1")
        refused(knn(h, 2, ptrs(A, B), nd, ptrs(None, QB), nq, i32(5, 5), ip, None), "query is NULL", "problem 0")
        refused(knn(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, i32(5, 101), ip, None), "k must lie", "problem 1")
        refused(knn(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, i32(0, 5), ip, None), "k must lie", "problem 0")
        refused(knn(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, i32(5, 5), ip_half, None), "idx_out", "problem 1")
        refused(knn(h, 2, ptrs(A, B), i32(50, -1), ptrs(QA, QB), nq, i32(5, 5), ip, None), "n_data", "problem 1")
        for r in (0.0, -0.5, np.inf, np.nan, 1e200, 1e-200):
            refused(hyb(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, f64(r, 0.1), i32(5, 5), ip, None, None), "radius", "problem 0")
            refused(rad(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, f64(0.1, r), None, cp, None, None, tq), "radius", "problem 1")
        refused(hyb(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, f64(0.1, 0.1), i32(5, 101), ip, None, None), "max_nn", "problem 1")
        refused(hyb(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, f64(0.1, 0.1), i32(0, 5), ip, None, None), "max_nn", "problem 0")
        refused(hyb(h, 2, ptrs(A, bad), nd, ptrs(QA, QB), nq, f64(0.1, 0.1), i32(5, 5), ip, None, None), "data", "problem 1")
        refused(hyb(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, f64(0.1, 0.1), i32(5, 5), None, None, None), "idx_out", "problem 0")
        refused(rad(h, 2, ptrs(A, B), nd, ptrs(QA, qbad[:30]), i32(20, 20), f64(0.1, 0.1), None, cp, None, None, tq), "query", "problem 1")
        refused(rad(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, f64(0.1, 0.1), None, None, None, None, tq), "count_out", "problem 0")
        refused(rad(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, f64(0.1, 0.1), i64(10, -1), cp, ip, None, tq), "capacity", "problem 1")
        refused(rad(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, f64(0.1, 0.1), None, cp, ip, None, tq), "capacity", "problem 0")
        refused(rad(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, f64(0.1, 0.1), None, cp, None, None, None), "total_out")
        # the handle works afterwards, and empty sides with NULL pointers are legal
        rc = knn(h, 2, ptrs(A, None), i32(50, 0), ptrs(QA, None), i32(20, 0), i32(5, 5), ip_half, None)
        assert rc == 0, L.teaser_hip_icp_last_error(h).decode()
        assert np.array_equal(idx[0].ravel()[:100].reshape(20, 5), S.knn_search(A, QA, 5)[0])
        rc = rad(h, 2, ptrs(A, B), nd, ptrs(QA, QB), nq, f64(0.2, 0.2), None, cp, None, None, tq)
        assert rc == 0 and total.tolist() == [len(S.radius_search(A, QA, 0.2)[0]), len(S.radius_search(B, QB, 0.2)[0])]
    finally:
        L.teaser_hip_icp_destroy(h)


def test_open3d_style_classes_and_distances():
    rng = np.random.default_rng(5)
    P, Q = rng.random((257, 3)), rng.random((65, 3))
    nns = tp.NearestNeighborSearch(P)
    assert_knn(nns.knn_search(Q, 4), S.knn_search(P, Q, 4))
    assert_radius(nns.fixed_radius_search(Q, 0.2), P, Q, 0.2)
    assert_hybrid(nns.hybrid_search(Q, 0.2, 6), P, Q, 0.2, 6)
    tree = tp.KDTreeFlann(P)
    ridx, rd2, splits = S.radius_search(P, Q[:1], 0.2)
    n, idx, d2 = tree.search_radius_vector_3d(Q[0], 0.2)
    assert n == len(ridx) and np.array_equal(idx, ridx) and R.bits_equal(d2, rd2)
    n, idx, d2 = tree.search_knn_vector_3d(Q[0], 100)
    assert n == 100 and np.array_equal(idx, S.knn_search(P, Q[:1], 100)[0][0])
    n, idx, d2 = tree.search_hybrid_vector_3d(Q[0], 0.2, 3)
    assert n == min(3, len(ridx)) and np.array_equal(idx, ridx[:n]) and R.bits_equal(d2, rd2[:n])
    assert R.bits_equal(tp.compute_point_cloud_distance(Q, P), np.sqrt(S.knn_search(P, Q, 1)[1][:, 0]))
    assert R.bits_equal(tp.compute_nearest_neighbor_distance(P), np.sqrt(R.self_knn(P, 2)[1][:, 1]))
    assert np.isinf(tp.compute_point_cloud_distance(Q, np.zeros((0, 3)))).all()
