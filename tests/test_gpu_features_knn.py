"""GPU tests of the k-nearest-neighbour matching (csrc/features.hip, kernels_features.hip: feat_knn_*) against the numpy
restatement of its semantics (features_knn_reference.py).  The contract (include/teaser_hip.h, "k nearest") is bit
identity, so every comparison is exact equality of int32 indices / pairs and float32 distances: no tolerance appears."""
import functools
import importlib
import os

import numpy as np
import pytest

import features_knn_reference as R
from util import ROOT

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")
feat = importlib.import_module("teaser-plusplus_amd.features")

# the kernel's three granularities: the 64-query block, the 64-point tile and the 256-point chunk
ND = [1, 63, 64, 65, 255, 256, 257, 513]
NQ = [1, 64, 65, 130]
KS = [1, 2, 5, 16]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def quantised(rng, n, dim):
    return rng.integers(0, 3, size=(n, dim)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def edge_problems(dim):
    """The ND x NQ problems of one dim and their reference lists for k = 16, computed once: the lists of a smaller k
    are the first k slots (the order is total, and unused slots hold -1 / +inf for every k)."""
    rng = np.random.default_rng(dim)
    data = [rng.random((nd, dim), dtype=np.float32) for nd in ND for _ in NQ]
    query = [rng.random((nq, dim), dtype=np.float32) for _ in ND for nq in NQ]
    ref = [R.knn(d, q, 16) for d, q in zip(data, query)]
    return data, query, ref


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim", [33, 7, 32, 64])
def test_edge_sizes_equal_the_reference(dim, k):
    data, query, ref = edge_problems(dim)
    idx, dist = tp.knn_features_batch(data, query, k, return_distance=True)
    assert len(idx) == len(dist) == len(ND) * len(NQ)
    for p, (ri, rd) in enumerate(ref):
        where = "nd %d nq %d" % (len(data[p]), len(query[p]))
        assert same(idx[p], np.ascontiguousarray(ri[:, :k])), where
        assert same(dist[p], np.ascontiguousarray(rd[:, :k])), where
    assert (idx[0][:, 1:] == -1).all() and np.isinf(dist[0][:, 1:]).all()  # nd = 1: k_eff = 1
    # the single-problem form, and the call without distances
    p = len(NQ) * ND.index(257) + NQ.index(65)
    assert same(tp.knn_features(data[p], query[p], k), idx[p])
    one = tp.knn_features(data[p], query[p], k, return_distance=True)
    assert same(one[0], idx[p]) and same(one[1], dist[p])


@pytest.mark.parametrize("dim", [33, 7])
def test_ties_go_to_the_lower_index(dim):
    """Features in {0, 1, 2}: every distance is a small integer and a row of 513 candidates is full of exact ties.
    Rows 10, 255, 256 and 300 -- both sides of the chunk boundary at 256 -- are copies of one row, which is also
    query 0: four candidates at distance 0, in index order."""
    rng = np.random.default_rng(70 + dim)
    data, query = quantised(rng, 513, dim), quantised(rng, 130, dim)
    data[[10, 255, 256, 300]] = query[0]
    for k in (1, 3, 5, 16):
        ri, rd = R.knn(data, query, k)
        idx, dist = tp.knn_features(data, query, k, return_distance=True)
        assert same(idx, ri) and same(dist, rd), k
        assert idx[0][:min(k, 4)].tolist() == [10, 255, 256, 300][:k] and (dist[0][:min(k, 4)] == 0).all()
        for mutual in (True, False):
            assert same(tp.match_features_knn(query, data, k, mutual), R.match_knn(query, data, k, mutual)), (k, mutual)
            assert same(tp.match_features_knn(data, query, k, mutual), R.match_knn(data, query, k, mutual)), (k, mutual)
    # every row equal: the k lowest indices, whatever the chunk
    flat = np.ones((300, dim), dtype=np.float32)
    for k in KS:
        idx, dist = tp.knn_features(flat, flat[:70], k, return_distance=True)
        assert idx.tolist() == [list(range(k))] * 70 and (dist == 0).all()


def mixed_batch():
    """Pairs of 3 to 600 rows, with an empty side and an empty pair."""
    rng = np.random.default_rng(11)
    sizes = [(3, 600), (600, 3), (257, 64), (0, 40), (130, 513), (40, 0), (300, 299), (0, 0), (65, 255)]
    src = [quantised(rng, a, 33) + rng.random((a, 33), dtype=np.float32) for a, _ in sizes]
    dst = [quantised(rng, b, 33) + rng.random((b, 33), dtype=np.float32) for _, b in sizes]
    return src, dst


def test_a_problem_alone_or_inside_a_batch_gives_the_same_bytes():
    src, dst = mixed_batch()
    for k, mutual in ((3, True), (3, False), (16, True)):
        batch = tp.match_features_knn_batch(src, dst, k, mutual)
        for p in range(len(src)):
            assert same(tp.match_features_knn(src[p], dst[p], k, mutual), batch[p]), (k, mutual, p)
            assert same(batch[p], R.match_knn(src[p], dst[p], k, mutual)), (k, mutual, p)
        assert batch[3].shape == (0, 2) and batch[5].shape == (0, 2) and batch[7].shape == (0, 2)
        again = tp.match_features_knn_batch(src[::-1], dst[::-1], k, mutual)
        assert all(same(a, b) for a, b in zip(again[::-1], batch))
    idx, dist = tp.knn_features_batch(dst, src, 5, return_distance=True)
    for p in range(len(src)):
        one = tp.knn_features(dst[p], src[p], 5, return_distance=True)
        assert same(one[0], idx[p]) and same(one[1], dist[p]), p
    assert idx[5].shape == (40, 5) and (idx[5] == -1).all() and np.isinf(dist[5]).all()  # no data: k_eff = 0
    assert idx[3].shape == (0, 5)
    assert tp.match_features_knn_batch([], [], 2) == [] and tp.knn_features_batch([], [], 2) == []


def test_the_partial_result_budget_does_not_change_a_byte():
    """Six pairs, k = 5 (served by the 8-slot kernel): a search holds 8 bytes per query, 256-row data chunk and slot.
    The budget is set to the bytes of the smallest of the 12 searches, so no two searches share a wave: 12 waves in
    the mutual call, 6 in the others."""
    rng = np.random.default_rng(12)
    sizes = [(300, 400), (513, 257), (260, 300), (400, 270), (350, 350), (258, 600)]
    src = [rng.random((a, 33), dtype=np.float32) for a, _ in sizes]
    dst = [rng.random((b, 33), dtype=np.float32) for _, b in sizes]
    k, slots = 5, 8
    part = [8 * slots * -(-nd // 256) * nq for a, b in sizes for nd, nq in ((b, a), (a, b))]
    budget = min(part)
    assert len(part) == 12 and all(x + y > budget for x in part for y in part) and len(sizes) >= 4
    want = [tp.match_features_knn_batch(src, dst, k, m) for m in (True, False)]
    want_knn = tp.knn_features_batch(dst, src, k, return_distance=True)
    h = feat._handle()
    h._set_budget(None, budget)
    try:
        got = [tp.match_features_knn_batch(src, dst, k, m) for m in (True, False)]
        got_knn = tp.knn_features_batch(dst, src, k, return_distance=True)
        h._set_budget(None, 1)  # (a wave always holds at least one search)
        tiny = tp.match_features_knn_batch(src, dst, k, True)
    finally:
        h._set_budget(None, None)
    for w, g in zip(want + list(want_knn) + [want[0]], got + list(got_knn) + [tiny]):
        assert len(w) == len(g) == 6 and all(same(a, b) for a, b in zip(w, g))
    assert all(same(a, R.match_knn(s, d, k, True)) for a, s, d in zip(want[0], src, dst))


@pytest.fixture(scope="module")
def config5():
    c5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    A, B, vox = c5["cloud_bin_0"], c5["cloud_bin_4"], float(c5["voxel_size"])
    fa, fb = tp.compute_fpfh_batch([A, B], 2 * vox, 5 * vox)
    return A, B, vox, fa, fb


def test_k1_mutual_equals_the_existing_matcher(config5):
    """The matcher's searches are k-NN searches with k = 1 (features.hip, run_match), so this compares two routes
    through one kernel: the host bookkeeping of the cross check against the device-side mutual filter.  It does not pin
    the matcher's searches independently; test_gpu_features_batch.test_matcher_edge_sizes_equal_the_oracle does."""
    _, _, _, fa, fb = config5
    old = tp.match_features_batch([fa, fb], [fb, fa], use_crosscheck=True)
    new = tp.match_features_knn_batch([fa, fb], [fb, fa], 1, mutual=True)
    assert len(old[0]) > 100 and same(new[0], old[0]) and same(new[1], old[1])
    assert same(tp.match_features_knn(fa, fb, 1), old[0])


def test_more_neighbours_give_a_superset_and_no_smaller_clique(config5):
    """pairs(k = 1, mutual) is a subset of pairs(k = 3, mutual), itself a subset of pairs(k = 3, one-directional): the
    first three entries of a list start with its first.  A superset of correspondences contains the smaller set's
    consistency graph as an induced subgraph, so its maximum clique is no smaller -- provided the exact search
    finished on both (a search that hit its time limit reports an incumbent: the inequality is then not checked)."""
    A, B, vox, fa, fb = config5
    p1, p3, p3all = (tp.match_features_knn(fa, fb, k, m) for k, m in ((1, True), (3, True), (3, False)))
    s1, s3, s3all = (set(map(tuple, p.tolist())) for p in (p1, p3, p3all))
    assert len(s1) == len(p1) and len(s3) == len(p3) and len(p3all) == 3 * len(fa)
    assert s1 <= s3 <= s3all and len(s1) < len(s3) < len(s3all)
    params = tp.RobustRegistrationSolver.Params(noise_bound=vox, cbar2=1.0, estimate_scaling=False,
                                                rotation_gnc_factor=1.4, rotation_max_iterations=10000,
                                                rotation_cost_threshold=1e-16, max_clique_time_limit=10)
    solver = tp.RobustRegistrationSolver(params)
    cliques, limit = [], False
    for pairs in (p1, p3):
        solver.solve_correspondences(A, B, [tuple(r) for r in pairs.tolist()])
        limit |= solver.last_status == 5
        cliques.append(len(solver.getInlierMaxClique()))
    print("config 5: %d / %d / %d pairs, max clique %d (k = 1) and %d (k = 3)%s"
          % (len(p1), len(p3), len(p3all), cliques[0], cliques[1], ", time limit hit" if limit else ""))
    if not limit:
        assert cliques[1] >= cliques[0]


def test_non_finite_features_are_refused_and_the_handle_stays_usable():
    rng = np.random.default_rng(13)
    good, other = rng.random((70, 33), dtype=np.float32), rng.random((90, 33), dtype=np.float32)
    bad = good.copy()
    bad[17] = np.nan
    want = tp.match_features_knn(good, other, 3)
    for call in (lambda: tp.match_features_knn_batch([good, bad], [other, other], 3, True),
                 lambda: tp.match_features_knn_batch([good, bad], [other, other], 3, False),
                 lambda: tp.match_features_knn_batch([good, other], [other, bad], 3, True),
                 lambda: tp.knn_features_batch([other, other], [good, bad], 3)):
        with pytest.raises(tp.TeaserHipError) as e:
            call()
        assert "BAD_ARG" in str(e.value) and "non-finite" in str(e.value) and "(problem 1)" in str(e.value)
        assert same(tp.match_features_knn(good, other, 3), want)  # the next valid call is correct
    # a non-finite DATA row never enters a list: with enough finite rows left every list is full
    idx, dist = tp.knn_features(bad, other, 16, return_distance=True)
    ri, rd = R.knn(bad, other, 16)
    assert same(idx, ri) and same(dist, rd) and 17 not in idx
    assert same(tp.match_features_knn(other, bad, 2, mutual=False), R.match_knn(other, bad, 2, mutual=False))


def test_raw_calls_refuse_bad_k_and_a_small_pair_cap():
    rng = np.random.default_rng(14)
    a, b = rng.random((50, 33), dtype=np.float32), rng.random((60, 33), dtype=np.float32)
    needed = len(tp.match_features_knn(a, b, 4, mutual=False))
    assert needed == 200
    L, h = tp.lib(), feat._handle()
    fp, ip, i64p = feat._fp, feat._ip, feat._i64p
    n_a, n_b = np.array([50, 50], dtype=np.int32), np.array([60, 60], dtype=np.int32)
    bufs = [np.zeros((200, 2), dtype=np.int32) for _ in range(2)]
    cnt = np.zeros(2, dtype=np.int64)

    def raw(k, caps):
        caps = np.array(caps, dtype=np.int64)
        with pytest.raises(tp.TeaserHipError) as e:
            h.call(L.teaser_hip_features_match_knn_batch, 2, (fp * 2)(a.ctypes.data_as(fp), a.ctypes.data_as(fp)),
                   n_a.ctypes.data_as(ip), (fp * 2)(b.ctypes.data_as(fp), b.ctypes.data_as(fp)), n_b.ctypes.data_as(ip),
                   33, k, 0, (ip * 2)(bufs[0].ctypes.data_as(ip), bufs[1].ctypes.data_as(ip)), caps.ctypes.data_as(i64p),
                   cnt.ctypes.data_as(i64p))
        assert "BAD_ARG" in str(e.value)
        return str(e.value)
    assert "k must be in [1, 16]" in raw(0, [200, 200]) and "k must be in [1, 16]" in raw(17, [200, 200])
    msg = raw(4, [200, 199])
    assert "pair_cap" in msg and "(problem 1)" in msg and "200" in msg and cnt.tolist() == [200, 200]
    assert same(bufs[0], tp.match_features_knn(a, b, 4, mutual=False))  # (the problem with room was written)
    idx = np.zeros((50, 2), dtype=np.int32)
    with pytest.raises(tp.TeaserHipError, match="idx is NULL.*problem 0"):
        h.call(L.teaser_hip_features_knn_batch, 1, (fp * 1)(b.ctypes.data_as(fp)), n_b.ctypes.data_as(ip),
               (fp * 1)(a.ctypes.data_as(fp)), n_a.ctypes.data_as(ip), 33, 2, (ip * 1)(None), None)
    h.call(L.teaser_hip_features_knn_batch, 1, (fp * 1)(b.ctypes.data_as(fp)), n_b.ctypes.data_as(ip),
           (fp * 1)(a.ctypes.data_as(fp)), n_a.ctypes.data_as(ip), 33, 2, (ip * 1)(idx.ctypes.data_as(ip)), None)
    assert same(idx, R.knn(b, a, 2)[0])


def test_clouds_in_equals_fpfh_then_matching(config5):
    A, B, vox, fa, fb = config5
    rng = np.random.default_rng(15)
    small = rng.uniform(0, 0.3, size=(400, 3)).astype(np.float32)
    empty = np.zeros((0, 3), dtype=np.float32)
    src, dst = [A, small, empty, B], [B, small[::-1].copy(), small, A]
    rn, rf = [2 * vox, 0.1, 0.1, 2 * vox], [5 * vox, 0.15, 0.15, 5 * vox]  # (dense enough for a normal at every point)
    feats = tp.compute_fpfh_batch(src + dst, rn + rn, rf + rf)
    assert same(feats[0], fa) and same(feats[4], fb)
    for k, mutual in ((1, True), (4, True), (4, False)):
        want = tp.match_features_knn_batch(feats[:4], feats[4:], k, mutual)
        got, (fs, fd), (ns, nd) = tp.correspondences_knn_batch(src, dst, rn, rf, k, mutual, return_features=True,
                                                              return_normals=True)
        assert all(same(a, b) for a, b in zip(got, want)) and len(got[0]) > 100 and got[2].shape == (0, 2)
        assert all(same(a, b) for a, b in zip(fs + fd, feats))
        assert [x.shape for x in ns + nd] == [(len(c), 3) for c in src + dst]
    assert same(tp.correspondences_knn(A, B, 2 * vox, 5 * vox, 4, mutual=False), want[0])
    assert same(tp.correspondences_knn_batch(src, dst, rn, rf, 1)[0], tp.correspondences_batch(src, dst, rn, rf)[0])
