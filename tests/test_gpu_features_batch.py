"""GPU tests of the batched correspondence front-end (csrc/features.hip, teaser-plusplus_amd/features.py): one call
for many clouds / pairs against the CPU oracle (oracle/features_oracle.c), the reference's fixtures
(tests/golden/features_golden.npz) and the single-call path.  The front-end's contract is bit identity, so every
comparison is exact: no tolerance appears, except the project's pose parity bar of the end-to-end test."""
import ctypes as C
import functools
import importlib
import os

import numpy as np
import pytest

from features_batch_cases import ball_cloud, config5_pairs, sparse_cloud
from oracle import features as F
from oracle import oracle
from util import ROOT

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")
feat = importlib.import_module("teaser-plusplus_amd.features")
G = np.load(os.path.join(ROOT, "tests", "golden", "features_golden.npz"))


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def same_bytes(x, y):
    """Nested lists / tuples of arrays: identical structure and identical bytes."""
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(same_bytes(a, b) for a, b in zip(x, y))
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.fixture(scope="module")
def pairs64():
    src, dst, vox = config5_pairs(64)
    out = tp.correspondences_batch(src, dst, 2 * vox, 5 * vox, return_features=True, return_normals=True)
    return src, dst, vox, out


def test_mixed_clouds_in_one_call_equal_the_oracle():
    C5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    vox = float(C5["voxel_size"])
    cases = [(G["bunny_pts"], 0.03, 0.05), (G["canstick"], 0.03, 0.05), (G["matcher_object"], 0.02, 0.04),
             (np.zeros((0, 3), dtype=np.float32), 0.03, 0.05), (sparse_cloud(), 0.03, 0.05),
             (C5["cloud_bin_0"], 2 * vox, 5 * vox), (C5["cloud_bin_4"], 2 * vox, 5 * vox)]
    f, nrm = tp.compute_fpfh_batch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases],
                                   return_normals=True)
    assert len(f) == len(nrm) == len(cases)
    for k, (pts, rn, rf) in enumerate(cases):
        if len(pts) == 0:
            assert f[k].shape == (0, 33) and nrm[k].shape == (0, 3)
            continue
        fo, no = F.fpfh_features(pts, rn, rf)
        assert same(nrm[k], no), k
        assert same(f[k], fo), k
    assert np.isnan(nrm[4][-1]).all()  # the isolated points of the sparse cloud: NaN normals, as PCL


def test_64_pairs_equal_the_single_call_path_and_the_oracle(pairs64):
    src, dst, vox, (pairs, feats, nrms) = pairs64
    est, matcher = tp.FPFHEstimation(), tp.Matcher()
    for b in range(64):
        fa = est.computeFPFHFeatures(src[b], 2 * vox, 5 * vox)
        na = est.getNormals()
        fb = est.computeFPFHFeatures(dst[b], 2 * vox, 5 * vox)
        nb = est.getNormals()
        assert same(feats[0][b], fa) and same(feats[1][b], fb), b
        assert same(nrms[0][b], na) and same(nrms[1][b], nb), b
        corr = matcher.calculateCorrespondences(src[b], dst[b], fa, fb, False, True, False, 0)
        assert [tuple(r) for r in pairs[b].tolist()] == corr, b
    for b in (0, 21, 42, 63):
        foa, noa = F.fpfh_features(src[b], 2 * vox, 5 * vox)
        fob, nob = F.fpfh_features(dst[b], 2 * vox, 5 * vox)
        assert same(feats[0][b], foa) and same(feats[1][b], fob) and same(nrms[0][b], noa) and same(nrms[1][b], nob)
        assert pairs[b].tolist() == F.match(foa, fob, crosscheck=True).tolist()
        assert len(pairs[b]) > 100


def test_a_pair_alone_or_anywhere_in_a_batch_gives_the_same_bytes(pairs64):
    src, dst, vox, out = pairs64
    kw = dict(return_features=True, return_normals=True)
    alone = tp.correspondences_batch(src[:1], dst[:1], 2 * vox, 5 * vox, **kw)
    order = np.random.default_rng(3).permutation(np.arange(1, 64)).tolist()
    order.insert(37, 0)
    shuffled = tp.correspondences_batch([src[k] for k in order], [dst[k] for k in order], 2 * vox, 5 * vox, **kw)
    again = tp.correspondences_batch(src, dst, 2 * vox, 5 * vox, **kw)

    def element(o, k):
        return [o[0][k], o[1][0][k], o[1][1][k], o[2][0][k], o[2][1][k]]
    assert same_bytes(element(alone, 0), element(out, 0))
    assert same_bytes(element(shuffled, 37), element(out, 0))
    assert same_bytes(again, out)


def test_matcher_fixture_in_a_batch():
    obj, scene, can = G["matcher_object"], G["matcher_scene"], G["canstick"]
    fo, fs, fc = tp.compute_fpfh_batch([obj, scene, can], [0.02, 0.02, 0.03], [0.04, 0.04, 0.05])
    m = tp.match_features_batch([fo, fs, fc], [fs, fo, fc])
    assert len(m[0]) == 189 and m[0].tolist() == G["matcher_matches"].tolist()
    assert m[0].tolist() == F.match(fo, fs, crosscheck=True).tolist()
    assert sorted((b, a) for a, b in m[1].tolist()) == [tuple(r) for r in m[0].tolist()]  # the swapped-roles path
    assert all(a == b for a, b in m[2].tolist()) and len(m[2]) >= 0.9 * len(fc)
    assert m[2].tolist() == F.match(fc, fc, crosscheck=True).tolist()
    m2 = tp.match_features_batch([fo, fs, fc], [fs, fo, fc], use_crosscheck=False)
    assert m2[0].tolist() == F.match(fo, fs, crosscheck=False).tolist()
    # the facade method returns what one call per pair returns
    assert tp.Matcher().calculateCorrespondencesBatch([obj, scene], [scene, obj], [fo, fs], [fs, fo], False, True,
                                                      False, 0)[0] == [tuple(r) for r in m[0].tolist()]


# the search kernel's three granularities: the 64-query block, the 64-point tile and the 256-point chunk
EDGE_N = [(a, b) for a in (1, 63, 64, 65, 255, 256, 257, 513) for b in (1, 64, 65, 130)]


@functools.lru_cache(maxsize=None)
def edge_features(dim):
    """Both orders of every EDGE_N size pair (the second order runs the swapped-roles path), random features; then a
    pair full of exact ties, both orders: features in {0, 1, 2}, 513 x 130, rows 10, 255, 256 and 300 of the larger
    side -- both sides of the chunk boundary at 256 -- copies of row 0 of the smaller (the construction of
    test_gpu_features_knn.test_ties_go_to_the_lower_index).  Returns (src list, dst list)."""
    rng = np.random.default_rng(1300 + dim)
    src, dst = [], []
    for a, b in EDGE_N:
        x, y = rng.random((a, dim), dtype=np.float32), rng.random((b, dim), dtype=np.float32)
        src += [x, y]
        dst += [y, x]
    big, small = (rng.integers(0, 3, size=(n, dim)).astype(np.float32) for n in (513, 130))
    big[[10, 255, 256, 300]] = small[0]
    return src + [big, small], dst + [small, big]


@pytest.mark.parametrize("use_crosscheck", [True, False])
@pytest.mark.parametrize("dim", [33, 7])
def test_matcher_edge_sizes_equal_the_oracle(dim, use_crosscheck):
    """The matcher is served by the k-NN kernels with K = 1, so comparing it with k = 1 k-NN matching compares a kernel
    with itself.  This pins it against the CPU oracle instead (oracle/features_oracle.c feat_match: a plain double
    loop, strict <, ascending index), exactly, at every block / tile / chunk edge and on exact ties, one call."""
    src, dst = edge_features(dim)
    # the oracle's own tie rule, checked where it matters: its 1-NN on the tie pair is numpy's first minimum (the
    # distances there are small integers, exact in float whatever the summation order)
    big, small = src[-2], src[-1]
    for data, query in ((big, small), (small, big)):
        nn = np.zeros(len(query), dtype=np.int32)
        ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        F.lib().feat_nn1(data.ctypes.data_as(fp), C.c_int32(len(data)), query.ctypes.data_as(fp),
                         C.c_int32(len(query)), C.c_int32(dim), nn.ctypes.data_as(ip))
        d = ((query[:, None, :] - data[None, :, :]) ** 2).sum(axis=2)
        assert nn.tolist() == d.argmin(axis=1).tolist()

    got = tp.match_features_batch(src, dst, use_crosscheck=use_crosscheck)
    assert len(got) == 2 * len(EDGE_N) + 2
    for p, (a, b) in enumerate(zip(src, dst)):
        want = F.match(a, b, crosscheck=use_crosscheck)
        assert len(want) >= 1
        assert same(got[p], want), "n_src %d n_dst %d%s" % (len(a), len(b), " (ties)" if p >= 2 * len(EDGE_N) else "")
    # small row 0 has four rows at distance 0 in big: it goes to the lowest, 10, whose nearest is row 0 in turn
    assert [10, 0] in got[-2].tolist() and [0, 10] in got[-1].tolist()
    if use_crosscheck:
        assert not any(r in got[-1].tolist() for r in ([0, 255], [0, 256], [0, 300]))


def test_long_lists_inside_a_batch():
    """One call that uses the LDS sort and the rank sort at once."""
    ball, can = ball_cloud(), G["canstick"]
    est = tp.FPFHEstimation()
    f = est.computeFPFHFeaturesBatch([ball, can], [0.2, 0.03], [1.1, 0.05])
    nrm = est.getNormals()
    for k, (pts, rn, rf) in enumerate([(ball, 0.2, 1.1), (can, 0.03, 0.05)]):
        fo, no = F.fpfh_features(pts, rn, rf)
        assert same(f[k], fo) and same(nrm[k], no), k


def test_wave_splitting_does_not_change_a_byte(pairs64):
    """A list budget of 256 KB and a partial-result budget of 4 MB.  Every point is its own neighbour (8 bytes), so
    the lists of the 128 clouds hold at least 8 bytes per point: more than three list budgets.  A pair's two searches
    hold 8 bytes per query and 256-row data chunk: summed over the 64 pairs more than three partial-result budgets.
    So both the clouds and the searches fall into at least three waves, whatever the radii catch."""
    src, dst, vox, out = pairs64
    total = sum(len(c) for c in src + dst)
    list_budget, part_budget = 256 << 10, 4 << 20
    assert 8 * total > 3 * list_budget
    part = sum(8 * (-(-len(a) // 256) * len(b) + -(-len(b) // 256) * len(a)) for a, b in zip(src, dst))
    assert part > 3 * part_budget
    h = feat._handle()
    h._set_budget(list_budget, part_budget)
    try:
        split = tp.correspondences_batch(src, dst, 2 * vox, 5 * vox, return_features=True, return_normals=True)
        matched = tp.match_features_batch(out[1][0], out[1][1])  # waves of searches in the matching-only call
    finally:
        h._set_budget(None, None)
    assert same_bytes(split, out)
    assert same_bytes(matched, out[0])
    assert same_bytes(tp.match_features_batch(out[1][0], out[1][1]), out[0])  # and with the default budgets


def test_bad_arguments_are_refused_and_the_handle_stays_usable():
    can = G["canstick"]
    good = tp.compute_fpfh_batch([can], 0.03, 0.05)[0]
    L = tp.lib()
    h = feat._handle()

    def refused(fn, *args, **kw):
        with pytest.raises(tp.TeaserHipError) as e:
            fn(*args, **kw)
        assert "BAD_ARG" in str(e.value)
        assert same(tp.compute_fpfh_batch([can], 0.03, 0.05)[0], good)  # the next valid call is correct
        return str(e.value)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        msg = refused(tp.compute_fpfh_batch, [can, can], [0.03, bad], 0.05)
        assert "normal_radius" in msg and "(problem 1)" in msg
        msg = refused(tp.compute_fpfh_batch, [can, can, can], 0.03, [0.05, 0.05, bad])
        assert "fpfh_radius" in msg and "(problem 2)" in msg
        msg = refused(tp.correspondences_batch, [can, can], [can, can], [0.03, bad], 0.05)
        assert "normal_radius" in msg and "(problem 1)" in msg
    # raw calls: a negative n, a NULL cloud where n > 0, dim out of range, pair_cap too small
    import ctypes as C
    fp, ip, dp, i64p = feat._fp, feat._ip, feat._dp, feat._i64p
    pts = np.ascontiguousarray(can, dtype=np.float32)
    out = np.zeros((len(pts), 33), dtype=np.float32)
    r1, r2 = np.array([0.03, 0.03]), np.array([0.05, 0.05])

    def raw_fpfh(n, clouds):
        n = np.array(n, dtype=np.int32)
        return refused(h.call, L.teaser_hip_features_fpfh_batch, 2, (fp * 2)(*clouds), n.ctypes.data_as(ip),
                       r1.ctypes.data_as(dp), r2.ctypes.data_as(dp), (fp * 2)(out.ctypes.data_as(fp), out.ctypes.data_as(fp)),
                       None)
    msg = raw_fpfh([len(pts), -1], [pts.ctypes.data_as(fp), pts.ctypes.data_as(fp)])
    assert "n must be >= 0" in msg and "(problem 1)" in msg
    msg = raw_fpfh([len(pts), len(pts)], [pts.ctypes.data_as(fp), None])
    assert "cloud is NULL" in msg and "(problem 1)" in msg

    msg = refused(h.call, L.teaser_hip_features_fpfh_batch, 2, (fp * 2)(pts.ctypes.data_as(fp), pts.ctypes.data_as(fp)),
                  np.array([len(pts)] * 2, dtype=np.int32).ctypes.data_as(ip), r1.ctypes.data_as(dp),
                  r2.ctypes.data_as(dp), (fp * 2)(out.ctypes.data_as(fp), None), None)
    assert "fpfh_out is NULL" in msg and "(problem 1)" in msg

    needed = len(tp.match_features_batch([good], [good])[0])

    def raw_match(dim=33, cap=None, n=None, null=(), corr=False):
        """Two problems (good, good); problem 1 gets the bad value: n = (n_src, n_dst), cap, or a NULL among
        'src', 'dst', 'pairs' -- or a whole NULL array among 'pair_cap', 'n_pairs'.  corr: through
        correspondences_batch (clouds in) instead of match_batch (features in)."""
        a = pts if corr else good
        n_a = np.array([len(a), len(a) if n is None else n[0]], dtype=np.int32)
        n_b = np.array([len(a), len(a) if n is None else n[1]], dtype=np.int32)
        bufs = [np.zeros((2 * len(a), 2), dtype=np.int32) for _ in range(2)]
        caps = np.array([2 * len(a), 2 * len(a) if cap is None else cap], dtype=np.int64)
        cnt = np.zeros(2, dtype=np.int64)
        ap = a.ctypes.data_as(fp)
        args = [2, (fp * 2)(ap, None if "src" in null else ap), n_a.ctypes.data_as(ip),
                (fp * 2)(ap, None if "dst" in null else ap), n_b.ctypes.data_as(ip)]
        args += [r1.ctypes.data_as(dp), r2.ctypes.data_as(dp), 1] if corr else [dim, 1]
        args += [(ip * 2)(bufs[0].ctypes.data_as(ip), None if "pairs" in null else bufs[1].ctypes.data_as(ip)),
                 None if "pair_cap" in null else caps.ctypes.data_as(i64p),
                 None if "n_pairs" in null else cnt.ctypes.data_as(i64p)]
        args += [None] * 4 if corr else []
        fn = L.teaser_hip_features_correspondences_batch if corr else L.teaser_hip_features_match_batch
        return refused(h.call, fn, *args), cnt.tolist()
    assert "dim" in raw_match(dim=0)[0] and "dim" in raw_match(dim=65)[0]
    msg, cnt = raw_match(cap=needed - 1)
    assert "pair_cap" in msg and "(problem 1)" in msg and str(needed) in msg and cnt == [needed, needed]
    for corr, src_name, dst_name in ((False, "src_feat", "dst_feat"), (True, "src_xyz", "dst_xyz")):
        msg = raw_match(null=("src",), corr=corr)[0]
        assert src_name + " is NULL" in msg and "(problem 1)" in msg
        msg = raw_match(null=("dst",), corr=corr)[0]
        assert dst_name + " is NULL" in msg and "(problem 1)" in msg
        msg = raw_match(null=("pairs",), corr=corr)[0]
        assert "pairs is NULL" in msg and "(problem 1)" in msg
        assert "pair_cap must not be NULL" in raw_match(null=("pair_cap",), corr=corr)[0]
        assert "n_pairs must not be NULL" in raw_match(null=("n_pairs",), corr=corr)[0]
        for n in ((-1, len(pts)), (len(pts), -3)):
            msg = raw_match(n=n, corr=corr)[0]
            assert "must be >= 0" in msg and "(problem 1)" in msg
    # non-finite features leave a query without a nearest neighbour
    nanf = good.copy()
    nanf[:] = np.nan
    msg = refused(tp.match_features_batch, [good, nanf], [good, good])
    assert "non-finite" in msg and "(problem 1)" in msg
    # valid corner cases: an empty batch, empty clouds, empty sides
    assert tp.compute_fpfh_batch([], 0.03, 0.05) == [] and tp.match_features_batch([], []) == []
    assert tp.correspondences_batch([], [], 0.03, 0.05) == []
    e = np.zeros((0, 3), dtype=np.float32)
    p = tp.correspondences_batch([e, can, can], [can, e, can], 0.03, 0.05)
    assert p[0].shape == (0, 2) and p[1].shape == (0, 2)
    assert p[2].tolist() == tp.match_features_batch([good], [good])[0].tolist()
    assert same(tp.compute_fpfh_batch([can], 0.03, 0.05)[0], good)


def test_end_to_end_registration_of_batched_correspondences(pairs64):
    """correspondences_batch -> solve_correspondences with helpers.py's parameters against oracle.solve on the same
    correspondences: clique size and edge count, and -- where the oracle reports the clique unique -- clique and pose
    (1e-4 / 1e-4 m, the project's parity bar).  Where the maximum clique is not unique two correct solvers may hold
    different cliques, so the exact statements left are checked: the GPU's clique is a clique of the oracle's graph of
    the oracle's size, and the oracle's estimators on that clique give the GPU's pose (1e-4 / 1e-4 m) and inlier
    lists.  (test_gpu_features.pose_cross_checks adds residual-fraction heuristics tuned on the unperturbed pair; one
    of the perturbed pairs measures 0.89 against its 0.9, so they are not used here.)"""
    src, dst, vox, (pairs, _, _) = pairs64
    p = dict(noise_bound=vox, cbar2=1.0, estimate_scaling=False, rotation_gnc_factor=1.4,
             rotation_max_iterations=10000, rotation_cost_threshold=1e-16)
    s = tp.RobustRegistrationSolver(tp.RobustRegistrationSolver.Params(**p))
    for b in range(8):
        c = pairs[b]
        sol = s.solve_correspondences(src[b], dst[b], [tuple(r) for r in c.tolist()])
        sc, dc = src[b][c[:, 0]].astype(np.float64).T, dst[b][c[:, 1]].astype(np.float64).T
        o = oracle.solve(sc, dc, **dict(p, estimate_scaling=0))
        assert sol.valid and o["valid"]
        clique = s.getInlierMaxClique()
        assert len(clique) == len(o["max_clique"]) and s.raw_solution().num_edges == o["num_edges"]
        if o["clique_unique"]:
            assert clique == o["max_clique"].tolist()
            assert np.linalg.norm(sol.rotation - o["rotation"]) < 1e-4
            assert np.linalg.norm(sol.translation - o["translation"]) < 1e-4
            continue
        _, bm = oracle.inlier_bitmap(sc, dc, vox, 1.0, False)
        dense = np.unpackbits(bm.view(np.uint8), axis=1, bitorder="little")[:, :len(c)].astype(bool)
        assert dense[np.ix_(clique, clique)].sum() == len(clique) * (len(clique) - 1)
        sub = oracle.solve(sc[:, clique], dc[:, clique], **dict(p, estimate_scaling=0))
        assert sub["valid"] and len(sub["max_clique"]) == len(clique)
        assert np.linalg.norm(sol.rotation - sub["rotation"]) < 1e-4
        assert np.linalg.norm(sol.translation - sub["translation"]) < 1e-4
        assert s.getRotationInliers() == [int(v) for v in sub["rotation_inliers"]]
        assert s.getTranslationInliers() == [int(v) for v in sub["translation_inliers"]]
