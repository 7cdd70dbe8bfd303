"""The Open3D-form FPFH on the MI355X (include/teaser_hip.h, "FPFH (Open3D form)") against the numpy restatement
(tests/fpfh_o3d_reference.py) with EQUALITY of the SPFH and FPFH bits: the contract uses only IEEE operations in a
stated order, so there is no tolerance.  The case list is the host driver's (tests/test_fpfh_o3d_host.py)."""
import functools
import importlib
import os

import numpy as np
import pytest

import fpfh_o3d_reference as R
import normals_reference as RN
from util import ROOT

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
    """The shared cases with the restatement's (fpfh, spfh), computed once."""
    out = []
    for name, P, N, search, radius, max_nn in R.case_list():
        F, H = R.compute_fpfh_feature(P, N, search, radius, max_nn)
        out.append((name, P, N, param(search, radius, max_nn), F, H))
    return out


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def run(sel, **kw):
    cs = [cases()[k] for k in sel]
    return tp.compute_fpfh_feature_batch([c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs], return_spfh=True, **kw)


def check(sel, got, what):
    for k, (F, H) in zip(sel, got):
        name, _, _, _, Fr, Hr = cases()[k]
        assert same(H, Hr), "%s: SPFH of %s" % (what, name)
        assert same(F, Fr), "%s: FPFH of %s" % (what, name)


def test_the_case_list_in_one_batch_alone_and_reversed():
    """Every size, the tied lattice, duplicates, the shifted cloud, max_nn 2 and 100, isolated points, k-NN with
    n < max_nn, an empty cloud, hybrid and k-NN records mixed: one batch, every cloud alone, the batch reversed."""
    sel = list(range(len(cases())))
    names = [c[0] for c in cases()]
    assert "n0" in names and {c[3][0] for c in cases()} == {"hybrid", "knn"}
    check(sel, run(sel), "one batch")
    for k in sel:
        check([k], run([k]), "alone")
    check(sel[::-1], run(sel[::-1]), "reversed")
    hit = np.concatenate([c[5] for c in cases() if len(c[5])])
    assert (hit[:, [5, 16, 27]] > 0).any() and (hit.sum(axis=1) > 0).any()


def test_a_small_list_bound_changes_no_bit():
    """fpfh_list_bytes so small that the 257-point cloud (max_nn 10: 120 bytes of lists per point, pieces of 64 points)
    runs in five pieces and five passes, the lists computed twice."""
    default = tp.get_icp_option("fpfh_list_bytes")
    sel = list(range(len(cases())))
    k257 = [c[0] for c in cases()].index("n257")
    assert -(-257 // 64) >= 3
    try:
        tp.set_icp_option("fpfh_list_bytes", 64 * 10 * 12)
        check([k257], run([k257]), "small bound, alone")
        check(sel, run(sel), "small bound, one batch")
        tp.set_icp_option("fpfh_list_bytes", 1)
        check(sel, run(sel), "bound 1, one batch")
    finally:
        tp.set_icp_option("fpfh_list_bytes", default)
    assert tp.get_icp_option("fpfh_list_bytes") == default
    with pytest.raises(tp.TeaserHipError, match="fpfh_list_bytes"):
        tp.set_icp_option("fpfh_list_bytes", 0)


def test_knn_records_do_not_depend_on_the_ring_cap():
    sel = [k for k, c in enumerate(cases()) if c[3][0] == "knn"]
    assert len(sel) >= 4
    cap = tp.get_icp_option("knn_ring_cap")
    try:
        tp.set_icp_option("knn_ring_cap", 0)
        check(sel, run(sel), "knn_ring_cap 0")
    finally:
        tp.set_icp_option("knn_ring_cap", cap)
    check(sel, run(sel), "knn_ring_cap default")


@pytest.mark.parametrize("orient", [0, 1, 2])
def test_normals_inside_the_call_equal_the_two_calls(orient):
    rng = np.random.default_rng(21)
    clouds = [rng.random((n, 3)) for n in (257, 0, 64, 5)]
    nsp = [Hybrid(0.2, 30), KNN(10), KNN(12), Hybrid(0.5, 3)]
    if orient == 1:
        nsp = [p.towards([0.5, 0.5, 3.0]) for p in nsp]
    if orient == 2:
        nsp = [p.along([0.0, 1.0, 0.0]) for p in nsp]
    sps = [Hybrid(0.3, 40), KNN(5), ("knn", 2), KNN(30)]
    normals = tp.estimate_normals_batch(clouds, nsp)
    two = tp.compute_fpfh_feature_batch(clouds, normals, sps, return_spfh=True)
    one = tp.compute_fpfh_feature_batch(clouds, None, sps, normal_search=nsp, return_spfh=True, return_normals=True)
    for (F, H, N), (F2, H2), N2 in zip(one, two, normals):
        assert same(N, N2) and same(H, H2) and same(F, F2)
    # given and estimated normals in one call
    mixed = tp.compute_fpfh_feature_batch(clouds, [normals[0], None, None, normals[3]], sps,
                                          normal_search=[None, nsp[1], nsp[2], None], return_normals=True)
    for (F, N), (F2, _), N2 in zip(mixed, two, normals):
        assert same(F, F2) and same(N, N2)


@functools.lru_cache(maxsize=None)
def config5():
    c5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    return c5["cloud_bin_0"].astype(np.float64), c5["cloud_bin_4"].astype(np.float64), float(c5["voxel_size"])


def test_extract_fpfh_on_a_crop_of_config5_equals_the_restatement():
    """The tutorial's two calls on the 1 200 points of cloud_bin_0 nearest to its first point, against the restatement fed
    with the restatement's own normals."""
    A, _, _ = config5()
    crop = np.ascontiguousarray(A[np.argsort(((A - A[0]) ** 2).sum(axis=1), kind="stable")[:1200]])
    v = 0.05
    F, N = tp.extract_fpfh(crop, v, return_normals=True)
    Nr = RN.estimate_normals(crop, RN.HYBRID, 2 * v, 30)[0]
    Fr, _ = R.compute_fpfh_feature(crop, Nr, R.HYBRID, 5 * v, 100)
    rows = int((F.view(np.uint64) == Fr.view(np.uint64)).all(axis=1).sum())
    print("extract_fpfh: %d of %d rows bit-equal, normals bit-equal in %d of %d rows, max |dF| %.3g" % (
        rows, len(F), int((N.view(np.uint64) == Nr.view(np.uint64)).all(axis=1).sum()), len(N), np.abs(F - Fr).max()))
    assert same(F, Fr)


def test_ransac_registers_config5_on_these_features():
    """registration_ransac_based_on_feature_matching with the parameters and the assertions of
    tests/test_gpu_ransac_python.py, on extract_fpfh's rows; the pose is accepted as tests/test_gpu_features.py accepts
    the solver's on this pair: more than 0.4 of the moved source within a voxel of the target."""
    import json
    from scipy.spatial import cKDTree
    A, B, vox = config5()
    fa, fb = (f for f in tp.compute_fpfh_feature_batch([A, B], None, Hybrid(5 * vox, 100), normal_search=Hybrid(2 * vox, 30)))
    assert fa.shape == (len(A), 33) and fb.shape == (len(B), 33) and fa.dtype == np.float64
    got = tp.registration_ransac_based_on_feature_matching(
        A, B, fa, fb, True, 1.5 * vox, None, ransac_n=3,
        checkers=[tp.CorrespondenceCheckerBasedOnEdgeLength(0.9), tp.CorrespondenceCheckerBasedOnDistance(1.5 * vox)],
        criteria=tp.RANSACConvergenceCriteria(4000, 0.999), seed=77)
    assert got.best_trial >= 0 and got.trials <= 4000 and len(got.correspondence_set) >= 3
    T = got.transformation
    g5 = json.load(open(os.path.join(ROOT, "tests", "golden", "config5_result_golden.json")))
    Rg, tg = np.asarray(g5["rotation"]).reshape(3, 3), np.asarray(g5["translation"])
    cos = min(1.0, max(-1.0, (np.trace(T[:3, :3].T @ Rg) - 1) / 2))
    d, _ = cKDTree(B).query(A @ T[:3, :3].T + T[:3, 3])
    print("RANSAC on the Open3D-form FPFH: %d inliers, fitness %.3f; against the committed TEASER++ pose: rotation %.4g "
          "rad, translation %.4g; %.3f of the source within a voxel" % (
              len(got.correspondence_set), got.fitness, np.arccos(cos), np.linalg.norm(T[:3, 3] - tg), (d < vox).mean()))
    assert (d < vox).mean() > 0.4


def test_python_refusals():
    P, N = R.random_cloud(20, 1)
    with pytest.raises(ValueError, match="KDTreeSearchParamRadius"):
        tp.compute_fpfh_feature(P, N, tp.KDTreeSearchParamRadius(0.3))
    with pytest.raises(ValueError, match="orient"):
        tp.compute_fpfh_feature(P, N, Hybrid(0.3, 10).towards([0, 0, 1]))
    with pytest.raises(ValueError, match="20 points and 19 normals"):
        tp.compute_fpfh_feature(P, N[:19], Hybrid(0.3, 10))
    bad = N.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        tp.compute_fpfh_feature(P, bad, Hybrid(0.3, 10))
    with pytest.raises(ValueError, match="neither normals"):
        tp.compute_fpfh_feature_batch([P], None, Hybrid(0.3, 10))
    with pytest.raises(ValueError, match="max_nn"):
        tp.compute_fpfh_feature(P, N, ("hybrid", 0.3, 1))
    # the C entry point names the argument and the cloud
    import ctypes as C
    rec = (tp.icp.IcpNormalSearchC * 1)(tp.icp.IcpNormalSearchC(2, 10, 0.3, 0, 0, (C.c_double * 3)()))
    dp = C.POINTER(C.c_double)
    out = np.zeros((20, 33))
    n = np.array([20], dtype=np.int32)
    with pytest.raises(tp.TeaserHipError, match="radius-only"):
        tp.icp._handle(-1).call(tp.lib().teaser_hip_icp_fpfh_batch, 1, (dp * 1)(P.ctypes.data_as(dp)),
                                (dp * 1)(N.ctypes.data_as(dp)), n.ctypes.data_as(C.POINTER(C.c_int32)), rec, None,
                                (dp * 1)(out.ctypes.data_as(dp)), None, None)
    assert same(tp.compute_fpfh_feature(P, N, Hybrid(0.3, 10)), R.compute_fpfh_feature(P, N, R.HYBRID, 0.3, 10)[0])
