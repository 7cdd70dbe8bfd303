"""The composed Python calls of RANSAC registration on the GPU: registration_ransac_based_on_feature_matching on the
config-5 fixture clouds equals the calls composed by hand, bit for bit -- match_features_knn_batch (k = 1, one
direction), the mutual filter with its fallback, then registration_ransac_based_on_correspondence -- and
examples/teaser_python_fpfh.py --ransac runs."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")

pytestmark = pytest.mark.gpu


def result_bits(r):
    return (r.transformation.tobytes(), np.float64(r.fitness).tobytes(), np.float64(r.inlier_rmse).tobytes(),
            r.best_trial, r.trials, r.valid_trials, r.correspondence_set.tobytes())


_scene = {}


def scene():
    if not _scene:
        c5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
        A, B, vox = c5["cloud_bin_0"], c5["cloud_bin_4"], float(c5["voxel_size"])
        fa, fb = tp.compute_fpfh_batch([A, B], 2 * vox, 5 * vox)
        _scene.update(A=A.astype(np.float64), B=B.astype(np.float64), vox=vox, fa=fa, fb=fb)
    return _scene


def by_hand(fa, fb, mutual_filter, ransac_n):
    fwd = tp.match_features_knn_batch([fa], [fb], 1, False)[0]
    if not mutual_filter:
        return fwd, len(fwd)
    rev = tp.match_features_knn_batch([fb], [fa], 1, False)[0]  # (j, i): j's nearest source row
    nearest_src = dict(rev.tolist())
    kept = np.array([p for p in fwd.tolist() if nearest_src.get(p[1]) == p[0]], dtype=np.int32).reshape(-1, 2)
    return (kept if len(kept) >= ransac_n else fwd), len(kept)


@pytest.mark.parametrize("mutual_filter", [False, True])
def test_feature_matching_equals_the_calls_composed_by_hand(mutual_filter):
    s = scene()
    kw = dict(ransac_n=3, checkers=[tp.CorrespondenceCheckerBasedOnEdgeLength(0.9),
                                    tp.CorrespondenceCheckerBasedOnDistance(1.5 * s["vox"])],
              criteria=tp.RANSACConvergenceCriteria(4000, 0.999), seed=77)
    got = tp.registration_ransac_based_on_feature_matching(s["A"], s["B"], s["fa"], s["fb"], mutual_filter,
                                                           1.5 * s["vox"], None, **kw)
    pairs, kept = by_hand(s["fa"], s["fb"], mutual_filter, 3)
    assert len(pairs) == (len(s["A"]) if not mutual_filter else kept) and 3 <= kept <= len(s["A"])
    assert np.array_equal(tp.feature_matching_correspondences(s["fa"], s["fb"], mutual_filter), pairs)
    want = tp.registration_ransac_based_on_correspondence(s["A"], s["B"], pairs, 1.5 * s["vox"], None, **kw)
    assert result_bits(got) == result_bits(want)
    assert got.best_trial >= 0 and got.trials <= 4000 and len(got.correspondence_set) >= 3
    print("mutual_filter %s: %d pairs, %d inliers, %d of %d trials valid" % (
        mutual_filter, len(pairs), len(got.correspondence_set), got.valid_trials, got.trials))


def test_mutual_filter_falls_back_to_all_pairs_below_ransac_n():
    """Four source rows whose nearest target rows do not answer back: fewer than ransac_n pairs survive the filter."""
    fa = np.array([[0.0, 0], [1, 0], [2, 0], [3, 0]], dtype=np.float32)
    fb = np.array([[10.0, 0], [1.6, 0], [-20, 0], [30, 0]], dtype=np.float32)  # every source row's nearest: row 1
    fwd, kept = by_hand(fa, fb, True, 3)
    assert kept == 1 and len(fwd) == 4  # only (2, 1) is mutual
    pairs = tp.feature_matching_correspondences(fa, fb, True, ransac_n=3)
    assert np.array_equal(pairs, tp.match_features_knn_batch([fa], [fb], 1, False)[0]) and len(pairs) == 4
    assert len(tp.feature_matching_correspondences(fa, fb, True, ransac_n=1)) == 1
    P = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    kw = dict(ransac_n=3, criteria=tp.RANSACConvergenceCriteria(50, 0.999), seed=5)
    got = tp.registration_ransac_based_on_feature_matching(P, P + 1.0, fa, fb, True, 0.5, None, **kw)
    want = tp.registration_ransac_based_on_correspondence(P, P + 1.0, pairs, 0.5, None, **kw)
    assert result_bits(got) == result_bits(want)


def test_fpfh_example_prints_ransac_beside_teaser():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "teaser_python_fpfh.py"), "--ransac",
                          "--ransac-iterations", "10000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "RANSAC on the same" in out.stdout and "RANSAC against TEASER++" in out.stdout and "max clique" in out.stdout
    print(out.stdout)
