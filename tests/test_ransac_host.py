"""The host side of RANSAC registration without a GPU: csrc/ransac.hip compiled by g++ against the HIP stand-in header
with stand-in launchers that run the one-lane functions of csrc/ransac_device.h on the CPU
(tests/ransac_host_driver.cpp), under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: the
packing, the chunk plan at chunk_trials 64, 4096 and 65536, the walk over the strict improvements, speculative chunks
dropped, a list longer than one launch hands over, the stage call and every refusal.  Then the Python surface: names,
defaults and the argument errors that need no device."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")


def test_ransac_packs_plans_walks_and_refuses(tmp_path):
    exe = str(tmp_path / "ransac_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ransac_host_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]


def test_python_surface_names_and_defaults():
    names = ["RANSACConvergenceCriteria", "CorrespondenceCheckerBasedOnEdgeLength",
             "CorrespondenceCheckerBasedOnDistance", "registration_ransac_based_on_correspondence",
             "registration_ransac_based_on_correspondence_batch", "registration_ransac_based_on_feature_matching",
             "ransac_trials_batch"]
    for name in names:
        assert name in tp.__all__ and hasattr(tp, name), name
    p = tp.ransac.RansacParamsC()
    assert tp.lib().teaser_hip_ransac_params_default(p) == 0
    assert (p.ransac_n, p.max_iteration, p.confidence, p.seed) == (3, 100000, 0.999, 0)
    assert p.edge_length_threshold == 0 and p.distance_threshold == 0 and p.with_scaling == 0
    crit = tp.RANSACConvergenceCriteria()
    assert (crit.max_iteration, crit.confidence) == (100000, 0.999)
    q = tp.ransac._params(0.05, tp.TransformationEstimationPointToPoint(), 4,
                          [tp.CorrespondenceCheckerBasedOnEdgeLength(0.9), tp.CorrespondenceCheckerBasedOnDistance(0.1)],
                          tp.RANSACConvergenceCriteria(500, 0.5), 2 ** 64 - 1)
    assert (q.max_correspondence_distance, q.ransac_n, q.max_iteration, q.confidence) == (0.05, 4, 500, 0.5)
    assert (q.edge_length_threshold, q.distance_threshold, q.seed) == (0.9, 0.1, 2 ** 64 - 1)


def test_python_argument_errors_name_what_is_not_offered():
    P, corr = np.zeros((4, 3)), np.zeros((4, 2), dtype=np.int32)
    call = tp.registration_ransac_based_on_correspondence
    with pytest.raises(ValueError, match="point-to-plane"):
        call(P, P, corr, 0.1, tp.TransformationEstimationPointToPlane())

    class Scaled:
        with_scaling = True

    with pytest.raises(ValueError, match="with_scaling"):
        call(P, P, corr, 0.1, Scaled())
    with pytest.raises(ValueError, match="normal-angle checker"):
        call(P, P, corr, 0.1, checkers=[tp.CorrespondenceCheckerBasedOnNormal(0.5)])
    with pytest.raises(TypeError, match="CorrespondenceChecker"):
        call(P, P, corr, 0.1, checkers=[object()])
    with pytest.raises(ValueError, match="more than one distance"):
        call(P, P, corr, 0.1, checkers=[tp.CorrespondenceCheckerBasedOnDistance(1), tp.CorrespondenceCheckerBasedOnDistance(2)])
    with pytest.raises(ValueError, match="threshold must be > 0"):
        call(P, P, corr, 0.1, checkers=[tp.CorrespondenceCheckerBasedOnEdgeLength(0.0)])
    with pytest.raises(TypeError, match="criteria"):
        call(P, P, corr, 0.1, criteria=0.9)
    with pytest.raises(ValueError, match="corres 0 must be an n x 2"):
        call(P, P, np.zeros((4, 3), dtype=np.int32), 0.1)
    with pytest.raises(ValueError, match="2 values for 1 problems"):
        tp.registration_ransac_based_on_correspondence_batch([P], [P], [corr], [0.1, 0.2])
    with pytest.raises(ValueError, match="seed: 2 values for 1 problems"):  # an array holds one value per problem too
        tp.registration_ransac_based_on_correspondence_batch([P], [P], [corr], 0.1, seed=np.array([1, 2]))
    assert tp.registration_ransac_based_on_correspondence_batch([], [], [], 0.1) == []  # no problems: no device needed
