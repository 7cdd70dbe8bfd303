"""The C++ facade of ISS keypoint detection (include/teaser/keypoints.h: teaser::ISSParams, computeISSKeypoints,
teaser::ISSKeypoints) through tests/cxx/keypoints_example.cpp: its own checks on a lattice with literal expectations,
then a config-5 cloud with the default parameters bit for bit against the restatement and the Python interface."""
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import keypoints_reference as RK
import outlier_reference as RO
from keypoints_cxx import build_keypoints_example
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def test_cxx_facade_detects_iss_keypoints():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_keypoints_example()
    own = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert own.returncode == 0 and "checks 1" in own.stdout, own.stderr
    Z = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    X = np.ascontiguousarray(Z["cloud_bin_4"][:1200], dtype=np.float64)
    with tempfile.TemporaryDirectory() as d:
        X.tofile(os.path.join(d, "cloud.bin"))
        out = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    vals = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()}
    ind = np.array([int(v) for v in vals["indices"]], dtype=np.int64)
    sal = np.array([float.fromhex(v) for v in vals["saliency"]])
    cnt = np.array([int(v) for v in vals["counts"]], dtype=np.int32).reshape(-1, 2)
    radii = np.array([float.fromhex(v) for v in vals["radii"]])
    ref = RK.iss_keypoints(X)
    assert len(ind) > 0 and np.array_equal(ind, np.flatnonzero(ref["keep"]))
    assert RO.bits_equal(sal, ref["saliency"]) and np.array_equal(cnt, ref["count"]) and RO.bits_equal(radii, ref["radii"])
    py_ind, py = tp.compute_iss_keypoints(X, return_saliency=True)
    assert np.array_equal(py_ind, ind) and py["saliency"].tobytes() == sal.tobytes() and np.array_equal(py["count"], cnt)
