"""The C++ facade of normal estimation (include/teaser/icp.h: teaser::NormalSearch, estimateNormals, the point-to-plane
overloads without dst_normals) through tests/cxx/normals_example.cpp: its own checks on a plane, then the config-5 pair
-- normals of the target in both search modes against the restatement at the bar of tests/test_gpu_normals.py and bit
for bit against the Python interface, and the self-estimating point-to-plane call against the Python one."""
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import icp_reference as R
import normals_reference as RN
from normals_cxx import build_normals_example
from test_gpu_normals import check, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def test_cxx_facade_estimates_normals_and_refines_with_them():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_normals_example()
    own = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert own.returncode == 0 and "checks 1" in own.stdout, own.stderr
    P, Q, r, init = R.config5_problem()
    with tempfile.TemporaryDirectory() as d:
        P.tofile(os.path.join(d, "src.bin"))
        Q.tofile(os.path.join(d, "dst.bin"))
        init.tofile(os.path.join(d, "init.bin"))
        out = subprocess.run([exe, d, float(r).hex(), float(2 * r).hex()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    vals = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()}
    arr = lambda name, shape: np.array([float.fromhex(v) for v in vals[name]]).reshape(shape)  # noqa: E731
    n = len(Q)
    hyb = tp.KDTreeSearchParamHybrid(2 * r, 30).along([0, 0, 1])
    got = (arr("hybrid_normals", (n, 3)), arr("hybrid_covariances", (n, 3, 3)), arr("hybrid_eigenvalues", (n, 3)))
    check(got, RN.estimate_normals(Q, 0, 2 * r, 30, 2, (0.0, 0.0, 1.0)), "C++ hybrid")
    py = tp.estimate_normals(Q, hyb, covariances=True, eigenvalues=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, py))
    knn = tp.estimate_normals(Q, tp.KDTreeSearchParamKNN(30).towards([0, 0, 0]))
    assert arr("knn_normals", (n, 3)).tobytes() == knn.tobytes()
    res = tp.registration_icp(P, Q, r, init, tp.TransformationEstimationPointToPlane(tp.TukeyLoss(0.1)),
                              target_normals=hyb)
    assert arr("T", (4, 4)).tobytes() == res.transformation.tobytes()
    assert float.fromhex(vals["fitness"][0]) == res.fitness and float.fromhex(vals["rmse"][0]) == res.inlier_rmse
    assert int(vals["iterations"][0]) == res.iterations and res.iterations >= 2
    assert int(vals["correspondences"][0]) == len(res.correspondence_set)
