"""The Python calls of plane segmentation on the GPU return the C ABI's bits: segment_plane is segment_plane_batch of
one, the batch is teaser_hip_plane_segment_batch called by hand, float32 input is converted, not refused; and
examples/teaser_python_fpfh.py --remove-plane runs on a synthetic pair (a floor under two copies of a cluttered shape)."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import plane_scenes as SC
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")

pytestmark = pytest.mark.gpu


def test_python_calls_return_the_c_abis_bits():
    P = SC.planted(1200, 0.5, 81)
    plane, inliers = tp.segment_plane(P, 0.01, 3, 400, 0.9999, 82)
    r = tp.segment_plane_batch([P, P.astype(np.float32)], 0.01, [3, 4], 400, 0.9999, [82, 83])
    assert plane.tobytes() == r[0].plane_model.tobytes() and np.array_equal(inliers, r[0].inliers)
    assert np.array_equal(np.nonzero(r[0].mask)[0], inliers) and inliers.dtype == np.int32 and len(inliers) > 400
    assert r[1].best_trial >= 0 and len(r[1].mask) == 1200
    # by hand through ctypes
    L, pl = tp.lib(), tp.plane
    h = pl._cache.get(-1)
    prm = pl._params(0.01, 3, 400, 0.9999, 82)
    out, inl, msk = pl.PlaneResultC(), np.zeros(1200, dtype=np.int32), np.zeros(1200, dtype=np.uint8)
    with h.lock:
        rc = L.teaser_hip_plane_segment(h.h, P.ctypes.data_as(pl._dp), 1200, C.byref(prm), C.byref(out),
                                        inl.ctypes.data_as(pl._ip), msk.ctypes.data_as(pl._u8p))
    assert rc == 0 and out.n_inliers == len(inliers)
    assert np.array(out.plane[:]).tobytes() == plane.tobytes() and np.array_equal(inl[:out.n_inliers], inliers)
    assert np.array_equal(msk, r[0].mask)
    assert (out.fitness, out.inlier_rmse, out.best_trial, out.trials, out.valid_trials) == (
        r[0].fitness, r[0].inlier_rmse, r[0].best_trial, r[0].trials, r[0].valid_trials)
    t = tp.plane_trials_batch([P], 0.01, int(out.best_trial), 1, 3, 82)[0]
    assert t["count"][0] == out.n_inliers and t["flags"][0] == pl.FLAG_VALID
    assert t["E"][0] / np.sqrt(float(t["count"][0])) == out.inlier_rmse


def write_ply(path, P):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(P))
        for p in P:
            f.write("%.9g %.9g %.9g\n" % tuple(p))


def test_fpfh_example_removes_the_dominant_plane(tmp_path):
    rng = np.random.default_rng(5)
    shape = rng.uniform(-0.5, 0.5, size=(1500, 3)) * [1.0, 0.6, 0.3] + [0, 0, 0.4]
    floor = np.stack([rng.uniform(-1, 1, 2500), rng.uniform(-1, 1, 2500), rng.normal(0, 0.002, 2500)], 1)
    A = np.concatenate([shape, floor])
    c, s = np.cos(0.3), np.sin(0.3)
    B = A @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + [0.1, -0.05, 0.02]
    write_ply(str(tmp_path / "a.ply"), A)
    write_ply(str(tmp_path / "b.ply"), B)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "teaser_python_fpfh.py"), str(tmp_path / "a.ply"),
                          str(tmp_path / "b.ply"), "--voxel", "0.05", "--remove-plane", "0.02"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dominant plane of the source" in out.stdout and "dominant plane of the target" in out.stdout
    assert "removed after" in out.stdout and "max clique" in out.stdout
    print(out.stdout)
