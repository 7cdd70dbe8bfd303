"""include/teaser/odometry.h on the MI355X: tests/cxx/odometry_example.cpp computes two pairs of frames given by formulas
in one call and one by one; the record it prints (successes, counts and hashes of the matrices' bytes) must be the one
the Python calls give on the same arrays."""
import importlib
import subprocess

import numpy as np
import pytest

from odometry_cxx import build_odometry_example

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) % (1 << 64)
    return "%016x" % h


def frames():
    w, h, padded, out = 48, 36, 52, []
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for k in range(3):
        d = np.full((h, padded), 9, dtype=np.uint16)
        d[:, :w] = 1500 + 3 * i + 2 * (j + k) + (i * (j + k)) % 5
        g = (((i * 3 + (j + k) * 5 + (i * (j + k)) % 7) % 32).astype(np.float32) / np.float32(32.0)).astype(np.float32)
        out.append(tp.RGBDImage(g, d[:, :w], 1000.0, 3.0))
    return out


def test_the_cxx_header_gives_the_bits_of_the_python_calls():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    out = subprocess.run([build_odometry_example()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
    f = frames()
    K = tp.PinholeCameraIntrinsic(48, 36, 40.0, 40.0, 23.5, 17.5)
    opt = tp.OdometryOption([4, 3, 2])
    res = tp.compute_rgbd_odometry_batch(f[:2], f[1:], K, option=opt)
    want = ["pair %d success %d count %d iterations %d transformation %s information %s" %
            (k, r.success, r.count, r.iterations, fnv(r.transformation), fnv(r.information)) for k, r in enumerate(res)]
    c = tp.compute_rgbd_odometry_batch(f[:1], f[1:2], K, jacobian=tp.RGBDOdometryJacobianFromColorTerm, option=opt)[0]
    want.append("color success %d count %d transformation %s information %s" % (c.success, c.count, fnv(c.transformation), fnv(c.information)))
    assert out.stdout.strip().split("\n")[:3] == want, (out.stdout, want)
