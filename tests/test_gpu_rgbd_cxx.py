"""tests/cxx/rgbd_example.cpp on the MI355X: teaser::createPointCloudFromRGBDImage, teaser::projectToRGBDImage and
teaser::FrameConverter of include/teaser/rgbd.h on a frame given by formulas, and the record the example prints --
counts and FNV-1a hashes of the bytes of every output -- against the Python calls on the same frame."""
import importlib
import re
import subprocess

import numpy as np
import pytest

from rgbd_cxx import build_rgbd_example

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def fixture_frame():
    """The arrays of the example: 40 x 30, depth rows 44 samples apart."""
    w, h = 40, 30
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    big = np.full((h, 44), 9, dtype=np.uint16)
    big[:, :w] = np.where((i * 7 + j * 13) % 50 == 0, 0, 500 + (i * 131 + j * 77) % 3000)
    rgb = np.stack([(i * 3 + j) % 256, (i + j * 5) % 256, (i * j) % 256], axis=2).astype(np.uint8)
    E = np.eye(4)
    E[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    E[:3, 3] = [0.5, -0.25, 0.125]
    return big[:, :w], rgb, tp.PinholeCameraIntrinsic(w, h, 32.0, 32.0, 19.5, 14.5), E


def test_cxx_example_prints_the_record_of_the_python_calls():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_rgbd_example()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
    rec = dict(re.findall(r"^(\w+) (\w+)$", out.stdout, flags=re.M))
    depth, rgb, K, E = fixture_frame()
    assert depth.strides[0] == 88
    pts, cols = tp.create_point_cloud_from_rgbd_image(rgb, depth, K, E, 1000.0, 3.0, True)
    r = tp.unproject_depth_batch([depth], K, [rgb], E, 1000.0, 3.0, convert_rgb_to_intensity=True, return_pixels=True)[0]
    assert r.points.tobytes() == pts.tobytes()
    d, c = tp.project_to_rgbd_image(pts, cols, K.width, K.height, K, E, 1000.0, 3.0)
    n_hit = tp.project_depth_batch([pts], K.width, K.height, K, None, E)[0].n_hit
    want = dict(count=str(len(pts)), points=fnv(pts), colors=fnv(cols), pixels=fnv(r.pixels), n_hit=str(n_hit),
                depth=fnv(d), color=fnv(c), checks="1")
    assert rec == want, (rec, want)
