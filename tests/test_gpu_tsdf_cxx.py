"""tests/cxx/tsdf_example.cpp on the MI355X: teaser::UniformTSDFVolume of include/teaser/tsdf.h on two frames given by
formulas, and the record the example prints -- counts and FNV-1a hashes of the bytes of every output -- against the
Python calls on the same frames."""
import importlib
import re
import subprocess

import numpy as np
import pytest

from tsdf_cxx import build_tsdf_example

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def fixture_frames():
    """The arrays of the example: two frames of 40 x 30, depth rows 44 samples apart."""
    w, h = 40, 30
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    depths, colors, E = [], [], []
    for k in range(2):
        big = np.full((h, 44), 9, dtype=np.uint16)
        big[:, :w] = np.where((i * 7 + j * 13) % 50 == 0, 0, 900 + 4 * i + 3 * j + 20 * k + (i * j) % 7)
        depths.append(big[:, :w])
        colors.append(np.stack([(i * 3 + j + 40 * k) % 256, (i + j * 5) % 256, (i * j + k) % 256], axis=2).astype(np.uint8))
        E.append(np.eye(4))
    E[1][:3, 3] = [0.0625, -0.03125, 0.015625]
    return depths, colors, tp.PinholeCameraIntrinsic(w, h, 32.0, 32.0, 19.5, 14.5), E


def test_cxx_example_prints_the_record_of_the_python_calls():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_tsdf_example()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
    rec = dict(re.findall(r"^(\w+) (\w+)$", out.stdout, flags=re.M))
    depths, colors, K, E = fixture_frames()
    assert depths[0].strides[0] == 88
    with tp.UniformTSDFVolume(1.0, 16, 0.15, tp.TSDFVolumeColorType.RGB8, (-0.5, -0.5, 0.5)) as vol:
        vol.integrate_batch(depths, K, E, colors)
        pc, vp = vol.extract_point_cloud(), vol.extract_voxel_point_cloud()
        want = dict(count=str(len(pc.points)), points=fnv(pc.points), normals=fnv(pc.normals), colors=fnv(pc.colors),
                    vcount=str(len(vp.points)), vpoints=fnv(vp.points), vcolors=fnv(vp.colors),
                    tsdf=fnv(vol.extract_volume_tsdf()), color=fnv(vol.extract_volume_color()), checks="1")
    assert rec == want, (rec, want)
