"""examples/teaser_python_tsdf.py --scalable on the MI355X at a small size: eight 160 x 120 depth frames of the analytic
wall-and-balls scene in a ScalableTSDFVolume with the voxels of the 64^3 cube.  The figures the example prints are not
bounded but EQUAL to the numpy restatement's (tests/stsdf_reference.py) on the frames the example renders, which this
test renders again through the example's own functions: the blocks opened, the frame-block pairs, the number of points
and the largest distance to the analytic surface to its last digit."""
import importlib
import os
import re
import subprocess
import sys

import pytest

import stsdf_reference as S
import tsdf_reference as T
from util import ROOT

pytestmark = pytest.mark.gpu
EXAMPLE = os.path.join(ROOT, "examples", "teaser_python_tsdf.py")


def test_the_scalable_volume_of_the_example_equals_the_restatement():
    out = subprocess.run([sys.executable, EXAMPLE, "--width", "160", "--height", "120", "--resolution", "64", "--frames", "8", "--scalable"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    ex = importlib.import_module("teaser_python_tsdf")
    K, depths, extrinsics = ex.scene_frames(160, 120, 8)
    length, R, trunc, _ = ex.volume_settings(64)
    vol = S.ScalableVolume(length / R, trunc, S.NONE, 4)
    for d, E in zip(depths, extrinsics):
        vol.integrate(T.frame(d, (K.fx, K.fy, K.cx, K.cy), E, None, 1000.0, 6.0))
    points = vol.extract_point_cloud()[0]
    m = re.search(r"(\d+) blocks opened \((\d+) frame-block pairs\), (\d+) bytes held beside the dense cube's (\d+)", out.stdout)
    n = re.search(r"scalable extraction: (\d+) points with normals", out.stdout)
    far = re.search(r"scalable distance to the analytic surface: max ([\d.e+-]+),", out.stdout)
    assert m and n and far, out.stdout
    assert [int(x) for x in m.groups()] == [vol.opened, vol.touched, len(vol.blocks) * 8 * 16 ** 3, 8 * 64 ** 3]
    assert 1 < len(vol.blocks) and int(n.group(1)) == len(points) > 1000
    assert far.group(1) == "%.17g" % ex.distance_to_surface(points).max()
