"""examples/teaser_python_fpfh.py --cloud-distance on BASELINE config 5: the registered source's distances to the target
come from the neighbour search between the two clouds; --cloud-distance with --batch is refused before anything runs."""
import os
import re
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
EXAMPLE = os.path.join(ROOT, "examples", "teaser_python_fpfh.py")


def example(*args):
    return subprocess.run([sys.executable, EXAMPLE] + list(args), capture_output=True, text=True, timeout=600, cwd=ROOT)


def test_cloud_distance_after_registration():
    out = example("--cloud-distance")
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"source-to-target distance after registration: mean ([0-9.]+) max ([0-9.]+), (\d+) of (\d+) source "
                  r"points closer than the voxel size", out.stdout)
    assert m, out.stdout
    mean, largest, close, n = float(m.group(1)), float(m.group(2)), int(m.group(3)), int(m.group(4))
    p = re.search(r"(\d+) / (\d+) points, (\d+) correspondences", out.stdout)
    assert p and int(p.group(1)) == n
    # a 3DMatch pair overlaps in part: the registered overlap lies on the target (closer than a voxel), the rest does not
    assert 0 < mean < largest and 0 < close < n
    assert close > n // 10 and largest > 0.05


def test_cloud_distance_and_batch_together_are_an_error():
    out = example("--cloud-distance", "--batch", "2")
    assert out.returncode == 2 and "--cloud-distance" in out.stderr
