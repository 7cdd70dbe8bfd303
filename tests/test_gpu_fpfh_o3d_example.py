"""examples/teaser_python_fpfh.py --open3d-fpfh on BASELINE config 5: Open3D's normals + FPFH in place of the PCL form,
alone, composed with --ransac --fgr --knn, and with --batch."""
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


def test_open3d_fpfh_registers_config5_with_ransac_fgr_and_knn():
    out = example("--open3d-fpfh", "--knn", "2", "--ransac", "--ransac-iterations", "10000", "--fgr")
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Open3D-form FPFH: 5208 + 5034 rows of 33 float64" in out.stdout
    m = re.search(r"(\d+) / (\d+) points, (\d+) correspondences, max clique (\d+)", out.stdout)
    assert m and int(m.group(3)) >= 3 and int(m.group(4)) >= 3, out.stdout  # what a registration needs
    assert "RANSAC against TEASER++" in out.stdout and "FGR" in out.stdout
    print(out.stdout)


def test_open3d_fpfh_with_batch():
    out = example("--open3d-fpfh", "--batch", "2", "--icp-iterations", "5")
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"2 pairs: \d+ \.\. \d+ points after down-sampling, \d+ \.\. \d+ correspondences", out.stdout)
