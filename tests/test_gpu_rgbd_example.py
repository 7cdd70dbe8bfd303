"""examples/teaser_python_rgbd.py on the MI355X: two depth frames of an analytic scene rendered from two known camera
poses, unprojected in one call, registered (voxel grid, FPFH, TEASER++, ICP) and projected back into the target's camera.
The planted pose is recovered to within a voxel: 0.05 in translation, and in rotation the angle a voxel subtends at the
scene's distance of about 2 (0.05 / 2 rad = 1.43 degrees).  Of the target pixels the registered source covers, nine in ten
agree with the frame within a voxel (with the true pose 99.7 % do; the rest are occlusion rims), and the source covers
more than four in ten of the target's pixels (69 % with the true pose: one splatted point per pixel leaves holes)."""
import os
import re
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
EXAMPLE = os.path.join(ROOT, "examples", "teaser_python_rgbd.py")


def test_the_planted_pose_is_recovered_and_the_projection_agrees():
    out = subprocess.run([sys.executable, EXAMPLE], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    u = re.search(r"320 x 240 frames -> (\d+) / (\d+) points", out.stdout)
    assert u and int(u.group(1)) == int(u.group(2)) == 320 * 240, out.stdout  # every ray hits the wall or a ball
    m = re.search(r"ICP pose error: rotation ([\d.]+) deg, translation ([\d.]+)", out.stdout)
    assert m, out.stdout
    assert float(m.group(1)) < 1.43 and float(m.group(2)) < 0.05, out.stdout
    p = re.search(r"projection: (\d+) of (\d+) target pixels covered by the registered source; (\d+) of them", out.stdout)
    assert p, out.stdout
    covered, valid, agree = (int(g) for g in p.groups())
    assert valid == 320 * 240 and covered > 0.4 * valid and agree > 0.9 * covered, out.stdout
