"""examples/teaser_python_fpfh.py --drop-boundary 90 on BASELINE config 5: the rim of both clouds goes before the
descriptors are computed, fewer points remain than without the option, and TEASER++ still returns a valid solution.
(tests/test_gpu_fpfh_o3d_example.py sets no bound on the pose of this example, so none is set here: the printed counts
and `valid` are what is checked.)"""
import os
import re
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
EXAMPLE = os.path.join(ROOT, "examples", "teaser_python_fpfh.py")


def test_drop_boundary_leaves_fewer_points_and_a_valid_solution():
    out = subprocess.run([sys.executable, EXAMPLE, "--drop-boundary", "90"], capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    d = re.search(r"(\d+) of (\d+) / (\d+) of (\d+) points dropped, (\d+) / (\d+) remain", out.stdout)
    assert d, out.stdout
    da, na, db, nb, ra, rb = (int(g) for g in d.groups())
    assert (na, nb) == (5208, 5034) and 0 < da < na and 0 < db < nb and ra == na - da and rb == nb - db
    m = re.search(r"(\d+) / (\d+) points, (\d+) correspondences, max clique (\d+)", out.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (ra, rb), out.stdout
    assert int(m.group(3)) >= 3 and int(m.group(4)) >= 3, out.stdout  # what a registration needs
    w = re.search(r"without --drop-boundary: (\d+) correspondences; with it: (\d+); solution valid: (\w+)", out.stdout)
    assert w and int(w.group(2)) == int(m.group(3)) and int(w.group(1)) >= 3 and w.group(3) == "True", out.stdout
    print(out.stdout)
