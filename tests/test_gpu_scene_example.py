"""examples/teaser_python_scene.py on the MI355X at a small size: eight 160 x 120 frames of the analytic wall-and-balls
scene, all but the last fused into a 64^3 volume, its triangle mesh put into a RaycastingScene, rendered from the
held-out pose and compared with the TSDF ray cast of the same pose, and the volume's point cloud measured against the
mesh.

The bounds are reasoned, not picked from a run.  Depth: both renderings place the surface inside the lattice cell where
the TSDF changes sign -- the mesh by interpolating along the cell's edges, anywhere in the cell (at most its diagonal,
sqrt(3) voxels, from the crossing on the ray), the ray cast by interpolating between two samples one step apart (one
voxel of z-depth, at most 1.3 voxels along a corner ray of this camera) -- so where both see the same sheet of the
surface they differ by less than sqrt(3) + 1.3 < 3.1 voxels; silhouette pixels, where they may see different sheets, are
far fewer than one in twenty, hence the bound on the median and on the 95th percentile and none on the maximum.  Scan to
mesh: a point of extract_point_cloud lies on a lattice edge by the interpolation rule of the mesh vertices, so wherever
the mesh exists it IS a mesh vertex up to the rounding of vertex and point to float32 (half an ulp of 4 m per
coordinate, twice): below 2e-6 m.  Points on the rim of the observed region may have no mesh beside them, so the bound is
on the median."""
import os
import re
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
EXAMPLE = os.path.join(ROOT, "examples", "teaser_python_scene.py")


def test_the_mesh_renders_like_the_volume_and_the_scan_lies_on_it():
    out = subprocess.run([sys.executable, EXAMPLE, "--width", "160", "--height", "120", "--resolution", "64", "--frames", "8"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    mesh = re.search(r"mesh: (\d+) vertices, (\d+) triangles from 7 frames in 64\^3 voxels", out.stdout)
    scene = re.search(r"scene: (\d+) triangles built in [\d.]+ ms; 160 x 120 view [\d.]+ ms; (\d+) closest-point queries", out.stdout)
    depth = re.search(r"held-out pose: (\d+) mesh pixels, (\d+) ray-cast pixels, (\d+) both, median ([\d.e+-]+), 95th percentile ([\d.e+-]+),", out.stdout)
    scan = re.search(r"scan to mesh: (\d+) points, median ([\d.e+-]+) m, 95th percentile ([\d.e+-]+) m", out.stdout)
    assert mesh and scene and depth and scan, out.stdout
    assert int(mesh.group(2)) == int(scene.group(1)) > 1000 and int(scene.group(2)) == int(scan.group(1)) > 1000
    assert int(depth.group(3)) > 160 * 120 // 2, out.stdout                      # the held-out camera sees the model
    assert float(depth.group(4)) < 3.1 and float(depth.group(5)) < 3.1, out.stdout
    assert float(scan.group(2)) < 2e-6, out.stdout
