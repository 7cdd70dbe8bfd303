"""examples/teaser_python_tsdf.py --scalable --mesh PATH on the MI355X at a small size: eight 160 x 120 depth frames of
the analytic wall-and-balls scene in a ScalableTSDFVolume with the voxels of the 64^3 cube, its triangle mesh extracted
and written as a PLY file.  The figures the example prints are not bounded but EQUAL to the restatement's
(tests/stsdf_mesh_reference.py) on the frames the example renders, which this test renders again through the example's
own functions; the file is read back by teaser::PLYReader (tests/cxx/ply_example.cpp, as tests/test_ply_io.py runs it)
and, parsed in Python, holds the restatement's vertices and triangles."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import stsdf_mesh_reference as R
import stsdf_reference as S
import tsdf_reference as T
from test_gpu_tsdf_mesh_cxx import parse_ply
from util import ROOT

pytestmark = pytest.mark.gpu
EXAMPLE = os.path.join(ROOT, "examples", "teaser_python_tsdf.py")


def test_the_scalable_mesh_of_the_example_equals_the_restatement(tmp_path):
    path = str(tmp_path / "scalable.ply")
    out = subprocess.run([sys.executable, EXAMPLE, "--width", "160", "--height", "120", "--resolution", "64", "--frames", "8",
                          "--scalable", "--mesh", path], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    ex = importlib.import_module("teaser_python_tsdf")
    K, depths, extrinsics = ex.scene_frames(160, 120, 8)
    length, res, trunc, _ = ex.volume_settings(64)
    vol = S.ScalableVolume(length / res, trunc, S.NONE, 4)
    for d, E in zip(depths, extrinsics):
        vol.integrate(T.frame(d, (K.fx, K.fy, K.cx, K.cy), E, None, 1000.0, 6.0))
    blocks, cubes, crossing, differ = R.face_statistics(vol)
    assert blocks > 1 and crossing >= 1 and differ >= 1
    want = R.extract_triangle_mesh(vol)
    line = r"mesh: (\d+) vertices, (\d+) triangles, [\d.]+ ms; distance to the analytic surface: max ([\d.]+); written to (\S+)"
    dense, scalable = re.search(r"^" + line, out.stdout, flags=re.M), re.search(r"^scalable " + line, out.stdout, flags=re.M)
    assert dense and scalable, out.stdout  # the same line for both volume classes
    assert [int(scalable.group(1)), int(scalable.group(2))] == [len(want.vertices), len(want.triangles)] and len(want.triangles) > 1000
    assert scalable.group(3) == "%.6f" % ex.distance_to_surface(want.vertices).max() and scalable.group(4) == path
    reader = os.path.join(ROOT, "tests", "cxx", "ply_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), reader + ".cpp", "-o", reader])
    back = subprocess.run([reader, path], capture_output=True, text=True)
    assert back.returncode == 0, back.stdout + back.stderr
    tok = back.stdout.split()  # the count, the sums of the float32 coordinates, the first point's x
    assert int(tok[0]) == len(want.vertices) and np.float32(tok[4]) == np.float32(want.vertices[0, 0])
    assert np.allclose([float(x) for x in tok[1:4]], want.vertices.astype(np.float32).astype(np.float64).sum(0), rtol=0, atol=1e-6)
    v, c, t = parse_ply(path)
    assert c is None and v.tobytes() == want.vertices.tobytes() and t.tobytes() == want.triangles.tobytes()
