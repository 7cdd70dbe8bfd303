"""tests/cxx/stsdf_mesh_example.cpp on the MI355X: teaser::ScalableTSDFVolume::extractTriangleMesh of
include/teaser/tsdf.h on the two frames of tests/test_gpu_tsdf_cxx.py, the record the example prints -- counts and FNV-1a
hashes of the bytes of every output -- against the Python call on the same frames and against the restatement
(tests/stsdf_mesh_reference.py), and the PLY files teaser::PLYWriter::writeMesh writes against those write_triangle_mesh
writes: the same bytes, and parsed back the arrays they were written from."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import stsdf_mesh_reference as R
import stsdf_reference as S
import tsdf_reference as T
from test_gpu_tsdf_cxx import fixture_frames, fnv
from test_gpu_tsdf_mesh_cxx import parse_ply
from tsdf_cxx import LIBDIR
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def build_mesh_example():
    src, exe = (os.path.join(ROOT, "tests", "cxx", "stsdf_mesh_example" + e) for e in (".cpp", ""))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L" + LIBDIR, "-lteaser_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_mesh_equals_python_and_the_ply_files_agree(tmp_path):
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_mesh_example()
    cb, ca = str(tmp_path / "cxx_binary.ply"), str(tmp_path / "cxx_ascii.ply")
    out = subprocess.run([exe, cb, ca], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
    rec = dict(re.findall(r"^(\w+) (\w+)$", out.stdout, flags=re.M))
    depths, colors, K, E = fixture_frames()
    with tp.ScalableTSDFVolume(0.0625, 0.15, tp.TSDFVolumeColorType.RGB8, 16, 1) as vol:
        vol.integrate_batch(depths, K, E, colors)
        mesh = tp.extract_triangle_mesh(vol, vertex_normals=True)
        blocks = vol.block_count
    want = dict(blocks=str(blocks), vertices=str(len(mesh.vertices)), triangles=str(len(mesh.triangles)), vertex_bits=fnv(mesh.vertices),
                color_bits=fnv(mesh.vertex_colors), normal_bits=fnv(mesh.vertex_normals), triangle_bits=fnv(mesh.triangles), checks="1")
    assert rec == want, (rec, want)
    assert len(mesh.triangles) > 100 and blocks > 1
    # the restatement on the same frames: the scene crosses block faces
    ref = S.ScalableVolume(0.0625, 0.15, S.RGB8, 1)
    for d, c, e in zip(depths, colors, E):
        ref.integrate(T.frame(d, (K.fx, K.fy, K.cx, K.cy), e, c))
    m = R.extract_triangle_mesh(ref, normals=True)
    assert R.face_statistics(ref)[2] >= 1
    assert (fnv(m.vertices), fnv(m.colors), fnv(m.normals), fnv(m.triangles)) == (rec["vertex_bits"], rec["color_bits"], rec["normal_bits"],
                                                                                 rec["triangle_bits"])
    pb, pa = str(tmp_path / "py_binary.ply"), str(tmp_path / "py_ascii.ply")
    tp.write_triangle_mesh(pb, mesh)
    tp.write_triangle_mesh(pa, mesh, binary=False)
    assert open(pb, "rb").read() == open(cb, "rb").read() and open(pa, "rb").read() == open(ca, "rb").read()
    rgb = np.floor(np.clip(mesh.vertex_colors, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    for path in (cb, ca, pb, pa):
        v, c, t = parse_ply(path)
        assert v.tobytes() == mesh.vertices.tobytes() and np.array_equal(c, rgb) and t.tobytes() == mesh.triangles.tobytes(), path
