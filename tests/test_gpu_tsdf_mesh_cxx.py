"""tests/cxx/tsdf_mesh_example.cpp on the MI355X: teaser::UniformTSDFVolume::extractTriangleMesh of
include/teaser/tsdf.h on the two frames of tests/test_gpu_tsdf_cxx.py, the record the example prints -- counts and FNV-1a
hashes of the bytes of every output -- against the Python call on the same frames, and the PLY files teaser::PLYWriter::
writeMesh writes against those write_triangle_mesh writes: the same bytes, and parsed back the arrays they were written
from."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_tsdf_cxx import fixture_frames, fnv
from tsdf_cxx import LIBDIR
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def build_mesh_example():
    src, exe = (os.path.join(ROOT, "tests", "cxx", "tsdf_mesh_example" + e) for e in (".cpp", ""))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L" + LIBDIR, "-lteaser_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def parse_ply(path):
    """(vertices, colours as uint8 or None, triangles) of a PLY file of the kind the two writers write."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    n = int(next(x for x in lines if x.startswith("element vertex")).split()[2])
    m = int(next(x for x in lines if x.startswith("element face")).split()[2])
    colored = "property uchar red" in lines
    assert "property double x" in lines and "property list uchar int vertex_indices" in lines
    if lines[1].startswith("format ascii"):
        rows = [r.split() for r in body.decode().split("\n") if r]
        assert len(rows) == n + m
        vert = np.array([[float(x) for x in r[:3]] for r in rows[:n]], dtype=np.float64).reshape(n, 3)
        rgb = np.array([[int(x) for x in r[3:6]] for r in rows[:n]], dtype=np.uint8).reshape(n, 3) if colored else None
        assert all(r[0] == "3" for r in rows[n:])
        return vert, rgb, np.array([[int(x) for x in r[1:]] for r in rows[n:]], dtype=np.int32).reshape(m, 3)
    assert lines[1] == "format binary_little_endian 1.0"
    vt = np.dtype([("xyz", "<f8", 3)] + ([("rgb", "u1", 3)] if colored else []))
    ft = np.dtype([("n", "u1"), ("idx", "<i4", 3)])
    assert len(body) == n * vt.itemsize + m * ft.itemsize
    v = np.frombuffer(body[:n * vt.itemsize], dtype=vt)
    t = np.frombuffer(body[n * vt.itemsize:], dtype=ft)
    assert (t["n"] == 3).all()
    return v["xyz"].copy(), v["rgb"].copy() if colored else None, t["idx"].copy()


def test_cxx_mesh_equals_python_and_the_ply_files_agree(tmp_path):
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_mesh_example()
    cb, ca = str(tmp_path / "cxx_binary.ply"), str(tmp_path / "cxx_ascii.ply")
    out = subprocess.run([exe, cb, ca], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
    rec = dict(re.findall(r"^(\w+) (\w+)$", out.stdout, flags=re.M))
    depths, colors, K, E = fixture_frames()
    with tp.UniformTSDFVolume(1.0, 16, 0.15, tp.TSDFVolumeColorType.RGB8, (-0.5, -0.5, 0.5)) as vol:
        vol.integrate_batch(depths, K, E, colors)
        mesh = vol.extract_triangle_mesh(vertex_normals=True)
    want = dict(vertices=str(len(mesh.vertices)), triangles=str(len(mesh.triangles)), vertex_bits=fnv(mesh.vertices),
                color_bits=fnv(mesh.vertex_colors), normal_bits=fnv(mesh.vertex_normals), triangle_bits=fnv(mesh.triangles), checks="1")
    assert rec == want, (rec, want)
    assert len(mesh.triangles) > 100
    pb, pa = str(tmp_path / "py_binary.ply"), str(tmp_path / "py_ascii.ply")
    tp.write_triangle_mesh(pb, mesh)
    tp.write_triangle_mesh(pa, mesh, binary=False)
    assert open(pb, "rb").read() == open(cb, "rb").read() and open(pa, "rb").read() == open(ca, "rb").read()
    rgb = np.floor(np.clip(mesh.vertex_colors, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    for path in (cb, ca, pb, pa):
        v, c, t = parse_ply(path)
        assert v.tobytes() == mesh.vertices.tobytes() and np.array_equal(c, rgb) and t.tobytes() == mesh.triangles.tobytes(), path
