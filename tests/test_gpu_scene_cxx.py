"""tests/cxx/scene_example.cpp on the MI355X: teaser::RaycastingScene of include/teaser/scene.h on the lattice sheet, and
the record the example prints -- counts and FNV-1a hashes of the bytes of every array -- against the Python calls on the
same rays and points."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import scene_reference as R
from test_gpu_tsdf_cxx import fnv
from tsdf_cxx import LIBDIR
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def build_scene_example():
    src, exe = (os.path.join(ROOT, "tests", "cxx", "scene_example" + e) for e in (".cpp", ""))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), src,
                           "-o", exe, "-L" + LIBDIR, "-lteaser_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_scene_equals_python():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_scene_example()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
    rec = dict(re.findall(r"^(\w+) (\w+)$", out.stdout, flags=re.M))
    ij = np.array([(i, j) for i in range(9) for j in range(9)], dtype=np.float32)
    i, j = ij[:, 0], ij[:, 1]
    z = np.zeros(81, np.float32)
    down = np.stack([i, j, z + 5, z, z, z - 1], axis=1)
    slant = np.stack([i - 2, j + np.float32(0.25), z + 3, z + np.float32(0.5), z + np.float32(0.125), z - 1], axis=1)
    rays = np.stack([down, slant], axis=1).reshape(-1, 6).astype(np.float32)
    pts = np.stack([i + np.float32(0.5), j * np.float32(1.25) - 1, (i - j) * np.float32(0.5)], axis=1).astype(np.float32)
    E = np.diag([1.0, -1.0, -1.0, 1.0])
    E[:3, 3] = [-4.0, 3.0, 6.0]
    with tp.RaycastingScene() as s:
        s.add_triangles(*R.sheet())
        hit, near = s.cast_rays(rays), s.compute_closest_points(pts)
        occ = s.test_occlusions(rays, 5.0, 5.0)
        view = s.cast_views(tp.PinholeCameraIntrinsic(17, 9, 12.0, 12.0, 8.0, 4.0), [E])[0]
    want = dict(hits=str(int(np.isfinite(hit["t_hit"]).sum())), occluded=str(int(occ.sum())), t_bits=fnv(hit["t_hit"]),
                geometry_bits=fnv(hit["geometry_ids"]), primitive_bits=fnv(hit["primitive_ids"]), uv_bits=fnv(hit["primitive_uvs"]),
                normal_bits=fnv(hit["primitive_normals"]), closest_bits=fnv(near["points"]), distance_bits=fnv(near["distance"]),
                closest_primitive_bits=fnv(near["primitive_ids"]), closest_uv_bits=fnv(near["primitive_uvs"]),
                view_t_bits=fnv(view["t_hit"]), view_normal_bits=fnv(view["primitive_normals"]), checks="1")
    assert rec == want, (rec, want)
    assert 81 <= int(want["hits"]) < 162 and int(want["occluded"]) == 81 and np.isfinite(view["t_hit"]).any()
