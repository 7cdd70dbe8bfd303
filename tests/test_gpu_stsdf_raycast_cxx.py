"""tests/cxx/stsdf_raycast_example.cpp on the MI355X: teaser::ScalableTSDFVolume::rayCast and rayCastBatch of
include/teaser/tsdf.h on the two frames of tests/test_gpu_tsdf_cxx.py, and the record the example prints -- hit counts and
FNV-1a hashes of the bytes of every map -- against the Python calls on the same frames."""
import importlib
import os
import re
import subprocess

import pytest

from test_gpu_tsdf_cxx import fixture_frames, fnv
from tsdf_cxx import LIBDIR
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def build_raycast_example():
    src, exe = (os.path.join(ROOT, "tests", "cxx", "stsdf_raycast_example" + e) for e in (".cpp", ""))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L" + LIBDIR, "-lteaser_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cxx_ray_cast_equals_python():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_raycast_example()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
    rec = dict(re.findall(r"^(\w+) (\w+)$", out.stdout, flags=re.M))
    depths, colors, K, E = fixture_frames()
    with tp.ScalableTSDFVolume(0.0625, 0.15, tp.TSDFVolumeColorType.RGB8) as vol:
        vol.integrate_batch(depths, K, E, colors)
        one = tp.ray_cast(vol, K, E[1], weight_threshold=2.0)
        small = tp.ray_cast(vol, K, E[0], 17, 9, weight_threshold=2.0)
    want = dict(hits=str(one.hits), hits_small=str(small.hits), depth_bits=fnv(one.depth), vertex_bits=fnv(one.vertex_map),
                normal_bits=fnv(one.normal_map), color_bits=fnv(one.color), small_depth_bits=fnv(small.depth), checks="1")
    assert rec == want, (rec, want)
    assert 100 < one.hits < 40 * 30 and one.depth.shape == (30, 40) and one.color.shape == (30, 40, 3)
