"""tests/cxx/fpfh_o3d_example.cpp on the MI355X: teaser::computeFPFHFeature and teaser::FPFHOpen3D of
include/teaser/fpfh_open3d.h against rows known in closed form, the batch against the single calls, extractFPFH against
estimateNormals followed by compute."""
import importlib
import subprocess

import pytest

from fpfh_o3d_cxx import build_fpfh_o3d_example

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def test_cxx_fpfh_o3d_example_computes_the_known_rows():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_fpfh_o3d_example()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
