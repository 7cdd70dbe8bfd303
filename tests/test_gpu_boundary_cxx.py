"""tests/cxx/boundary_example.cpp on the MI355X: teaser::computeBoundaryPoints and teaser::BoundaryDetector of
include/teaser/boundary.h on the planar lattice, whose boundary is its perimeter; the batch against the single call."""
import importlib
import subprocess

import pytest

from boundary_cxx import build_boundary_example

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def test_cxx_boundary_example_finds_the_perimeter():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_boundary_example()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
