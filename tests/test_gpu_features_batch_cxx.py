"""The C++ facade's batch methods (include/teaser/fpfh.h, matcher.h) on the GPU: tests/cxx/fpfh_batch_example.cpp
compares them with the single-cloud / single-pair methods bit for bit."""
import os
import subprocess

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("eigen", [False, True])
def test_cxx_batch_methods_equal_the_single_call_methods(eigen):
    from fpfh_batch_cxx import build_fpfh_batch_example
    exe = build_fpfh_batch_example(eigen)
    for args in ([], [os.path.join(ROOT, "tests", "golden", "bun_zipper_res3.ply")]):
        out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "batch == single 1" in out.stdout
