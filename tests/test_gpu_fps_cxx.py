"""The C++ facade of farthest-point down-sampling (include/teaser/fps.h: teaser::farthestPointDownSample,
teaser::FarthestPointSampler) through tests/cxx/fps_example.cpp: a 5 x 5 grid whose selection, ties included, is worked
out by hand (tests/test_fps_reference.py::test_the_grid_of_the_cxx_example checks the same numbers without a GPU),
single, batched and on both routes."""
import importlib
import subprocess

import pytest

from fps_cxx import build_fps_example

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def test_cxx_facade_samples_the_grid():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_fps_example()
    own = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert own.returncode == 0 and "checks 1" in own.stdout, own.stderr
