"""tests/cxx/search_example.cpp on the MI355X: teaser::NearestNeighborSearch and the two point-cloud distances of
include/teaser/search.h against literal lists on a dyadic lattice."""
import importlib
import subprocess

import pytest

from search_cxx import build_search_example

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def test_cxx_search_example_finds_the_literal_neighbours():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_search_example()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
