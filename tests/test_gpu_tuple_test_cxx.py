"""teaser::Matcher::tupleTestBatch and the k-NN calls' tuple arguments (include/teaser/matcher.h) on the GPU:
tests/cxx/tuple_example.cpp compares every batched result with teaser_hip_tuple_test called in the same program."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("eigen", [False, True])
def test_cxx_tuple_methods_equal_the_host_routine(eigen):
    from tuple_cxx import build_tuple_example
    exe = build_tuple_example(eigen)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
