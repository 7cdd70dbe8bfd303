"""What the batched tuple test promises without a GPU: the C++ facade example compiles against the header (it runs on
the GPU: test_gpu_tuple_test_cxx.py) and fails loudly without a device, and the Python call checks its arguments and
refuses to run without a device instead of falling back to the host routine."""
import importlib
import subprocess

import numpy as np
import pytest

import tuple_test_reference as R

tp = importlib.import_module("teaser-plusplus_amd")


@pytest.mark.parametrize("eigen", [False, True])
def test_cxx_tuple_example_builds_and_fails_loudly_without_device(eigen):
    from tuple_cxx import build_tuple_example
    exe = build_tuple_example(eigen)
    if tp.device_count() == 0:
        assert subprocess.call([exe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 77


def test_python_call_checks_arguments_and_has_no_cpu_path():
    src, dst, pairs = R.scene()
    assert "teaser_hip_features_tuple_test_batch" in tp.EXPORTED_SYMBOLS and "tuple_test_batch" in tp.__all__
    with pytest.raises(ValueError, match="tuple_scale"):
        tp.tuple_test_batch([src, src], [dst, dst], [pairs, pairs], [0.9, 0.9, 0.9], 11)
    with pytest.raises(ValueError, match="m x 2"):
        tp.tuple_test_batch([src], [dst], [np.zeros((4, 3), dtype=np.int32)], 0.9, 11)
    with pytest.raises(ValueError, match="same length"):
        tp.tuple_test_batch([src], [dst, dst], [pairs], 0.9, 11)
    if tp.device_count() == 0:
        with pytest.raises(tp.TeaserHipError):
            tp.tuple_test_batch([src], [dst], [pairs], R.SCALE, 11)
