"""The boundary-point entry point is exported and declared with its argument count, the header section exists, the C++
header (include/teaser/boundary.h) compiles against the library, and without a GPU the calls fail loudly with the
no-device error (the example with exit code 77)."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from boundary_cxx import build_boundary_example
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")


def test_entry_point_is_exported_and_declared():
    assert "teaser_hip_icp_boundary_points_batch" in tp.EXPORTED_SYMBOLS
    f = tp.lib().teaser_hip_icp_boundary_points_batch
    assert f is not None and len(f.argtypes) == 13
    raw = C.CDLL(os.path.join(ROOT, "teaser-plusplus_amd", "libteaser_hip.so"))
    assert raw.teaser_hip_icp_boundary_points_batch is not None
    header = open(os.path.join(ROOT, "include", "teaser_hip.h")).read()
    assert "/* Boundary points (Open3D's PointCloud.compute_boundary_points" in header
    m = re.search(r"TEASER_HIP_API int32_t teaser_hip_icp_boundary_points_batch\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 13
    # a NULL handle is refused before anything is read
    assert f(None, 1, None, None, None, None, None, None, None, None, None, None, None) == 1  # TEASER_HIP_ERR_BAD_ARG


def test_without_a_device_the_call_fails_loudly():
    if tp.device_count() > 0:
        return  # on the GPU box tests/test_gpu_boundary.py covers the call
    P = np.zeros((4, 3))
    N = np.tile([0.0, 0.0, 1.0], (4, 1))
    with pytest.raises(tp.TeaserHipError, match="NO_DEVICE"):
        tp.compute_boundary_points(P, N, radius=0.5)
    with pytest.raises(tp.TeaserHipError, match="NO_DEVICE"):
        tp.compute_boundary_points_batch([P], [N], ("knn", 3))


def test_cxx_header_compiles_and_fails_loudly_without_gpu():
    exe = build_boundary_example()
    rc = subprocess.call([exe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert rc == (0 if tp.device_count() > 0 else 77)
