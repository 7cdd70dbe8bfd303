"""The ray-cast entry points of the TSDF volume are exported and declared with their argument counts, the header states
the contract under its heading, the view record has the size the header asserts and the defaults it names, a NULL handle
is refused before anything is read, and the Python side checks its arguments before the device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from test_tsdf_abi import _NoDeviceVolume
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")
tsdf = importlib.import_module("teaser-plusplus_amd.tsdf")

ENTRY_POINTS = (("teaser_hip_tsdf_view_default", 1), ("teaser_hip_tsdf_ray_cast_views", 8))


def test_entry_points_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "teaser_hip.h")).read()
    for text in ("/* TSDF ray casting:", "t.geometry.VoxelBlockGrid.ray_cast", "bit parity with an Open3D\n * binary is NOT claimed",
                 "At most 2 R + 2 steps", "HIT when f_prev > 0.0f && w >= wthr_f && f <= 0.0f", "a non-rigid extrinsic is NOT inverted",
                 "A missed pixel is 0 in every output", 'static_assert(sizeof(teaser_tsdf_view_c) == 200'):
        assert text in header, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "TSDF ray casting" in design and "kernel-resource-usage" in design
    raw = C.CDLL(os.path.join(ROOT, "teaser-plusplus_amd", "libteaser_hip.so"))
    for name, argc in ENTRY_POINTS:
        assert name in tp.EXPORTED_SYMBOLS
        f = getattr(tp.lib(), name)
        assert f is not None and len(f.argtypes) == argc and getattr(raw, name) is not None
        m = re.search(r"TEASER_HIP_API int32_t %s\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == argc, name
    hits = (C.c_int64 * 1)(-3)
    view = tsdf.TsdfViewC()
    assert tp.lib().teaser_hip_tsdf_ray_cast_views(None, 1, C.byref(view), None, None, None, None, hits) == 1  # BAD_ARG
    assert hits[0] == -3


def test_the_view_record_and_its_defaults():
    assert C.sizeof(tsdf.TsdfViewC) == 200
    assert [(n, getattr(tsdf.TsdfViewC, n).offset) for n in ("width", "height", "fx", "extrinsic", "depth_min", "weight_threshold", "reserved")] == \
        [("width", 0), ("height", 4), ("fx", 8), ("extrinsic", 40), ("depth_min", 168), ("weight_threshold", 184), ("reserved", 192)]
    v = tsdf.TsdfViewC()
    C.memset(C.byref(v), 0xAB, C.sizeof(v))
    assert tp.lib().teaser_hip_tsdf_view_default(C.byref(v)) == 0
    assert (v.width, v.height, v.fx, v.fy, v.cx, v.cy, v.reserved) == (0, 0, 0.0, 0.0, 0.0, 0.0, 0)
    assert (v.depth_min, v.depth_max, v.weight_threshold) == (0.1, 3.0, 3.0)
    assert np.array_equal(np.array(v.extrinsic[:]).reshape(4, 4), np.eye(4))
    assert tp.lib().teaser_hip_tsdf_view_default(None) == 1


def test_python_side_without_a_device():
    assert tp.TSDFRayCastResult is not None
    K = tp.PinholeCameraIntrinsic(5, 3, 4.0, 4.0, 2.0, 1.0)
    vol = _NoDeviceVolume(tp.TSDFVolumeColorType.RGB8)
    with pytest.raises(ValueError, match="closed"):
        vol.ray_cast(K, np.eye(4))
    assert vol.ray_cast_batch(K, []) == []
    with pytest.raises(ValueError, match="4 x 4"):
        vol.ray_cast(K, np.eye(3))
    with pytest.raises(ValueError, match="width and height"):
        vol.ray_cast(K.intrinsic_matrix, np.eye(4))
    with pytest.raises(ValueError, match="one for all or a list"):
        vol.ray_cast_batch(K, [np.eye(4)] * 2, depth_max=[1.0, 2.0, 3.0])
    f = np.float32
    color = np.array([[[0.25, 0.5, 1.0], [1.0, 0.0, 0.0]]], dtype=f)
    depth = np.array([[1.5, 0.0]], dtype=f)
    rgbd = tp.TSDFRayCastResult(depth, None, None, color, 1, tp.TSDFVolumeColorType.RGB8).as_rgbd_image()
    assert rgbd.depth is depth and rgbd.color.dtype == f and rgbd.color.shape == (1, 2)
    assert rgbd.color[0, 0] == (f(0.2990) * f(0.25) + f(0.5870) * f(0.5)) + f(0.1140) * f(1.0) and rgbd.color[0, 1] == f(0.2990)
    gray = tp.TSDFRayCastResult(depth, None, None, np.repeat(depth[..., None], 3, axis=2), 1, tp.TSDFVolumeColorType.Gray32).as_rgbd_image()
    assert gray.color.tobytes() == depth.tobytes()
    with pytest.raises(ValueError, match="no colour"):
        tp.TSDFRayCastResult(depth, None, None, None, 1, tp.TSDFVolumeColorType.NoColor).as_rgbd_image()
