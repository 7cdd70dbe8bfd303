"""The entry points of the ray-casting scene are exported and declared with their argument counts, the header states the
contract under its heading, the view record has the size the header asserts and the defaults it names, a NULL handle is
refused before anything is read, creation without a device answers NO_DEVICE, and the Python side checks its arguments
before the device."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")
scene = importlib.import_module("teaser-plusplus_amd.scene")

ENTRY_POINTS = (("teaser_hip_scene_create", 2), ("teaser_hip_scene_destroy", 1), ("teaser_hip_scene_last_error", 1),
                ("teaser_hip_scene_fill_scratch", 3), ("teaser_hip_scene_add_triangles", 6), ("teaser_hip_scene_commit", 1),
                ("teaser_hip_scene_triangle_count", 2), ("teaser_hip_scene_cast_rays", 8), ("teaser_hip_scene_test_occlusions", 6),
                ("teaser_hip_scene_closest_points", 9), ("teaser_hip_scene_view_default", 1), ("teaser_hip_scene_cast_views", 8))


def test_entry_points_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "teaser_hip.h")).read()
    for text in ("/* Ray casting scene:", "t.geometry.RaycastingScene", "bit parity with an Open3D or\n * Embree binary is NOT claimed",
                 "The triangle is DEAD when n == (0, 0, 0)", "det == 0: miss", "The winner of a ray is the minimum of (t, g)",
                 "ClosestPtPointTriangle", "The search structure is NOT part of the contract", "No floating-point atomic is used",
                 "static_assert(sizeof(teaser_scene_view_c) == 184", "Not offered: signed distance and occupancy"):
        assert text in header, text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Ray casting scene" in design and "kernel-resource-usage" in design
    raw = C.CDLL(os.path.join(ROOT, "teaser-plusplus_amd", "libteaser_hip.so"))
    for name, argc in ENTRY_POINTS:
        assert name in tp.EXPORTED_SYMBOLS and "_batch" not in name
        f = getattr(tp.lib(), name)
        assert f is not None and len(f.argtypes) == argc and getattr(raw, name) is not None
        m = re.search(r"TEASER_HIP_API (?:int32_t|const char\*) %s\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == argc, name
    assert sorted(n for n in tp.EXPORTED_SYMBOLS if n.startswith("teaser_hip_scene_")) == sorted(n for n, _ in ENTRY_POINTS)
    L = tp.lib()
    t = (C.c_float * 1)(-3.0)
    ray = (C.c_float * 6)(0, 0, 1, 0, 0, -1)
    assert L.teaser_hip_scene_cast_rays(None, ray, 1, t, None, None, None, None) == 1 and t[0] == -3.0  # BAD_ARG, nothing written
    assert L.teaser_hip_scene_closest_points(None, ray, 1, None, t, None, None, None, None) == 1 and t[0] == -3.0
    assert L.teaser_hip_scene_add_triangles(None, ray, 2, None, 0, None) == 1 and L.teaser_hip_scene_commit(None) == 1
    filled = C.c_int64(7)
    assert L.teaser_hip_scene_fill_scratch(None, 0, C.byref(filled)) != 0 and filled.value == 7
    assert L.teaser_hip_scene_destroy(None) == 0 and L.teaser_hip_scene_last_error(None) == b""


def test_the_view_record_and_its_defaults(tmp_path):
    assert C.sizeof(scene.SceneViewC) == 184
    assert [(n, getattr(scene.SceneViewC, n).offset) for n in ("width", "height", "fx", "extrinsic", "pixel_offset", "reserved")] == \
        [("width", 0), ("height", 4), ("fx", 8), ("extrinsic", 40), ("pixel_offset", 168), ("reserved", 176)]
    v = scene.SceneViewC()
    C.memset(C.byref(v), 0xAB, C.sizeof(v))
    assert tp.lib().teaser_hip_scene_view_default(C.byref(v)) == 0
    assert (v.width, v.height, v.fx, v.fy, v.cx, v.cy, v.reserved, v.pixel_offset) == (0, 0, 0.0, 0.0, 0.0, 0.0, 0, 0.5)
    assert np.array_equal(np.array(v.extrinsic[:]).reshape(4, 4), np.eye(4))
    assert tp.lib().teaser_hip_scene_view_default(None) == 1
    # the header's static assertions hold for a C and for a C++ compiler
    src = tmp_path / "sizes.c"
    src.write_text('#include "teaser_hip.h"\n_Static_assert(sizeof(teaser_scene_view_c) == 184, "size");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
    cxx = tmp_path / "scene.cpp"
    cxx.write_text('#include "teaser/scene.h"\nstatic_assert(sizeof(teaser_scene_view_c) == 184, "size");\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(cxx)])


def test_creation_without_a_device_is_a_loud_error():
    if tp.device_count() > 0:
        return  # on the GPU box the parity tests cover creation
    h = C.c_void_p()
    assert tp.lib().teaser_hip_scene_create(0, C.byref(h)) == 3 and not h   # TEASER_HIP_ERR_NO_DEVICE: never a CPU fallback
    with pytest.raises(tp.TeaserHipError, match="NO_DEVICE"):
        tp.RaycastingScene()


class _NoDeviceScene(tp.RaycastingScene):
    def __init__(self):
        import threading
        self._lib, self._h, self._lock = tp.lib(), None, threading.Lock()


def test_python_side_without_a_device():
    s = _NoDeviceScene()
    with pytest.raises(ValueError, match="closed"):
        s.cast_rays(np.zeros((2, 6)))
    with pytest.raises(ValueError, match="last dimension of 6"):
        s.cast_rays(np.zeros((2, 5)))
    with pytest.raises(ValueError, match="last dimension of 3"):
        s.compute_distance(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="n x 3"):
        s.add_triangles(np.zeros((4, 2)), np.zeros((1, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="indices"):
        s.add_triangles(np.zeros((4, 3)), np.array([[0, 1, -1]]))
    assert s.cast_views(np.eye(3), []) == []
    with pytest.raises(ValueError, match="4 x 4"):
        s.cast_views(tp.PinholeCameraIntrinsic(5, 3, 4.0, 4.0, 2.0, 1.0), [np.eye(3)])
    with pytest.raises(ValueError, match="width and height"):
        s.cast_views(np.eye(3), [np.eye(4)])
    s.close()
