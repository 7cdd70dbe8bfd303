"""The triangle-mesh entry points of the TSDF volume are exported and declared with their argument counts, the header
states the contract (tables, their SHA-256, the scratch per voxel, the extension), a NULL handle is refused before
anything is read, the tables come without a GPU, and the Python and PLY sides check their arguments before the device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import tsdf_mesh_reference as M
from test_tsdf_abi import _NoDeviceVolume
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")

ENTRY_POINTS = (("teaser_hip_tsdf_extract_triangle_mesh", 9), ("teaser_hip_tsdf_mesh_tables", 2))


def test_entry_points_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "teaser_hip.h")).read()
    assert "teaser_hip_tsdf_extract_triangle_mesh: Open3D's UniformTSDFVolume::ExtractTriangleMesh" in header
    assert M.TRI_TABLE_SHA256 in header and "5 bytes per voxel" in header and "an EXTENSION" in header
    assert M.TRI_TABLE_SHA256 in open(os.path.join(ROOT, "DESIGN.md")).read()
    raw = C.CDLL(os.path.join(ROOT, "teaser-plusplus_amd", "libteaser_hip.so"))
    for name, argc in ENTRY_POINTS:
        assert name in tp.EXPORTED_SYMBOLS
        f = getattr(tp.lib(), name)
        assert f is not None and len(f.argtypes) == argc and getattr(raw, name) is not None
        m = re.search(r"TEASER_HIP_API int32_t %s\(([^;]*)\);" % name, header)
        assert m and len(m.group(1).split(",")) == argc, name
    L = tp.lib()
    nv, nt = C.c_int64(-3), C.c_int64(-3)
    assert L.teaser_hip_tsdf_extract_triangle_mesh(None, 0, None, None, None, 0, None, C.byref(nv), C.byref(nt)) == 1  # BAD_ARG
    assert (nv.value, nt.value) == (-3, -3)


def test_the_tables_need_no_device():
    edge, tri = (C.c_int32 * 256)(), (C.c_int8 * 4096)()
    assert tp.lib().teaser_hip_tsdf_mesh_tables(edge, tri) == 0
    assert (edge[0], edge[1], edge[2], edge[3], edge[255]) == (0, 0x109, 0x203, 0x30a, 0)
    assert list(tri[16:20]) == [0, 8, 3, -1] and list(tri[:16]) == [-1] * 16 and list(tri[4080:]) == [-1] * 16
    assert tp.lib().teaser_hip_tsdf_mesh_tables(None, None) == 1


def test_python_side_without_a_device(tmp_path):
    assert tp.TSDFTriangleMesh is not None and tp.write_triangle_mesh is not None
    with pytest.raises(ValueError, match="closed"):
        _NoDeviceVolume(tp.TSDFVolumeColorType.RGB8).extract_triangle_mesh()
    mesh = tp.TSDFTriangleMesh(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.1, 1e-300]]), np.array([[0, 2, 1]], dtype=np.int32),
                               np.array([[0.0, 0.5, 1.0], [2.0, -1.0, np.nan], [0.2, 0.4, 0.6]]))
    assert mesh.vertex_normals is None
    for binary in (True, False):
        path = str(tmp_path / ("m%d.ply" % binary))
        tp.write_triangle_mesh(path, mesh, binary=binary)
        raw = open(path, "rb").read()
        head, body = raw.split(b"end_header\n")
        assert head.startswith(b"ply\nformat " + (b"binary_little_endian" if binary else b"ascii") + b" 1.0\nelement vertex 3\nproperty double x\n")
        assert b"property uchar blue\nelement face 1\nproperty list uchar int vertex_indices\n" in head
        if binary:
            assert len(body) == 3 * 27 + 13
            assert np.frombuffer(body[:24], dtype=np.float64).tolist() == [0.0, 0.0, 0.0] and list(body[24:27]) == [0, 128, 255]
            assert list(body[27 + 24:27 + 27]) == [255, 0, 0] and body[81] == 3 and np.frombuffer(body[82:], dtype=np.int32).tolist() == [0, 2, 1]
        else:
            rows = body.decode().split("\n")
            assert rows[0] == "0 0 0 0 128 255" and float(rows[2].split()[2]) == 1e-300 and rows[3] == "3 0 2 1"
    with pytest.raises(ValueError, match="one row per vertex"):
        tp.write_triangle_mesh(str(tmp_path / "bad.ply"), tp.TSDFTriangleMesh(mesh.vertices, mesh.triangles, np.zeros((2, 3))))
