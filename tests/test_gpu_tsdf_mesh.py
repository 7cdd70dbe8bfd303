"""The triangle mesh of the TSDF volume on the MI355X against the restatement (tests/tsdf_mesh_reference.py, Open3D's
serial loop with its dict, pinned in tests/test_tsdf_mesh_reference.py): everything must be EQUAL -- the counts, the bits
of the vertices, their colours and normals, and the triangle rows.  One cube with each of the 256 sign patterns (every
row of the table) and RGB8 colours; random signs with a third, a tenth or none of the weights zeroed at 3 and 6 voxels
a side (the creator rule, indices reused across columns) in the three colour types; 17 voxels a side (289 columns: two
blocks);
the integrated cases of 64 (a row of columns is exactly one wave), 65 and 16 voxels a side with unobserved regions and
NaN colours; no cube, no surface; either capacity one row short; the same bytes twice and an untouched volume."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tsdf_mesh_reference as M
import tsdf_reference as T
from test_gpu_tsdf import integrate_all, make_volume, same

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def device_volume(vol):
    """A device volume holding the state of the restatement's Volume."""
    d = tp.UniformTSDFVolume(vol.length, vol.R, vol.sdf_trunc, vol.color_type, vol.origin)
    d.inject_volume_tsdf(vol.tsdf_weight())
    if vol.color_type != T.NONE:
        d.inject_volume_color(vol.colors())
    return d


def check(d, ref, what):
    """ref: the restatement's mesh with normals."""
    m = d.extract_triangle_mesh(vertex_normals=True)
    assert (len(m.vertices), len(m.triangles)) == (len(ref.vertices), len(ref.triangles)), what
    assert same(m.triangles, ref.triangles), what
    assert same(m.vertices, ref.vertices) and same(m.vertex_normals, ref.normals), what
    assert (m.vertex_colors is None) == (ref.colors is None) and (ref.colors is None or same(m.vertex_colors, ref.colors)), what
    plain = d.extract_triangle_mesh()
    assert plain.vertex_normals is None and same(plain.vertices, ref.vertices) and same(plain.triangles, ref.triangles), what


def test_every_sign_pattern_of_one_cube():
    vol = M.random_volume(2, 11, T.RGB8, zero_weights=0.0)
    magnitude = np.abs(vol.tsdf) + T.f32(0.125)
    seen = 0
    with device_volume(vol) as d:
        for pattern in range(256):
            for i, (x, y, z) in enumerate(M.SHIFT):
                vol.tsdf[x, y, z] = -magnitude[x, y, z] if (pattern >> i) & 1 else magnitude[x, y, z]
            d.inject_volume_tsdf(vol.tsdf_weight())
            ref = M.extract_triangle_mesh(vol, normals=True)
            assert len(ref.triangles) == (M.TRI_TABLE[pattern].index(-1) if -1 in M.TRI_TABLE[pattern] else 15) // 3
            check(d, ref, pattern)
            seen += len(ref.triangles)
    assert seen == sum(16 - row.count(-1) for row in M.TRI_TABLE) // 3


@pytest.mark.parametrize("R,seed,ctype,zeroed", [(3, 21, T.RGB8, 0.1), (3, 22, T.NONE, 0.1), (6, 2, T.GRAY32, 1.0 / 3.0),
                                                 (6, 24, T.RGB8, 1.0 / 3.0), (6, 29, T.NONE, 0.1), (6, 30, T.GRAY32, 0.0),
                                                 (17, 25, T.NONE, 0.1)])
def test_random_signs_with_zeroed_weights(R, seed, ctype, zeroed):
    """A third of the weights zeroed leaves a few scattered cubes; a tenth leaves runs of neighbouring ones."""
    vol = M.random_volume(R, seed, ctype, zero_weights=zeroed)
    ref = M.extract_triangle_mesh(vol, normals=True)
    assert len(ref.triangles) > (5000 if R == 17 else 4)
    with device_volume(vol) as d:
        check(d, ref, (R, seed))


@pytest.mark.parametrize("name", ["r64", "r65_gray", "sphere", "r16_gray_small", "r5_rgb"])
def test_integrated_cases(name):
    cs = T.cases()[name]
    ref = M.result(name)
    assert len(ref.triangles) > 0
    with make_volume(cs) as d:
        integrate_all(d, cs.frames)
        check(d, ref, name)


def test_the_analytic_sphere():
    vol = M.sphere_volume()
    with device_volume(vol) as d:
        check(d, M.extract_triangle_mesh(vol, normals=True), "sphere")


def test_no_cube_and_no_surface():
    for R in (1, 2, 16):
        with tp.UniformTSDFVolume(1.0, R, 0.1, T.RGB8) as d:
            m = d.extract_triangle_mesh(vertex_normals=True)
            assert m.vertices.shape == (0, 3) and m.triangles.shape == (0, 3) and m.triangles.dtype == np.int32
            assert m.vertex_colors.shape == (0, 3) and m.vertex_normals.shape == (0, 3)
    vol = M.random_volume(1, 3)
    vol.weight[:] = T.f32(1)
    with device_volume(vol) as d:
        assert len(d.extract_triangle_mesh().vertices) == 0


def test_capacities_and_determinism():
    name = "sphere"
    cs, ref = T.cases()[name], M.result(name)
    n, m = len(ref.vertices), len(ref.triangles)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L = tp.lib()
    fn = L.teaser_hip_tsdf_extract_triangle_mesh
    with make_volume(cs) as d:
        integrate_all(d, cs.frames)
        before = d.extract_point_cloud()
        nv, nt = C.c_int64(-1), C.c_int64(-1)
        d._call(fn, 0, None, None, None, 0, None, C.byref(nv), C.byref(nt))
        assert (nv.value, nt.value) == (n, m)
        # the exact capacities: rows behind the counts stay
        V, Cc, N = (np.full((n + 1, 3), -7.5) for _ in range(3))
        Tr = np.full((m + 1, 3), -7, dtype=np.int32)
        d._call(fn, n, V.ctypes.data_as(dp), Cc.ctypes.data_as(dp), N.ctypes.data_as(dp), m, Tr.ctypes.data_as(ip), C.byref(nv), C.byref(nt))
        assert same(V[:n], ref.vertices) and same(Cc[:n], ref.colors) and same(N[:n], ref.normals) and same(Tr[:m], ref.triangles)
        assert (V[n] == -7.5).all() and (Cc[n] == -7.5).all() and (N[n] == -7.5).all() and (Tr[m] == -7).all()
        # the same bytes again
        V2, Tr2 = np.full((n, 3), -7.5), np.full((m, 3), -7, dtype=np.int32)
        d._call(fn, n, V2.ctypes.data_as(dp), None, None, m, Tr2.ctypes.data_as(ip), C.byref(nv), C.byref(nt))
        assert V2.tobytes() == V[:n].tobytes() and Tr2.tobytes() == Tr[:m].tobytes()
        # one row short, the vertices only and then the triangles only: refused, nothing written, the counts reported
        for dv, dt in ((1, 0), (0, 1)):
            V2[:], Tr2[:] = -7.5, -7
            nv.value = nt.value = -1
            with pytest.raises(tp.TeaserHipError, match="vertex_capacity %d, vertex count %d; triangle_capacity %d, triangle count %d" % (n - dv, n, m - dt, m)):
                d._call(fn, n - dv, V2.ctypes.data_as(dp), None, None, m - dt, Tr2.ctypes.data_as(ip), C.byref(nv), C.byref(nt))
            assert (nv.value, nt.value) == (n, m) and (V2 == -7.5).all() and (Tr2 == -7).all()
        check(d, ref, name)                               # the handle stays usable
        after = d.extract_point_cloud()                   # and the volume is what it was
        assert same(after.points, before.points) and same(after.normals, before.normals) and same(after.colors, before.colors)
        assert same(before.points, T.result(name).points)
    with tp.UniformTSDFVolume(1.0, 4, 0.1) as d:
        with pytest.raises(tp.TeaserHipError, match="without colour"):
            d._call(fn, 1, V.ctypes.data_as(dp), V.ctypes.data_as(dp), None, 0, None, C.byref(nv), C.byref(nt))
