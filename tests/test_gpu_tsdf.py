"""The TSDF volume on the MI355X against the numpy restatement (tests/tsdf_reference.py, pinned by hand in
tests/test_tsdf_reference.py): everything must be EQUAL -- the bits of tsdf, weight and colour through download, the
counts, the points, the normals and the colours of both extractions.  Volumes of 1, 2, 5, 64 (a row of columns is exactly
one wave), 65 and 16 voxels a side; 1, chunk, chunk + 1 and 2 chunk + 1 frames in one call, each equal to the same
frames one call at a time; frames of 7 x 5 and 64 x 48, uint16 and float32 depth with 0, NaN, -1 and +inf samples, padded
rows, cameras behind and inside the volume and one that sees nothing, rotated extrinsics, the three colour types."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tsdf_reference as T

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def make_volume(cs):
    length, R, trunc, ctype, origin = cs.vol
    return tp.UniformTSDFVolume(length, R, trunc, ctype, origin)


def integrate_all(vol, frames, one_by_one=False):
    if not frames:
        return vol.integrate_batch([], T.camera(7, 5), [])
    f0 = frames[0]
    K = tp.PinholeCameraIntrinsic(f0.depth.shape[1], f0.depth.shape[0], *f0.K)
    if one_by_one:
        for f in frames:
            vol.integrate(f.depth, K, f.E, f.color, f.depth_scale, f.depth_trunc)
    else:
        vol.integrate_batch([f.depth for f in frames], K, [f.E for f in frames], [f.color for f in frames],
                            [f.depth_scale for f in frames], [f.depth_trunc for f in frames])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(vol, name):
    r, ctype = T.result(name), T.cases()[name].vol[3]
    tw = vol.extract_volume_tsdf()
    bad = np.flatnonzero((tw.view(np.uint32) != r.tw.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (name, len(bad), bad[:5], tw[bad[:5]], r.tw[bad[:5]])
    if ctype != T.NONE:
        assert same(vol.extract_volume_color(), r.color), name
    pc = vol.extract_point_cloud()
    assert len(pc.points) == len(r.points), (name, len(pc.points), len(r.points))
    assert same(pc.points, r.points) and same(pc.normals, r.normals), name
    assert (pc.colors is None) == (r.colors is None) and (r.colors is None or same(pc.colors, r.colors)), name
    assert vol.extract_point_cloud(normals=False).normals is None
    vp = vol.extract_voxel_point_cloud()
    assert same(vp.points, r.vpoints) and same(vp.colors, r.vcolors) and vp.normals is None, name


@pytest.mark.parametrize("name", list(T.cases()))
def test_one_call_equals_the_restatement(name):
    cs = T.cases()[name]
    with make_volume(cs) as vol:
        integrate_all(vol, cs.frames)
        check(vol, name)


@pytest.mark.parametrize("name", ["r16_rgb_%d" % n for n in (T.CHUNK, T.CHUNK + 1, 2 * T.CHUNK + 1)] + ["r5_gray", "r65_gray"])
def test_a_call_per_frame_equals_one_call(name):
    """Two volumes alive at once: one fed in one call, one frame by frame."""
    cs = T.cases()[name]
    with make_volume(cs) as a, make_volume(cs) as b:
        integrate_all(a, cs.frames)
        integrate_all(b, cs.frames, one_by_one=True)
        assert same(a.extract_volume_tsdf(), b.extract_volume_tsdf())
        assert same(a.extract_volume_color(), b.extract_volume_color())
        check(b, name)


def test_capacity_reset_and_the_round_trip():
    name = "sphere"
    cs, r = T.cases()[name], T.result(name)
    dp = C.POINTER(C.c_double)
    with make_volume(cs) as vol:
        # the empty volume
        pc = vol.extract_point_cloud()
        assert pc.points.shape == (0, 3) and pc.normals.shape == (0, 3) and vol.extract_voxel_point_cloud().points.shape == (0, 3)
        assert not vol.extract_volume_tsdf().any() and not vol.extract_volume_color().any()
        integrate_all(vol, cs.frames)
        n = len(r.points)
        L, cnt = tp.lib(), C.c_int64(-1)
        # capacity exactly the count
        P, N, Cc = np.full((n + 1, 3), -7.5), np.full((n + 1, 3), -7.5), np.full((n + 1, 3), -7.5)
        vol._call(L.teaser_hip_tsdf_extract_point_cloud, n, P.ctypes.data_as(dp), N.ctypes.data_as(dp), Cc.ctypes.data_as(dp), C.byref(cnt))
        assert cnt.value == n and same(P[:n], r.points) and same(N[:n], r.normals) and same(Cc[:n], r.colors)
        assert (P[n] == -7.5).all() and (N[n] == -7.5).all() and (Cc[n] == -7.5).all()
        # one below: refused, the count named, nothing written
        P[:] = -7.5
        cnt.value = -1
        with pytest.raises(tp.TeaserHipError, match="capacity %d is below the count %d" % (n - 1, n)):
            vol._call(L.teaser_hip_tsdf_extract_point_cloud, n - 1, P.ctypes.data_as(dp), None, None, C.byref(cnt))
        assert cnt.value == n and (P == -7.5).all()
        check(vol, name)                               # the handle stays usable
        # reset, then the state back through inject
        vol.reset()
        assert not vol.extract_volume_tsdf().any() and not vol.extract_volume_color().any()
        assert len(vol.extract_point_cloud().points) == 0
        vol.inject_volume_tsdf(r.tw)
        vol.inject_volume_color(r.color)
        check(vol, name)
        # refusals of the frame checks leave the volume alone
        f = cs.frames[0]
        K = tp.PinholeCameraIntrinsic(64, 48, *f.K)
        with pytest.raises(tp.TeaserHipError, match=r"depth_scale must be finite and > 0 \(frame 1\)"):
            vol.integrate_batch([f.depth, f.depth], K, [f.E, f.E], [f.color, f.color], [1000.0, 0.0])
        with pytest.raises(tp.TeaserHipError, match=r"fx and fy .*\(frame 0\)"):
            vol.integrate(f.depth, np.array([[0.0, 0, 1], [0, 1.0, 1], [0, 0, 1]]), f.E, f.color)
        check(vol, name)
    with pytest.raises(ValueError, match="closed"):
        vol.reset()


def test_a_gray_volume_keeps_nan_colours_through_the_round_trip():
    name = "r16_gray_small"
    cs, r = T.cases()[name], T.result(name)
    with make_volume(cs) as vol:
        vol.inject_volume_tsdf(r.tw)
        vol.inject_volume_color(r.color)
        check(vol, name)
