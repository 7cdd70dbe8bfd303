"""The ray cast of the TSDF volume on the MI355X against the restatement (tests/tsdf_raycast_reference.py, pinned in
tests/test_tsdf_raycast_reference.py): everything must be EQUAL -- the bits of the depth, vertex, normal and colour maps
and the hit counts.  Random volumes of 2, 3, 6 and 17 voxels a side with a third of the weights zeroed, in the three
colour types, with the thresholds 0, 1 and 3; the integrated cases of 64, 65 and 16 voxels a side; views of 1 x 1, 8 x 8,
16 x 16 (one block), 17 x 9 and 33 x 17 pixels (partial tiles, several blocks); views of different sizes and an empty one
in one call against the same views alone and in reversed order; rays along the axes of the volume; cameras outside,
looking away and behind the surface; the depth alone; the same bytes twice and an untouched volume; 320 small views in
one call.  Every equality case but the all-miss ones, the 1 x 1 view and the 320 small views (which are judged
together) also requires of the restatement that some pixels hit and some miss."""
import importlib

import numpy as np
import pytest

import tsdf_raycast_reference as RC
import tsdf_reference as T
from test_gpu_tsdf import integrate_all, make_volume, same
from test_gpu_tsdf_mesh import device_volume

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")

SIZES = ((1, 1), (8, 8), (16, 16), (17, 9), (33, 17))


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def cast(d, views, **kw):
    """The views (tsdf_raycast_reference.view) in one call."""
    return d.ray_cast_batch([tp.PinholeCameraIntrinsic(w.width, w.height, *w.K) for w in views], [w.E for w in views],
                            depth_min=[w.depth_min for w in views], depth_max=[w.depth_max for w in views],
                            weight_threshold=[w.weight_threshold for w in views], **kw)


def equal(got, ref, what):
    assert got.hits == ref.hits, (what, got.hits, ref.hits)
    for name, a, b in (("depth", got.depth, ref.depth), ("vertex", got.vertex_map, ref.vertex), ("normal", got.normal_map, ref.normal),
                       ("color", got.color, ref.color)):
        assert (a is None) == (b is None), (what, name)
        if a is not None and not same(a, b):
            bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))


def check(d, vol, views, what, mixed=True):
    """The views in one call; mixed: every view but the all-miss ones and 1 x 1 must both hit and miss."""
    refs = [RC.cast(vol, w) for w in views]
    for w, r in zip(views, refs):
        if mixed and w.width * w.height > 1:
            assert 0 < r.hits < w.width * w.height, (what, w.width, w.height, r.hits)
    for k, (g, r) in enumerate(zip(cast(d, views), refs)):
        equal(g, r, (what, k))
    return refs


@pytest.mark.parametrize("R,seed,ctype,thr,weight", [(2, 4, T.RGB8, 1.0, 2.0), (2, 5, T.NONE, 0.0, 2.0), (3, 21, T.GRAY32, 0.0, 2.0),
                                                      (3, 22, T.NONE, 3.0, 4.0), (6, 2, T.NONE, 1.0, 2.0), (6, 24, T.RGB8, 3.0, 4.0),
                                                      (6, 30, T.GRAY32, 1.0, 2.0), (17, 25, T.RGB8, 0.0, 2.0), (17, 26, T.GRAY32, 3.0, 3.0),
                                                      (17, 27, T.NONE, 1.0, 2.0)])
def test_random_volumes_with_zeroed_weights(R, seed, ctype, thr, weight):
    vol = RC.random_volume(R, seed, ctype, weight)
    with device_volume(vol) as d:
        check(d, vol, RC.views_around(vol, thr, SIZES), (R, seed))


@pytest.mark.parametrize("name,thr", [("r64", 1.0), ("r65_gray", 2.0), ("sphere", 3.0), ("r16_rgb_9", 3.0), ("r16_gray_small", 1.0)])
def test_integrated_cases(name, thr):
    cs = T.cases()[name]
    vol = T.result(name).vol
    views = [RC.view(33, 17, np.eye(4), weight_threshold=thr), RC.view(17, 9, T.extrinsic(0.05, -0.1, 0.3, (0.02, -0.01, 0.1)), weight_threshold=thr),
             RC.view(16, 16, RC.look_at_volume(vol, 0.3, -0.2, 1.0), weight_threshold=thr)]
    with make_volume(cs) as d:
        integrate_all(d, cs.frames)
        check(d, vol, views, name)


def test_mixed_views_in_one_call_alone_and_reversed():
    vol = RC.random_volume(17, 31, T.RGB8)
    views = RC.views_around(vol, 1.0, ((33, 17), (8, 8), (0, 0), (17, 9)))
    with device_volume(vol) as d:
        refs = check(d, vol, views, "mixed", mixed=False)
        assert refs[2].depth.shape == (0, 0) and all(0 < refs[k].hits < views[k].width * views[k].height for k in (0, 1, 3))
        back = cast(d, views[::-1])[::-1]
        for k, w in enumerate(views):
            equal(back[k], refs[k], ("reversed", k))
            equal(cast(d, [w])[0], refs[k], ("alone", k))


def test_rays_along_the_axes_of_the_volume():
    """Identity rotation with the integer principal point (d_x = d_y = 0 exactly in that pixel), and the camera turned by
    90 degrees about x and about y: rays along z (the plane axis), along y (the contiguous axis) and along x."""
    vol = RC.random_volume(17, 33, T.GRAY32)
    centre = vol.origin + 0.5 * vol.length
    views = []
    for rx, ry in ((0.0, 0.0), (np.pi / 2, 0.0), (0.0, np.pi / 2)):
        E = T.extrinsic(rx, ry)
        E[:3, :3] = np.rint(E[:3, :3])  # the rotation exactly: zeros in the direction
        E[:3, 3] = -E[:3, :3] @ centre + np.array([0.0, 0.0, 1.3 * vol.length])
        views.append(RC.view(17, 9, E, K=(15.0, 14.0, 8.0, 4.0), depth_max=5.0, weight_threshold=1.0))
    o, Rt = RC.camera(vol, views[0].E)
    d = RC.rays(views[0].K, Rt, 17, 9)
    assert d[4, 8, 0] == 0 and d[4, 8, 1] == 0 and d[4, 8, 2] == 1
    with device_volume(vol) as d:
        check(d, vol, views, "axes")


def test_cameras_that_see_nothing_and_depth_limits():
    cs = T.cases()["sphere"]
    vol = T.result("sphere").vol
    seen = RC.view(33, 17, np.eye(4))
    away = RC.view(33, 17, T.extrinsic(0.0, np.pi, 0.0))                      # looks away from the volume
    outside = RC.view(17, 9, T.extrinsic(t=(0.0, 0.0, 1.5)), depth_max=6.0)   # the camera 1.5 behind: outside the volume
    beyond = RC.view(33, 17, np.eye(4), depth_min=1.45)                       # depth_min beyond every surface
    short = RC.view(33, 17, np.eye(4), depth_max=0.6)                         # depth_max in front of the ball
    with make_volume(cs) as d:
        integrate_all(d, cs.frames)
        refs = check(d, vol, [seen, outside], "seen")
        assert refs[1].depth.max() > 2.0
        for w in (away, beyond, short):
            r = check(d, vol, [w], "nothing", mixed=False)[0]
            assert r.hits == 0 and not r.depth.any() and not r.vertex.any() and not r.color.any()
        # a camera inside the ball: behind the surface, nothing until a positive voxel has been passed
        inside = RC.view(17, 9, T.extrinsic(t=(0.0, 0.0, -1.0)), depth_min=0.0)
        check(d, vol, [inside], "inside", mixed=False)


def test_depth_alone_twice_and_an_untouched_volume():
    vol = RC.random_volume(17, 35, T.RGB8)
    views = RC.views_around(vol, 1.0, ((33, 17), (17, 9)))
    with device_volume(vol) as d:
        tw, col = d.extract_volume_tsdf(), d.extract_volume_color()
        first = cast(d, views)
        only = cast(d, views, vertex_map=False, normal_map=False, color=False)
        again = cast(d, views)
        for k, w in enumerate(views):
            ref = RC.cast(vol, w)
            assert 0 < ref.hits < w.width * w.height
            equal(first[k], ref, ("first", k))
            assert only[k].vertex_map is None and only[k].normal_map is None and only[k].color is None
            assert same(only[k].depth, ref.depth) and only[k].hits == ref.hits
            for a, b in ((first[k].depth, again[k].depth), (first[k].vertex_map, again[k].vertex_map), (first[k].normal_map, again[k].normal_map),
                         (first[k].color, again[k].color)):
                assert a.tobytes() == b.tobytes()
        assert same(d.extract_volume_tsdf(), tw) and same(d.extract_volume_color(), col)
        rgbd = first[0].as_rgbd_image()
        assert same(rgbd.color, RC.intensity(first[0].color)) and rgbd.depth is first[0].depth
    with tp.UniformTSDFVolume(1.0, 4, 0.1) as d:
        r = d.ray_cast(tp.PinholeCameraIntrinsic(5, 3, 4.0, 4.0, 2.0, 1.0), np.eye(4))
        assert r.color is None and r.hits == 0 and r.depth.shape == (3, 5) and r.depth.dtype == np.float32
        with pytest.raises(tp.TeaserHipError, match=r"depth_max must not be below depth_min \(view 0\)"):
            d.ray_cast(tp.PinholeCameraIntrinsic(5, 3, 4.0, 4.0, 2.0, 1.0), np.eye(4), depth_min=2.0, depth_max=1.0)


def test_320_views_in_one_call():
    """More views than any grid extent or 8-bit index could hide: 320 views of 1 x 1 to 5 x 3 pixels from 320 directions
    in one call (the block map then has 320 entries of one block each), every one equal to the restatement."""
    vol = RC.random_volume(6, 37, T.RGB8)
    views = [RC.view(1 + k % 5, 1 + k % 3, RC.look_at_volume(vol, 0.4 * np.sin(0.7 * k), 0.4 * np.cos(0.3 * k), 1.3 * vol.length),
                     depth_max=3.0 * vol.length, weight_threshold=float(k % 3)) for k in range(320)]
    with device_volume(vol) as d:
        refs = check(d, vol, views, "wide", mixed=False)
    hits, pixels = sum(r.hits for r in refs), sum(w.width * w.height for w in views)
    assert 0 < hits < pixels and sum(r.hits > 0 for r in refs) > 100 and sum(r.hits == 0 for r in refs) > 10
