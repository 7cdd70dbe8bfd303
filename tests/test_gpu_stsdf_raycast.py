"""The ray cast of the scalable TSDF volume on the MI355X.  Everything must be EQUAL, compared as bytes -- the depth,
vertex, normal and colour maps and the hit counts:
  1. against the restatement (tests/stsdf_raycast_reference.py, pinned in tests/test_stsdf_raycast_reference.py): random
     sets of five blocks from [-2, 2)^3 with a third of the weights zeroed, the three colour types and the thresholds 0, 1
     and 3; volumes the device integrated from the scenes of tests/stsdf_reference.py; views of 1 x 1 to 33 x 17 pixels
     mixed in one call, alone and reversed; rays along the axes; cameras that see nothing; the depth alone; 320 views in
     one call; a volume that grows between two casts; an empty volume;
  2. against the DENSE ray cast, independently of the new restatement: eight injected blocks that hold the voxels of a
     UniformTSDFVolume, cameras inside the box;
  3. the same bytes twice, after fill_scratch(0x00) and after fill_scratch(0xFF), and untouched blocks."""
import importlib

import numpy as np
import pytest

import stsdf_raycast_reference as SR
import stsdf_reference as S
import tsdf_raycast_reference as RC
import tsdf_reference as T
from test_gpu_stsdf import integrate, make_volume, same
from test_gpu_tsdf_raycast import cast, equal
from test_stsdf_raycast_reference import dense_and_blocks

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")

SIZES = ((1, 1), (8, 8), (16, 16), (17, 9), (33, 17))


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def device_blocks(vol, **kw):
    """The restatement's volume on the device, through inject_blocks."""
    d = tp.ScalableTSDFVolume(vol.vl, vol.sdf_trunc, vol.color_type, 16, vol.stride, **kw)
    if vol.blocks:
        d.inject_blocks(vol.keys(), vol.block_tsdf_weight(), vol.block_colors() if vol.color_type != T.NONE else None)
    return d


def check(d, vol, views, what, mixed=True):
    """The views in one call; mixed: every view of more than one pixel must both hit and miss."""
    lat = SR.Lattice(vol)
    refs = [SR.cast(vol, w, lat) for w in views]
    for w, r in zip(views, refs):
        if mixed and w.width * w.height > 1:
            assert 0 < r.hits < w.width * w.height, (what, w.width, w.height, r.hits)
    for k, (g, r) in enumerate(zip(cast(d, views), refs)):
        equal(g, r, (what, k))
    return refs


@pytest.mark.parametrize("seed,ctype,thr,weight", SR.RANDOM_SETS)
def test_random_block_sets(seed, ctype, thr, weight):
    vol = SR.random_blocks(seed, ctype, weight)
    with device_blocks(vol) as d:
        check(d, vol, SR.views_of(vol, thr, SIZES), seed)


@pytest.mark.parametrize("name,thr", [("rgb_64", 3.0), ("gray_64_stride1", 1.0), ("none_64", 2.0), ("identity", 2.0)])
def test_volumes_the_device_integrated(name, thr):
    cs, vol = S.cases()[name], S.result(name).vol
    f0 = cs.frames[0]
    views = [RC.view(33, 17, f0.E, K=S.camera(33, 17), weight_threshold=thr), RC.view(17, 9, cs.frames[1].E, K=S.camera(17, 9), depth_max=0.85, weight_threshold=1.0),  # the front of the ball alone
             RC.view(16, 16, T.extrinsic(0.1, -0.3, 0.0, (0.4, 0.0, 1.0)), K=T.camera(16, 16), weight_threshold=thr)]
    with make_volume(cs) as d:
        integrate(d, cs.frames)
        check(d, vol, views, name)


@pytest.mark.parametrize("color_type", (T.NONE, T.RGB8, T.GRAY32))
def test_eight_blocks_are_the_dense_volume_on_the_device(color_type):
    """Independent of the new restatement: UniformTSDFVolume.ray_cast_batch of the dense volume against
    ScalableTSDFVolume.ray_cast_batch of the eight blocks that hold its voxels (see the test of the same name in
    tests/test_stsdf_raycast_reference.py for why the two must agree)."""
    from test_gpu_tsdf_mesh import device_volume
    dense, vol = dense_and_blocks(5 + color_type, color_type)
    views = [RC.view(33, 17, T.extrinsic(0.1, -0.15, 0.2, (-1.0, -0.9, -0.4)), depth_min=0.05), RC.view(1, 1, T.extrinsic(0.0, 0.0, 0.0, (-1.0, -1.1, -0.3)), depth_min=0.05, weight_threshold=1.0),
             RC.view(33, 17, T.extrinsic(-0.3, 0.4, 0.0, (-0.9, -1.0, -0.7)), depth_min=0.05, weight_threshold=1.0)]
    with device_volume(dense) as a, device_blocks(vol) as b:
        ra, rb = cast(a, views), cast(b, views)
    assert sum(r.hits for r in ra) > 150
    for k, (x, y) in enumerate(zip(ra, rb)):
        assert x.hits == y.hits, k
        for m in ("depth", "vertex_map", "normal_map") + (("color",) if color_type != T.NONE else ()):
            assert same(getattr(x, m), getattr(y, m)), (k, m)


def test_mixed_views_in_one_call_alone_and_reversed():
    vol = SR.random_blocks(21, T.RGB8)
    views = SR.views_of(vol, 1.0, ((33, 17), (8, 8), (0, 0), (17, 9), (1, 1)))
    with device_blocks(vol) as d:
        refs = check(d, vol, views, "mixed", mixed=False)
        assert refs[2].depth.shape == (0, 0) and all(0 < refs[k].hits < views[k].width * views[k].height for k in (0, 1, 3))
        back = cast(d, views[::-1])[::-1]
        for k, w in enumerate(views):
            equal(back[k], refs[k], ("reversed", k))
            equal(cast(d, [w])[0], refs[k], ("alone", k))
        # the module-level functions serve either class
        equal(tp.ray_cast(d, tp.PinholeCameraIntrinsic(33, 17, *views[0].K), views[0].E, depth_min=views[0].depth_min,
                          depth_max=views[0].depth_max, weight_threshold=1.0), refs[0], "tp.ray_cast")
        both = tp.ray_cast_batch(d, [tp.PinholeCameraIntrinsic(w.width, w.height, *w.K) for w in views[:2]], [w.E for w in views[:2]],
                                 depth_min=views[0].depth_min, depth_max=[w.depth_max for w in views[:2]], weight_threshold=1.0)
        equal(both[1], refs[1], "tp.ray_cast_batch")
        rgbd = both[0].as_rgbd_image()
        assert same(rgbd.color, RC.intensity(both[0].color)) and rgbd.depth is both[0].depth


def test_rays_along_the_axes():
    """Exact rotations and an integer principal point: the pixel there has two d_k == 0, along z, y and x in turn, in both
    directions."""
    vol = SR.random_blocks(23, T.GRAY32)
    keys = vol.keys().astype(np.float64)
    centre = 0.5 * (keys.min(axis=0) + keys.max(axis=0) + 1.0) * vol.ul
    views = []
    for rx, ry in ((0.0, 0.0), (np.pi / 2, 0.0), (0.0, np.pi / 2), (np.pi, 0.0), (-np.pi / 2, 0.0), (0.0, -np.pi / 2)):
        E = T.extrinsic(rx, ry)
        E[:3, :3] = np.rint(E[:3, :3])  # the rotation exactly: zeros in the direction
        E[:3, 3] = -E[:3, :3] @ centre + np.array([0.0, 0.0, 1.5])
        views.append(RC.view(17, 9, E, K=(15.0, 14.0, 8.0, 4.0), depth_max=5.0, weight_threshold=1.0))
    _, Rt = RC.camera(type("O", (), {"origin": np.zeros(3)}), views[0].E)
    d = RC.rays(views[0].K, Rt, 17, 9)
    assert d[4, 8, 0] == 0 and d[4, 8, 1] == 0 and d[4, 8, 2] == 1
    with device_blocks(vol) as d:
        check(d, vol, views, "axes")


def test_cameras_that_see_nothing():
    vol = SR.random_blocks(24, T.RGB8)
    seen = SR.views_of(vol, 1.0, ((33, 17),))[0]
    flip = np.diag([-1.0, 1.0, -1.0, 1.0])  # the same centre, looking the other way
    away = RC.view(33, 17, flip @ seen.E, depth_min=seen.depth_min, depth_max=seen.depth_max, weight_threshold=1.0)
    short = RC.view(33, 17, seen.E, depth_min=0.0, depth_max=0.05, weight_threshold=1.0)
    beyond = RC.view(17, 9, seen.E, depth_min=50.0, depth_max=60.0, weight_threshold=1.0)
    high = RC.view(17, 9, seen.E, depth_min=seen.depth_min, depth_max=seen.depth_max, weight_threshold=2.5)  # above every weight
    with device_blocks(vol) as d:
        check(d, vol, [seen], "seen")
        for w in (away, short, beyond, high):
            r = check(d, vol, [w], "nothing", mixed=False)[0]
            assert r.hits == 0 and not r.depth.any() and not r.vertex.any() and not r.color.any()


def test_depth_alone_twice_the_scratch_and_untouched_blocks():
    vol = SR.random_blocks(25, T.RGB8)
    views = SR.views_of(vol, 1.0, ((33, 17), (17, 9)))
    with device_blocks(vol) as d:
        keys, tw, col = d.extract_blocks()
        first = cast(d, views)
        only = cast(d, views, vertex_map=False, normal_map=False, color=False)
        again = cast(d, views)
        assert d.fill_scratch(0x00) > 0
        zeros = cast(d, views)
        assert d.fill_scratch(0xFF) > 0
        ones = cast(d, views)
        lat = SR.Lattice(vol)
        for k, w in enumerate(views):
            ref = SR.cast(vol, w, lat)
            assert 0 < ref.hits < w.width * w.height
            equal(first[k], ref, ("first", k))
            assert only[k].vertex_map is None and only[k].normal_map is None and only[k].color is None
            assert same(only[k].depth, ref.depth) and only[k].hits == ref.hits
            for other in (again[k], zeros[k], ones[k]):
                equal(other, ref, ("again", k))
        k2, tw2, col2 = d.extract_blocks()
        assert same(k2, keys) and same(tw2, tw) and same(col2, col)
        with pytest.raises(tp.TeaserHipError, match=r"depth_max must not be below depth_min \(view 0\)"):
            tp.ray_cast(d, tp.PinholeCameraIntrinsic(5, 3, 4.0, 4.0, 2.0, 1.0), np.eye(4), depth_min=2.0, depth_max=1.0)


def test_an_empty_volume():
    with tp.ScalableTSDFVolume(0.02, 0.06, T.RGB8) as d:
        r = tp.ray_cast(d, tp.PinholeCameraIntrinsic(33, 17, 30.0, 30.0, 16.0, 8.0), np.eye(4))
        assert r.hits == 0 and r.depth.shape == (17, 33) and r.depth.dtype == np.float32
        assert not r.depth.any() and not r.vertex_map.any() and not r.normal_map.any() and not r.color.any()
        assert d.ray_cast_batch(tp.PinholeCameraIntrinsic(5, 3, 4.0, 4.0, 2.0, 1.0), []) == []
    with tp.ScalableTSDFVolume(0.02, 0.06) as d:
        assert tp.ray_cast(d, tp.PinholeCameraIntrinsic(5, 3, 4.0, 4.0, 2.0, 1.0), np.eye(4)).color is None
    vol = SR.random_blocks(26, T.NONE)
    with device_blocks(vol) as d:  # closed again: as empty as a new one
        d.reset()
        w = SR.views_of(vol, 1.0, ((17, 9),))[0]
        r = cast(d, [w])[0]
        assert r.hits == 0 and not r.depth.any() and not r.normal_map.any()


def test_a_volume_that_grows_between_two_casts():
    """initial_blocks = 2 and slab_blocks = 2: the first frames open blocks in the first slabs, the camera moved sideways
    opens blocks in new ones; the directory's device copy must follow."""
    cs = S.cases()["rgb_64"]
    sideways = [k for k, f in enumerate(cs.frames) if f.E[0, 3] == -0.5]
    assert sideways and sideways[0] >= 2
    cut = sideways[0]
    before, after = S.run(cs, cs.frames[:cut]), S.result("rgb_64").vol
    assert len(after.blocks) > len(before.blocks) > 2
    views = [RC.view(33, 17, cs.frames[0].E, K=S.camera(33, 17), weight_threshold=1.0),
             RC.view(17, 9, cs.frames[cut].E, K=S.camera(17, 9), weight_threshold=1.0)]
    with make_volume(cs, initial_blocks=2, slab_blocks=2) as d:
        integrate(d, cs.frames[:cut])
        first = check(d, before, views, "before the growth", mixed=False)
        integrate(d, cs.frames[cut:])
        second = check(d, after, views, "after the growth", mixed=False)
    assert second[1].hits != first[1].hits or second[1].depth.tobytes() != first[1].depth.tobytes()


def test_320_views_in_one_call():
    """More views than any grid extent or 8-bit index could hide: 320 views of 4 x 3 pixels from 320 directions in one
    call (the block map then has 320 entries of one block each), every one equal to the restatement."""
    vol = SR.random_blocks(27, T.RGB8)
    box = SR.views_of(vol, 1.0, ((4, 3),))[0]
    keys = vol.keys().astype(np.float64)
    lo, hi = keys.min(axis=0), keys.max(axis=0) + 1.0
    world = type("B", (), {"origin": lo * vol.ul, "length": float((hi - lo).max()) * vol.ul})
    views = [RC.view(4, 3, RC.look_at_volume(world, 0.4 * np.sin(0.7 * k), 0.4 * np.cos(0.3 * k), 1.1 * world.length), depth_min=0.05,
                     depth_max=box.depth_max, weight_threshold=float(k % 3)) for k in range(320)]
    with device_blocks(vol) as d:
        refs = check(d, vol, views, "wide", mixed=False)
    hits, pixels = sum(r.hits for r in refs), sum(w.width * w.height for w in views)
    assert 0 < hits < pixels and sum(r.hits > 0 for r in refs) > 100
