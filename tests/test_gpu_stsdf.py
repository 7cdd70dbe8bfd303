"""The scalable TSDF volume on the MI355X.  Everything must be EQUAL, compared as bytes:
  1. against the numpy restatement (tests/stsdf_reference.py, pinned by hand in tests/test_stsdf_reference.py): the block
     keys, the bits of tsdf, weight and colour of every block, both extractions and the touched / opened / out_of_range
     counts -- frames of 7 x 5 and 64 x 48, strides 1, 4 and one larger than the image, uint16 and float32 depth with 0,
     NaN, -1 and +inf samples, padded rows, rotated extrinsics, a camera that sees nothing, the three colour types;
  2. against the DENSE volume, independently of the new restatement's voxels: every open block equals a
     UniformTSDFVolume(ul, 16, sdf_trunc, origin = b ul) fed the frames the touch rule assigns to the block;
  3. any split of the frames into calls; 4. growth, the limits and the round trip; 5. the scratch."""
import ctypes as C
import importlib

import numpy as np
import pytest

import stsdf_reference as S
import tsdf_reference as T

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def make_volume(cs, **kw):
    return tp.ScalableTSDFVolume(cs.vl, cs.trunc, cs.ctype, 16, cs.stride, **kw)


def integrate(vol, frames, one_by_one=False):
    """Returns the sums of (touched, opened, out_of_range) over the calls."""
    total = np.zeros(3, dtype=np.int64)
    if not frames:
        vol.integrate_batch([], T.camera(7, 5), [])
        return total
    f0 = frames[0]
    K = tp.PinholeCameraIntrinsic(f0.depth.shape[1], f0.depth.shape[0], *f0.K)
    if one_by_one:
        for f in frames:
            vol.integrate(f.depth, K, f.E, f.color, f.depth_scale, f.depth_trunc)
            total += vol.last_counts
    else:
        vol.integrate_batch([f.depth for f in frames], K, [f.E for f in frames], [f.color for f in frames],
                            [f.depth_scale for f in frames], [f.depth_trunc for f in frames])
        total += vol.last_counts
    return total


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(vol, name):
    r = S.result(name)
    keys, tw, col = vol.extract_blocks()
    assert vol.block_count == len(r.keys) and same(keys, r.keys), (name, keys.tolist(), r.keys.tolist())
    bad = np.argwhere(tw.view(np.uint32) != r.tw.view(np.uint32))
    assert len(bad) == 0, (name, len(bad), bad[:5])
    assert (col is None) == (r.color is None) and (col is None or same(col, r.color)), name
    pc = vol.extract_point_cloud()
    assert len(pc.points) == len(r.points), (name, len(pc.points), len(r.points))
    assert same(pc.points, r.points), name
    assert same(pc.normals, r.normals), (name, np.flatnonzero((pc.normals != r.normals).any(axis=1))[:5])
    assert (pc.colors is None) == (r.colors is None) and (r.colors is None or same(pc.colors, r.colors)), name
    assert vol.extract_point_cloud(normals=False).normals is None
    vp = vol.extract_voxel_point_cloud()
    assert same(vp.points, r.vpoints) and same(vp.colors, r.vcolors) and vp.normals is None, name


@pytest.mark.parametrize("name", list(S.cases()))
def test_one_call_equals_the_restatement(name):
    cs, r = S.cases()[name], S.result(name)
    with make_volume(cs) as vol:
        counts = integrate(vol, cs.frames)
        assert counts.tolist() == [r.touched, r.opened, r.out_of_range], name
        check(vol, name)


def test_every_block_is_the_dense_volume_of_its_frames():
    name = "identity"
    cs = S.cases()[name]
    # which frame reaches which block: the touch rule alone, on the points of "Depth frames"
    per_frame = [S.ScalableVolume(cs.vl, cs.trunc, cs.ctype, cs.stride).touch(f)[0] for f in cs.frames]
    blocks = sorted(set().union(*per_frame))
    assert 1 < len(blocks) <= 30 and any(b not in per_frame[0] for b in blocks)
    ul = cs.vl * 16.0
    with make_volume(cs) as vol:
        integrate(vol, cs.frames)
        keys, tw, col = vol.extract_blocks()
        assert [tuple(k) for k in keys.tolist()] == blocks
        for n, b in enumerate(blocks):
            with tp.UniformTSDFVolume(ul, 16, cs.trunc, cs.ctype, [k * ul for k in b]) as dense:
                integrate_dense(dense, [f for f, t in zip(cs.frames, per_frame) if b in t])
                assert same(dense.extract_volume_tsdf(), tw[n]), b
                assert same(dense.extract_volume_color(), col[n]), b


def integrate_dense(vol, frames):
    f0 = frames[0]
    K = tp.PinholeCameraIntrinsic(f0.depth.shape[1], f0.depth.shape[0], *f0.K)
    vol.integrate_batch([f.depth for f in frames], K, [f.E for f in frames], [f.color for f in frames],
                        [f.depth_scale for f in frames], [f.depth_trunc for f in frames])


@pytest.mark.parametrize("n", [1, S.CHUNK, S.CHUNK + 1, 2 * S.CHUNK + 1])
def test_a_call_per_frame_equals_one_call(n):
    """Two volumes alive at once: one fed in one call, one frame by frame."""
    name = "split_%d" % n
    cs = S.cases()[name]
    with make_volume(cs) as a, make_volume(cs) as b:
        ca, cb = integrate(a, cs.frames), integrate(b, cs.frames, one_by_one=True)
        assert ca.tolist() == cb.tolist()
        ka, ta, cola = a.extract_blocks()
        kb, tb, colb = b.extract_blocks()
        assert same(ka, kb) and same(ta, tb) and same(cola, colb)
        check(b, name)


def test_growth_by_single_blocks_gives_the_same_bits():
    name = "rgb_64"
    cs = S.cases()[name]
    with make_volume(cs, initial_blocks=1, slab_blocks=1) as vol:
        integrate(vol, cs.frames[:2])
        integrate(vol, cs.frames[2:])
        check(vol, name)
    with make_volume(cs, initial_blocks=3, slab_blocks=5) as vol:
        integrate(vol, cs.frames, one_by_one=True)
        check(vol, name)


def test_max_blocks_refuses_before_anything_changes():
    name = "none_64"
    cs, r = S.cases()[name], S.result(name)
    need = len(r.keys)
    first = len(S.run(cs, cs.frames[:1]).blocks)
    assert first < need
    with make_volume(cs, max_blocks=need - 1) as vol:
        integrate(vol, cs.frames[:1])
        keys, tw, _ = vol.extract_blocks()
        assert len(keys) == first
        with pytest.raises(tp.TeaserHipError, match="OOM.*max_blocks = %d" % (need - 1)):
            integrate(vol, cs.frames[1:])
        k2, t2, _ = vol.extract_blocks()
        assert same(keys, k2) and same(tw, t2)      # the directory and every voxel as they were
        integrate(vol, cs.frames[:1])               # a smaller call succeeds: the handle stays usable
        assert vol.block_count == first
    with make_volume(cs, max_blocks=need) as vol:
        integrate(vol, cs.frames)
        check(vol, name)


def test_capacity_reset_and_the_round_trip():
    name = "rgb_64"
    cs, r = S.cases()[name], S.result(name)
    dp = C.POINTER(C.c_double)
    with make_volume(cs) as vol:
        pc = vol.extract_point_cloud()
        assert pc.points.shape == (0, 3) and pc.normals.shape == (0, 3) and vol.extract_voxel_point_cloud().points.shape == (0, 3)
        assert vol.block_count == 0 and vol.block_keys().shape == (0, 3)
        integrate(vol, cs.frames)
        n = len(r.points)
        L, cnt = tp.lib(), C.c_int64(-1)
        # capacity exactly the count
        P, N, Cc = np.full((n + 1, 3), -7.5), np.full((n + 1, 3), -7.5), np.full((n + 1, 3), -7.5)
        vol._call(L.teaser_hip_stsdf_extract_point_cloud, n, P.ctypes.data_as(dp), N.ctypes.data_as(dp), Cc.ctypes.data_as(dp), C.byref(cnt))
        assert cnt.value == n and same(P[:n], r.points) and same(N[:n], r.normals) and same(Cc[:n], r.colors)
        assert (P[n] == -7.5).all() and (N[n] == -7.5).all() and (Cc[n] == -7.5).all()
        # one below: refused, the count named, nothing written
        P[:] = -7.5
        cnt.value = -1
        with pytest.raises(tp.TeaserHipError, match="capacity %d is below the count %d" % (n - 1, n)):
            vol._call(L.teaser_hip_stsdf_extract_point_cloud, n - 1, P.ctypes.data_as(dp), None, None, C.byref(cnt))
        assert cnt.value == n and (P == -7.5).all()
        nb = len(r.keys)
        keys = np.full((nb, 3), -9, dtype=np.int32)
        with pytest.raises(tp.TeaserHipError, match="capacity %d is below the count %d" % (nb - 1, nb)):
            vol._call(L.teaser_hip_stsdf_block_keys, nb - 1, keys.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(cnt))
        assert cnt.value == nb and (keys == -9).all()
        check(vol, name)                               # the handle stays usable
        # reset, then the state back through inject, the blocks in another order
        vol.reset()
        assert vol.block_count == 0 and len(vol.extract_point_cloud().points) == 0
        order = np.arange(nb)[::-1]
        vol.inject_blocks(r.keys[order], r.tw[order], r.color[order])
        check(vol, name)
        with pytest.raises(tp.TeaserHipError, match="a block occurs twice"):
            vol.inject_blocks(r.keys[[0, 1, 0]], r.tw[[0, 1, 0]])
        bad = r.tw[:1].copy()
        bad[0, 5, 0] = np.inf
        with pytest.raises(tp.TeaserHipError, match="tsdf_weight has a non-finite value"):
            vol.inject_blocks(r.keys[:1], bad)
        # refusals of the frame checks leave the volume alone
        f = cs.frames[0]
        K = tp.PinholeCameraIntrinsic(64, 48, *f.K)
        with pytest.raises(tp.TeaserHipError, match=r"depth_scale must be finite and > 0 \(frame 1\)"):
            vol.integrate_batch([f.depth, f.depth], K, [f.E, f.E], [f.color, f.color], [1000.0, 0.0])
        with pytest.raises(tp.TeaserHipError, match=r"extrinsic is singular \(frame 0\)"):
            vol.integrate(f.depth, K, np.zeros((4, 4)), f.color)
        check(vol, name)
    with pytest.raises(ValueError, match="closed"):
        vol.reset()


def test_a_gray_volume_keeps_nan_colours_through_the_round_trip():
    name = "gray_7"
    cs, r = S.cases()[name], S.result(name)
    assert np.isnan(r.color).any()
    with make_volume(cs) as vol:
        integrate(vol, cs.frames)
        keys, tw, col = vol.extract_blocks()
        assert np.isnan(col).any() and same(col, r.color)
        vol.reset()
        assert vol.block_count == 0
        vol.inject_blocks(keys, tw, col)
        check(vol, name)
    with make_volume(cs) as vol:                  # and into a volume that never saw a frame
        vol.inject_blocks(r.keys, r.tw, r.color)
        check(vol, name)


def outputs(vol):
    keys, tw, col = vol.extract_blocks()
    pc, vp = vol.extract_point_cloud(), vol.extract_voxel_point_cloud()
    return [keys, tw, col, pc.points, pc.normals, pc.colors, vp.points, vp.colors]


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_no_result_depends_on_what_the_scratch_held(byte):
    name = "rgb_64"
    cs = S.cases()[name]
    with make_volume(cs) as vol:
        integrate(vol, cs.frames)       # the buffers exist from here on
        outputs(vol)
        vol.reset()
        assert vol.fill_scratch(byte) > 0
        counts = integrate(vol, cs.frames[:3])
        vol.fill_scratch(byte)
        counts += integrate(vol, cs.frames[3:])
        r = S.result(name)
        assert counts.tolist() == [r.touched, r.opened, r.out_of_range]
        vol.fill_scratch(byte)
        check(vol, name)
        vol.fill_scratch(byte)
        assert all(same(a, b) for a, b in zip(outputs(vol), outputs(vol)))
