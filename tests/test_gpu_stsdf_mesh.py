"""The triangle mesh of the scalable TSDF volume on the MI355X.  Everything must be EQUAL, compared as bytes:
  1. against the restatement written as Open3D's loop (tests/stsdf_mesh_reference.py, pinned in
     tests/test_stsdf_mesh_reference.py): vertices, colours, normals and triangles of the fixture scenes -- every one of
     them with cubes across block faces and edges whose creator by rank is not the dense one --, of the one cube whose
     eight corners lie in eight blocks in all 256 sign patterns, and of random injected block sets with zeroed weights
     and NaN Gray32 colours;
  2. against the DENSE mesh of a real UniformTSDFVolume of 32^3 moved over through extract_blocks / inject_blocks:
     the same vertices bit for bit keyed by lattice edge, the same triangles through that key;
  3. whatever the slab sizes, the order the blocks were opened in and the growth of the directory between two calls;
  4. the capacity rule, the same bytes twice, after fill_scratch(0x00) and fill_scratch(0xFF), with and without normals."""
import ctypes as C
import importlib

import numpy as np
import pytest

import stsdf_mesh_reference as R
import stsdf_reference as S
import tsdf_mesh_reference as M
import tsdf_reference as T
from test_gpu_stsdf import integrate, make_volume, same

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def parts(m):
    """A TSDFTriangleMesh of the library or a Mesh of the restatement as (vertices, colours, normals, triangles)."""
    if hasattr(m, "vertex_colors"):
        return [m.vertices, m.vertex_colors, m.vertex_normals, m.triangles]
    return [m.vertices, m.colors, m.normals, m.triangles]


def same_mesh(a, b):
    return all((x is None) == (y is None) and (x is None or same(np.ascontiguousarray(x), np.ascontiguousarray(y)))
               for x, y in zip(parts(a), parts(b)))


def check(vol, want, what):
    """With normals and without, through the method and through the package's function."""
    got = vol.extract_mesh(vertex_normals=True)
    assert got.triangles.dtype == np.int32 and got.vertices.dtype == np.float64
    assert (len(got.vertices), len(got.triangles)) == (len(want.vertices), len(want.triangles)), what
    for name, x, y in zip(("vertices", "colours", "normals", "triangles"), parts(got), parts(want)):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.shape == y.shape and x.dtype == y.dtype, (what, name)
            row = 3 * x.itemsize
            bad = np.flatnonzero((np.ascontiguousarray(x).view(np.uint8).reshape(len(x), row) !=
                                  np.ascontiguousarray(y).view(np.uint8).reshape(len(y), row)).any(axis=1))
            assert len(bad) == 0, (what, name, len(bad), bad[:5])
    plain = tp.extract_triangle_mesh(vol)
    assert plain.vertex_normals is None and same_mesh(plain, M.Mesh(want.vertices, want.colors, None, want.triangles, None)), what


def injected(vol_ref, order=None, **kw):
    """A device volume with the blocks of the restatement's volume, injected in the given order."""
    vol = tp.ScalableTSDFVolume(vol_ref.vl, vol_ref.sdf_trunc, vol_ref.color_type, 16, 4, **kw)
    keys = vol_ref.keys()
    if len(keys):
        order = np.arange(len(keys)) if order is None else order
        color = vol_ref.block_colors()[order] if vol_ref.color_type != T.NONE else None
        vol.inject_blocks(keys[order], vol_ref.block_tsdf_weight()[order], color)
    return vol


@pytest.mark.parametrize("name", R.FIXTURES)
def test_the_fixture_scenes_equal_the_restatement(name):
    cs, want = S.cases()[name], R.result(name)
    blocks, cubes, crossing, differ = R.face_statistics(R.volume(name))
    assert blocks == 0 or (crossing >= 1 and differ >= 1)  # no parity on a scene that never meets the hard case
    with make_volume(cs) as vol:
        assert len(vol.extract_mesh().vertices) == 0 and vol.extract_mesh().triangles.shape == (0, 3)  # no open block: 0 / 0
        integrate(vol, cs.frames)
        check(vol, want, name)


def test_all_sign_patterns_of_the_cube_in_eight_blocks():
    """Local (15, 15, 15) of block (-1, -1, -1): its eight corners lie in eight blocks.  One volume serves all patterns: the
    eight corner voxels are injected again for each."""
    first = R.corner_cube_volume(0, color_type=T.RGB8)
    keys, tw, col = first.keys(), first.block_tsdf_weight().copy(), first.block_colors()
    assert len(keys) == 8
    active = 0
    with tp.ScalableTSDFVolume(first.vl, first.sdf_trunc, T.RGB8) as vol, tp.ScalableTSDFVolume(first.vl, first.sdf_trunc, T.RGB8) as holed:
        for pattern in range(256):
            ref = R.corner_cube_volume(pattern, color_type=T.RGB8)
            want = R.extract_triangle_mesh(ref, normals=True)
            vol.inject_blocks(keys, ref.block_tsdf_weight(), col)
            check(vol, want, pattern)
            active += len(want.triangles) > 0
            # one of the eight blocks left closed (another one for every pattern): no mesh
            keep = np.arange(8) != pattern % 8
            holed.reset()
            holed.inject_blocks(keys[keep], ref.block_tsdf_weight()[keep], col[keep])
            got = holed.extract_mesh(vertex_normals=True)
            assert holed.block_count == 7 and got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3), pattern
    assert active == 254


@pytest.mark.parametrize("name", sorted(R.RANDOM_SETS))
def test_random_block_sets_equal_the_restatement(name):
    ref, want = R.random_set(name), R.result(name)
    assert (ref.block_tsdf_weight()[..., 1] == 0).mean() > 0.3
    assert ref.color_type != T.GRAY32 or np.isnan(ref.block_colors()).any()
    with injected(ref) as vol:
        check(vol, want, name)


def test_the_dense_identity_against_a_real_dense_volume():
    """A UniformTSDFVolume of 32^3 with origin 0 and the eight blocks {0, 1}^3 that hold its voxels: the dense mesh's
    vertices bit for bit as a set keyed by lattice edge, its triangles through that key; only the order differs."""
    src = M.random_volume(32, 41, T.RGB8)
    with tp.UniformTSDFVolume(src.length, 32, src.sdf_trunc, T.RGB8) as dense, \
            tp.ScalableTSDFVolume(src.vl, src.sdf_trunc, T.RGB8) as vol, tp.ScalableTSDFVolume(src.vl, src.sdf_trunc, T.RGB8) as carrier:
        assert vol.voxel_length == dense.voxel_length
        dense.inject_volume_tsdf(src.tsdf_weight())
        dense.inject_volume_color(src.colors())
        tw = dense.extract_volume_tsdf().reshape(32, 32, 32, 2)
        col = dense.extract_volume_color().reshape(32, 32, 32, 3)
        keys = np.array(R.CUBE_2, dtype=np.int32)
        cut = lambda a: np.stack([a[16 * x:16 * x + 16, 16 * y:16 * y + 16, 16 * z:16 * z + 16].reshape(4096, -1) for x, y, z in R.CUBE_2])
        # through inject_blocks and extract_blocks of one handle into another
        carrier.inject_blocks(keys[::-1], cut(tw)[::-1], cut(col)[::-1])
        vol.inject_blocks(*carrier.extract_blocks())
        md, ms = dense.extract_triangle_mesh(vertex_normals=True), vol.extract_mesh(vertex_normals=True)
    assert len(md.vertices) > 5000 and len(ms.vertices) == len(md.vertices) and len(ms.triangles) == len(md.triangles)
    # a vertex lies on one lattice edge: the key is recovered from the restatement, which the dense GPU mesh equals
    ref_dense = T.Volume(src.length, 32, src.sdf_trunc, T.RGB8)
    ref_dense.tsdf[:], ref_dense.weight[:], ref_dense.color[:] = src.tsdf, src.weight, src.color
    rd = M.extract_triangle_mesh(ref_dense, normals=True)
    rs = R.extract_triangle_mesh(R.blocks_of_dense(ref_dense), normals=True)
    assert same_mesh(md, rd) and same_mesh(ms, rs)
    at = {tuple(int(v) for v in e): k for k, e in enumerate(rd.edges)}
    to_dense = np.array([at[e] for e in rs.edges], dtype=np.int64)
    assert same(np.ascontiguousarray(md.vertices[to_dense]), ms.vertices)
    assert same(np.ascontiguousarray(md.vertex_colors[to_dense]), ms.vertex_colors)
    assert same(np.ascontiguousarray(md.vertex_normals[to_dense]), ms.vertex_normals)
    key = lambda t: sorted(map(tuple, t.tolist()))
    assert key(to_dense[ms.triangles.astype(np.int64)]) == key(md.triangles.astype(np.int64))
    assert not np.array_equal(to_dense, np.arange(len(to_dense)))


def test_slab_sizes_and_the_opening_order_do_not_change_a_byte():
    name = "rgb_64"
    cs, want = S.cases()[name], R.result(name)
    with make_volume(cs, initial_blocks=1, slab_blocks=1) as vol:
        integrate(vol, cs.frames)
        check(vol, want, "slabs of one block")
    ref = R.volume(name)
    n = len(ref.keys())
    with injected(ref, np.arange(n)[::-1], initial_blocks=3, slab_blocks=5) as vol:
        check(vol, want, "injected in reverse order")
    with injected(ref, np.random.default_rng(5).permutation(n)) as vol:
        check(vol, want, "injected in random order")


def test_a_mesh_between_frames_that_open_blocks():
    name = "rgb_64"
    cs, want = S.cases()[name], R.result(name)
    first = S.run(cs, cs.frames[:1])
    assert 0 < len(first.blocks) < len(R.volume(name).blocks)
    with make_volume(cs, initial_blocks=4, slab_blocks=4) as vol:
        integrate(vol, cs.frames[:1])
        check(vol, R.extract_triangle_mesh(first, normals=True), "after the first frame")
        integrate(vol, cs.frames[1:])   # opens blocks: the directory and the scratch grow
        check(vol, want, "after all frames")


def test_the_capacity_rule():
    name = "none_7"
    cs, want = S.cases()[name], R.result(name)
    n, m = len(want.vertices), len(want.triangles)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    fn = tp.lib().teaser_hip_stsdf_extract_triangle_mesh
    with make_volume(cs) as vol:
        integrate(vol, cs.frames)
        nv, nt = C.c_int64(-1), C.c_int64(-1)
        vol._call(fn, 0, None, None, None, 0, None, C.byref(nv), C.byref(nt))   # the counts alone
        assert (nv.value, nt.value) == (n, m)
        V, N, Tr = np.full((n + 1, 3), -7.5), np.full((n + 1, 3), -7.5), np.full((m + 1, 3), -7, dtype=np.int32)
        vol._call(fn, n, V.ctypes.data_as(dp), None, N.ctypes.data_as(dp), m, Tr.ctypes.data_as(ip), C.byref(nv), C.byref(nt))
        assert same(V[:n], want.vertices) and same(N[:n], want.normals) and same(Tr[:m], want.triangles)
        assert (V[n] == -7.5).all() and (N[n] == -7.5).all() and (Tr[m] == -7).all()   # rows behind the counts
        for dv, dt in ((1, 0), (0, 1)):     # one short on each array: refused, both counts named and filled, no row written
            V[:], N[:], Tr[:] = -7.5, -7.5, -7
            nv.value = nt.value = -1
            with pytest.raises(tp.TeaserHipError, match="a capacity is below its count: vertex_capacity %d, vertex count %d; "
                                                        "triangle_capacity %d, triangle count %d" % (n - dv, n, m - dt, m)):
                vol._call(fn, n - dv, V.ctypes.data_as(dp), None, N.ctypes.data_as(dp), m - dt, Tr.ctypes.data_as(ip), C.byref(nv), C.byref(nt))
            assert (nv.value, nt.value) == (n, m) and (V == -7.5).all() and (N == -7.5).all() and (Tr == -7).all()
        with pytest.raises(tp.TeaserHipError, match="vertex_colors is given for a volume without colour"):
            vol._call(fn, n, V.ctypes.data_as(dp), N.ctypes.data_as(dp), None, m, Tr.ctypes.data_as(ip), C.byref(nv), C.byref(nt))
        with pytest.raises(tp.TeaserHipError, match="vertex_count_out and triangle_count_out must not be NULL"):
            vol._call(fn, 0, None, None, None, 0, None, None, C.byref(nt))
        check(vol, want, name)    # the handle stays usable
        vol.reset()
        assert len(vol.extract_mesh().triangles) == 0


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_no_result_depends_on_what_the_scratch_held(byte):
    name = "gray_64_stride1"
    cs, want = S.cases()[name], R.result(name)
    with make_volume(cs) as vol:
        integrate(vol, cs.frames)
        a = vol.extract_mesh(vertex_normals=True)      # the buffers exist from here on
        before = vol.extract_blocks()
        assert vol.fill_scratch(byte) >= 5 * 4096 * vol.block_count
        check(vol, want, "after fill_scratch")
        vol.fill_scratch(byte)
        b = vol.extract_mesh(vertex_normals=True)
        assert same_mesh(a, b) and same_mesh(b, vol.extract_mesh(vertex_normals=True))   # the same bytes twice
        after = vol.extract_blocks()
        assert all(same(x, y) for x, y in zip(before, after))   # the mesh leaves the blocks and the directory alone
