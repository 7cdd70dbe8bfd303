"""The restatement of the triangle mesh of the scalable TSDF volume (tests/stsdf_mesh_reference.py) pinned without a GPU:
the creator at a block face by hand (the case in which the dense rule is wrong), a cube whose neighbour block is absent,
a vertex whose base voxel lies in the next block, the closed form by rank against the loop with its dict on the fixture
scenes and on random blocks, the dense identity (eight blocks that hold a dense 32^3 volume give the dense restatement's
mesh, only the order differs), the analytic sphere cut by the three mid-planes (closed, Euler characteristic 2, wound
outwards: no cracks across block faces), and what the fixtures must show so that no parity test passes on a scene that
never meets the hard case."""
import numpy as np
import pytest

import stsdf_mesh_reference as R
import stsdf_raycast_reference as SR
import stsdf_reference as S
import tsdf_mesh_reference as M
import tsdf_reference as T

U = R.U
f32 = np.float32


def filled(keys, tsdf=0.5, weight=1.0, vl=1.0 / 16.0, trunc=0.25):
    """The blocks `keys`, every voxel with the given tsdf and weight; returns the dict volume_of_blocks takes."""
    return {b: (np.full((U, U, U), tsdf, dtype=f32), np.full((U, U, U), weight, dtype=f32), None) for b in keys}


def put(blocks, g, tsdf=None, weight=None):
    b, l = tuple(k // U for k in g), tuple(k % U for k in g)
    if tsdf is not None:
        blocks[b][0][l] = f32(tsdf)
    if weight is not None:
        blocks[b][1][l] = f32(weight)


def test_the_creator_at_a_block_face_is_not_the_dense_one():
    """The x-edge with base voxel h = (5, 7, 0): local y != 0, local z = 0.  A = h - e_y - e_z and C = h - e_z lie in
    block (0, 0, -1), B = h - e_y and D = h in block (0, 0, 0).  A has a corner of weight 0 that neither B nor C has, so
    B, C and D are ACTIVE: the dense rule names B, the rank names C, where the edge is number 4."""
    blocks = filled([(0, 0, -1), (0, 0, 0)])
    h = (5, 7, 0)
    put(blocks, h, tsdf=-0.5)
    put(blocks, (5, 6, -1), weight=0.0)
    vol = SR.volume_of_blocks(1.0 / 16.0, 0.25, T.NONE, blocks)
    A, B, C, D = (5, 6, -1), (5, 6, 0), (5, 7, -1), (5, 7, 0)
    active = R.active_set(vol)
    assert A not in active and B in active and C in active and D in active
    assert [c for c, _ in R.edge_cubes(h + (0,))] == [A, B, C, D]  # ascending global order
    assert R.rank(A) < R.rank(C) < R.rank(B) < R.rank(D)
    creator, slot, dense = R.creators(vol)[h + (0,)]
    assert creator == C and slot == 4 and dense == B
    m = R.extract_triangle_mesh(vol)
    # the loop meets the edge in C: the vertex is numbered among those of block (0, 0, -1), before any of block (0, 0, 0)
    first_of_upper_block = min(k for k, e in enumerate(m.edges) if min(R.rank(c) for c, _ in R.edge_cubes(e) if c in active)[2] == 0)
    assert m.edges.index(h + (0,)) < first_of_upper_block
    assert R.closed_form_numbering(vol) == m.edges
    assert R.face_statistics(vol)[3] >= 1


def test_a_cube_at_local_15_with_an_absent_neighbour_gives_nothing():
    blocks = filled([(0, 0, 0)])
    put(blocks, (15, 8, 8), tsdf=-0.5)
    vol = SR.volume_of_blocks(1.0 / 16.0, 0.25, T.NONE, blocks)
    active = R.active_set(vol)
    assert active and all(c[0] == 14 for c in active)  # the four cubes below x = 15 only
    m = R.extract_triangle_mesh(vol, normals=True)
    assert (15, 8, 8, 0) not in m.edges and len(m.edges) == 5 and all(e[0] <= 15 for e in m.edges)
    # a lone block whose sign change needs the next block: no cube at all
    lone = filled([(0, 0, 0)])
    for y in range(U):
        for z in range(U):
            put(lone, (15, y, z), tsdf=-0.5)
    lone[(0, 0, 0)][1][:15] = f32(0)  # only the last layer is observed
    m = R.extract_triangle_mesh(SR.volume_of_blocks(1.0 / 16.0, 0.25, T.NONE, lone), normals=True)
    assert m.vertices.shape == (0, 3) and m.triangles.shape == (0, 3) and m.normals.shape == (0, 3)
    # with the next block open the edge carries a vertex
    blocks.update(filled([(1, 0, 0)]))
    m = R.extract_triangle_mesh(SR.volume_of_blocks(1.0 / 16.0, 0.25, T.NONE, blocks))
    assert (15, 8, 8, 0) in m.edges and len(m.edges) == 6


def test_a_vertex_whose_base_voxel_lies_in_the_next_block():
    """Voxel (16, 8, 8) -- local (0, 8, 8) of block (1, 0, 0) -- is the only negative one.  The y-edge from it is contained
    in the cubes (15 | 16, 8, 7 | 8); the smallest rank is (15, 8, 7) of block (0, 0, 0), where the edge is number 5.
    vl = 1 / 16, half = 1 / 32, f0 = 0.25, f1 = 0.75: the vertex is (1 + 1/32, 1/2 + 1/32 + 1/64, 1/2 + 1/32)."""
    blocks = filled([(0, 0, 0), (1, 0, 0)], tsdf=0.75)
    put(blocks, (16, 8, 8), tsdf=-0.25)
    vol = SR.volume_of_blocks(1.0 / 16.0, 0.25, T.NONE, blocks)
    creator, slot, dense = R.creators(vol)[(16, 8, 8, 1)]
    assert creator == (15, 8, 7) and slot == 5 and dense == (15, 8, 7)
    m = R.extract_triangle_mesh(vol, normals=True)
    k = m.edges.index((16, 8, 8, 1))
    assert np.array_equal(m.vertices[k], [1.0 + 1.0 / 32.0, 0.5 + 1.0 / 32.0 + 1.0 / 64.0, 0.5 + 1.0 / 32.0])
    assert len(m.edges) == 6 and len(m.triangles) == 8  # an octahedron round the voxel
    assert m.normals[k][1] > 0.9  # the gradient points away from the negative voxel along the edge
    assert R.closed_form_numbering(vol) == m.edges


@pytest.mark.parametrize("name", ["none_7", "rgb_64", "gray_64_stride1", "far", "rgb_7_wide_stride"])
def test_the_closed_form_numbering_is_the_loops_on_the_fixtures(name):
    vol = S.result(name).vol
    m = R.result(name)
    assert len(m.edges) > 100 and R.closed_form_numbering(vol) == m.edges
    assert m.triangles.min() == 0 and m.triangles.max() == len(m.vertices) - 1
    assert np.isfinite(m.vertices).all() and np.isfinite(m.normals).all()


@pytest.mark.parametrize("name", sorted(R.RANDOM_SETS))
def test_the_closed_form_numbering_is_the_loops_on_random_blocks(name):
    vol = R.random_set(name)
    m = R.result(name)
    assert any(min(b) < 0 for b in vol.blocks)
    assert len(m.edges) > 500 and R.closed_form_numbering(vol) == m.edges
    blocks, cubes, crossing, differ = R.face_statistics(vol)
    # two blocks adjacent along x are visited in global order (x is outermost), so only the larger sets must differ
    assert cubes > 100 and (len(vol.blocks) == 1 or crossing > 0) and (len(vol.blocks) < 7 or differ > 0)


def test_the_l_shape_misses_its_corner_block():
    keys = set(R.RANDOM_SETS["l_shape"][0])
    assert len(keys) == 7 and (0, 0, 0) not in keys and keys | {(0, 0, 0)} == {(x - 1, y - 1, z - 1) for x, y, z in R.CUBE_2}
    # the cube whose eight corners lie in eight blocks has one in the missing block: never ACTIVE
    assert (-1, -1, -1) not in R.active_set(R.random_set("l_shape"))


FIXTURE_TABLE = {"none_7": (16, 1214, 281, 5), "rgb_64": (38, 1496, 347, 8)}


def test_what_the_fixtures_show():
    """(blocks, ACTIVE cubes, those with a local index of 15, edges whose rank-creator is not the dense one)."""
    for name, want in FIXTURE_TABLE.items():
        assert R.face_statistics(S.result(name).vol) == want, name
    assert R.face_statistics(S.result("gray_64_stride1").vol)[3] == 3 and R.face_statistics(S.result("far").vol)[3] == 2
    for name in ("split_9", "identity"):  # these never meet the hard case: no parity test may rest on them alone
        assert R.face_statistics(S.result(name).vol)[3] == 0
    for name in R.FIXTURES:
        blocks, cubes, crossing, differ = R.face_statistics(S.result(name).vol)
        assert (crossing >= 1 and differ >= 1) or blocks == 0, name
    assert sum(1 for name in R.FIXTURES if len(S.result(name).vol.blocks) > 0) >= 6


def dense_at_origin(vol):
    """The fields of the dense volume `vol` in a volume with origin 0."""
    out = T.Volume(vol.length, vol.R, vol.sdf_trunc, vol.color_type)
    out.tsdf[:], out.weight[:] = vol.tsdf, vol.weight
    if vol.color_type != T.NONE:
        out.color[:] = vol.color
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_dense_identity(dense, m_dense, m_blocks):
    """The vertices bit for bit as a set keyed by lattice edge, the triangles after mapping indices through that key:
    only the order differs."""
    at = {e: k for k, e in enumerate(tuple(int(v) for v in e) for e in m_dense.edges)}
    assert len(at) == len(m_dense.edges) and sorted(at) == sorted(m_blocks.edges)
    to_dense = np.array([at[e] for e in m_blocks.edges], dtype=np.int64)
    for a, b in ((m_dense.vertices, m_blocks.vertices), (m_dense.colors, m_blocks.colors), (m_dense.normals, m_blocks.normals)):
        assert (a is None) == (b is None)
        if a is not None:
            assert same_bits(np.ascontiguousarray(a[to_dense]), b)
    mapped = to_dense[m_blocks.triangles.astype(np.int64)]
    key = lambda t: sorted(map(tuple, t.tolist()))
    assert len(mapped) == len(m_dense.triangles) and key(mapped) == key(m_dense.triangles.astype(np.int64))
    assert not np.array_equal(to_dense, np.arange(len(to_dense)))  # the order does differ


@pytest.mark.parametrize("ctype", [T.NONE, T.RGB8, T.GRAY32])
def test_dense_identity(ctype):
    dense = dense_at_origin(M.random_volume(32, 40 + ctype, ctype))
    m_dense = M.extract_triangle_mesh(dense, normals=True)
    assert len(m_dense.vertices) > 5000
    vol = R.blocks_of_dense(dense)
    assert sorted(vol.blocks) == sorted(R.CUBE_2) and vol.vl == dense.vl
    check_dense_identity(dense, m_dense, R.extract_triangle_mesh(vol, normals=True))


def test_the_sphere_cut_into_eight_blocks_is_a_closed_outward_surface():
    dense = M.sphere_volume(R=32)
    vol = R.blocks_of_dense(dense)
    m = R.extract_triangle_mesh(vol, normals=True)
    for axis in range(3):  # the surface crosses the three mid-planes
        assert any(e[axis] == 15 and e[3] == axis for e in m.edges) or any(e[axis] == 16 for e in m.edges)
    tri = m.triangles.astype(np.int64)
    V, F = len(m.vertices), len(tri)
    assert V > 500 and tri.min() == 0 and tri.max() == V - 1
    directed = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    keys = directed[:, 0] * V + directed[:, 1]
    assert len(np.unique(keys)) == len(keys)  # no directed edge twice
    assert np.array_equal(np.sort(keys), np.sort(directed[:, 1] * V + directed[:, 0]))  # each with its opposite: no crack
    assert V - len(keys) // 2 + F == 2
    p = m.vertices
    n = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    assert ((n * (p[tri].mean(axis=1) - 0.5)).sum(axis=1) > 0).all()  # the emitted winding faces outwards
    assert ((m.normals * (p - 0.5)).sum(axis=1) > 0).all()  # and the gradient points outwards
    check_dense_identity(dense, M.extract_triangle_mesh(dense, normals=True), m)


@pytest.mark.parametrize("pattern", [1, 2, 0x55, 0x0f, 0x96, 254])
def test_one_cube_in_eight_blocks(pattern):
    vol = R.corner_cube_volume(pattern, color_type=T.RGB8)
    assert R.active_set(vol) == {(-1, -1, -1): pattern}
    m = R.extract_triangle_mesh(vol, normals=True)
    crossed = [i for i in range(12) if M.EDGE_TABLE[pattern] >> i & 1]
    assert m.edges == [(-1 + M.EDGE_SHIFT[i][0], -1 + M.EDGE_SHIFT[i][1], -1 + M.EDGE_SHIFT[i][2], M.EDGE_SHIFT[i][3]) for i in crossed]
    row = [e for e in M.TRI_TABLE[pattern] if e >= 0]
    assert m.triangles.tolist() == [[crossed.index(row[t]), crossed.index(row[t + 2]), crossed.index(row[t + 1])] for t in range(0, len(row), 3)]
    for missing in ((-1, -1, -1), (0, -1, 0), (0, 0, 0)):
        assert len(R.extract_triangle_mesh(R.corner_cube_volume(pattern, missing)).vertices) == 0
