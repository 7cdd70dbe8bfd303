"""The marching-cubes tables and the restatement of the triangle mesh (tests/tsdf_mesh_reference.py) pinned without a GPU:
the tables by property (they were written out from memory, so nothing here trusts a row: edge masks from corner signs,
rows against the masks, every case's patch a surface whose border lies in the cube's faces and joins exactly the crossed
edges of each face), the rows the contract is sure of, the library's copy and its SHA-256; the loop by hand on R = 2
cubes, on a zero weight, and by topology on an analytic sphere; and the header's closed-form numbering against the
loop's."""
import ctypes as C
import importlib

import numpy as np

import tsdf_mesh_reference as M
import tsdf_reference as T

tp = importlib.import_module("teaser-plusplus_amd")

FACES = [(k, v) for k in range(3) for v in (0, 1)]


def corner_mask(c):
    return sum(1 << i for i, (a, b) in enumerate(M.EDGE_TO_VERT) if ((c >> a) ^ (c >> b)) & 1)


def faces_of_edge(e):
    a, b = M.EDGE_TO_VERT[e]
    return {(k, v) for k, v in FACES if M.SHIFT[a][k] == v and M.SHIFT[b][k] == v}


def row_of(c):
    row = M.TRI_TABLE[c]
    n = row.index(-1) if -1 in row else 16
    return row[:n], row[n:]


def test_shift_edge_shift_and_edge_to_vert_agree():
    for i, (a, b) in enumerate(M.EDGE_TO_VERT):
        bx, by, bz, axis = M.EDGE_SHIFT[i]
        far = [bx, by, bz]
        far[axis] += 1
        assert M.SHIFT[a] == (bx, by, bz) and M.SHIFT[b] == tuple(far), i


def test_edge_table_is_the_mask_of_the_corner_signs():
    assert len(M.EDGE_TABLE) == 256
    for c in range(256):
        assert M.EDGE_TABLE[c] == corner_mask(c) == M.EDGE_TABLE[255 - c], c
    assert (M.EDGE_TABLE[1], M.EDGE_TABLE[2], M.EDGE_TABLE[3]) == (0x109, 0x203, 0x30a)


def test_tri_table_rows_use_exactly_the_crossed_edges():
    assert len(M.TRI_TABLE) == 256
    for c in range(256):
        assert len(M.TRI_TABLE[c]) == 16
        used, tail = row_of(c)
        assert len(used) % 3 == 0 and len(used) <= 15 and all(t == -1 for t in tail), c
        assert all(0 <= e < 12 for e in used) and sum(1 << e for e in set(used)) == M.EDGE_TABLE[c], c


def test_every_case_is_a_surface_that_closes_on_the_cube_faces():
    for c in range(256):
        used, _ = row_of(c)
        directed = {}
        for t in range(0, len(used), 3):
            a, b, d = used[t:t + 3]
            assert len({a, b, d}) == 3, c
            for e in ((a, b), (b, d), (d, a)):
                directed.setdefault(frozenset(e), []).append(e)
        once = []
        for uses in directed.values():
            assert len(uses) <= 2, c
            if len(uses) == 2:
                assert uses[0] == uses[1][::-1], (c, uses)  # opposite directions: one orientation across the patch
            else:
                once.append(uses[0])
        for a, b in once:
            assert faces_of_edge(a) & faces_of_edge(b), (c, a, b)  # an open edge lies in a cube face
        for face in FACES:
            crossed = sorted(e for e in range(12) if (M.EDGE_TABLE[c] >> e) & 1 and face in faces_of_edge(e))
            ends = sorted(e for seg in once if face in faces_of_edge(seg[0]) & faces_of_edge(seg[1]) for e in seg)
            assert len(crossed) in (0, 2, 4) and ends == crossed, (c, face)  # one segment, or two disjoint ones


def test_the_rows_the_contract_is_sure_of():
    assert row_of(0)[0] == [] and row_of(255)[0] == []
    assert row_of(1)[0] == [0, 8, 3] and row_of(2)[0] == [0, 1, 9] and row_of(3)[0] == [1, 8, 3, 9, 8, 1]
    assert row_of(253)[0] == [0, 9, 1] and row_of(254)[0] == [0, 3, 8]  # the recalled rows pass the properties as recalled


def test_the_library_hands_out_the_same_tables():
    edge, tri = (C.c_int32 * 256)(), (C.c_int8 * 4096)()
    L = tp.lib()
    assert L.teaser_hip_tsdf_mesh_tables(edge, tri) == 0
    assert list(edge) == M.EDGE_TABLE
    assert np.array_equal(np.frombuffer(tri, dtype=np.int8).reshape(256, 16), np.array(M.TRI_TABLE, dtype=np.int8))
    assert M.tri_table_sha256(np.frombuffer(tri, dtype=np.int8)) == M.tri_table_sha256() == M.TRI_TABLE_SHA256
    assert L.teaser_hip_tsdf_mesh_tables(None, tri) == 1 and L.teaser_hip_tsdf_mesh_tables(edge, None) == 1


def cube_volume(negative_corners, color_type=T.RGB8):
    """R = 2: one cube; the listed corners hold -0.25, the others 0.75; colours 10 i + (0, 1, 2) at corner i."""
    vol = T.Volume(2.0, 2, 0.5, color_type, (10.0, 20.0, 30.0))
    vol.weight[:] = T.f32(1)
    for i, (x, y, z) in enumerate(M.SHIFT):
        vol.tsdf[x, y, z] = T.f32(-0.25 if i in negative_corners else 0.75)
        vol.color[x, y, z] = [10.0 * i, 10.0 * i + 1.0, 10.0 * i + 2.0]
    return vol


def test_case_1_by_hand():
    """vl = 1, half = 0.5; corner 0 negative: edges 0, 3, 8 from voxel (0,0,0), f0 = 0.25, f1 = 0.75, so each vertex lies
    0.25 along its axis from (0.5, 0.5, 0.5); colour (0.75 c0 + 0.25 c1) / 1.0 with c = corner colour / 255."""
    m = M.extract_triangle_mesh(cube_volume({0}))
    assert m.edges == [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 0, 2)]  # slots 0, 3, 8 in this order
    assert np.array_equal(m.vertices, np.array([[10.75, 20.5, 30.5], [10.5, 20.75, 30.5], [10.5, 20.5, 30.75]]))
    assert m.triangles.dtype == np.int32 and m.triangles.tolist() == [[0, 1, 2]]  # {0, 8, 3} -> (v0, v3, v8)
    c = lambda i: np.array([10.0 * i, 10.0 * i + 1.0, 10.0 * i + 2.0]) / 255.0
    want = np.array([(0.75 * c(0) + 0.25 * c(k)) / 1.0 for k in (1, 3, 4)])
    assert np.array_equal(m.colors, want)
    assert m.normals is None and M.extract_triangle_mesh(cube_volume({0}, T.NONE)).colors is None


def test_case_3_by_hand():
    """Corners 0 and 1 negative: edges 1, 3, 8, 9 in slot order; row {1, 8, 3, 9, 8, 1} with the last two swapped."""
    m = M.extract_triangle_mesh(cube_volume({0, 1}), normals=True)
    assert m.edges == [(1, 0, 0, 1), (0, 0, 0, 1), (0, 0, 0, 2), (1, 0, 0, 2)]
    assert np.array_equal(m.vertices, np.array([[11.5, 20.75, 30.5], [10.5, 20.75, 30.5], [10.5, 20.5, 30.75], [11.5, 20.5, 30.75]]))
    assert m.triangles.tolist() == [[0, 1, 2], [3, 0, 2]]  # (v1, v3, v8), (v9, v1, v8)
    c = lambda i: np.array([10.0 * i, 10.0 * i + 1.0, 10.0 * i + 2.0]) / 255.0
    assert np.array_equal(m.colors, np.array([0.75 * c(1) + 0.25 * c(2), 0.75 * c(0) + 0.25 * c(3), 0.75 * c(0) + 0.25 * c(4),
                                               0.75 * c(1) + 0.25 * c(5)]))
    # the surface is the plane y + z = const between the voxel centres: the gradient has no x component
    assert m.normals.shape == (4, 3) and np.allclose(np.linalg.norm(m.normals, axis=1), 1.0) and (m.normals[:, 1:] > 0).all()


def test_a_zero_weight_corner_gives_an_empty_mesh():
    vol = cube_volume({0})
    vol.weight[1, 1, 1] = T.f32(0)
    m = M.extract_triangle_mesh(vol, normals=True)
    assert m.vertices.shape == (0, 3) and m.triangles.shape == (0, 3) and m.colors.shape == (0, 3) and m.normals.shape == (0, 3)
    assert M.extract_triangle_mesh(T.Volume(1.0, 1, 0.1)).vertices.shape == (0, 3)  # R = 1 has no cube


def test_the_sphere_is_a_closed_outward_surface():
    vol = M.sphere_volume()
    m = M.extract_triangle_mesh(vol)
    tri = m.triangles.astype(np.int64)
    V, F = len(m.vertices), len(tri)
    assert V > 500 and tri.min() == 0 and tri.max() == V - 1
    directed = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    keys = directed[:, 0] * V + directed[:, 1]
    assert len(np.unique(keys)) == len(keys)  # no directed edge twice
    assert np.array_equal(np.sort(keys), np.sort(directed[:, 1] * V + directed[:, 0]))  # each with its opposite
    E = len(keys) // 2
    assert V - E + F == 2
    p = m.vertices
    n = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    assert ((n * (p[tri].mean(axis=1) - 0.5)).sum(axis=1) > 0).all()  # the emitted winding faces outwards


def test_the_closed_form_numbering_is_the_loops():
    for vol in (M.sphere_volume(), M.random_volume(6, 5), M.random_volume(6, 6, zero_weights=0.0)):
        m = M.extract_triangle_mesh(vol)
        assert len(m.edges) > 20 and M.closed_form_numbering(vol) == [tuple(int(v) for v in e) for e in m.edges]
