"""The triangle mesh of the scalable TSDF volume restated in Python: the parity target of tests/test_stsdf_mesh_host.py
and tests/test_gpu_stsdf_mesh.py, pinned by hand, by the dense identity and by topology in
tests/test_stsdf_mesh_reference.py.  It follows include/teaser_hip.h ("Scalable TSDF triangle mesh") as Open3D's loop on
stsdf_reference.ScalableVolume: the blocks in ascending order, the cubes of a block in x, y, z order, a dict from the
GLOBAL lattice edge to the index of its vertex, vertices appended when an edge is first met.  It is deliberately NOT the
closed form of the header (creator by rank, slot): closed_form_numbering() below is that, and the tests compare the two.
The tables are those of tests/tsdf_mesh_reference.py.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import stsdf_raycast_reference as SR
import stsdf_reference as S
import tsdf_mesh_reference as M
import tsdf_reference as T

U = S.U
f32 = np.float32
SHIFT, EDGE_SHIFT, EDGE_TO_VERT, EDGE_TABLE, TRI_TABLE = M.SHIFT, M.EDGE_SHIFT, M.EDGE_TO_VERT, M.EDGE_TABLE, M.TRI_TABLE
Mesh = M.Mesh  # edges: the GLOBAL lattice edge (hx, hy, hz, axis) of every vertex


def padded(vol, b):
    """Block b with one more layer on every axis from the blocks b + {0, 1}^3: tsdf and weight, 17^3 each; a voxel of a
    block that is not open has tsdf 0 and weight 0."""
    F, W = np.zeros((U + 1,) * 3, dtype=f32), np.zeros((U + 1,) * 3, dtype=f32)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                nb = vol.blocks.get((b[0] + dx, b[1] + dy, b[2] + dz))
                if nb is None:
                    continue
                dst = tuple(slice(0, U) if d == 0 else slice(U, U + 1) for d in (dx, dy, dz))
                src = tuple(slice(0, U) if d == 0 else slice(0, 1) for d in (dx, dy, dz))
                F[dst], W[dst] = nb.tsdf[src], nb.weight[src]
    return F, W


def active_cubes(vol, b):
    """(cube_index of the 16^3 cubes whose base voxel lies in block b, ACTIVE mask)."""
    F, W = padded(vol, b)
    index = np.zeros((U, U, U), dtype=np.int64)
    observed = np.ones((U, U, U), dtype=bool)
    for i, (dx, dy, dz) in enumerate(SHIFT):
        s = (slice(dx, dx + U), slice(dy, dy + U), slice(dz, dz + U))
        index |= (F[s] < f32(0)).astype(np.int64) << i
        observed &= W[s] != 0
    return index, observed & (index != 0) & (index != 255)


def voxel(vol, g):
    """(the block of global voxel g, its local index)."""
    b = tuple(int(k) // U for k in g)  # floor division
    return vol.blocks[b], tuple(int(k) % U for k in g)


def extract_triangle_mesh(vol, normals=False):
    """Open3D's loop over the sorted blocks.  Only the cubes it does not skip are visited, in the contract's order."""
    half = vol.vl * 0.5
    colored = vol.color_type != T.NONE
    edge_to_vertex = {}
    vertices, colors, triangles = [], [], []
    for b in sorted(vol.blocks):
        index, active = active_cubes(vol, b)
        for x, y, z in np.argwhere(active):  # C order: x, then y, then z
            g = (U * b[0] + int(x), U * b[1] + int(y), U * b[2] + int(z))
            cube_index = int(index[x, y, z])
            edge_to_index = [-1] * 12
            for i in range(12):
                if not EDGE_TABLE[cube_index] & (1 << i):
                    continue
                key = (g[0] + EDGE_SHIFT[i][0], g[1] + EDGE_SHIFT[i][1], g[2] + EDGE_SHIFT[i][2], EDGE_SHIFT[i][3])
                if key in edge_to_vertex:
                    edge_to_index[i] = edge_to_vertex[key]
                    continue
                edge_to_index[i] = edge_to_vertex[key] = len(vertices)
                a = tuple(g[k] + SHIFT[EDGE_TO_VERT[i][0]][k] for k in range(3))
                e = tuple(g[k] + SHIFT[EDGE_TO_VERT[i][1]][k] for k in range(3))
                assert a == key[:3]
                (blk0, l0), (blk1, l1) = voxel(vol, a), voxel(vol, e)
                f0, f1 = abs(float(blk0.tsdf[l0])), abs(float(blk1.tsdf[l1]))
                p = [half + vol.vl * float(key[0]), half + vol.vl * float(key[1]), half + vol.vl * float(key[2])]
                p[key[3]] = p[key[3]] + (f0 * vol.vl) / (f0 + f1)
                vertices.append(p)  # no origin: the vertex is formed from the global edge index
                if colored:
                    c0, c1 = blk0.color[l0], blk1.color[l1]
                    if vol.color_type == T.RGB8:
                        c0, c1 = c0 / 255.0, c1 / 255.0
                    with np.errstate(invalid="ignore"):
                        c = (f1 * c0 + f0 * c1) / (f0 + f1)
                    colors.append(np.where(np.isnan(c), np.nan, c) if vol.color_type == T.GRAY32 else c)
            row = TRI_TABLE[cube_index]
            t = 0
            while row[t] != -1:
                triangles.append((edge_to_index[row[t]], edge_to_index[row[t + 2]], edge_to_index[row[t + 1]]))
                t += 3
    n = len(vertices)
    vert = np.array(vertices, dtype=np.float64).reshape(n, 3)
    nrm = None
    if normals:
        lat = SR.Lattice(vol)
        g = 0.99 * vol.vl
        nrm = np.zeros((n, 3))
        for a in range(3):
            hi, lo = vert.copy(), vert.copy()
            hi[:, a] = vert[:, a] + g
            lo[:, a] = vert[:, a] - g
            nrm[:, a] = SR.trilinear(vol, lat, hi) - SR.trilinear(vol, lat, lo) if n else 0.0
        s = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        with np.errstate(all="ignore"):
            nrm = np.where((s > 0)[:, None], nrm / np.sqrt(s)[:, None], nrm)
    edges = sorted(edge_to_vertex, key=edge_to_vertex.get)
    return Mesh(vert, np.array(colors, dtype=np.float64).reshape(n, 3) if colored else None, nrm,
                np.array(triangles, dtype=np.int32).reshape(-1, 3), edges)


def active_set(vol):
    """global cube -> cube_index for every ACTIVE cube."""
    out = {}
    for b in vol.blocks:
        index, active = active_cubes(vol, b)
        for x, y, z in np.argwhere(active):
            out[(U * b[0] + int(x), U * b[1] + int(y), U * b[2] + int(z))] = int(index[x, y, z])
    return out


def rank(c):
    """rank(cube) of the contract: the block (the directory is sorted by it), then the local index, x outermost."""
    return tuple(k // U for k in c) + tuple(k % U for k in c)


def edge_cubes(key):
    """The four cubes that contain the lattice edge `key`, in ascending GLOBAL order, each with the edge's slot there."""
    h, axis = key[:3], key[3]
    others = [k for k in range(3) if k != axis]
    out = []
    for du in (1, 0):
        for dv in (1, 0):
            c = list(h)
            c[others[0]] -= du
            c[others[1]] -= dv
            out.append((tuple(c), EDGE_SHIFT.index((h[0] - c[0], h[1] - c[1], h[2] - c[2], axis))))
    return out


def creators(vol, active=None):
    """lattice edge -> (creator by rank, its slot, creator by global lexicographic order -- the dense rule) for every
    edge that carries a vertex."""
    active = active if active is not None else active_set(vol)
    out = {}
    for c, cube_index in active.items():
        for i in range(12):
            if not EDGE_TABLE[cube_index] & (1 << i):
                continue
            key = (c[0] + EDGE_SHIFT[i][0], c[1] + EDGE_SHIFT[i][1], c[2] + EDGE_SHIFT[i][2], EDGE_SHIFT[i][3])
            if key in out:
                continue
            cand = [(q, slot) for q, slot in edge_cubes(key) if q in active]
            by_rank = min(cand, key=lambda qs: rank(qs[0]))
            out[key] = (by_rank[0], by_rank[1], min(q for q, _ in cand))
    return out


def closed_form_numbering(vol):
    """The lattice edges that carry a vertex in the order of the header's closed form: ascending (rank(creator), slot)."""
    found = [(rank(c), slot, key) for key, (c, slot, _) in creators(vol).items()]
    return [key for _, _, key in sorted(found)]


def face_statistics(vol):
    """What a fixture shows of the hard cases: (blocks, ACTIVE cubes, those with a local index of 15 on some axis, edges
    whose rank-creator is not the global-lexicographic one)."""
    active = active_set(vol)
    crossing = sum(1 for c in active if any(k % U == U - 1 for k in c))
    differ = sum(1 for c, _, dense in creators(vol, active).values() if c != dense)
    return len(vol.blocks), len(active), crossing, differ


def blocks_of_dense(dense, vl=None):
    """The dense volume `dense` (R a multiple of 16, origin 0) cut into (R / 16)^3 blocks of a ScalableVolume."""
    assert dense.R % U == 0 and not np.any(dense.origin)
    n = dense.R // U
    blocks = {}
    for bx in range(n):
        for by in range(n):
            for bz in range(n):
                s = (slice(U * bx, U * bx + U), slice(U * by, U * by + U), slice(U * bz, U * bz + U))
                blocks[(bx, by, bz)] = (dense.tsdf[s], dense.weight[s], dense.color[s] if dense.color_type != T.NONE else None)
    return SR.volume_of_blocks(dense.vl if vl is None else vl, dense.sdf_trunc, dense.color_type, blocks)


def random_blocks(keys, seed, color_type=T.NONE, zero_weights=1.0 / 3.0, vl=0.02, trunc=0.06):
    """The blocks `keys` with random signs and magnitudes, a share of the weights zeroed and random colours (a Gray32
    volume with some NaN), following tsdf_mesh_reference.random_volume."""
    rng = np.random.default_rng(seed)
    blocks = {}
    for b in sorted(tuple(int(k) for k in key) for key in keys):
        tsdf = rng.uniform(-1.0, 1.0, (U, U, U)).astype(f32)
        tsdf[rng.random((U, U, U)) < 0.05] = f32(0)     # coincident vertices
        tsdf[rng.random((U, U, U)) < 0.02] = f32(-0.0)  # not < 0: a corner outside the surface
        wgt = (rng.random((U, U, U)) >= zero_weights).astype(f32) * f32(2)
        col = None
        if color_type == T.RGB8:
            col = rng.integers(0, 256, (U, U, U, 3)).astype(np.float64)
        elif color_type == T.GRAY32:
            col = np.repeat(rng.random((U, U, U, 1)), 3, axis=3)
            col[rng.random((U, U, U)) < 0.1] = np.nan
        blocks[b] = (tsdf, wgt, col)
    return SR.volume_of_blocks(vl, trunc, color_type, blocks)


L_SHAPE = [(-1, -1, -1), (0, -1, -1), (-1, 0, -1), (-1, -1, 0), (0, 0, -1), (0, -1, 0), (-1, 0, 0)]  # 2 x 2 x 2 without (0, 0, 0)
CUBE_2 = [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]

# name -> (keys, seed, colour type): one block, two blocks adjacent along each axis, 2 x 2 x 2 blocks, the L shape with
# its corner block missing, far apart; negative block indices throughout
RANDOM_SETS = {
    "one": ([(-3, 2, -1)], 21, T.GRAY32),
    "pair_x": ([(-1, 0, 0), (0, 0, 0)], 22, T.RGB8),
    "pair_y": ([(2, -2, 1), (2, -1, 1)], 23, T.NONE),
    "pair_z": ([(0, 0, -1), (0, 0, 0)], 24, T.GRAY32),
    "cube_2": ([(x - 1, y - 1, z - 1) for x, y, z in CUBE_2], 25, T.RGB8),
    "l_shape": (L_SHAPE, 26, T.GRAY32),
}

# the fixture scenes of stsdf_reference.cases() the parity tests run on
FIXTURES = ("none_7", "gray_7", "rgb_7_wide_stride", "rgb_64", "gray_64_stride1", "far", "nothing", "empty")

_volumes, _results = {}, {}


def random_set(name):
    if name not in _volumes:
        keys, seed, ctype = RANDOM_SETS[name]
        _volumes[name] = random_blocks(keys, seed, ctype)
    return _volumes[name]


def volume(name):
    """The volume of a fixture scene or of a random set."""
    return random_set(name) if name in RANDOM_SETS else S.result(name).vol


def result(name, normals=True):
    """The mesh of a fixture scene or a random set, computed once and left unchanged."""
    if (name, normals) not in _results:
        m = extract_triangle_mesh(volume(name), normals)
        for a in (m.vertices, m.colors, m.normals, m.triangles):
            if a is not None:
                a.setflags(write=False)
        _results[(name, normals)] = m
    return _results[(name, normals)]


def corner_cube_volume(pattern, missing=None, color_type=T.NONE, vl=0.02, trunc=0.06):
    """Eight blocks {-1, 0}^3 (without `missing`) in which only the cube at local (15, 15, 15) of block (-1, -1, -1) has
    observed corners -- its eight corners lie in the eight blocks -- with sign pattern `pattern` (bit i: corner i < 0)."""
    blocks = {}
    for i, (dx, dy, dz) in enumerate(SHIFT):
        b = (dx - 1, dy - 1, dz - 1)
        if b == missing:
            continue
        tsdf, wgt = np.zeros((U, U, U), dtype=f32), np.zeros((U, U, U), dtype=f32)
        l = tuple(0 if d else U - 1 for d in (dx, dy, dz))
        tsdf[l] = f32(-(0.1 + 0.1 * i)) if (pattern >> i) & 1 else f32(0.15 + 0.05 * i)
        wgt[l] = f32(1 + i)
        col = None
        if color_type == T.RGB8:
            col = np.zeros((U, U, U, 3))
            col[l] = (10.0 * i, 255.0 - 3.0 * i, 7.0 + i)
        blocks[b] = (tsdf, wgt, col)
    return SR.volume_of_blocks(vl, trunc, color_type, blocks)
