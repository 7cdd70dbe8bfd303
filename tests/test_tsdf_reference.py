"""tests/tsdf_reference.py pinned by hand: every number below is worked out from the text of include/teaser_hip.h
("TSDF volume") on inputs small enough to follow, so that the restatement the host and GPU tests compare with cannot drift
along with the code under test."""
import importlib

import numpy as np

import tsdf_reference as T

tp = importlib.import_module("teaser-plusplus_amd")
f32 = np.float32


def test_two_frames_into_a_two_voxel_cube():
    """length 2, R = 2, origin (-1, -1, 1): voxel centres x, y in {-0.5, 0.5}, z in {1.5, 2.5}.  Identity extrinsic,
    fx = fy = 2, cx = cy = 0.5 on a 2 x 2 frame: u_f = 2 c_0 / c_2 + 1, which is 1/3, 0.6 for x = 0 (u = 0) and 5/3, 1.4
    for x = 1 (u = 1) at z = 0, 1; likewise v = y.  xx, yy = +-0.25, so m = sqrtf(1.125) for every pixel; trunc 1."""
    vol = T.Volume(2.0, 2, 1.0, T.NONE, (-1.0, -1.0, 1.0))
    K = (2.0, 2.0, 0.5, 0.5)
    m = np.sqrt(f32(1.125))
    assert m.dtype == f32
    d1 = np.array([[2.0, 2.0], [1.0, 0.0]], dtype=f32)  # d1[v, u]
    vol.integrate(d1, K, np.eye(4))
    a, b = f32(0.5) * m, f32(-0.5) * m  # sdf = (d - c_2) m with d - c_2 = +-0.5
    # [x, y, z]: pixel (v = y, u = x); depth 2 for y = 0, depth 1 for (x 0, y 1), none for (x 1, y 1)
    want = np.zeros((2, 2, 2), dtype=f32)
    want[0, 0] = want[1, 0] = [a, b]    # 2 - 1.5, 2 - 2.5
    want[0, 1] = [b, 0.0]               # 1 - 1.5; (1 - 2.5) m = -1.59 <= -trunc: skipped
    wgt = np.array([[[1, 1], [1, 0]], [[1, 1], [0, 0]]], dtype=f32)
    assert vol.tsdf.tobytes() == want.tobytes() and vol.weight.tobytes() == wgt.tobytes()
    vol.integrate(np.full((2, 2), 3.0, dtype=f32), K, np.eye(4))  # sdf = 1.5 m (t clamps to 1) and 0.5 m
    one = f32(1.0)
    want2 = np.zeros((2, 2, 2), dtype=f32)
    want2[0, 0] = want2[1, 0] = [(a * one + one) / f32(2.0), (b * one + a) / f32(2.0)]
    want2[0, 1] = [(b * one + one) / f32(2.0), a]   # the voxel the first frame skipped starts from weight 0
    want2[1, 1] = [one, a]
    assert vol.tsdf.tobytes() == want2.tobytes()
    assert vol.weight.tobytes() == (wgt + one).tobytes()
    assert vol.tsdf_weight()[5].tolist() == [float(want2[1, 0, 1]), 2.0]  # Open3D's order (x R + y) R + z


def one_voxel(cx, d, width=1, trunc=0.25, fmt=f32):
    """R = 1 with its centre at (0, 0, 1) seen by the identity camera with fx = fy = 1, cy = 0: c = (0, 0, 1),
    u_f = cx + 0.5, v_f = 0.5.  Returns (tsdf, weight)."""
    vol = T.Volume(1.0, 1, trunc, T.NONE, (-0.5, -0.5, 0.5))
    vol.integrate(np.full((1, width), d, dtype=fmt), (1.0, 1.0, cx, 0.0), np.eye(4))
    return float(vol.tsdf[0, 0, 0]), float(vol.weight[0, 0, 0])


def test_the_image_bounds():
    # the lower bound: the smallest float32 cx whose u_f = cx + 0.5f reaches 0.0001f is taken, the one below is not
    cx = f32(-0.4999)
    while f32(cx) + f32(0.5) >= f32(0.0001):
        cx = np.nextafter(cx, f32(-1.0))
    assert f32(cx) + f32(0.5) < f32(0.0001) <= np.nextafter(cx, f32(0.0)) + f32(0.5)
    assert one_voxel(float(cx), 1.0)[1] == 0.0 and one_voxel(float(np.nextafter(cx, f32(0.0))), 1.0)[1] == 1.0
    # the upper bound on a frame 4 wide: u_f < safe_w = 4.0f - 0.0001f
    safe_w = f32(4.0) - f32(0.0001)
    cx = f32(3.4999)
    while f32(cx) + f32(0.5) < safe_w:
        cx = np.nextafter(cx, f32(4.0))
    assert one_voxel(float(cx), 1.0, width=4)[1] == 0.0
    assert one_voxel(float(np.nextafter(cx, f32(0.0))), 1.0, width=4)[1] == 1.0   # u = 3, the last column
    assert one_voxel(0.25, 1.0)[1] == 1.0 and one_voxel(float("nan"), 1.0)[1] == 0.0   # a NaN skips


def test_truncation_and_the_clamp():
    # u = 0 = cx: xx = yy = 0, m = 1, sdf = d - 1
    assert one_voxel(0.0, 0.75) == (0.0, 0.0)                      # sdf == -trunc_f: skipped
    up = float(np.nextafter(f32(0.75), f32(1.0)))
    t, w = one_voxel(0.0, up)
    assert w == 1.0 and t == float((f32(up) - f32(1.0)) * f32(4.0)) and -1.0 < t < 0.0
    assert one_voxel(0.0, 3.0) == (1.0, 1.0)                       # sdf inv_f = 8: clamped
    assert one_voxel(0.0, 1.125) == (0.5, 1.0)
    assert one_voxel(0.0, 0.0)[1] == 0.0 and one_voxel(0.0, -1.0)[1] == 0.0 and one_voxel(0.0, np.nan)[1] == 0.0
    assert one_voxel(0.0, np.inf) == (1.0, 1.0)                    # +inf is a valid float32 sample
    # uint16: 1125 / 1000 in float32, and zero at or beyond depth_trunc
    assert one_voxel(0.0, 1125, fmt=np.uint16)[0] == float((f32(1125.0) / f32(1000.0) - f32(1.0)) * f32(4.0))
    vol = T.Volume(1.0, 1, 0.25, T.NONE, (-0.5, -0.5, 0.5))
    vol.integrate(np.full((1, 1), 1125, dtype=np.uint16), (1.0, 1.0, 0.0, 0.0), np.eye(4), depth_trunc=float(f32(1125.0) / f32(1000.0)))
    assert vol.weight[0, 0, 0] == 0.0


def test_colour_averages_in_double():
    vol = T.Volume(1.0, 1, 0.25, T.RGB8, (-0.5, -0.5, 0.5))
    K = (1.0, 1.0, 0.0, 0.0)
    for rgb in ([10, 20, 30], [11, 20, 250], [12, 21, 0]):
        vol.integrate(np.full((1, 1), 1.0, dtype=f32), K, np.eye(4), np.array([[rgb]], dtype=np.uint8))
    want = [((10.0 * 1.0 + 11.0) / 2.0 * 2.0 + 12.0) / 3.0, ((20.0 + 20.0) / 2.0 * 2.0 + 21.0) / 3.0,
            ((30.0 + 250.0) / 2.0 * 2.0 + 0.0) / 3.0]
    assert vol.color[0, 0, 0].tolist() == want and vol.weight[0, 0, 0] == 3.0
    g = T.Volume(1.0, 1, 0.25, T.GRAY32, (-0.5, -0.5, 0.5))
    g.integrate(np.full((1, 1), 1.0, dtype=f32), K, np.eye(4), np.array([[0.3]], dtype=f32))
    assert g.color[0, 0, 0].tolist() == [float(f32(0.3))] * 3


def line_volume(values):
    """R = 4, vl = 1: only the voxels (x, 0, 0) are observed, with the given values."""
    vol = T.Volume(4.0, 4, 1.0, T.NONE)
    vol.tsdf[:, 0, 0] = values
    vol.weight[:, 0, 0] = 1.0
    return vol


def test_the_neighbour_rule():
    """Signs alternate along x: the crossings 0-1 and 1-2 are emitted, 2-3 is not (the neighbour's index 3 is not
    < R - 1)."""
    vol = line_volume([0.5, -0.5, 0.5, -0.5])
    assert vol.surface_rows().tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]]
    assert line_volume([0.5, -0.5, 0.99, -0.5]).surface_rows().tolist() == [[0, 0, 0, 0]]   # 0.99 is not < 0.98
    assert line_volume([0.5, -0.98, 0.5, 0.5]).surface_rows().tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]]  # -0.98 is usable
    vol = line_volume([0.5, -0.5, 0.5, -0.5])
    vol.weight[1, 0, 0] = 0.0
    assert len(vol.surface_rows()) == 0
    assert len(T.Volume(2.0, 2, 1.0).surface_rows()) == 0 and len(T.Volume(1.0, 1, 1.0).surface_rows()) == 0


def slab(color_type=T.RGB8):
    """R = 4, vl = 1, origin (10, 20, 30): +0.5 for x <= 1; behind it -0.25 on the row y = 0 and -0.5 elsewhere."""
    vol = T.Volume(4.0, 4, 1.0, color_type, (10.0, 20.0, 30.0))
    vol.weight[:] = 1.0
    vol.tsdf[:2] = 0.5
    vol.tsdf[2:] = -0.5
    vol.tsdf[2:, 0, :] = -0.25
    vol.color[:2] = [30.0, 60.0, 90.0]
    vol.color[2:] = [60.0, 90.0, 120.0]
    return vol


def test_one_point_its_colour_and_its_normal():
    vol = slab()
    rows = vol.surface_rows().tolist()
    # the crossing between x = 1 and x = 2 in every (y, z); along y between y = 0 and 1 nothing (same sign)
    assert rows == [[1, y, z, 0] for y in range(4) for z in range(4)]
    P, N, C = vol.extract_point_cloud()
    k = rows.index([1, 2, 1, 0])                    # r0 = 0.5, r1 = 0.5 in the rows y >= 1
    assert P[k].tolist() == [(1.5 * 0.5 + 2.5 * 0.5) / 1.0 + 10.0, 2.5 + 20.0, 1.5 + 30.0]
    assert C[k].tolist() == [((c0 * 0.5 + c1 * 0.5) / 1.0) / 255.0 for c0, c1 in ((30.0, 60.0), (60.0, 90.0), (90.0, 120.0))]
    # T along x: 0.5 left of the surface at distance 0.99, -0.5 right of it; along y and z the field is the same on
    # both sides: the normal is (-1, 0, 0)
    assert np.abs(N[k] - [-1.0, 0.0, 0.0]).max() < 1e-12
    k = rows.index([1, 0, 0, 0])                    # r0 = 0.5, r1 = 0.25
    px = (1.5 * 0.25 + 2.5 * 0.5) / 0.75
    assert P[k].tolist() == [px + 10.0, 0.5 + 20.0, 0.5 + 30.0]
    assert C[k].tolist() == [((c0 * 0.25 + c1 * 0.5) / 0.75) / 255.0 for c0, c1 in ((30.0, 60.0), (60.0, 90.0), (90.0, 120.0))]


def test_a_normal_at_the_edge_counts_outside_corners_as_zero():
    vol = slab(T.NONE)
    # a corner outside: at q = (0.25, 0.25, 0.25) only voxel (0, 0, 0) is inside, with weight 0.75^3
    assert vol.trilinear(np.array([[0.25, 0.25, 0.25]]))[0] == ((0.75 * 0.75) * 0.75) * 0.5
    assert vol.trilinear(np.array([[3.75, 3.75, 3.75]]))[0] == ((0.75 * 0.75) * 0.75) * -0.5   # corner 000 alone
    assert vol.trilinear(np.array([[3.75, 0.5, 3.5]]))[0] == ((0.75 * 1.0) * 1.0) * -0.25
    P, N, C = vol.extract_point_cloud()
    assert C is None
    k = vol.surface_rows().tolist().index([1, 0, 0, 0])
    px = (1.5 * 0.25 + 2.5 * 0.5) / 0.75            # 2.1666..., a_x = 1.6666...: between voxels x = 1 and 2
    r = px - 0.5 - 1.0
    # n_y: below the row y = 0 the corners y = -1 are outside (0) and y = 0 weighs 0.01; above, y = 0 weighs 0.01 and
    # y = 1 weighs 0.99.  x-interpolation: row 0 gives (1 - r) 0.5 - r 0.25 (about 0), row 1 gives (1 - r) 0.5 - r 0.5.
    row0, row1 = (1.0 - r) * 0.5 + r * -0.25, (1.0 - r) * 0.5 + r * -0.5
    ny = (0.01 * row0 + 0.99 * row1) - 0.01 * row0
    # n_x: T at a_x = 1.6666 +- 0.99 on the row y = 0, z = 0 alone (a_y = a_z = 0)
    hi, lo = r + 0.99 - 1.0, r - 0.99 + 1.0         # fractions in the cells x = 2 .. 3 and x = 0 .. 1
    nx = ((1.0 - hi) * -0.25 + hi * -0.25) - ((1.0 - lo) * 0.5 + lo * 0.5)
    nz = 0.0                                        # z = -1 is outside as well, but the row's own value there is ~0
    n = np.array([nx, ny, nz])
    assert np.abs(N[k] - n / np.linalg.norm(n)).max() < 1e-9
    assert abs(np.linalg.norm(N[k]) - 1.0) < 1e-12 and N[k][1] < -0.1
    # no observed voxel at all: no rows, and a zero gradient stays (0, 0, 0)
    flat = T.Volume(4.0, 4, 1.0)
    assert flat.extract_point_cloud()[0].shape == (0, 3) and flat.extract_voxel_point_cloud()[0].shape == (0, 3)


def test_the_voxel_cloud():
    vol = line_volume([0.5, -0.5, 0.99, -0.98])
    vol.origin[:] = [1.0, 2.0, 3.0]
    P, C = vol.extract_voxel_point_cloud()
    assert P.tolist() == [[1.5, 2.5, 3.5], [2.5, 2.5, 3.5], [4.5, 2.5, 3.5]]
    assert C.tolist() == [[0.75] * 3, [0.25] * 3, [(float(f32(-0.98)) + 1.0) * 0.5] * 3]


def test_the_running_sum_is_not_a_product():
    """vl = 1/12 is not a binary fraction: twelve-fold addition of s rounds differently from base + z s, and a product
    form would leave other bits in the volume."""
    vol = T.Volume(1.0, 12, 0.2, T.NONE, (-0.5, -0.5, 0.5))
    E_f = T.extrinsic(0.3, -0.2, 0.1, (0.01, 0.02, 0.03)).astype(f32)
    run = {z: [a.copy() for a in c] for z, c in vol.column_points(E_f, True)}
    prod = {z: c for z, c in vol.column_points(E_f, False)}
    assert all(np.array_equal(run[0][r], prod[0][r]) for r in range(3))
    assert any(not np.array_equal(run[z][r], prod[z][r]) for z in range(1, 12) for r in range(3))
    # z additions, one after the other, from the column's start
    s = [E_f[r, 2] * vol.vl_f for r in range(3)]
    c = [a.copy() for a in run[0]]
    for z in range(1, 12):
        c = [c[r] + s[r] for r in range(3)]
        assert all(np.array_equal(c[r], run[z][r]) for r in range(3))
    K = T.camera(64, 48)
    d = T.as_uint16(T.sphere_depth(64, 48, K, (0.0, 0.0, 1.0), 0.3, 1.35))
    a, b = T.Volume(1.0, 12, 0.2, T.NONE, (-0.5, -0.5, 0.5)), T.Volume(1.0, 12, 0.2, T.NONE, (-0.5, -0.5, 0.5))
    a.integrate(d, K, E_f.astype(np.float64))
    b.integrate(d, K, E_f.astype(np.float64), running=False)
    assert a.weight.sum() > 100 and a.tsdf.tobytes() != b.tsdf.tobytes()


def test_the_cases_cover_what_they_claim():
    cs = T.cases()
    assert [cs[n].vol[1] for n in ("r1", "r2", "r5_rgb", "r64", "r65_gray")] == [1, 2, 5, 64, 65]
    assert sorted(len(cs["r16_rgb_%d" % n].frames) for n in (1, 8, 9, 17)) == [1, T.CHUNK, T.CHUNK + 1, 2 * T.CHUNK + 1]
    frames = cs["r16_rgb_17"].frames
    assert {f.depth.dtype for f in frames} == {np.dtype(np.uint16), np.dtype(np.float32)}
    assert any(f.depth.strides[0] > f.depth.shape[1] * f.depth.itemsize for f in frames)          # padded rows
    assert any(f.color.strides[0] > f.color.shape[1] * 3 for f in frames)
    special = frames[1].depth
    assert np.isnan(special).any() and np.isinf(special).any() and (special < 0).any() and (special == 0).any()
    assert any(not f.depth.any() for f in frames)                                                 # sees nothing
    # every frame of the pool is exercised: most touch voxels, the camera behind the volume touches none
    touched = []
    for f in frames[:9]:
        v = T.Volume(*cs["r16_rgb_17"].vol)
        v.integrate(f.depth, f.K, f.E, f.color, f.depth_scale, f.depth_trunc)
        touched.append(int((v.weight > 0).sum()))
    assert touched[5] == 0 and touched[7] == 0 and touched[6] > 0 and min(touched[:5]) > 100, touched
    for name in ("plane", "sphere", "r16_rgb_17", "r65_gray", "r64"):
        r = T.result(name)
        assert len(r.points) > 50 and len(r.vpoints) > len(r.points) / 3, (name, len(r.points))
        assert np.isfinite(r.points).all() and np.isfinite(r.normals).all()
    assert len(T.result("empty").points) == 0 and len(T.result("r1").points) == 0
    # the sphere's points lie on the ball or the wall within a voxel
    r = T.result("sphere")
    dist = np.minimum(np.abs(np.linalg.norm(r.points - [0.0, 0.0, 1.0], axis=1) - 0.3), np.abs(r.points[:, 2] - 1.35))
    assert dist.max() < 1.0 / 16


def test_the_package_exports_the_names():
    for name in ("UniformTSDFVolume", "TSDFVolumeColorType", "TSDFPointCloud"):
        assert name in tp.__all__ and getattr(tp, name) is not None, name
    assert (tp.TSDFVolumeColorType.NoColor, tp.TSDFVolumeColorType.RGB8, tp.TSDFVolumeColorType.Gray32) == (0, 1, 2)
