"""The numpy restatement of the depth-frame contract of include/teaser_hip.h ("Depth frames"): frames to clouds
(``unproject``) and clouds to frames (``project``), with every float32 and float64 step explicit and in the stated
order.  numpy's elementwise operations round every product and every sum on its own, which is the contract's "no fused
product-add"; parentheses give the order of the sums.

A worked frame (tests/test_rgbd_reference.py pins it).  width = height = 2, uint16, depth_scale = 1000, depth_trunc =
3.0, fx = fy = 2, cx = cy = 0.5, identity pose, samples
    [[1000, 0], [4000, 500]]
* (0, 0): zf = 1000 / 1000 = 1.0; x = ((0 - 0.5) 1.0) / 2 = -0.25, y = -0.25, z = 1.0.
* (0, 1): zf = 0: invalid.
* (1, 0): zf = 4.0 >= 3.0, truncated to 0: invalid.
* (1, 1): zf = 0.5; x = ((1 - 0.5) 0.5) / 2 = 0.125, y = 0.125, z = 0.5.
valid_only = 1: count 2, points (-0.25, -0.25, 1), (0.125, 0.125, 0.5), pixels 0, 3.  valid_only = 0: count 4, rows 1 and
2 are NaN.  Projecting the two points back with the same camera and depth_scale = 1000: u = (2 -0.25) / 1 + 0.5 = 0,
v = 0, d = 1000 at pixel (0, 0); u = (2 0.125) / 0.5 + 0.5 = 1, v = 1, d = 500 at pixel (1, 1): the depth image
[[1000, 0], [0, 500]], the index image [[0, -1], [-1, 1]], n_hit 2.

TEST INFRASTRUCTURE ONLY."""
import numpy as np

F32, F64 = np.float32, np.float64
QNAN = np.nan  # 0x7ff8000000000000: what a NaN component is stored as


class Frame:
    """teaser_icp_frame_c without the layout fields (the arrays carry formats and row bytes)."""

    def __init__(self, fx, fy, cx, cy, pose=None, depth_scale=1000.0, depth_trunc=1000.0, stride=1, valid_only=1,
                 intensity=0):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.pose = np.eye(4) if pose is None else np.array(pose, dtype=F64).reshape(4, 4)
        self.depth_scale, self.depth_trunc = float(depth_scale), float(depth_trunc)
        self.stride, self.valid_only, self.intensity = int(stride), int(valid_only), int(intensity)

    def but(self, **kw):
        f = Frame(self.fx, self.fy, self.cx, self.cy, self.pose, self.depth_scale, self.depth_trunc, self.stride,
                  self.valid_only, self.intensity)
        for k, v in kw.items():
            assert hasattr(f, k), k
            setattr(f, k, v)
        return f


class Camera:
    """teaser_icp_projection_c."""

    def __init__(self, width, height, fx, fy, cx, cy, extrinsic=None, depth_scale=1000.0, depth_max=3.0):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.extrinsic = np.eye(4) if extrinsic is None else np.array(extrinsic, dtype=F64).reshape(4, 4)
        self.depth_scale, self.depth_max = float(depth_scale), float(depth_max)


def color_format(color):
    """0 none, 1 uint8 x 3, 2 float32 x 1, 3 float32 x 3."""
    if color is None:
        return 0
    if color.dtype == np.uint8:
        assert color.ndim == 3 and color.shape[2] == 3
        return 1
    assert color.dtype == F32
    return 2 if color.ndim == 2 else 3


def canonical(a):
    a = np.array(a, dtype=F64)
    a[np.isnan(a)] = QNAN
    return a


def depth_as_float(depth, f):
    """zf of every sample, float32."""
    with np.errstate(all="ignore"):
        if depth.dtype == np.uint16:
            zf = depth.astype(F32) / F32(f.depth_scale)
            assert zf.dtype == F32
            zf[zf.astype(F64) >= f.depth_trunc] = F32(0.0)
            return zf
        assert depth.dtype == F32
        return depth.copy()


def colors_of(color, fmt, intensity):
    """n x 3 float64 of the pixels `color` (n x 3, or n for format 2) of a colour image of format `fmt`."""
    with np.errstate(all="ignore"):
        if fmt == 1 and intensity:
            r, g, b = (color[..., k].astype(F32) for k in range(3))
            i = ((F32(0.2990) * r + F32(0.5870) * g) + F32(0.1140) * b) / F32(255.0)
            assert i.dtype == F32
            return canonical(np.repeat(i.astype(F64).reshape(-1, 1), 3, axis=1))
        if fmt == 1:
            return color.astype(F64).reshape(-1, 3) / 255.0
        if fmt == 2:
            return canonical(np.repeat(color.astype(F64).reshape(-1, 1), 3, axis=1))
        return canonical(color.astype(F64).reshape(-1, 3))


def unproject(depth, color, f):
    """(count, points count x 3, colours count x 3 or None, pixels count int32)."""
    h, w = depth.shape
    ii, jj = np.meshgrid(np.arange(0, h, f.stride), np.arange(0, w, f.stride), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()  # the visiting order
    zf = depth_as_float(depth, f)[ii, jj] if len(ii) else np.zeros(0, dtype=F32)
    valid = zf > 0
    with np.errstate(all="ignore"):
        z = zf.astype(F64)
        x = ((jj.astype(F64) - f.cx) * z) / f.fx
        y = ((ii.astype(F64) - f.cy) * z) / f.fy
        M = f.pose
        P = np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], axis=1)
    P = canonical(P.reshape(-1, 3))
    P[~valid] = QNAN
    C = colors_of(color[ii, jj], color_format(color), f.intensity) if color is not None else None
    pix = (ii * w + jj).astype(np.int32)
    if f.valid_only:
        P, pix = P[valid], pix[valid]
        C = C[valid] if C is not None else None
    return len(P), P, C, pix


def round_half_away(u):
    a = np.abs(u)
    fl = np.floor(a)
    return np.copysign(fl + ((a - fl) >= 0.5), u)


def project(points, colors, cam):
    """(depth h x w float32, colour h x w x 3 float32 or None, index h x w int32, n_hit)."""
    P = np.asarray(points, dtype=F64).reshape(-1, 3)
    n, w, h = len(P), cam.width, cam.height
    E = cam.extrinsic
    keys = np.full(w * h, np.iinfo(np.uint64).max, dtype=np.uint64)
    with np.errstate(all="ignore"):
        c = [((E[r, 0] * P[:, 0] + E[r, 1] * P[:, 1]) + E[r, 2] * P[:, 2]) + E[r, 3] for r in range(3)]
        zc = c[2]
        keep = (zc > 0) & (zc <= cam.depth_max)
        u = (cam.fx * c[0]) / zc + cam.cx
        v = (cam.fy * c[1]) / zc + cam.cy
        keep &= np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 2.0 ** 31) & (np.abs(v) < 2.0 ** 31)
        ur, vr = round_half_away(u), round_half_away(v)
        keep &= (ur >= 0) & (ur < w) & (vr >= 0) & (vr < h)
        d = (zc * cam.depth_scale).astype(F32)
        keep &= np.isfinite(d)
    k = np.flatnonzero(keep)
    pix = vr[k].astype(np.int64) * w + ur[k].astype(np.int64)
    key = (d[k].view(np.uint32).astype(np.uint64) << np.uint64(32)) | k.astype(np.uint64)
    np.minimum.at(keys, pix, key)
    hit = keys != np.iinfo(np.uint64).max
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(0.0)).astype(F32)
    index = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    cimg = None
    if colors is not None:
        C = np.asarray(colors, dtype=F64).reshape(-1, 3)
        cimg = np.zeros((w * h, 3), dtype=F32)
        cimg[hit] = C[index[hit]].astype(F32)
        cimg = cimg.reshape(h, w, 3)
    return depth.reshape(h, w), cimg, index.reshape(h, w), int(hit.sum())


def project_scalar(points, cam):
    """The projection again, one point at a time in Python floats: (depth, index) by the (d, k) rule."""
    import math
    import struct
    w, h, E = cam.width, cam.height, cam.extrinsic
    best = {}
    for k, (X, Y, Z) in enumerate(np.asarray(points, dtype=F64).reshape(-1, 3).tolist()):
        c = [((E[r, 0] * X + E[r, 1] * Y) + E[r, 2] * Z) + E[r, 3] for r in range(3)]
        zc = float(c[2])
        if not (zc > 0 and zc <= cam.depth_max):
            continue
        u, v = (cam.fx * float(c[0])) / zc + cam.cx, (cam.fy * float(c[1])) / zc + cam.cy
        if not (math.isfinite(u) and math.isfinite(v) and abs(u) < 2.0 ** 31 and abs(v) < 2.0 ** 31):
            continue
        ui = math.copysign(math.floor(abs(u)) + (1 if abs(u) - math.floor(abs(u)) >= 0.5 else 0), u)
        vi = math.copysign(math.floor(abs(v)) + (1 if abs(v) - math.floor(abs(v)) >= 0.5 else 0), v)
        if not (0 <= ui < w and 0 <= vi < h):
            continue
        try:
            d = struct.unpack("f", struct.pack("f", zc * cam.depth_scale))[0]
        except OverflowError:
            continue
        if not math.isfinite(d):
            continue
        px = int(vi) * w + int(ui)
        if px not in best or (d, k) < best[px]:
            best[px] = (d, k)
    depth, index = np.zeros(w * h, dtype=F32), np.full(w * h, -1, dtype=np.int32)
    for px, (d, k) in best.items():
        depth[px], index[px] = d, k
    return depth.reshape(h, w), index.reshape(h, w)


# ---- the cases the host driver and the GPU tests share ------------------------------------------------------------------
def pose(seed=3):
    """A rotation about a skew axis with a translation."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, rng.normal(size=3)
    return T


def padded(a, extra, fill):
    """A view of `a` whose rows lie `extra` elements apart more than they are long (what a cropped image is)."""
    big = np.full((a.shape[0], a.shape[1] + extra) + a.shape[2:], fill, dtype=a.dtype)
    big[:, :a.shape[1]] = a
    view = big[:, :a.shape[1]]
    assert view.strides[0] > a.strides[0] and np.array_equal(view, a, equal_nan=a.dtype.kind == "f")
    return view


def random_depth(rng, w, h):
    """uint16 samples of which about a third are 0 and some lie beyond 3 m."""
    d = rng.integers(200, 4000, size=(h, w)).astype(np.uint16)
    d[rng.random((h, w)) < 0.3] = 0
    return d


def random_color(rng, w, h, fmt):
    if fmt == 0:
        return None
    if fmt == 1:
        return rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    return rng.random((h, w) if fmt == 2 else (h, w, 3)).astype(F32)


def unproject_cases():
    """[(name, depth, colour or None, Frame)].  Frame shapes: 1 x 1; 7 x 5 at strides 1, 2, 3; 64 x 4 (one tile of 256);
    257 x 1 and 1 x 257 (one past a tile); 65 x 9 (three tiles, the last one partial) all valid, none valid, a
    checkerboard, only the last pixel valid.  Depth values at the truncation boundary; float32 frames with NaN, -1, a
    subnormal and +inf.  Padded rows, every colour format with and without intensity, a pose, valid_only 0 and 1."""
    rng = np.random.default_rng(2031)
    base = Frame(525.0, 520.0, 3.25, 2.5, depth_scale=1000.0, depth_trunc=3.0)
    T = pose()
    out = [("1x1", np.array([[1234]], dtype=np.uint16), None, base)]
    for s in (1, 2, 3):
        out.append(("7x5_stride%d" % s, random_depth(rng, 7, 5), random_color(rng, 7, 5, 1), base.but(stride=s, pose=T)))
    out.append(("64x4_one_tile", random_depth(rng, 64, 4), None, base.but(pose=T)))
    out.append(("257x1", random_depth(rng, 257, 1), random_color(rng, 257, 1, 3), base))
    out.append(("1x257", random_depth(rng, 1, 257), random_color(rng, 1, 257, 2), base.but(pose=T)))
    full = rng.integers(200, 2999, size=(9, 65)).astype(np.uint16)
    board = full.copy()
    board[(np.add.outer(np.arange(9), np.arange(65)) % 2) == 1] = 0
    last = np.zeros((9, 65), dtype=np.uint16)
    last[8, 64] = 777
    for name, d in (("all", full), ("none", np.zeros((9, 65), dtype=np.uint16)), ("checkerboard", board), ("last", last)):
        out.append(("65x9_" + name, d, random_color(rng, 65, 9, 1), base.but(pose=T)))
        out.append(("65x9_%s_every_pixel" % name, d, random_color(rng, 65, 9, 1), base.but(pose=T, valid_only=0)))
    edge = np.array([[0, 2999, 3000, 3001, 65535]], dtype=np.uint16)
    out.append(("truncation", edge, None, base))
    out.append(("truncation_every_pixel", edge, None, base.but(valid_only=0)))
    odd = np.array([[np.nan, -1.0, 1e-45, np.inf, 0.75, 0.0, -0.0, 1e-40]], dtype=F32)
    out.append(("float32_odd", odd, None, base.but(pose=T)))
    out.append(("float32_odd_every_pixel", odd, random_color(rng, 8, 1, 3), base.but(valid_only=0)))
    fl = (rng.random((6, 11)) * 4.0).astype(F32)
    fl[rng.random((6, 11)) < 0.25] = 0.0
    out.append(("float32_beyond_trunc", fl, random_color(rng, 11, 6, 2), base.but(pose=T, stride=2)))
    for fmt in (1, 2, 3):
        for inten in ((0, 1) if fmt == 1 else (0,)):
            out.append(("color%d_intensity%d_padded" % (fmt, inten), padded(random_depth(rng, 13, 7), 3, 9),
                        padded(random_color(rng, 13, 7, fmt), 2, 1), base.but(pose=T, intensity=inten, stride=2 if fmt == 3 else 1)))
    out.append(("0x5", np.zeros((5, 0), dtype=np.uint16), None, base))
    out.append(("5x0", np.zeros((0, 5), dtype=F32), None, base))
    return out


def project_cases():
    """[(name, points, colours or None, Camera)]: no point, one point, points behind the camera, beyond depth_max and at
    it, u at k + 0.5 and at -0.5 (fx = 1, cx = 0.5, zc = 1: the values are exact), duplicated points, 1 000 points on one
    pixel, images of 3 x 2 and 65 x 33, with and without colours."""
    rng = np.random.default_rng(2032)
    none = np.zeros((0, 3))
    out = [("n0", none, None, Camera(3, 2, 2.0, 2.0, 1.0, 0.5)),
           ("one", np.array([[0.1, -0.2, 1.5]]), np.array([[0.25, 0.5, 0.75]]), Camera(3, 2, 2.0, 2.0, 1.0, 1.0))]
    cam = Camera(3, 2, 1.0, 1.0, 0.5, 0.5, depth_scale=1000.0, depth_max=3.0)
    z = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 3.0], [1.0, 0.0, np.nextafter(3.0, 4.0)], [2.0, 1.0, 1.0],
                  [0.0, 0.0, 3.5]])
    out.append(("depth_limits", z, rng.random((6, 3)), cam))
    # u = x + 0.5 exactly: -1 -> -0.5 (rounds to -1: outside), 0 -> 0.5 (rounds to 1), 1 -> 1.5 (2), 2 -> 2.5 (3: outside)
    halves = np.array([[-1.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0.0, -1.0, 1.0], [0.0, 1.0, 1.0]])
    out.append(("halves", halves, None, cam))
    dup = np.tile(np.array([[0.25, 0.25, 2.0]]), (7, 1))
    dup = np.vstack([np.array([[0.25, 0.25, 2.5]]), dup, np.array([[0.25, 0.25, 2.0 + 1e-9]])])  # the last rounds to the same float
    out.append(("duplicates", dup, rng.random((9, 3)), Camera(3, 2, 2.0, 2.0, 1.0, 0.5)))
    crowd = np.column_stack([rng.normal(size=1000) * 10, rng.normal(size=1000) * 10, rng.integers(1, 40, size=1000) / 16.0])
    out.append(("crowd_1x1", crowd, rng.random((1000, 3)), Camera(1, 1, 1e-4, 1e-4, 0.0, 0.0)))
    T = np.linalg.inv(pose(5))
    cloud = np.column_stack([rng.random(3000) * 2 - 1, rng.random(3000) * 1.2 - 0.6, rng.random(3000) * 3 + 0.5])
    world = (np.linalg.inv(T) @ np.column_stack([cloud, np.ones(3000)]).T).T[:, :3]
    out.append(("65x33", world, rng.random((3000, 3)), Camera(65, 33, 40.0, 38.0, 31.5, 16.25, T, 1000.0, 3.0)))
    out.append(("65x33_no_colour", world[:700], None, Camera(65, 33, 40.0, 38.0, 31.5, 16.25, T, 1000.0, 3.0)))
    out.append(("3x2", cloud[:50] * [1.0, 1.0, 1.0], rng.random((50, 3)), Camera(3, 2, 2.0, 2.0, 1.0, 0.5)))
    out.append(("0x4", cloud[:5], None, Camera(0, 4, 2.0, 2.0, 1.0, 0.5)))
    return out


def round_trip_frame():
    """A uint16 frame whose round trip is exact: fx, fy and depth_scale powers of two, cx and cy integers, identity pose.
    x = ((j - cx) z) / fx and u = (fx x) / z + cx lose nothing when z = d / 2^k has few bits: every product and quotient
    here is a dyadic number of fewer than 53 bits."""
    rng = np.random.default_rng(2033)
    w, h = 37, 21
    d = rng.integers(1, 2048, size=(h, w)).astype(np.uint16)
    d[rng.random((h, w)) < 0.2] = 0
    d[0, 0] = 4095  # beyond the truncation
    f = Frame(32.0, 64.0, 18.0, 10.0, depth_scale=1024.0, depth_trunc=3.0)
    cam = Camera(w, h, 32.0, 64.0, 18.0, 10.0, None, 1024.0, 3.0)
    return d, f, cam


WIDE_BATCH = 320
TILE = 256  # pixels per tile of the unprojection's tile maps


def wide_batch():
    """(frames, clouds): for each of 320 problems the index of its case in unproject_cases() and in project_cases(), the
    lists in turn -- every shape (1 x 1, 7 x 5 at three strides, 64 x 4, 257 x 1, 65 x 9, the empty ones), both depth
    types and every colour variant recur about eleven times.  What the wide test rests on is asserted from the sizes
    alone."""
    ucases, pcases = unproject_cases(), project_cases()
    frames = [i % len(ucases) for i in range(WIDE_BATCH)]
    clouds = [i % len(pcases) for i in range(WIDE_BATCH)]
    assert WIDE_BATCH > 256
    tiles = sum((ucases[k][1].size + TILE - 1) // TILE for k in frames)
    assert tiles > 256  # d_tile_frame and d_tile_prob past 256 entries (a strided frame may need fewer tiles: 16 cases)
    assert sum((ucases[k][1].shape[1] * ucases[k][1].shape[0] + TILE - 1) // TILE
               for k in frames if ucases[k][3].stride == 1) > 256
    assert {ucases[k][1].dtype for k in frames} == {np.dtype(np.uint16), np.dtype(F32)}
    assert {ucases[k][3].stride for k in frames} == {1, 2, 3}
    assert any(len(pcases[k][1]) >= 1000 and pcases[k][3].width == 1 for k in clouds[256:])  # the race for one pixel
    return frames, clouds
