"""The TSDF volume restated in numpy: the parity target of tests/test_tsdf_host.py and tests/test_gpu_tsdf.py, pinned by
hand in tests/test_tsdf_reference.py.  It follows include/teaser_hip.h ("TSDF volume") line by line: float32 numpy scalars
and arrays where the contract says float32 (numpy rounds every float32 operation once and fuses nothing), float64 where it
says double, and loops where the order matters -- over the frames, along z (the running sum) and over the eight corners
of the trilinear value.  Across voxels nothing depends on order, so those run as arrays.  Arrays are indexed [x, y, z];
their C order is Open3D's voxel order (x R + y) R + z.

The module also holds the scenes and the case lists the host and GPU tests share.
TEST INFRASTRUCTURE ONLY."""
from types import SimpleNamespace

import numpy as np

f32 = np.float32
NONE, RGB8, GRAY32 = 0, 1, 2
CHUNK = 8  # kTsdfChunk of csrc/tsdf_device.h: the frames one pass applies


def depth_as_float(depth, depth_scale, depth_trunc):
    """The depth samples as float32: the rule of "Depth frames"."""
    if depth.dtype == np.uint16:
        zf = depth.astype(f32) / f32(depth_scale)
        zf[zf.astype(np.float64) >= depth_trunc] = f32(0)
        return zf
    return np.array(depth, dtype=f32)


class Volume:
    def __init__(self, length, resolution, sdf_trunc, color_type=NONE, origin=(0.0, 0.0, 0.0)):
        R = self.R = int(resolution)
        self.length, self.sdf_trunc, self.color_type = float(length), float(sdf_trunc), color_type
        self.origin = np.array(origin, dtype=np.float64)
        self.vl = self.length / R
        self.vl_f = f32(self.vl)
        self.half_f = self.vl_f * f32(0.5)
        self.trunc_f = f32(self.sdf_trunc)
        self.inv_f = f32(1.0) / self.trunc_f
        self.org_f = self.origin.astype(f32)
        self.tsdf = np.zeros((R, R, R), dtype=f32)
        self.weight = np.zeros((R, R, R), dtype=f32)
        self.color = np.zeros((R, R, R, 3), dtype=np.float64)

    # ---- integration ----------------------------------------------------------------------------------------
    def column_points(self, E_f, running=True):
        """Per z the camera points (c_0, c_1, c_2) of all columns, each R x R float32.  running=False is the product
        form base + z s, which the contract does NOT use (tests/test_tsdf_reference.py shows that it differs)."""
        R = self.R
        idx = np.arange(R, dtype=f32)
        px = ((self.half_f + self.vl_f * idx) + self.org_f[0])[:, None]
        py = ((self.half_f + self.vl_f * idx) + self.org_f[1])[None, :]
        pz = self.half_f + self.org_f[2]
        base = [((E_f[r, 0] * px + E_f[r, 1] * py) + E_f[r, 2] * pz) + E_f[r, 3] for r in range(3)]
        s = [E_f[r, 2] * self.vl_f for r in range(3)]
        c = [b.copy() for b in base]
        for z in range(R):
            yield z, (c if running else [base[r] + f32(z) * s[r] for r in range(3)])
            c = [c[r] + s[r] for r in range(3)]

    def integrate(self, depth, K, E, color=None, depth_scale=1000.0, depth_trunc=3.0, running=True):
        h, w = depth.shape
        d_img = depth_as_float(depth, depth_scale, depth_trunc)
        E_f = np.asarray(E, dtype=np.float64).astype(f32)
        fx, fy, cx, cy = (f32(v) for v in K)
        inv_fx, inv_fy = f32(1.0) / fx, f32(1.0) / fy
        safe_w, safe_h = f32(w) - f32(0.0001), f32(h) - f32(0.0001)
        if h == 0 or w == 0:
            return
        with np.errstate(all="ignore"):
            for z, (c0, c1, c2) in self.column_points(E_f, running):
                ok = c2 > 0
                u_f = ((c0 * fx) / c2 + cx) + f32(0.5)
                v_f = ((c1 * fy) / c2 + cy) + f32(0.5)
                ok &= (u_f >= f32(0.0001)) & (u_f < safe_w) & (v_f >= f32(0.0001)) & (v_f < safe_h)
                u = np.where(ok, u_f, f32(0)).astype(np.int32)
                v = np.where(ok, v_f, f32(0)).astype(np.int32)
                d = d_img[v, u]
                ok &= d > 0
                xx, yy = (u.astype(f32) - cx) * inv_fx, (v.astype(f32) - cy) * inv_fy
                m = np.sqrt((xx * xx + yy * yy) + f32(1.0))
                sdf = (d - c2) * m
                ok &= sdf > -self.trunc_f
                q = sdf * self.inv_f
                t = np.where(q < f32(1.0), q, f32(1.0))
                wgt = self.weight[:, :, z]
                w1 = wgt + f32(1.0)
                new = (self.tsdf[:, :, z] * wgt + t) / w1
                assert new.dtype == f32 and m.dtype == f32 and u_f.dtype == f32
                if self.color_type != NONE:
                    if self.color_type == RGB8:
                        s = color[v, u, :].astype(np.float64)
                    else:
                        s = np.repeat(color[v, u].astype(np.float64)[:, :, None], 3, axis=2)
                    col = self.color[:, :, z, :]
                    cn = (col * wgt.astype(np.float64)[:, :, None] + s) / w1.astype(np.float64)[:, :, None]
                    if self.color_type == GRAY32:
                        cn = np.where(np.isnan(cn), np.nan, cn)  # THE quiet NaN
                    self.color[:, :, z, :] = np.where(ok[:, :, None], cn, col)
                self.tsdf[:, :, z] = np.where(ok, new, self.tsdf[:, :, z])
                self.weight[:, :, z] = np.where(ok, w1, wgt)

    # ---- the voxels -------------------------------------------------------------------------------------------
    def tsdf_weight(self):
        """R^3 x 2 float32 in Open3D's voxel order."""
        return np.stack([self.tsdf.ravel(), self.weight.ravel()], axis=1)

    def colors(self):
        return self.color.reshape(-1, 3).copy()

    def usable(self):
        return (self.weight != 0) & (self.tsdf < f32(0.98)) & (self.tsdf >= f32(-0.98))

    # ---- extraction -------------------------------------------------------------------------------------------
    def trilinear(self, q):
        """T(q) for the rows of q (n x 3, volume coordinates)."""
        R = self.R
        a = q / self.vl - 0.5
        fl = np.floor(a)
        r = a - fl
        idx = fl.astype(np.int64)
        total = None
        for corner in range(8):  # 000, 001, ..., 111 as (x y z) offsets
            off = np.array([corner >> 2, (corner >> 1) & 1, corner & 1])
            at = idx + off
            inside = ((at >= 0) & (at < R)).all(axis=1)
            safe = np.clip(at, 0, R - 1)
            f = np.where(inside, self.tsdf[safe[:, 0], safe[:, 1], safe[:, 2]], f32(0)).astype(np.float64)
            wgt = [r[:, k] if off[k] else 1.0 - r[:, k] for k in range(3)]
            term = ((wgt[0] * wgt[1]) * wgt[2]) * f
            total = term if total is None else total + term
        return total

    def surface_rows(self):
        """The (x, y, z, i) of every emitted row, in Open3D's order."""
        R, f, ok = self.R, self.tsdf, self.usable()
        mask = np.zeros((R, R, R, 3), dtype=bool)
        n = max(R - 2, 0)  # voxels whose neighbour's index along the axis is < R - 1
        for i in range(3):
            s0, s1 = [slice(None)] * 3, [slice(None)] * 3
            s0[i], s1[i] = slice(0, n), slice(1, n + 1)
            s0, s1 = tuple(s0), tuple(s1)
            mask[s0 + (i,)] = ok[s0] & ok[s1] & (f[s0] * f[s1] < 0)
        return np.argwhere(mask)

    def extract_point_cloud(self, normals=True):
        """(points, normals or None, colors or None)."""
        rows = self.surface_rows()
        n = len(rows)
        x, y, z, i = rows.T if n else (np.zeros(0, dtype=np.int64),) * 4
        e = np.eye(3, dtype=np.int64)[i] if n else np.zeros((0, 3), dtype=np.int64)
        f0, f1 = self.tsdf[x, y, z], self.tsdf[x + e[:, 0], y + e[:, 1], z + e[:, 2]]
        r0, r1 = np.abs(f0), np.abs(f1)
        den = (r0 + r1).astype(np.float64)
        r0, r1 = r0.astype(np.float64), r1.astype(np.float64)
        half = self.vl * 0.5
        p = np.stack([half + self.vl * x.astype(np.float64), half + self.vl * y.astype(np.float64),
                      half + self.vl * z.astype(np.float64)], axis=1).reshape(n, 3)
        k = np.arange(n)
        p0 = p[k, i]
        p[k, i] = (p0 * r1 + (p0 + self.vl) * r0) / den
        points = p + self.origin
        colors = None
        if self.color_type != NONE:
            c0, c1 = self.color[x, y, z], self.color[x + e[:, 0], y + e[:, 1], z + e[:, 2]]
            colors = (c0 * r1[:, None] + c1 * r0[:, None]) / den[:, None]
            if self.color_type == RGB8:
                colors = colors / 255.0
            else:
                colors = np.where(np.isnan(colors), np.nan, colors)
        nrm = None
        if normals:
            g = 0.99 * self.vl
            nrm = np.zeros((n, 3))
            for a in range(3):
                hi, lo = p.copy(), p.copy()
                hi[:, a] = p[:, a] + g
                lo[:, a] = p[:, a] - g
                nrm[:, a] = self.trilinear(hi) - self.trilinear(lo) if n else 0.0
            s = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
            with np.errstate(all="ignore"):
                nrm = np.where((s > 0)[:, None], nrm / np.sqrt(s)[:, None], nrm)
        return points, nrm, colors

    def extract_voxel_point_cloud(self):
        at = np.argwhere(self.usable())
        half = self.vl * 0.5
        points = (half + self.vl * at.astype(np.float64)) + self.origin
        c = (self.tsdf[at[:, 0], at[:, 1], at[:, 2]].astype(np.float64) + 1.0) * 0.5
        return points.reshape(-1, 3), np.repeat(c[:, None], 3, axis=1).reshape(-1, 3)


# ---- scenes and cases -----------------------------------------------------------------------------------------------
def camera(w, h):
    """(fx, fy, cx, cy) of the cases' cameras."""
    return (0.9 * w, 0.85 * w, (w - 1) / 2.0, (h - 1) / 2.0)


def extrinsic(rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0)):
    """World to camera: rotations about x, y, z (radians), then the translation."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    E = np.eye(4)
    E[:3, :3] = Rz @ Ry @ Rx
    E[:3, 3] = t
    return E


def sphere_depth(w, h, K, centre, radius, wall):
    """Metres, float64: per pixel the nearer of a sphere and the wall z = wall, seen from the camera's own frame."""
    fx, fy, cx, cy = K
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones_like(i)], axis=2)
    a, b = (d * d).sum(axis=2), -2.0 * (d @ np.asarray(centre, dtype=np.float64))
    disc = b * b - 4.0 * a * (np.dot(centre, centre) - radius * radius)
    with np.errstate(invalid="ignore"):
        hit = (-b - np.sqrt(disc)) / (2.0 * a)
    return np.where((disc >= 0) & (hit > 0) & (hit < wall), hit, wall)


def as_uint16(metres, pad=0):
    """Millimetres; with pad the rows lie `pad` samples further apart than their width."""
    mm = np.rint(metres * 1000.0).astype(np.uint16)
    if not pad:
        return mm
    big = np.full((mm.shape[0], mm.shape[1] + pad), 7, dtype=np.uint16)
    big[:, :mm.shape[1]] = mm
    return big[:, :mm.shape[1]]


def rgb_image(w, h, seed, pad=0):
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = np.stack([(i * 5 + j * 3 + seed) % 256, (i * 11 + j + 7 * seed) % 256, (i * j + seed) % 256], axis=2).astype(np.uint8)
    if not pad:
        return img
    big = np.full((h, w + pad, 3), 9, dtype=np.uint8)
    big[:, :w] = img
    return big[:, :w]


def gray_image(w, h, seed):
    i, j = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    return (f32(0.25) + f32(0.5) * np.sin(f32(0.3) * i + f32(0.2) * j + f32(seed)) ** 2).astype(f32)


def frame(depth, K, E, color=None, depth_scale=1000.0, depth_trunc=3.0):
    return SimpleNamespace(depth=depth, K=K, E=E, color=color, depth_scale=depth_scale, depth_trunc=depth_trunc)


def pool(w, h, color_type, n=2 * CHUNK + 1):
    """n frames of one scene (a ball in front of a wall, the volume around the ball) with everything a frame can be:
    uint16 and float32 depth, padded rows, rotated cameras, a camera behind the volume, one inside it, one that sees
    nothing, and float32 samples 0, NaN, -1 and +inf."""
    K = camera(w, h)
    base = sphere_depth(w, h, K, (0.0, 0.0, 1.0), 0.3, 1.35)
    out = []
    for k in range(n):
        kind = k % 9
        E = extrinsic(0.02 * (k % 5) - 0.04, 0.03 * (k % 4) - 0.05, 0.5 * (k % 3), (0.01 * (k % 7) - 0.03, 0.02 * (k % 3) - 0.02, 0.015 * (k % 2)))
        if kind in (1, 4):  # float32 metres with the special samples
            d = base.astype(f32) + f32(0.002 * k)
            d[0, 0], d[1, 2], d[2, 1], d[h // 2, w // 2] = 0.0, np.nan, -1.0, np.inf
            d[h // 3, w // 3] = f32(-0.0)
        else:
            d = as_uint16(base + 0.001 * k, pad=3 if kind == 2 else 0)
        if kind == 5:
            E = extrinsic(t=(0.0, 0.0, -3.0))  # the volume lies behind the camera
        if kind == 6:
            E = extrinsic(0.1, -0.1, 0.0, (0.0, 0.0, -1.0))  # the camera sits inside the volume
        if kind == 7:
            d = np.zeros((h, w), dtype=np.uint16)  # sees nothing
        if kind == 8:
            E = extrinsic(0.0, np.pi / 2, 0.0)  # looks along x: most of the volume is outside the frustum
        c = None
        if color_type == RGB8:
            c = rgb_image(w, h, k, pad=2 if kind == 2 else 0)
        elif color_type == GRAY32:
            c = gray_image(w, h, k)
            if kind == 4:
                c[h // 2 - 1, w // 2] = np.nan
        out.append(frame(d, K, E, c, 1000.0, 1.3 if kind == 3 else 3.0))
    return out


def volume_args(R, color_type, sdf_trunc=None):
    """A cube of side 1 around the ball: (length, R, sdf_trunc, color_type, origin)."""
    return (1.0, R, sdf_trunc if sdf_trunc is not None else max(0.04, 2.5 / R), color_type, (-0.5, -0.5, 0.5))


_cases = None


def cases():
    """name -> SimpleNamespace(vol=(length, R, sdf_trunc, color_type, origin), frames=[...], host: in the host driver's
    file too).  Built once."""
    global _cases
    if _cases is not None:
        return _cases
    c = {}

    def add(name, R, color_type, frames, host, **kw):
        c[name] = SimpleNamespace(name=name, vol=volume_args(R, color_type, **kw), frames=frames, host=host)
    small = pool(7, 5, NONE)
    add("r1", 1, NONE, small[:2], True)
    add("r2", 2, NONE, small[:3], True)
    add("r5_rgb", 5, RGB8, pool(7, 5, RGB8)[:5], True)
    add("r5_gray", 5, GRAY32, pool(7, 5, GRAY32)[:5], True)
    add("r64", 64, NONE, pool(64, 48, NONE)[:2], False)
    add("r65_gray", 65, GRAY32, pool(64, 48, GRAY32)[:2], False)
    rgb = pool(64, 48, RGB8)
    for n in (1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        add("r16_rgb_%d" % n, 16, RGB8, rgb[:n], n in (1, CHUNK + 1))
    add("r16_gray_small", 16, GRAY32, pool(7, 5, GRAY32)[:CHUNK + 1], True)
    K = camera(64, 48)
    add("plane", 16, NONE, [frame(as_uint16(np.full((48, 64), 1.03)), K, np.eye(4))], True)
    add("sphere", 16, RGB8, [frame(as_uint16(sphere_depth(64, 48, K, (0.0, 0.0, 1.0), 0.3, 1.35)), K, extrinsic(0.0, 0.02 * k, 0.0),
                                   rgb_image(64, 48, k)) for k in range(3)], True)
    add("empty", 16, RGB8, [], True)
    _cases = c
    return c


_results = {}


def result(name):
    """The restatement's outputs for a case, computed once: tw, color (or None), points, normals, colors (or None),
    vpoints, vcolors, and the Volume itself."""
    if name in _results:
        return _results[name]
    cs = cases()[name]
    length, R, trunc, ctype, origin = cs.vol
    vol = Volume(length, R, trunc, ctype, origin)
    for f in cs.frames:
        vol.integrate(f.depth, f.K, f.E, f.color, f.depth_scale, f.depth_trunc)
    points, normals, colors = vol.extract_point_cloud()
    vpoints, vcolors = vol.extract_voxel_point_cloud()
    r = SimpleNamespace(vol=vol, tw=vol.tsdf_weight(), color=vol.colors() if ctype != NONE else None, points=points,
                        normals=normals, colors=colors, vpoints=vpoints, vcolors=vcolors)
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _results[name] = r
    return r
