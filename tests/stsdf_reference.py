"""The scalable TSDF volume restated in numpy: the parity target of tests/test_stsdf_host.py and tests/test_gpu_stsdf.py,
pinned by hand in tests/test_stsdf_reference.py.  It follows include/teaser_hip.h ("Scalable TSDF volume") line by line.
A block IS a dense volume, so its voxels are tests/tsdf_reference.py's Volume with length = ul, resolution = 16 and
origin = b ul; the points of the touch rule are tests/rgbd_reference.py's unproject.  What is restated here is what is
new: the inverse of the extrinsic, the touch rule, which frame reaches which block, and the extractions across block
faces.  Python floats and float64 arrays round every operation once and fuse nothing.

The module also holds the scenes and the case lists the host and GPU tests share.
TEST INFRASTRUCTURE ONLY."""
from types import SimpleNamespace

import numpy as np

import rgbd_reference as RG
import tsdf_reference as T

f32 = np.float32
NONE, RGB8, GRAY32 = T.NONE, T.RGB8, T.GRAY32
CHUNK = T.CHUNK
U = 16
LO, HI = -float(2 ** 20), float(2 ** 20 - 1)  # a block index lies in [-2^20, 2^20)


def camera_pose(E):
    """The inverse of the extrinsic by the closed form of the contract (rows 0 .. 2; row 3 is not read)."""
    A = [[float(E[r][c]) for c in range(3)] for r in range(3)]
    t = [float(E[r][3]) for r in range(3)]
    c = [[A[1][1] * A[2][2] - A[1][2] * A[2][1], A[1][2] * A[2][0] - A[1][0] * A[2][2], A[1][0] * A[2][1] - A[1][1] * A[2][0]],
         [A[0][2] * A[2][1] - A[0][1] * A[2][2], A[0][0] * A[2][2] - A[0][2] * A[2][0], A[0][1] * A[2][0] - A[0][0] * A[2][1]],
         [A[0][1] * A[1][2] - A[0][2] * A[1][1], A[0][2] * A[1][0] - A[0][0] * A[1][2], A[0][0] * A[1][1] - A[0][1] * A[1][0]]]
    det = (A[0][0] * c[0][0] + A[0][1] * c[0][1]) + A[0][2] * c[0][2]
    assert det != 0.0 and np.isfinite(det)
    M = np.eye(4)
    for r in range(3):
        m = [c[k][r] / det for k in range(3)]
        M[r, :3] = m
        M[r, 3] = -((m[0] * t[0] + m[1] * t[1]) + m[2] * t[2])
    return M


def touched_by_points(P, sdf_trunc, ul):
    """(the set of blocks the points P (n x 3 float64) touch, the number of points with a block outside the range)."""
    P = P[np.isfinite(P).all(axis=1)]
    if len(P) == 0:
        return set(), 0
    lo, hi = np.floor((P - sdf_trunc) / ul), np.floor((P + sdf_trunc) / ul)
    out_of_range = int(((lo < LO) | (hi > HI)).any(axis=1).sum())
    box = np.unique(np.hstack([np.maximum(lo, LO), np.minimum(hi, HI)]), axis=0)
    blocks = set()
    for b in box:
        if (b[:3] > b[3:]).any():
            continue
        r = [range(int(b[a]), int(b[3 + a]) + 1) for a in range(3)]
        assert all(len(x) <= 4 for x in r)
        blocks.update((x, y, z) for x in r[0] for y in r[1] for z in r[2])
    return blocks, out_of_range


class ScalableVolume:
    def __init__(self, voxel_length, sdf_trunc, color_type=NONE, stride=4):
        self.vl, self.sdf_trunc, self.color_type, self.stride = float(voxel_length), float(sdf_trunc), color_type, int(stride)
        self.ul = self.vl * float(U)
        assert self.sdf_trunc <= self.ul
        self.blocks = {}   # (bx, by, bz) -> T.Volume
        self.log = []      # per frame the sorted blocks it touched
        self.touched = self.opened = self.out_of_range = 0

    # ---- integration ----------------------------------------------------------------------------------------
    def touch(self, f):
        h, w = f.depth.shape
        if h == 0 or w == 0:
            return set(), 0
        fr = RG.Frame(*f.K, pose=camera_pose(f.E), depth_scale=f.depth_scale, depth_trunc=f.depth_trunc, stride=self.stride,
                      valid_only=1)
        _, P, _, _ = RG.unproject(np.ascontiguousarray(f.depth), None, fr)
        return touched_by_points(P, self.sdf_trunc, self.ul)

    def integrate(self, f):
        blocks, oor = self.touch(f)
        self.out_of_range += oor
        self.touched += len(blocks)
        self.log.append(sorted(blocks))
        for b in sorted(blocks):
            if b not in self.blocks:
                self.opened += 1
                self.blocks[b] = T.Volume(self.ul, U, self.sdf_trunc, self.color_type, tuple(float(k) * self.ul for k in b))
                assert self.blocks[b].vl == self.vl
            self.blocks[b].integrate(f.depth, f.K, f.E, f.color, f.depth_scale, f.depth_trunc)

    # ---- the blocks -------------------------------------------------------------------------------------------
    def keys(self):
        return np.array(sorted(self.blocks), dtype=np.int32).reshape(-1, 3)

    def block_tsdf_weight(self):
        """blocks x 4096 x 2 float32 in key order, Open3D's voxel order inside."""
        return np.array([self.blocks[b].tsdf_weight() for b in sorted(self.blocks)], dtype=f32).reshape(-1, U ** 3, 2)

    def block_colors(self):
        return np.array([self.blocks[b].colors() for b in sorted(self.blocks)], dtype=np.float64).reshape(-1, U ** 3, 3)

    # ---- extraction -------------------------------------------------------------------------------------------
    def tsdf_at(self, G):
        """The tsdf at the global voxel indices G (n x 3 int64); 0 in a block that is not open."""
        B, L = G // U, G % U  # floor division and its remainder
        out = np.zeros(len(G), dtype=f32)
        for b in {tuple(int(v) for v in r) for r in np.unique(B, axis=0)} if len(G) else ():
            if b in self.blocks:
                m = (B == np.array(b)).all(axis=1)
                out[m] = self.blocks[b].tsdf[L[m, 0], L[m, 1], L[m, 2]]
        return out

    def trilinear(self, q):
        a = q / self.vl - 0.5
        fl = np.floor(a)
        r = a - fl
        idx = fl.astype(np.int64)
        total = None
        for corner in range(8):
            off = np.array([corner >> 2, (corner >> 1) & 1, corner & 1])
            f = self.tsdf_at(idx + off).astype(np.float64)
            wgt = [r[:, k] if off[k] else 1.0 - r[:, k] for k in range(3)]
            term = ((wgt[0] * wgt[1]) * wgt[2]) * f
            total = term if total is None else total + term
        return total

    def padded(self, b):
        """Block b with one more layer along each axis, from the blocks b + e_i: tsdf, usable and colour."""
        vol = self.blocks[b]
        F = np.zeros((U + 1,) * 3, dtype=f32)
        ok = np.zeros((U + 1,) * 3, dtype=bool)
        col = np.zeros((U + 1,) * 3 + (3,))
        F[:U, :U, :U], ok[:U, :U, :U], col[:U, :U, :U] = vol.tsdf, vol.usable(), vol.color
        for i in range(3):
            nb = self.blocks.get(tuple(b[k] + (k == i) for k in range(3)))
            if nb is None:
                continue
            dst = [slice(0, U)] * 3
            src = [slice(0, U)] * 3
            dst[i], src[i] = U, 0
            dst, src = tuple(dst), tuple(src)
            F[dst], ok[dst], col[dst] = nb.tsdf[src], nb.usable()[src], nb.color[src]
        return F, ok, col

    def surface_rows(self, b):
        """The (x, y, z, i) of the block's rows in order, with the padded arrays."""
        F, ok, col = self.padded(b)
        mask = np.zeros((U, U, U, 3), dtype=bool)
        own = (slice(0, U),) * 3
        for i in range(3):
            up = [slice(0, U)] * 3
            up[i] = slice(1, U + 1)
            up = tuple(up)
            mask[..., i] = ok[own] & ok[up] & (F[own] * F[up] < 0)
        return np.argwhere(mask), F, col

    def extract_point_cloud(self, normals=True):
        """(points, normals or None, colors or None, crossing: per row whether its neighbour lies in the next block)."""
        pts, cols, cross = [np.zeros((0, 3))], [np.zeros((0, 3))], [np.zeros((0, 2), dtype=np.int64)]
        for b in sorted(self.blocks):
            rows, F, col = self.surface_rows(b)
            n = len(rows)
            if n == 0:
                continue
            x, y, z, i = rows.T
            e = np.eye(3, dtype=np.int64)[i]
            f0, f1 = F[x, y, z], F[x + e[:, 0], y + e[:, 1], z + e[:, 2]]
            r0, r1 = np.abs(f0), np.abs(f1)
            den = (r0 + r1).astype(np.float64)
            r0, r1 = r0.astype(np.float64), r1.astype(np.float64)
            half = self.vl * 0.5
            p = np.stack([(half + self.vl * c.astype(np.float64)) + float(b[k]) * self.ul for k, c in enumerate((x, y, z))], axis=1)
            k = np.arange(n)
            p0 = p[k, i]
            p[k, i] = (p0 * r1 + (p0 + self.vl) * r0) / den
            pts.append(p)
            cross.append(np.stack([i, (rows[k, i] == U - 1).astype(np.int64)], axis=1))
            if self.color_type != NONE:
                c = (col[x, y, z] * r1[:, None] + col[x + e[:, 0], y + e[:, 1], z + e[:, 2]] * r0[:, None]) / den[:, None]
                cols.append(c / 255.0 if self.color_type == RGB8 else np.where(np.isnan(c), np.nan, c))
        points = np.concatenate(pts)
        colors = np.concatenate(cols) if self.color_type != NONE else None
        nrm = None
        if normals:
            g = 0.99 * self.vl
            nrm = np.zeros((len(points), 3))
            for a in range(3):
                hi, lo = points.copy(), points.copy()
                hi[:, a] = points[:, a] + g
                lo[:, a] = points[:, a] - g
                if len(points):
                    nrm[:, a] = self.trilinear(hi) - self.trilinear(lo)
            s = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
            with np.errstate(all="ignore"):
                nrm = np.where((s > 0)[:, None], nrm / np.sqrt(s)[:, None], nrm)
        return points, nrm, colors, np.concatenate(cross)

    def extract_voxel_point_cloud(self):
        parts = [self.blocks[b].extract_voxel_point_cloud() for b in sorted(self.blocks)]
        if not parts:
            return np.zeros((0, 3)), np.zeros((0, 3))
        return np.concatenate([p for p, _ in parts]), np.concatenate([c for _, c in parts])


# ---- scenes and cases -----------------------------------------------------------------------------------------------
def camera(w, h):
    """A narrower camera than the dense cases': the wall of the scene stays within a few blocks."""
    return (1.8 * w, 1.7 * w, (w - 1) / 2.0, (h - 1) / 2.0)


def pool(w, h, color_type, n=2 * CHUNK + 1):
    """n frames of the dense cases' scene (a ball in front of a wall) seen from z = -1.1, so that the blocks have negative
    indices on every axis: uint16 and float32 depth with the samples 0, NaN, -1 and +inf, padded rows, rotated cameras, a
    depth_trunc that cuts the wall away, a camera that sees nothing (every block is skipped by it) and one moved sideways
    (it opens blocks no earlier frame has seen)."""
    K = camera(w, h)
    base = T.sphere_depth(w, h, K, (0.0, 0.0, 1.0), 0.3, 1.35)
    out = []
    for k in range(n):
        kind = k % 6
        E = T.extrinsic(0.02 * (k % 5) - 0.04, 0.03 * (k % 4) - 0.05, 0.5 * (k % 3),
                        (0.01 * (k % 7) - 0.03, 0.02 * (k % 3) - 0.02, 1.1 + 0.015 * (k % 2)))
        if kind == 1:  # float32 metres with the special samples
            d = base.astype(f32) + f32(0.002 * k)
            d[0, 0], d[1, 2], d[2, 1], d[h // 2, w // 2] = 0.0, np.nan, -1.0, np.inf
            d[h // 3, w // 3] = f32(-0.0)
        else:
            d = T.as_uint16(base + 0.001 * k, pad=3 if kind == 2 else 0)
        if kind == 4:
            d = np.zeros((h, w), dtype=np.uint16)  # sees nothing
        if kind == 5:
            E = T.extrinsic(0.0, 0.0, 0.0, (-0.5, 0.0, 1.1))  # moved sideways
        c = None
        if color_type == RGB8:
            c = T.rgb_image(w, h, k, pad=2 if kind == 2 else 0)
        elif color_type == GRAY32:
            c = T.gray_image(w, h, k)
            if kind == 1:
                c[h // 2 - 1, w // 2] = np.nan
        out.append(T.frame(d, K, E, c, 1000.0, 1.3 if kind == 3 else 3.0))
    return out


FAR = float(2 ** 20) * 0.32  # where the index range of a volume with 2 cm voxels ends

_cases = None


def cases():
    """name -> SimpleNamespace(vl, trunc, ctype, stride, frames, host: in the host driver's file too).  Built once."""
    global _cases
    if _cases is not None:
        return _cases
    c = {}

    def add(name, ctype, stride, frames, host, vl=0.02, trunc=0.06):
        c[name] = SimpleNamespace(name=name, vl=vl, trunc=trunc, ctype=ctype, stride=stride, frames=frames, host=host)
    big = {t: pool(64, 48, t, 6) for t in (NONE, RGB8, GRAY32)}
    small = {t: pool(7, 5, t) for t in (NONE, RGB8, GRAY32)}
    add("rgb_64", RGB8, 4, big[RGB8], False)
    add("gray_64_stride1", GRAY32, 1, big[GRAY32][:2], False)
    add("none_64", NONE, 4, big[NONE][:3], True)
    add("none_7", NONE, 1, small[NONE][:6], True)
    add("gray_7", GRAY32, 1, small[GRAY32][:6], True)
    add("rgb_7_wide_stride", RGB8, 9, small[RGB8][:6], True)  # a stride larger than the image: pixel (0, 0) alone
    add("nothing", RGB8, 4, [big[RGB8][4]], True)
    add("empty", GRAY32, 4, [], True)
    for n in (1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        add("split_%d" % n, RGB8, 1, small[RGB8][:n], n == CHUNK + 1)
    # the dense identity: few blocks
    add("identity", RGB8, 2, pool(16, 12, RGB8, 6), False, vl=0.04, trunc=0.1)
    # the end of the index range: a camera that straddles it and one far beyond it
    f = small[NONE][0]
    add("far", NONE, 1, [T.frame(f.depth, f.K, T.extrinsic(t=(-FAR, 0.0, 1.1))), T.frame(f.depth, f.K, T.extrinsic(t=(-2.0 * FAR, 3.0 * FAR, 1.1))),
                        T.frame(f.depth, f.K, T.extrinsic(t=(FAR, 0.0, 1.1)))], True)
    _cases = c
    return c


_results = {}


def run(cs, frames=None):
    vol = ScalableVolume(cs.vl, cs.trunc, cs.ctype, cs.stride)
    for f in (cs.frames if frames is None else frames):
        vol.integrate(f)
    return vol


def result(name):
    """The restatement's outputs for a case, computed once and left unchanged."""
    if name in _results:
        return _results[name]
    cs = cases()[name]
    vol = run(cs)
    points, normals, colors, crossing = vol.extract_point_cloud()
    vpoints, vcolors = vol.extract_voxel_point_cloud()
    r = SimpleNamespace(vol=vol, keys=vol.keys(), tw=vol.block_tsdf_weight(), color=vol.block_colors() if cs.ctype != NONE else None,
                        points=points, normals=normals, colors=colors, crossing=crossing, vpoints=vpoints, vcolors=vcolors,
                        touched=vol.touched, opened=vol.opened, out_of_range=vol.out_of_range)
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _results[name] = r
    return r
