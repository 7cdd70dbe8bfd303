"""The ray cast of the scalable TSDF volume restated in numpy: the parity target of tests/test_stsdf_raycast_host.py and
tests/test_gpu_stsdf_raycast.py, pinned by hand in tests/test_stsdf_raycast_reference.py.  It follows
include/teaser_hip.h ("Scalable TSDF ray casting") line by line: float32 numpy arrays where the contract says float32
(numpy rounds every float32 operation once and fuses nothing), float64 where it says double.  The volume is
stsdf_reference.ScalableVolume, the camera and the rays are tsdf_raycast_reference's.  No pixel depends on another, so
the pixels run as arrays and only the march is a loop; a pixel that has ended keeps its state.  There is no block cache
here: every step looks its block up, which is what the contract says the cache must not change.
TEST INFRASTRUCTURE ONLY."""
from types import SimpleNamespace

import numpy as np

import stsdf_reference as S
import tsdf_raycast_reference as RC
import tsdf_reference as T

f32 = np.float32
U = S.U
RANGE = f32(2 ** 24)
MAX_STEPS = 2 ** 20


class Lattice:
    """The open blocks of a ScalableVolume as arrays: slot k is the k-th block in ascending order."""

    def __init__(self, vol):
        self.keys = sorted(vol.blocks)
        self.index = {b: k for k, b in enumerate(self.keys)}
        n = len(self.keys)
        self.tsdf = np.zeros((max(n, 1), U, U, U), dtype=f32)
        self.weight = np.zeros((max(n, 1), U, U, U), dtype=f32)
        self.color = np.zeros((max(n, 1), U, U, U, 3)) if vol.color_type != T.NONE else None  # read only with a colour type
        for k, b in enumerate(self.keys):
            self.tsdf[k], self.weight[k] = vol.blocks[b].tsdf, vol.blocks[b].weight
            if self.color is not None:
                self.color[k] = vol.blocks[b].color

    def find(self, B):
        """The slot of every row of B (n x 3 int64), -1 where the block is not open."""
        if len(B) == 0:
            return np.zeros(0, dtype=np.int64)
        uniq, inv = np.unique(B, axis=0, return_inverse=True)
        slots = np.array([self.index.get(tuple(u), -1) for u in uniq.tolist()], dtype=np.int64)
        return slots[inv.reshape(-1)]

    def voxels(self, G):
        """(open, slot, local) of the global voxel indices G (n x 3 int64): floor division and its remainder."""
        slot = self.find(G // U)
        return slot >= 0, np.maximum(slot, 0), G % U


def step_cap(vol, depth_min, depth_max):
    steps = np.floor((float(f32(depth_max)) - float(f32(depth_min))) / float(f32(vol.vl))) + 2.0
    return int(min(float(MAX_STEPS), steps))


def march(vol, o, d, dmin, dmax, wthr, n_cap, skip=True, trace=None, lat=None):
    """The rays d (n x 3 float32) from o (3 float32).  Per ray: hit, t, t_prev, f, f_prev of the hit, and the steps
    taken (samples read).  trace: a list that receives per step a SimpleNamespace of copies: t, B (float32 n x 3),
    open, active (before the hit test), t_exit (where the block is not open; NaN where no axis has d != 0).
    skip=False: a block that is not open is crossed a voxel at a time."""
    lat = lat if lat is not None else Lattice(vol)
    n = len(d)
    o, d = np.asarray(o, dtype=f32), np.asarray(d, dtype=f32).reshape(n, 3)
    vl_f, trunc_f, ul_f = f32(vol.vl), f32(vol.sdf_trunc), f32(vol.ul)
    dmin, t1, wthr = f32(dmin), f32(dmax), f32(wthr)
    t, t_prev, f_prev = np.full(n, dmin, dtype=f32), np.full(n, dmin, dtype=f32), np.full(n, -1, dtype=f32)
    f_hit = np.zeros(n, dtype=f32)
    active, hit, steps = np.full(n, len(lat.keys) > 0), np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        for _ in range(n_cap):
            active &= t <= t1
            if not active.any():
                break
            p = o[None, :] + t[:, None] * d
            g = np.floor(p / vl_f)
            assert p.dtype == f32 and g.dtype == f32
            active &= ((g >= -RANGE) & (g < RANGE)).all(axis=1)  # a NaN ends the ray, too
            gs = np.where(active[:, None], g, f32(0))
            B = np.floor(gs / f32(16))
            l = gs - f32(16) * B
            assert B.dtype == f32 and l.dtype == f32 and (l >= 0).all() and (l < 16).all()
            slot = lat.find(B.astype(np.int64))
            is_open = slot >= 0
            s, li = np.maximum(slot, 0), l.astype(np.int64)
            f = np.where(is_open, lat.tsdf[s, li[:, 0], li[:, 1], li[:, 2]], f32(0))
            w = np.where(is_open, lat.weight[s, li[:, 0], li[:, 1], li[:, 2]], f32(0))
            steps += active
            now = active & is_open & (f_prev > 0) & (w >= wthr) & (f <= 0)
            # the open block's step
            delta = f * trunc_f
            t_open = t + np.where(delta < vl_f, vl_f, delta)
            # the skip of a block that is not open
            t_exit, some = np.full(n, np.nan, dtype=f32), np.zeros(n, dtype=bool)
            for k in range(3):
                nz = d[:, k] != 0
                face = np.where(d[:, k] > 0, B[:, k] + f32(1), B[:, k]) * ul_f
                e = (face - o[k]) / d[:, k]
                t_exit = np.where(nz & (~some | (e < t_exit)), e, t_exit)
                some |= nz
            t_next = t + vl_f
            t_skip = np.where(some & (t_exit > t_next), t_exit, t_next) if skip else t_next
            assert t_open.dtype == f32 and t_skip.dtype == f32
            if trace is not None:
                trace.append(SimpleNamespace(t=t.copy(), B=B.copy(), open=is_open.copy(), active=active.copy(),
                                             t_exit=np.where(is_open, f32(np.nan), t_exit)))
            hit |= now
            f_hit = np.where(now, f, f_hit)
            active &= ~now
            t_prev = np.where(active, t, t_prev)
            f_prev = np.where(active, np.where(is_open, f, f32(0)), f_prev)
            t = np.where(active, np.where(is_open, t_open, t_skip), t)
            assert t.dtype == f32 and f_prev.dtype == f32
    return hit, t, t_prev, f_hit, f_prev, steps


def trilinear(vol, lat, q):
    """T(q) on the global lattice: stsdf_reference's form over the packed blocks."""
    a = q / vol.vl - 0.5
    fl = np.floor(a)
    r = a - fl
    idx = fl.astype(np.int64)
    total = None
    for corner in range(8):
        off = np.array([corner >> 2, (corner >> 1) & 1, corner & 1])
        is_open, s, l = lat.voxels(idx + off)
        f = np.where(is_open, lat.tsdf[s, l[:, 0], l[:, 1], l[:, 2]], f32(0)).astype(np.float64)
        wgt = [r[:, k] if off[k] else 1.0 - r[:, k] for k in range(3)]
        term = ((wgt[0] * wgt[1]) * wgt[2]) * f
        total = term if total is None else total + term
    return total


def color_at(vol, lat, q):
    """The colour rule at the rows of q (NEAR), float64 n x 3: a corner counts when its block is open and its weight
    is not 0."""
    a = q / vol.vl - 0.5
    fl = np.floor(a)
    r = a - fl
    idx = fl.astype(np.int64)
    num, den = np.zeros((len(q), 3)), np.zeros(len(q))
    with np.errstate(all="ignore"):
        for corner in range(8):
            off = np.array([corner >> 2, (corner >> 1) & 1, corner & 1])
            is_open, s, l = lat.voxels(idx + off)
            counts = is_open & (lat.weight[s, l[:, 0], l[:, 1], l[:, 2]] != 0)
            wgt = [r[:, k] if off[k] else 1.0 - r[:, k] for k in range(3)]
            omega = (wgt[0] * wgt[1]) * wgt[2]
            c = lat.color[s, l[:, 0], l[:, 1], l[:, 2]]
            num = np.where(counts[:, None], num + omega[:, None] * c, num)
            den = np.where(counts, den + omega, den)
        out = np.where((den > 0)[:, None], num / den[:, None], 0.0)
        if vol.color_type == T.RGB8:
            out = out / 255.0
    return out


def finish(vol, lat, o, d, t, t_prev, f, f_prev):
    """(depth, vertex, normal, color or None, near) of the hits given by their rays and march states."""
    ts = (t * f_prev - t_prev * f) / (f_prev - f)
    assert ts.dtype == f32
    q = o.astype(np.float64)[None, :] + ts.astype(np.float64)[:, None] * d.astype(np.float64)
    with np.errstate(all="ignore"):
        vertex = q.astype(f32)
        near = (np.abs(q) <= (2.0 ** 24 + 2.0) * vol.vl).all(axis=1)
    qn = np.where(near[:, None], q, 0.0)
    g = 0.99 * vol.vl
    nrm = np.zeros((len(q), 3))
    for k in range(3):
        hi, lo = qn.copy(), qn.copy()
        hi[:, k] = qn[:, k] + g
        lo[:, k] = qn[:, k] - g
        nrm[:, k] = trilinear(vol, lat, hi) - trilinear(vol, lat, lo)
    s = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
    with np.errstate(all="ignore"):
        nrm = np.where((s > 0)[:, None], nrm / np.sqrt(s)[:, None], nrm)
    normal = np.where(near[:, None], nrm, 0.0).astype(f32)
    color = None
    if vol.color_type != T.NONE:
        color = RC.to_f32(np.where(near[:, None], color_at(vol, lat, qn), 0.0))
    return ts, vertex, normal, color, near


def ray_cast(vol, K, E, width, height, depth_min=0.1, depth_max=3.0, weight_threshold=3.0, trace=None, skip=True, lat=None):
    """depth (h x w), vertex, normal, color (h x w x 3; color None without a colour type), all float32; hits; steps
    (h x w: the samples every ray read); hit (h x w bool)."""
    lat = lat if lat is not None else Lattice(vol)
    origin = SimpleNamespace(origin=np.zeros(3))
    o, Rt = RC.camera(origin, E)
    n = width * height
    d = RC.rays(K, Rt, width, height).reshape(n, 3)
    hit, t, t_prev, f, f_prev, steps = march(vol, o, d, depth_min, depth_max, weight_threshold,
                                             step_cap(vol, depth_min, depth_max), skip, trace, lat)
    depth, vertex, normal = np.zeros(n, dtype=f32), np.zeros((n, 3), dtype=f32), np.zeros((n, 3), dtype=f32)
    color = np.zeros((n, 3), dtype=f32) if vol.color_type != T.NONE else None
    at = np.flatnonzero(hit)
    if len(at):
        ts, vx, nr, col, _ = finish(vol, lat, o, d[at], t[at], t_prev[at], f[at], f_prev[at])
        depth[at], vertex[at], normal[at] = ts, vx, nr
        if color is not None:
            color[at] = col
    shape = (height, width)
    return SimpleNamespace(depth=depth.reshape(shape), vertex=vertex.reshape(shape + (3,)), normal=normal.reshape(shape + (3,)),
                           color=None if color is None else color.reshape(shape + (3,)), hits=int(hit.sum()),
                           steps=steps.reshape(shape), hit=hit.reshape(shape))


def cast(vol, w, lat=None, **kw):
    """A view of tsdf_raycast_reference.view."""
    return ray_cast(vol, w.K, w.E, w.width, w.height, w.depth_min, w.depth_max, w.weight_threshold, lat=lat, **kw)


# ---- the volumes and views the host and GPU tests share --------------------------------------------------------------
def volume_of_blocks(vl, trunc, color_type, blocks):
    """A ScalableVolume with the given blocks: key -> (tsdf, weight, color or None), arrays of 16^3 (x 3)."""
    vol = S.ScalableVolume(vl, trunc, color_type)
    for b, (tsdf, weight, color) in blocks.items():
        blk = T.Volume(vol.ul, U, trunc, color_type, tuple(float(k) * vol.ul for k in b))
        blk.tsdf[:], blk.weight[:] = tsdf, weight
        if color is not None:
            blk.color[:] = color
        vol.blocks[tuple(int(k) for k in b)] = blk
    return vol


def random_blocks(seed, color_type, weight=2.0, n=5, vl=0.02, trunc=0.06):
    """n blocks drawn from [-2, 2)^3 with random tsdf in (-1, 1), a third of the weights 0 and the others `weight`, and
    random colours (a Gray32 volume with a NaN)."""
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < n:
        keys.add(tuple(int(k) for k in rng.integers(-2, 2, 3)))
    blocks = {}
    for b in sorted(keys):
        tsdf = (rng.random((U, U, U)) * 1.9 - 0.95).astype(f32)
        wgt = ((rng.random((U, U, U)) > 1.0 / 3.0) * weight).astype(f32)
        col = None
        if color_type == T.RGB8:
            col = np.floor(rng.random((U, U, U, 3)) * 256.0)
        elif color_type == T.GRAY32:
            col = np.repeat(rng.random((U, U, U, 1)), 3, axis=3)
            col[3, 4, 5] = np.nan
        blocks[b] = (tsdf, wgt, col)
    return volume_of_blocks(vl, trunc, color_type, blocks)


RANDOM_SETS = ((11, T.RGB8, 0.0, 2.0), (12, T.GRAY32, 1.0, 2.0), (13, T.NONE, 3.0, 4.0), (14, T.RGB8, 3.0, 4.0),
               (15, T.NONE, 0.0, 2.0), (16, T.GRAY32, 1.0, 1.0))  # seed, colour type, threshold, weight


def views_of(vol, weight_threshold, sizes=((8, 8), (17, 9), (0, 5), (33, 17)), back=None):
    """Views of the given sizes from slightly different directions towards the centre of the blocks' bounding box."""
    keys = np.array(sorted(vol.blocks), dtype=np.float64).reshape(-1, 3)
    lo, hi = (keys.min(axis=0), keys.max(axis=0) + 1.0) if len(keys) else (np.zeros(3), np.ones(3))
    box = SimpleNamespace(origin=lo * vol.ul, length=float((hi - lo).max()) * vol.ul)
    back = back if back is not None else 1.1 * box.length
    return [RC.view(w, h, RC.look_at_volume(box, 0.1 * k - 0.05, 0.15 - 0.1 * k, back), depth_min=0.05,
                    depth_max=back + 1.5 * box.length, weight_threshold=weight_threshold) for k, (w, h) in enumerate(sizes)]
