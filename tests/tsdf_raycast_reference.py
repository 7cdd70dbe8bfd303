"""The ray cast of the TSDF volume restated in numpy: the parity target of tests/test_tsdf_raycast_host.py and
tests/test_gpu_tsdf_raycast.py, pinned by hand in tests/test_tsdf_raycast_reference.py.  It follows include/teaser_hip.h
("TSDF ray casting") line by line: float32 numpy arrays where the contract says float32 (numpy rounds every float32
operation once and fuses nothing), float64 where it says double.  No pixel depends on another, so the pixels run as
arrays and only the march is a loop; a pixel that has ended keeps its state.  The volume is tsdf_reference.Volume.
TEST INFRASTRUCTURE ONLY."""
from types import SimpleNamespace

import numpy as np

import tsdf_reference as T

f32 = T.f32


def camera(vol, E):
    """(o_f, Rt_f): the centre in volume coordinates and the camera-to-world rotation, float32."""
    E = np.asarray(E, dtype=np.float64)
    c = np.array([-((E[0, k] * E[0, 3] + E[1, k] * E[1, 3]) + E[2, k] * E[2, 3]) for k in range(3)])
    return (c - vol.origin).astype(f32), E[:3, :3].T.astype(f32)


def rays(K, Rt, width, height):
    """d: height x width x 3 float32."""
    fx, fy, cx, cy = (f32(x) for x in K)
    a = ((np.arange(width, dtype=f32) - cx) / fx)[None, :]
    b = ((np.arange(height, dtype=f32) - cy) / fy)[:, None]
    return np.stack([(Rt[k, 0] * a + Rt[k, 1] * b) + Rt[k, 2] for k in range(3)], axis=2)


def clip(o, d, L_f, dmin, dmax):
    """(t0, t1, ok) of the rays d (n x 3)."""
    n = len(d)
    t0, t1, ok = np.full(n, dmin, dtype=f32), np.full(n, dmax, dtype=f32), np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            nz = d[:, k] != 0
            lo, hi = (f32(0) - o[k]) / d[:, k], (L_f - o[k]) / d[:, k]
            lo, hi = np.where(hi < lo, hi, lo), np.where(hi < lo, lo, hi)
            t0 = np.where(nz & (t0 < lo), lo, t0)
            t1 = np.where(nz & (hi < t1), hi, t1)
            if not (o[k] >= 0 and o[k] < L_f):
                ok &= nz
    return t0, t1, ok


def march(vol, o, d, t0, t1, ok, wthr, trace=None):
    """Per ray: hit, t, t_prev, f, f_prev of the hit, and the steps taken (samples read).  trace: a list that receives
    per step (t, q, inside, active) copies."""
    n, R = len(d), vol.R
    t, t_prev, f_prev = t0.copy(), t0.copy(), np.full(n, -1, dtype=f32)
    f_hit = np.zeros(n, dtype=f32)
    active, hit, steps = ok.copy(), np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    R_f = f32(R)
    with np.errstate(all="ignore"):
        for _ in range(2 * R + 2):
            active &= t <= t1
            if not active.any():
                break
            p = o[None, :] + t[:, None] * d
            q = np.floor(p / vol.vl_f)
            assert p.dtype == f32 and q.dtype == f32
            inside = ((q >= 0) & (q < R_f)).all(axis=1)
            at = np.where(inside[:, None], q, f32(0)).astype(np.int64)
            f = np.where(inside, vol.tsdf[at[:, 0], at[:, 1], at[:, 2]], f32(0))
            w = np.where(inside, vol.weight[at[:, 0], at[:, 1], at[:, 2]], f32(0))
            if trace is not None:
                trace.append((t.copy(), q.copy(), inside.copy(), active.copy()))
            steps += active
            now = active & (f_prev > 0) & (w >= wthr) & (f <= 0)
            hit |= now
            f_hit = np.where(now, f, f_hit)
            active &= ~now
            delta = f * vol.trunc_f
            t_next = t + np.where(delta < vol.vl_f, vol.vl_f, delta)
            t_prev = np.where(active, t, t_prev)
            f_prev = np.where(active, f, f_prev)
            t = np.where(active, t_next, t)
            assert t.dtype == f32 and f_prev.dtype == f32
    return hit, t, t_prev, f_hit, f_prev, steps


def color_at(vol, q):
    """The colour rule at the rows of q (NEAR), float64 n x 3."""
    R = vol.R
    a = q / vol.vl - 0.5
    fl = np.floor(a)
    r = a - fl
    idx = fl.astype(np.int64)
    num, den = np.zeros((len(q), 3)), np.zeros(len(q))
    with np.errstate(all="ignore"):
        for corner in range(8):
            off = np.array([corner >> 2, (corner >> 1) & 1, corner & 1])
            at = idx + off
            safe = np.clip(at, 0, R - 1)
            counts = ((at >= 0) & (at < R)).all(axis=1) & (vol.weight[safe[:, 0], safe[:, 1], safe[:, 2]] != 0)
            wgt = [r[:, k] if off[k] else 1.0 - r[:, k] for k in range(3)]
            omega = (wgt[0] * wgt[1]) * wgt[2]
            c = vol.color[safe[:, 0], safe[:, 1], safe[:, 2]]
            num = np.where(counts[:, None], num + omega[:, None] * c, num)
            den = np.where(counts, den + omega, den)
        out = np.where((den > 0)[:, None], num / den[:, None], 0.0)
        if vol.color_type == T.RGB8:
            out = out / 255.0
    return out


def to_f32(x):
    """Rounded to float32, a NaN as THE quiet NaN."""
    with np.errstate(all="ignore"):
        y = np.asarray(x, dtype=np.float64).astype(f32)
    y[np.isnan(y)] = np.array([0x7fc00000], dtype=np.uint32).view(f32)[0]
    return y


def ray_cast(vol, K, E, width, height, depth_min=0.1, depth_max=3.0, weight_threshold=3.0, trace=None):
    """depth (h x w), vertex, normal, color (h x w x 3; color None without a colour type), all float32; hits; steps
    (h x w: the samples every ray read); hit (h x w bool)."""
    o, Rt = camera(vol, E)
    n = width * height
    d = rays(K, Rt, width, height).reshape(n, 3)
    t0, t1, ok = clip(o, d, f32(vol.length), f32(depth_min), f32(depth_max))
    hit, t, t_prev, f, f_prev, steps = march(vol, o, d, t0, t1, ok, f32(weight_threshold), trace)
    depth, vertex, normal = np.zeros(n, dtype=f32), np.zeros((n, 3), dtype=f32), np.zeros((n, 3), dtype=f32)
    color = np.zeros((n, 3), dtype=f32) if vol.color_type != T.NONE else None
    at = np.flatnonzero(hit)
    if len(at):
        th, tp, fh, fp = t[at], t_prev[at], f[at], f_prev[at]
        ts = (th * fp - tp * fh) / (fp - fh)
        assert ts.dtype == f32
        depth[at] = ts
        q = o.astype(np.float64)[None, :] + ts.astype(np.float64)[:, None] * d[at].astype(np.float64)
        vertex[at] = (q + vol.origin).astype(f32)
        near = ((q >= -(2.0 * vol.vl)) & (q <= vol.vl * float(vol.R) + 2.0 * vol.vl)).all(axis=1)
        qn = np.where(near[:, None], q, 0.0)
        g = 0.99 * vol.vl
        nrm = np.zeros((len(at), 3))
        for k in range(3):
            hi, lo = qn.copy(), qn.copy()
            hi[:, k] = qn[:, k] + g
            lo[:, k] = qn[:, k] - g
            nrm[:, k] = vol.trilinear(hi) - vol.trilinear(lo)
        s = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        with np.errstate(all="ignore"):
            nrm = np.where((s > 0)[:, None], nrm / np.sqrt(s)[:, None], nrm)
        normal[at] = np.where(near[:, None], nrm, 0.0).astype(f32)
        if color is not None:
            color[at] = to_f32(np.where(near[:, None], color_at(vol, qn), 0.0))
    shape = (height, width)
    return SimpleNamespace(depth=depth.reshape(shape), vertex=vertex.reshape(shape + (3,)), normal=normal.reshape(shape + (3,)),
                           color=None if color is None else color.reshape(shape + (3,)), hits=int(hit.sum()),
                           steps=steps.reshape(shape), hit=hit.reshape(shape))


def intensity(color):
    """The float32 intensity of an h x w x 3 float32 colour map in [0, 1]: the weights of "Depth frames"."""
    c = np.asarray(color, dtype=f32)
    return (f32(0.2990) * c[..., 0] + f32(0.5870) * c[..., 1]) + f32(0.1140) * c[..., 2]


def look_at_volume(vol, rx=0.0, ry=0.0, back=1.2):
    """World to camera: the camera `back` behind the volume's centre along its own z axis after the rotations."""
    E = T.extrinsic(rx, ry)
    centre = vol.origin + 0.5 * vol.length
    E[:3, 3] = -E[:3, :3] @ centre + np.array([0.0, 0.0, back])
    return E


# ---- the views and volumes the host and GPU tests share ---------------------------------------------------------------
def view(width, height, E, K=None, depth_min=0.1, depth_max=3.0, weight_threshold=3.0):
    return SimpleNamespace(width=width, height=height, E=np.array(E, dtype=np.float64), K=K if K is not None else T.camera(max(width, 1), max(height, 1)),
                           depth_min=depth_min, depth_max=depth_max, weight_threshold=weight_threshold)


def cast(vol, w):
    return ray_cast(vol, w.K, w.E, w.width, w.height, w.depth_min, w.depth_max, w.weight_threshold)


def random_volume(R, seed, color_type, weight=2.0):
    """tsdf_mesh_reference.random_volume with a third of the weights zeroed and the others `weight`."""
    import tsdf_mesh_reference as M
    vol = M.random_volume(R, seed, color_type)
    vol.weight[:] = (vol.weight != 0).astype(f32) * f32(weight)
    return vol


def views_around(vol, weight_threshold, sizes=((8, 8), (17, 9)), depth_max=None):
    """Views of the given sizes from slightly different directions, the camera 1.3 lengths behind the centre."""
    far = depth_max if depth_max is not None else 3.0 * vol.length
    return [view(w, h, look_at_volume(vol, 0.1 * k - 0.05, 0.15 - 0.1 * k, 1.3 * vol.length), depth_max=far,
                 weight_threshold=weight_threshold) for k, (w, h) in enumerate(sizes)]
