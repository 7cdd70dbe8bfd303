"""The numpy restatement of the RGB-D odometry contract (include/teaser_hip.h, "RGB-D odometry"), line by line: float32
numpy arrays where the contract says float32, float64 elsewhere, the operations in the order written, the sums in the
stated tree of blocks and groups.  tests/test_odometry_reference.py pins it by facts worked out by hand; the host driver
and the GPU must EQUAL it bit for bit.  Also the scenes and the one list of cases every odometry test shares, with the
results memoised (``result``, ``pyramid``)."""
import math
from types import SimpleNamespace

import numpy as np

f32, f64 = np.float32, np.float64
BLOCK = 256   # TEASER_HIP_ODOMETRY_BLOCK / kOdoBlock of csrc/icp_odometry_device.h
GROUP = 64    # TEASER_HIP_ODOMETRY_GROUP / kOdoGroup
SUMS = 29
COLOR, HYBRID = 0, 1
PLANES = ("I_s", "I_t", "D_s", "D_t", "X", "Y", "Z", "I_t_dx", "I_t_dy", "D_t_dx", "D_t_dy")
QNAN32 = np.array([0x7FC00000], dtype=np.uint32).view(f32)[0]
QNAN64 = np.array([0x7FF8000000000000], dtype=np.uint64).view(f64)[0]
GAUSS = (f32(0.25), f32(0.5), f32(0.25))
SOBEL_D, SOBEL_S = (f32(-1.0), f32(0.0), f32(1.0)), (f32(1.0), f32(2.0), f32(1.0))


def canon32(a):
    a = np.asarray(a, dtype=f32).copy()
    a[np.isnan(a)] = QNAN32
    return a


def canon64(a):
    a = np.array(a, dtype=f64)
    a[np.isnan(a)] = QNAN64
    return a


# ---- fdet_sincos_d (csrc/fdet_math.h) ---------------------------------------------------------------------------------
P1, P2, P3 = 1.57079632673412561417e+00, 6.07710050630396597660e-11, 2.02226624879595063154e-21


def rn(y):
    return (y + 6755399441055744.0) - 6755399441055744.0


def sincos(x):
    """The Python twin of fdet_sincos_d: Python floats are IEEE doubles and nothing is fused."""
    x = float(x)
    if abs(x) >= 65536.0:
        c = 2.0 ** 1008
        for _ in range(63):
            m1, m2, m3 = (4.0 * P1) * c, (4.0 * P2) * c, (4.0 * P3) * c
            if abs(x) >= m1:
                q = rn(x / m1)
                x = ((x - q * m1) - q * m2) - q * m3
            c = c * 2.0 ** -16
    k = rn(x * 0.63661977236758138)
    r = ((x - k * P1) - k * P2) - k * P3
    z = r * r
    S = C = 1.0
    for j in range(10, 0, -1):
        S = 1.0 - (z * (1.0 / float((2 * j) * (2 * j + 1)))) * S
    for j in range(11, 0, -1):
        C = 1.0 - (z * (1.0 / float((2 * j - 1) * (2 * j)))) * C
    sr, cr = r * S, C
    n = int(k) & 3 if k == k else 0
    return ((sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr))[n]


# ---- images -----------------------------------------------------------------------------------------------------------
def depth_as_float(depth, depth_scale, depth_trunc):
    """The rule of "Depth frames"."""
    if depth.dtype == np.uint16:
        zf = depth.astype(f32) / f32(depth_scale)
        zf[zf.astype(f64) >= depth_trunc] = f32(0.0)
        return zf
    return np.array(depth, dtype=f32)


def convert_depth(depth, depth_scale, depth_trunc, depth_min, depth_max):
    zf = depth_as_float(depth, depth_scale, depth_trunc)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(zf) | (zf.astype(f64) <= depth_min) | (zf.astype(f64) > depth_max)
    zf[bad] = QNAN32
    return zf


def convert_color(color):
    if color.dtype == np.uint8:
        c = color.astype(f32)
        return ((f32(0.2990) * c[:, :, 0] + f32(0.5870) * c[:, :, 1]) + f32(0.1140) * c[:, :, 2]) / f32(255.0)
    return canon32(color)


def filter3(p, kh, kv):
    h, w = p.shape
    xs, ys = np.arange(w), np.arange(h)
    xm, xp, ym, yp = np.maximum(xs - 1, 0), np.minimum(xs + 1, w - 1), np.maximum(ys - 1, 0), np.minimum(ys + 1, h - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        H = (kh[0] * p[:, xm] + kh[1] * p) + kh[2] * p[:, xp]
        return canon32((kv[0] * H[ym] + kv[1] * H) + kv[2] * H[yp])


def gauss(p):
    return filter3(p, GAUSS, GAUSS)


def down(p):
    h, w = p.shape[0] // 2, p.shape[1] // 2
    with np.errstate(invalid="ignore", over="ignore"):
        return canon32((((p[0:2 * h:2, 0:2 * w:2] + p[0:2 * h:2, 1:2 * w:2]) + p[1:2 * h:2, 0:2 * w:2]) + p[1:2 * h:2, 1:2 * w:2]) / f32(4.0))


def halved(x, l):
    for _ in range(l):
        x = x * 0.5
    return x


# ---- correspondences and sums -----------------------------------------------------------------------------------------
def level_pose(K, T, l):
    f, g, a, b = (halved(v, l) for v in K)
    M = np.zeros((3, 3))
    for r in range(3):
        A = [f * T[0, c] + a * T[2, c] if r == 0 else (g * T[1, c] + b * T[2, c] if r == 1 else T[2, c]) for c in range(3)]
        M[r] = [A[0] / f, A[1] / g, (A[2] - (A[0] * a) / f) - (A[1] * b) / g]
    Kt = np.array([f * T[0, 3] + a * T[2, 3], g * T[1, 3] + b * T[2, 3], T[2, 3]])
    return M, Kt


def correspondences(K, T, l, Ds, Dt, depth_diff_max, with_keys=False):
    """(target pixels ascending, their source pixels); with_keys also every candidate (pixel, zf bits, s)."""
    h, w = Ds.shape
    M, Kt = level_pose(K, np.asarray(T, dtype=f64), l)
    s = np.flatnonzero(~np.isnan(Ds.ravel()))
    v, u = s // w, s % w
    d = Ds.ravel()[s].astype(f64)
    with np.errstate(all="ignore"):
        q = [d * ((M[r, 0] * u.astype(f64) + M[r, 1] * v.astype(f64)) + M[r, 2]) + Kt[r] for r in range(3)]
        ok = q[2] > 0.0
        x, y = q[0] / q[2] + 0.5, q[1] / q[2] + 0.5
        ok &= (np.abs(x) < 2147483648.0) & (np.abs(y) < 2147483648.0)
        ut, vt = np.trunc(np.where(ok, x, 0.0)).astype(np.int64), np.trunc(np.where(ok, y, 0.0)).astype(np.int64)
        ok &= (ut >= 0) & (ut < w) & (vt >= 0) & (vt < h)
        pix = np.where(ok, vt * w + ut, 0)
        dt = Dt.ravel()[pix]
        ok &= ~np.isnan(dt)
        ok &= np.abs(q[2] - dt.astype(f64)) <= depth_diff_max
        zf = q[2].astype(f32)
        ok &= zf <= f32(3.4028234663852886e38)
    pix, bits, s = pix[ok], zf[ok].view(np.uint32).astype(np.uint64), s[ok].astype(np.uint64)
    keys = np.full(h * w, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    np.minimum.at(keys, pix, (bits << np.uint64(32)) | s)
    tp = np.flatnonzero(keys != np.uint64(0xFFFFFFFFFFFFFFFF))
    src = (keys[tp] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    if with_keys:
        return tp, src, (pix, bits, s)
    return tp, src


def ordered_sum(n_pixels, tp, values):
    """The contract's summation order: values (len(tp) x k) at the target pixels tp of a level with n_pixels pixels."""
    k = values.shape[1]
    nblk = (n_pixels + BLOCK - 1) // BLOCK
    V = np.zeros((nblk * BLOCK, k))
    V[tp] = values
    V = V.reshape(nblk, BLOCK // 64, 64, k)
    with np.errstate(all="ignore"):
        o = 32
        while o > 0:
            V[:, :, :o] = V[:, :, :o] + V[:, :, o:2 * o]
            o //= 2
        blocks = (V[:, 0, 0] + V[:, 1, 0]) + (V[:, 2, 0] + V[:, 3, 0])
        total = np.zeros(k)
        for g0 in range(0, nblk, GROUP):
            gs = np.zeros(k)
            for b in range(g0, min(g0 + GROUP, nblk)):
                gs = gs + blocks[b]
            total = total + gs
    return total


SQRT_I, SQRT_D = math.sqrt(1.0 - 0.968), math.sqrt(0.968)


def jacobian_rows(K, T, l, lev, tp, src, jacobian):
    """Per correspondence the rows J (n x rows x 6) and residuals r (n x rows) of one iteration."""
    f, g = halved(K[0], l), halved(K[1], l)
    T = np.asarray(T, dtype=f64)
    fl = {name: lev[name].ravel() for name in PLANES}
    P = [fl[c][src].astype(f64) for c in ("X", "Y", "Z")]
    with np.errstate(all="ignore"):
        p = [((T[r, 0] * P[0] + T[r, 1] * P[1]) + T[r, 2] * P[2]) + T[r, 3] for r in range(3)]
        dp = (fl["I_t"][tp] - fl["I_s"][src]).astype(f64)
        dg = fl["D_t"][tp].astype(f64) - p[2]
        iz = 1.0 / p[2]
        gIx, gIy = 0.125 * fl["I_t_dx"][tp].astype(f64), 0.125 * fl["I_t_dy"][tp].astype(f64)
        gDx, gDy = 0.125 * fl["D_t_dx"][tp].astype(f64), 0.125 * fl["D_t_dy"][tp].astype(f64)
        gDx, gDy = np.where(np.isnan(gDx), 0.0, gDx), np.where(np.isnan(gDy), 0.0, gDy)
        c0, c1 = (gIx * f) * iz, (gIy * g) * iz
        c2 = (-(c0 * p[0] + c1 * p[1])) * iz
        J0 = [(-p[2]) * c1 + p[1] * c2, p[2] * c0 - p[0] * c2, (-p[1]) * c0 + p[0] * c1, c0, c1, c2]
        if jacobian == COLOR:
            return np.stack(J0, 1)[:, None, :], dp[:, None]
        d0, d1 = (gDx * f) * iz, (gDy * g) * iz
        d2 = (-(d0 * p[0] + d1 * p[1])) * iz
        J0 = [SQRT_I * j for j in J0]
        J1 = [SQRT_D * (((-p[2]) * d1 + p[1] * d2) - p[1]), SQRT_D * ((p[2] * d0 - p[0] * d2) + p[0]),
              SQRT_D * ((-p[1]) * d0 + p[0] * d1), SQRT_D * d0, SQRT_D * d1, SQRT_D * (d2 - 1.0)]
        return np.stack([np.stack(J0, 1), np.stack(J1, 1)], 1), np.stack([SQRT_I * dp, SQRT_D * dg], 1)


def pixel_values(J, r):
    """The 29 values per correspondence: J_i J_j (i <= j by rows), J_i r, r r, 1.0; row 0 plus row 1."""
    n = len(J)
    v = np.zeros((n, SUMS))
    with np.errstate(all="ignore"):
        k = 0
        for i in range(6):
            for j in range(i, 6):
                v[:, k] = J[:, 0, i] * J[:, 0, j] if J.shape[1] == 1 else J[:, 0, i] * J[:, 0, j] + J[:, 1, i] * J[:, 1, j]
                k += 1
        for i in range(6):
            v[:, 21 + i] = J[:, 0, i] * r[:, 0] if J.shape[1] == 1 else J[:, 0, i] * r[:, 0] + J[:, 1, i] * r[:, 1]
        v[:, 27] = r[:, 0] * r[:, 0] if J.shape[1] == 1 else r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    v[:, 28] = 1.0
    return v


def solve(tot):
    """A x = -g by the contract's LDL^T; None: the pair fails.  Python floats, one operation at a time."""
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for r in range(6):
        for q in range(r, 6):
            A[r][q] = A[q][r] = float(tot[k])
            k += 1
    L = [[0.0] * 6 for _ in range(6)]
    dd, y, x = [0.0] * 6, [0.0] * 6, [0.0] * 6
    for j in range(6):
        sj = A[j][j]
        for m in range(j):
            sj -= (L[j][m] * L[j][m]) * dd[m]
        if not math.isfinite(sj) or sj == 0.0:
            return None
        dd[j] = sj
        for i in range(j + 1, 6):
            t = A[i][j]
            for m in range(j):
                t -= (L[i][m] * L[j][m]) * dd[m]
            L[i][j] = t / sj
    det = ((((dd[0] * dd[1]) * dd[2]) * dd[3]) * dd[4]) * dd[5]
    if not abs(det) >= 1e-6:
        return None
    for i in range(6):
        t = -float(tot[21 + i])
        for m in range(i):
            t -= L[i][m] * y[m]
        y[i] = t
    for i in range(6):
        y[i] = y[i] / dd[i]
    for i in range(5, -1, -1):
        t = y[i]
        for m in range(i + 1, 6):
            t -= L[m][i] * x[m]
        x[i] = t
    return x if all(math.isfinite(v) for v in x) else None


def update(T, x):
    (sa, ca), (sb, cb), (sc, cc) = sincos(x[0]), sincos(x[1]), sincos(x[2])
    U = [[cc * cb, (cc * sb) * sa - sc * ca, (cc * sb) * ca + sc * sa, x[3]],
         [sc * cb, (sc * sb) * sa + cc * ca, (sc * sb) * ca - cc * sa, x[4]],
         [-sb, cb * sa, cb * ca, x[5]]]
    N = np.eye(4)
    for r in range(3):
        for c in range(4):
            v = (U[r][0] * float(T[0, c]) + U[r][1] * float(T[1, c])) + U[r][2] * float(T[2, c])
            N[r, c] = v + U[r][3] if c == 3 else v
    return N


def information(K, Dt, tp):
    fx, fy, cx, cy = K
    h, w = Dt.shape
    vt, ut = tp // w, tp % w
    zf = Dt.ravel()[tp]
    with np.errstate(all="ignore"):
        x = ((((ut.astype(f64) - cx) * zf.astype(f64)) * (1.0 / fx)).astype(f32)).astype(f64)
        y = ((((vt.astype(f64) - cy) * zf.astype(f64)) * (1.0 / fy)).astype(f32)).astype(f64)
        z = zf.astype(f64)
        o, e = np.zeros(len(tp)), np.ones(len(tp))
        G = [[o, z, -y, e, o, o], [-z, o, x, o, e, o], [y, -x, o, o, o, e]]
        v = np.zeros((len(tp), SUMS))
        k = 0
        for i in range(6):
            for j in range(i, 6):
                v[:, k] = (G[0][i] * G[0][j] + G[1][i] * G[1][j]) + G[2][i] * G[2][j]
                k += 1
    v[:, 28] = 1.0
    tot = ordered_sum(h * w, tp, v)
    info = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            info[i, j] = info[j, i] = tot[k]
            k += 1
    return canon64(info), int(tot[28])


# ---- the call ---------------------------------------------------------------------------------------------------------
def option(iterations=(20, 10, 5), depth_diff_max=0.03, depth_min=0.0, depth_max=4.0):
    return SimpleNamespace(iterations=tuple(iterations), depth_diff_max=depth_diff_max, depth_min=depth_min, depth_max=depth_max)


def build_pyramid(pair, opt):
    """Steps 1 .. 7: a list of levels, each a dict plane name -> float32 image."""
    K, L = pair.K, len(opt.iterations)
    Is, It = gauss(convert_color(pair.source_color)), gauss(convert_color(pair.target_color))
    Ds = gauss(convert_depth(pair.source_depth, pair.depth_scale, pair.depth_trunc, opt.depth_min, opt.depth_max))
    Dt = gauss(convert_depth(pair.target_depth, pair.depth_scale, pair.depth_trunc, opt.depth_min, opt.depth_max))
    h, w = Ds.shape
    tp, src = correspondences(K, pair.odo_init, 0, Ds, Dt, opt.depth_diff_max)
    if len(tp) > 0:
        tot = ordered_sum(h * w, tp, np.stack([Is.ravel()[src].astype(f64), It.ravel()[tp].astype(f64), np.ones(len(tp))], 1))
        with np.errstate(all="ignore"):
            ss, st = 0.5 / (tot[0] / tot[2]), 0.5 / (tot[1] / tot[2])
            Is, It = canon32((ss * Is.astype(f64)).astype(f32)), canon32((st * It.astype(f64)).astype(f32))
    xs, ys = np.meshgrid(np.arange(w, dtype=f64), np.arange(h, dtype=f64))
    with np.errstate(all="ignore"):
        X = canon32((((xs - K[2]) * Ds.astype(f64)) * (1.0 / K[0])).astype(f32))
        Y = canon32((((ys - K[3]) * Ds.astype(f64)) * (1.0 / K[1])).astype(f32))
    levels = [dict(I_s=Is, I_t=It, D_s=Ds, D_t=Dt, X=X, Y=Y, Z=Ds.copy())]
    for _ in range(L - 1):
        p = levels[-1]
        n = {k: down(gauss(p[k])) for k in ("I_s", "I_t")}
        n.update({k: down(p[k]) for k in ("D_s", "D_t", "X", "Y", "Z")})
        levels.append(n)
    for p in levels:
        p["I_t_dx"], p["I_t_dy"] = filter3(p["I_t"], SOBEL_D, SOBEL_S), filter3(p["I_t"], SOBEL_S, SOBEL_D)
        p["D_t_dx"], p["D_t_dy"] = filter3(p["D_t"], SOBEL_D, SOBEL_S), filter3(p["D_t"], SOBEL_S, SOBEL_D)
    return levels


def pyramid_floats(levels):
    """The layout of images_out."""
    return np.concatenate([lev[name].ravel() for lev in levels for name in PLANES])


def compute(pair, opt):
    """success, transformation, information, count, iterations and the trace (a list of dicts)."""
    levels = build_pyramid(pair, opt)
    L = len(levels)
    T = np.array(pair.odo_init, dtype=f64)
    T[3] = [0.0, 0.0, 0.0, 1.0]
    trace, failed, count, done = [], False, 0, 0
    for l in range(L - 1, -1, -1):
        lev = levels[l]
        h, w = lev["D_s"].shape
        for _ in range(opt.iterations[L - 1 - l]):
            if failed:
                trace.append(dict(level=0, executed=0, count=0, failed=0, e=0.0, A=np.zeros(21), g=np.zeros(6), pose=np.zeros(16)))
                continue
            tp, src = correspondences(pair.K, T, l, lev["D_s"], lev["D_t"], opt.depth_diff_max)
            J, r = jacobian_rows(pair.K, T, l, lev, tp, src, pair.jacobian)
            tot = ordered_sum(h * w, tp, pixel_values(J, r))
            count, done = int(tot[28]), done + 1
            x = solve(tot)
            failed = x is None
            T = np.eye(4) if failed else update(T, x)
            trace.append(dict(level=l, executed=1, count=count, failed=int(failed), e=canon64(tot[27]), A=canon64(tot[:21]),
                              g=canon64(tot[21:27]), pose=T.ravel().copy()))
    info = np.zeros((6, 6))
    if not failed:
        tp, _ = correspondences(pair.K, T, 0, levels[0]["D_s"], levels[0]["D_t"], opt.depth_diff_max)
        info, count = information(pair.K, levels[0]["D_t"], tp)
    return SimpleNamespace(success=int(not failed), transformation=T, information=info, count=count, iterations=done,
                           trace=trace, levels=levels)


# ---- scenes -----------------------------------------------------------------------------------------------------------
PLANE_N, PLANE_D = np.array([0.1, -0.2, 1.0]) / np.linalg.norm([0.1, -0.2, 1.0]), 2.0
BALLS = (((-0.4, -0.3, 1.9), 0.35), ((0.5, 0.2, 1.8), 0.3), ((0.0, 0.45, 2.0), 0.25), ((0.35, -0.45, 1.95), 0.2))


def camera(w, h):
    return (0.9 * w, 0.85 * w, (w - 1) / 2.0, (h - 1) / 2.0)


def pose(rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0)):
    """Rz Ry Rx and the translation as a 4 x 4 matrix (numpy's own sine and cosine: a scene, not the contract)."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    E = np.eye(4)
    E[:3, :3] = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
                 @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    E[:3, 3] = t
    return E


def render(w, h, K, cam_pose):
    """(depth in metres float64, intensity float64 in (0, 1)) of the wall and its balls from the camera-to-world pose:
    every pixel a closed-form ray hit, the intensity a function of the hit point, so two views agree on it."""
    fx, fy, cx, cy = K
    i, j = np.meshgrid(np.arange(h, dtype=f64), np.arange(w, dtype=f64), indexing="ij")
    dirs = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones_like(i)], 2) @ cam_pose[:3, :3].T
    o = cam_pose[:3, 3]
    t = (PLANE_D - PLANE_N @ o) / (dirs @ PLANE_N)
    for c, rad in BALLS:
        oc = o - np.array(c)
        a, b, cc = (dirs * dirs).sum(2), 2.0 * (dirs @ oc), oc @ oc - rad * rad
        disc = b * b - 4.0 * a * cc
        with np.errstate(invalid="ignore"):
            hit = (-b - np.sqrt(disc)) / (2.0 * a)
        t = np.where((disc >= 0) & (hit > 0) & (hit < t), hit, t)
    X = o + dirs * t[:, :, None]
    tex = 0.5 + 0.2 * np.sin(9.0 * X[:, :, 0] + 2.0 * X[:, :, 2]) * np.cos(7.0 * X[:, :, 1]) + 0.15 * np.sin(5.0 * X[:, :, 0] - 11.0 * X[:, :, 1])
    return t, tex


def as_uint16(metres, pad=0):
    mm = np.rint(metres * 1000.0).astype(np.uint16)
    if not pad:
        return mm
    big = np.full((mm.shape[0], mm.shape[1] + pad), 7, dtype=np.uint16)
    big[:, :mm.shape[1]] = mm
    return big[:, :mm.shape[1]]


def as_rgb8(tex, pad=0):
    h, w = tex.shape
    g = np.clip(np.rint(tex * 255.0), 0, 255)
    img = np.stack([g, np.clip(g + 3, 0, 255), np.clip(g - 2, 0, 255)], 2).astype(np.uint8)
    if not pad:
        return img
    big = np.full((h, w + pad, 3), 9, dtype=np.uint8)
    big[:, :w] = img
    return big[:, :w]


def make_pair(w, h, motion, jacobian=HYBRID, odo_init=None, depth="u16", color="rgb8", pad=0, depth_trunc=3.0):
    """Source at the identity, target camera at `motion`^-1 ... the transformation source -> target IS `motion`."""
    K = camera(w, h)
    ds, cs = render(w, h, K, np.eye(4))
    dt, ct = render(w, h, K, np.linalg.inv(motion))
    dconv = (lambda d: as_uint16(d, pad)) if depth == "u16" else (lambda d: d.astype(f32))
    cconv = (lambda c: as_rgb8(c, pad)) if color == "rgb8" else (lambda c: c.astype(f32))
    return SimpleNamespace(K=K, source_depth=dconv(ds), source_color=cconv(cs), target_depth=dconv(dt), target_color=cconv(ct),
                           odo_init=np.eye(4) if odo_init is None else np.array(odo_init, dtype=f64), jacobian=jacobian,
                           depth_scale=1000.0, depth_trunc=depth_trunc, truth=motion)


SMALL = pose(0.01, -0.015, 0.008, (0.012, -0.008, 0.01))


_cases = None


def cases():
    """name -> SimpleNamespace(pair, opt, host: also in the host driver's file).  Built once."""
    global _cases
    if _cases is not None:
        return _cases
    c = {}

    def add(name, pair, opt=None, host=True):
        c[name] = SimpleNamespace(name=name, pair=pair, opt=opt or option((3, 2, 2)), host=host)
    add("8x8", make_pair(8, 8, SMALL))
    add("4x4", make_pair(4, 4, SMALL, jacobian=COLOR))
    add("37x29", make_pair(37, 29, SMALL, pad=3))
    add("64x48", make_pair(64, 48, SMALL), option((4, 3, 2)), host=False)
    add("64x48_color", make_pair(64, 48, SMALL, jacobian=COLOR, color="f32"), option((4, 3, 2)), host=False)
    # the reduction's block edges: exactly one block, one less, one more, one more than a group of blocks
    add("block", make_pair(16, 16, SMALL), option((2, 2)))
    add("block-1", make_pair(17, 15, SMALL), option((2, 2)))
    add("block+1", make_pair(257, 1, pose(t=(0.004, 0.0, 0.0))), option((2,)))
    add("group+1", make_pair(145, 113, SMALL), option((1, 1)), host=False)   # 145 x 113 = 64 x 256 + 1
    # float32 depth with the special samples, float32 intensity with a NaN
    p = make_pair(37, 29, SMALL, depth="f32", color="f32")
    for d in (p.source_depth, p.target_depth):
        d[0, 0], d[1, 2], d[2, 1], d[14, 18], d[9, 9] = 0.0, np.nan, -1.0, np.inf, f32(-0.0)
    add("f32_specials", p)
    add("big_init", make_pair(64, 48, pose(0.05, -0.06, 0.04, (0.06, -0.04, 0.03)),
                              odo_init=pose(0.04, -0.05, 0.03, (0.05, -0.03, 0.02))), option((3, 2, 2)), host=False)
    add("no_correspondence", make_pair(16, 12, SMALL, odo_init=pose(t=(0.0, 0.0, 5.0))))
    # a constant-depth plane under a pure zoom: several source pixels fall into one target pixel with EQUAL float32 depth
    flat = make_pair(24, 20, np.eye(4), depth="f32")
    flat.source_depth[:], flat.target_depth[:] = f32(1.5), f32(1.0)
    flat.odo_init = pose(t=(0.0, 0.0, -0.5))
    add("ties", flat, option((2, 1), depth_diff_max=0.6))
    add("depth_diff", make_pair(37, 29, pose(0.0, 0.0, 0.0, (0.1, 0.0, 0.0))), option((2, 2), depth_diff_max=0.01))
    add("depth_range", make_pair(37, 29, SMALL), option((2, 2), depth_min=1.7, depth_max=1.95))
    blank = make_pair(16, 12, SMALL, jacobian=COLOR)
    blank.source_color[:], blank.target_color[:] = 128, 128
    add("singular", blank, option((2, 2)))
    blank3 = make_pair(16, 12, SMALL, jacobian=COLOR)  # the same under the options most cases share: for mixed batches
    blank3.source_color[:], blank3.target_color[:] = 128, 128
    add("singular_3_levels", blank3, option((3, 2, 2)), host=False)
    add("skip_level", make_pair(37, 29, SMALL), option((0, 3)))
    add("no_iteration", make_pair(16, 12, SMALL, odo_init=pose(0.0, 0.01, 0.0, (0.01, 0.0, 0.0))), option((0,)))
    _cases = c
    return c


_results, _pyramids = {}, {}


def result(name):
    if name not in _results:
        cs = cases()[name]
        _results[name] = compute(cs.pair, cs.opt)
    return _results[name]


def pyramid(name):
    if name not in _pyramids:
        _pyramids[name] = pyramid_floats(result(name).levels)
    return _pyramids[name]



WIDE_BATCH = 320
WIDE_CYCLE = ("4x4", "8x8", "37x29", "no_correspondence", "f32_specials", "big_init")
WIDE_SINGULAR = (255, 257)  # where the pair that fails (a singular system) stands in the wide batch


def wide_batch():
    """The names of 320 cases that share the options (3, 2, 2): WIDE_CYCLE in turn, with the textureless pair, whose
    system is singular, at 255 and 257.  What the wide test rests on is asserted from the sizes alone."""
    names = [WIDE_CYCLE[i % len(WIDE_CYCLE)] for i in range(WIDE_BATCH)]
    for i in WIDE_SINGULAR:
        names[i] = "singular_3_levels"
    c = cases()
    assert len(names) > 256 and len({c[n].opt.iterations for n in names}) == 1 and c[names[0]].opt.iterations == (3, 2, 2)
    def blocks(n, l):
        h, w = c[n].pair.source_depth.shape
        return -(-((h >> l) * (w >> l)) // BLOCK)

    for l in range(3):  # blk_pair: the blocks of level 0 of all pairs, then level 1, ...: past 256 of them at every level
        assert sum(blocks(n, l) for n in names) > 256
    assert sum(blocks(n, 0) for n in names) > 1024
    assert names[256] not in (names[255], names[0]) and names[254] != names[258]
    return names
