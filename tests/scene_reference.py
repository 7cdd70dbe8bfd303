"""The numpy restatement of "Ray casting scene" (include/teaser_hip.h): brute force over ALL triangles, chunked, with
exactly the arithmetic of the header -- double on the float32 inputs, no fused product-add (numpy has none), every
three-term sum (a + b) + c, cross products by components.  There is no search structure here: this is what the
structure of the library must equal.  Also the scenes and queries the host and GPU tests share (cases())."""
import functools

import numpy as np

NONE = np.uint32(0xFFFFFFFF)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


class Triangles:
    """The triangles of a list of geometries [(vertices, triangles), ...] in global order."""

    def __init__(self, geoms):
        v0, v1, v2, gid, pid = [], [], [], [], []
        for k, (vert, tri) in enumerate(geoms):
            vert = np.asarray(vert, dtype=np.float32).reshape(-1, 3).astype(np.float64)
            tri = np.asarray(tri, dtype=np.uint32).reshape(-1, 3).astype(np.int64)
            v0.append(vert[tri[:, 0]]), v1.append(vert[tri[:, 1]]), v2.append(vert[tri[:, 2]])
            gid.append(np.full(len(tri), k, dtype=np.uint32)), pid.append(np.arange(len(tri), dtype=np.uint32))
        cat = lambda a, w: np.concatenate(a) if a else np.zeros((0,) + w)
        self.v0, self.v1, self.v2 = cat(v0, (3,)), cat(v1, (3,)), cat(v2, (3,))
        self.gid = cat(gid, ()).astype(np.uint32)
        self.pid = cat(pid, ()).astype(np.uint32)
        self.e1, self.e2 = self.v1 - self.v0, self.v2 - self.v0
        self.n = _cross(self.e1, self.e2)
        self.dead = np.all(self.n == 0.0, axis=1)
        with np.errstate(all="ignore"):
            self.normal = (self.n / np.sqrt(_dot(self.n, self.n))[:, None]).astype(np.float32)

    def __len__(self):
        return len(self.v0)


def _ray_pairs(T, rays):
    """hit (r x nt) and t, u, v of every (ray, triangle) pair."""
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, 6)
    valid = np.all(np.isfinite(rays), axis=1) & np.any(rays[:, 3:] != 0.0, axis=1)
    o, d = rays[:, None, :3].astype(np.float64), rays[:, None, 3:].astype(np.float64)
    with np.errstate(all="ignore"):
        p = _cross(d, T.e2[None])
        det = _dot(T.e1[None], p)
        inv = 1.0 / det
        s = o - T.v0[None]
        u = _dot(s, p) * inv
        q = _cross(s, T.e1[None])
        v = _dot(d, q) * inv
        t = _dot(T.e2[None], q) * inv
        hit = (valid[:, None] & ~T.dead[None] & (det != 0.0) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0)
               & (t >= 0.0) & (t < np.inf))
    return hit, t, u, v


def _empty_result(n, key, with_closest):
    out = {key: np.full(n, np.inf, dtype=np.float32), "geometry_ids": np.full(n, NONE, dtype=np.uint32),
           "primitive_ids": np.full(n, NONE, dtype=np.uint32), "primitive_uvs": np.zeros((n, 2), dtype=np.float32),
           "primitive_normals": np.zeros((n, 3), dtype=np.float32)}
    if with_closest:
        out["points"] = np.zeros((n, 3), dtype=np.float32)
    return out


def cast_rays(geoms, rays, chunk=256):
    T = geoms if isinstance(geoms, Triangles) else Triangles(geoms)
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, 6)
    out = _empty_result(len(rays), "t_hit", False)
    if len(T) == 0:
        return out
    for a in range(0, len(rays), chunk):
        hit, t, u, v = _ray_pairs(T, rays[a:a + chunk])
        tm = np.where(hit, t, np.inf)
        g = np.argmin(tm, axis=1)  # the first minimum: the smallest global index among equal t
        r = np.flatnonzero(hit.any(axis=1))
        g = g[r]
        out["t_hit"][a + r] = t[r, g].astype(np.float32)
        out["geometry_ids"][a + r], out["primitive_ids"][a + r] = T.gid[g], T.pid[g]
        out["primitive_uvs"][a + r] = np.stack([u[r, g], v[r, g]], axis=1).astype(np.float32)
        out["primitive_normals"][a + r] = T.normal[g]
    return out


def test_occlusions(geoms, rays, tnear=0.0, tfar=np.inf, chunk=256):
    T = geoms if isinstance(geoms, Triangles) else Triangles(geoms)
    rays = np.asarray(rays, dtype=np.float32).reshape(-1, 6)
    out = np.zeros(len(rays), dtype=np.uint8)
    if len(T) == 0:
        return out
    for a in range(0, len(rays), chunk):
        hit, t, _, _ = _ray_pairs(T, rays[a:a + chunk])
        out[a:a + chunk] = (hit & (tnear <= t) & (t <= tfar)).any(axis=1)
    return out


test_occlusions.__test__ = False  # not a pytest test


def closest_point_pairs(T, pts):
    """Ericson 5.1.5 for every (point, triangle) pair: c* (r x nt x 3), (v, w), d2*, the region 0 .. 6 and `live`."""
    p = np.asarray(pts, dtype=np.float32).reshape(-1, 1, 3).astype(np.float64)
    a, b, c, ab, ac = T.v0[None], T.v1[None], T.v2[None], T.e1[None], T.e2[None]
    with np.errstate(all="ignore"):
        ap = p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        rules = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0),
                 (d6 >= 0.0) & (d5 <= d6), (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0),
                 (va <= 0.0) & ((d4 - d3) >= 0.0) & ((d5 - d6) >= 0.0)]
        region = np.select(rules, [0, 1, 2, 3, 4, 5], default=6)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1.0 / ((va + vb) + vc)
        v_f, w_f = vb * denom, vc * denom
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        v = np.select([region == k for k in range(6)], [zero, one, v_ab, zero, zero, 1.0 - w_bc], default=v_f)
        w = np.select([region == k for k in range(6)], [zero, zero, zero, one, w_ac, w_bc], default=w_f)
        pts_of = [a + zero[..., None], b + zero[..., None], a + v_ab[..., None] * ab, c + zero[..., None],
                  a + w_ac[..., None] * ac, b + w_bc[..., None] * (c - b), (a + ab * v_f[..., None]) + ac * w_f[..., None]]
        cs = np.select([(region == k)[..., None] for k in range(6)], pts_of[:6], default=pts_of[6])
        x = cs - p
        dd = (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]
        live = ~T.dead[None] & (dd < np.inf) & np.all(np.isfinite(p), axis=2)
    return cs, v, w, dd, region, live


def closest_points(geoms, pts, chunk=256):
    T = geoms if isinstance(geoms, Triangles) else Triangles(geoms)
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    out = _empty_result(len(pts), "distance", True)
    if len(T) == 0:
        return out
    for a in range(0, len(pts), chunk):
        cs, v, w, dd, _, live = closest_point_pairs(T, pts[a:a + chunk])
        dm = np.where(live, dd, np.inf)
        g = np.argmin(dm, axis=1)
        r = np.flatnonzero(live.any(axis=1))
        g = g[r]
        out["distance"][a + r] = np.sqrt(dd[r, g]).astype(np.float32)
        out["points"][a + r] = cs[r, g].astype(np.float32)
        out["geometry_ids"][a + r], out["primitive_ids"][a + r] = T.gid[g], T.pid[g]
        out["primitive_uvs"][a + r] = np.stack([v[r, g], w[r, g]], axis=1).astype(np.float32)
        out["primitive_normals"][a + r] = T.normal[g]
    return out


def create_rays_pinhole(intrinsic, extrinsic, width, height, pixel_offset=0.5):
    """The rays of a view (height x width x 6 float32) by the formulas of the header."""
    K, E = np.asarray(intrinsic, dtype=np.float64), np.asarray(extrinsic, dtype=np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    with np.errstate(all="ignore"):
        a = ((np.arange(width, dtype=np.float64) + pixel_offset) - cx) / fx
        b = ((np.arange(height, dtype=np.float64) + pixel_offset) - cy) / fy
        rays = np.zeros((height, width, 6), dtype=np.float32)
        for k in range(3):
            rays[..., k] = np.float32(-((E[0, k] * E[0, 3] + E[1, k] * E[1, 3]) + E[2, k] * E[2, 3]))
            rays[..., 3 + k] = ((E[0, k] * a[None, :] + E[1, k] * b[:, None]) + E[2, k]).astype(np.float32)
    return rays


# ---- the scenes and queries of the tests ------------------------------------------------------------------------------

def sheet(n=9, offset=(0.0, 0.0, 0.0)):
    """An n x n integer-lattice sheet in the plane z = 0: 2 (n - 1)^2 triangles."""
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    vert = np.stack([ii.ravel(), jj.ravel(), np.zeros(n * n)], axis=1).astype(np.float32) + np.asarray(offset, dtype=np.float32)
    tri = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
            tri += [(a, b, c), (a, c, d)]
    return vert.astype(np.float32), np.array(tri, dtype=np.uint32)


def _rays(o, d):
    o, d = np.asarray(o, dtype=np.float32).reshape(-1, 3), np.asarray(d, dtype=np.float32).reshape(-1, 3)
    if len(d) == 1:
        d = np.repeat(d, len(o), axis=0)
    return np.concatenate([o, d], axis=1).astype(np.float32)


def lattice_rays(offset=(0.0, 0.0, 0.0)):
    ii, jj = np.meshgrid(np.arange(9.0), np.arange(9.0), indexing="ij")
    verts = np.stack([ii.ravel(), jj.ravel(), np.full(81, 5.0)], axis=1)
    edge = np.stack([ii.ravel()[:72] + 0.5, jj.ravel()[:72], np.full(72, 3.0)], axis=1)
    diag = np.stack([ii.ravel()[:64] % 8 + 0.5, jj.ravel()[:64] % 8 + 0.5, np.full(64, -2.0)], axis=1)
    parts = [_rays(verts, [0, 0, -1]),                       # through lattice vertices: two zero components, six-way ties
             _rays(edge, [0, 0, -1]), _rays(diag, [0, 0, 1]),  # along shared edges and diagonals, from both sides
             _rays(verts - [0, 3, 0], [0, 1, -1]), _rays(verts + [2, 0, -10], [-1, 0, 1]),  # one zero component
             _rays([[-1, 2, 0], [-1, 2.5, 0], [4, -3, 0], [9, 9, 0]], [[1, 0, 0], [1, 0, 0], [0, 1, 0], [-1, -1, 0]]),  # in the plane
             _rays([[2.25, 3.25, 0], [4, 4, 0], [0, 0, 0], [8, 8, 0], [3.5, 3.5, 0]], [0, 0, 1]),  # origins on the sheet
             _rays([[2.25, 3.25, 0], [4, 4, 0], [3, 2.5, 0]], [1, 1, 1]),
             _rays([[20, 20, 5], [-3, 4, 1], [4, 4, 1]], [[0, 0, -1], [0, 0, 1], [0, 0, 0]])]  # beside, away, no direction
    r = np.concatenate(parts)
    r[:, :3] += np.asarray(offset, dtype=np.float32)
    return r.astype(np.float32)


def lattice_points(offset=(0.0, 0.0, 0.0)):
    ii, jj = np.meshgrid(np.arange(9.0), np.arange(9.0), indexing="ij")
    on = np.stack([ii.ravel(), jj.ravel(), np.zeros(81)], axis=1)
    parts = [on, on + [0, 0, 2], on[:72] + [0.5, 0, 0], on[:72] + [0.5, 0, 1], on[:64] % 8 + [0.5, 0.5, -1],
             on[:64] % 8 + [0.25, 0.5, 3], [[-2, -2, 0], [10, 4, 0], [4, 12, -1], [8e4, 0, 0], [4, 4, 8e4], [-8e4, -8e4, 8e4]]]
    p = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in parts])
    return (p + np.asarray(offset, dtype=np.float64)).astype(np.float32)


def axis_aligned():
    """Triangles in planes x = c, y = c and z = c (boxes of zero thickness) and rays that graze their edges."""
    vert, tri = [], []
    for axis in range(3):
        for c in (0.0, 1.0, 2.5):
            for (p, q) in (((0, 0), (2, 0)), ((1, 1), (3, 2))):
                base = len(vert)
                for (s, t) in (p, q, (p[0], q[1] + 2)):
                    x = [0.0, 0.0, 0.0]
                    x[axis], x[(axis + 1) % 3], x[(axis + 2) % 3] = c, float(s), float(t)
                    vert.append(x)
                tri.append((base, base + 1, base + 2))
    vert, tri = np.array(vert, dtype=np.float32), np.array(tri, dtype=np.uint32)
    o, d = [], []
    for axis in range(3):
        for s in np.arange(-0.5, 3.51, 0.5):
            for t in (0.0, 1.0, 2.0, 3.0, 4.0):
                x = [0.0, 0.0, 0.0]
                x[axis], x[(axis + 1) % 3], x[(axis + 2) % 3] = -4.0, float(s), float(t)
                dd = [0.0, 0.0, 0.0]
                dd[axis] = 1.0
                o.append(x), d.append(dd)  # through edge points and vertices, perpendicular to the planes
                dd2 = list(dd)
                dd2[(axis + 1) % 3] = 0.5
                o.append(x), d.append(dd2)
    pts = np.array(o, dtype=np.float32) * 0.5 + 0.25
    return [(vert, tri)], _rays(o, d), pts


def with_dead(vert, tri):
    """The mesh with DEAD triangles mixed in: a repeated vertex, three collinear lattice points, one point thrice."""
    tri = [tuple(t) for t in tri]
    dead = [(0, 0, 1), (0, 1, 2), (40, 40, 40), (0, 10, 20), (3, 3, 3)]
    out, k = [], 0
    for i, t in enumerate(tri):
        if i % 25 == 0:
            out.append(dead[k % len(dead)])
            k += 1
        out.append(t)
    return vert, np.array(out, dtype=np.uint32)


def random_scene(seed, nt, scale=1.0):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1.0, 1.0, (nt, 1, 3))
    vert = (centre + rng.uniform(-0.15, 0.15, (nt, 3, 3))) * scale
    return vert.reshape(-1, 3).astype(np.float32), np.arange(3 * nt, dtype=np.uint32).reshape(-1, 3)


def random_queries(seed, n, scale=1.0):
    """Half the origins inside the bounds, half far outside; one ray in eight points away from the scene."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.0, 1.0, (n, 3))
    o[n // 2:] *= rng.uniform(20.0, 200.0, (n - n // 2, 1))
    target = rng.uniform(-1.0, 1.0, (n, 3))
    d = (target - o) * rng.uniform(0.1, 3.0, (n, 1))
    d[::8] *= -1.0
    d[5::64, 0] = 0.0
    return np.concatenate([o, d], axis=1).astype(np.float32) * np.float32(scale), (o * scale).astype(np.float32)


def mixed_sizes(seed=5):
    v1, t1 = random_scene(seed, 150, 1e-3)
    v2, t2 = random_scene(seed + 1, 60, 1e3)
    return [(v1, t1), (v2, t2)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (geoms, rays, points, host): the scenes of the host driver (host) and of the GPU tests (all)."""
    off = (1e4, -1e4, 1e4)
    out = {}
    for nt in (0, 1, 2, 3):
        rays, pts = random_queries(10 + nt, 257)
        geom = random_scene(nt, nt)
        if nt:  # two rays in three aim at a triangle
            aim = geom[0].reshape(nt, 3, 3).mean(axis=1)[np.arange(257) % nt] + np.random.default_rng(nt).uniform(-0.1, 0.1, (257, 3))
            rays[::3, 3:] *= np.float32(0.0)
            rays[:, 3:] = np.where(rays[:, 3:] == 0, rays[:, 3:], (aim - rays[:, :3]).astype(np.float32))
        out["small%d" % nt] = ([geom], rays, pts[:65], True)
    tri0 = np.array([[0.5, 0.25, 0.0], [1.5, 0.5, 0.25], [0.75, 1.5, -0.25]], dtype=np.float32)
    rays, pts = random_queries(20, 130)
    rays[:, 3:] = (tri0.mean(axis=0) * np.float32(1.0) - rays[:, :3]) + np.float32(0.05) * rays[:, 3:]
    out["duplicates"] = ([(np.tile(tri0, (200, 1)), np.arange(600, dtype=np.uint32).reshape(-1, 3))], rays, pts, True)
    k = np.arange(300, dtype=np.float64)[:, None]
    line = (np.array([[-0.1, 0.0, 0.0], [0.1, 0.0, 0.05], [0.0, 0.1, -0.05]])[None] + (k * [0.01, 0.02, -0.005])[:, None, :])
    rays, pts = random_queries(21, 200)
    rays[:, 3:] = ((k[:200] * [0.01, 0.02, -0.005]) - rays[:, :3].astype(np.float64)).astype(np.float32)
    out["line"] = ([(line.reshape(-1, 3).astype(np.float32), np.arange(900, dtype=np.uint32).reshape(-1, 3))], rays, pts, True)
    out["lattice"] = ([sheet()], lattice_rays(), lattice_points(), True)
    out["offset"] = ([sheet(offset=off)], lattice_rays(off), lattice_points(off), True)
    g, r, p = axis_aligned()
    out["axis_aligned"] = (g, r, p, True)
    out["dead"] = ([with_dead(*sheet())], lattice_rays(), lattice_points(), True)
    rays, pts = random_queries(22, 300)
    out["mixed_sizes"] = (mixed_sizes(), np.concatenate([rays, rays * np.float32(1e3), rays * np.float32(1e-3)]),
                          np.concatenate([pts, pts * np.float32(1e3), pts * np.float32(1e-3)]), True)
    rays, pts = random_queries(23, 400)
    out["two_geometries"] = ([random_scene(30, 40), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)),
                              random_scene(31, 70)], rays, pts, True)
    rays, pts = random_queries(24, 512)
    out["random_host"] = ([random_scene(32, 300)], rays, pts, True)
    rays, pts = random_queries(25, 4096)
    out["random"] = ([random_scene(33, 2000)], rays, pts, False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(cast_rays, closest_points) of a case, computed once."""
    geoms, rays, pts, _ = cases()[name]
    T = Triangles(geoms)
    return cast_rays(T, rays), closest_points(T, pts)


def views_case():
    """Two views of different sizes and a 0 x 0 one over the lattice sheet: (K, E, width, height) each."""
    c, s = np.cos(0.3), np.sin(0.3)
    E1 = np.array([[1, 0, 0, -4.0], [0, c, -s, -3.0], [0, s, c, 6.0], [0, 0, 0, 1]])
    E2 = np.array([[c, 0, s, -3.5], [0, -1, 0, 4.25], [s, 0, -c, 5.0], [0, 0, 0, 1]])
    K1 = np.array([[12.0, 0, 8.0], [0, 12.0, 4.0], [0, 0, 1]])
    K2 = np.array([[40.0, 0, 31.5], [0, 42.0, 23.5], [0, 0, 1]])
    return [(K1, E1, 17, 9), (K2, E2, 64, 48), (K1, E1, 0, 0)]
