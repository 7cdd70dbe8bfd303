"""A ray-casting scene for triangle meshes on the GPU with the surface of open3d.t.geometry.RaycastingScene: meshes in,
then the first surface a ray meets, occlusion tests and the closest point of the surface to a point.

    scene = RaycastingScene()
    scene.add_triangles(mesh)                              # a TSDFTriangleMesh, or (vertices, triangles)
    hit = scene.cast_rays(rays)                            # t_hit, geometry_ids, primitive_ids, primitive_uvs, primitive_normals
    d = scene.compute_distance(cloud.points)               # scan to mesh
    depth = scene.render_depth(intrinsic, extrinsic)       # float32 metres, 0 where nothing was met

The arithmetic is written out in include/teaser_hip.h ("Ray casting scene"): double on float32 inputs, the nearest hit
by (t, global triangle index), Ericson's closest point; every output equals a brute force over all triangles and has the
same bits for any grouping of the queries into calls.  Bit parity with an Open3D or Embree binary is not claimed.  Rays
are ``n x 6`` float32 (origin, direction; the direction is used as given, so t counts in units of its length).  Every
scene has a handle of its own (a lock serialises its calls).  Without a GPU the constructor raises TeaserHipError
(NO_DEVICE): there is no CPU path.

Not offered: signed distance and occupancy, count_intersections / list_intersections, lines and other primitives,
refitting after vertex motion, mesh sampling."""
import ctypes as C
import threading

import numpy as np

from .rgbd import _each, _fxfycxcy, _is_intrinsic, _is_scalar

_vp, _fp, _i64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64)
_u32p, _u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)

INVALID_ID = 0xFFFFFFFF  # Open3D's RaycastingScene.INVALID_ID


class SceneViewC(C.Structure):
    """teaser_scene_view_c (include/teaser_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("extrinsic", C.c_double * 16), ("pixel_offset", C.c_double), ("reserved", C.c_int64)]


assert C.sizeof(SceneViewC) == 184  # as the header asserts


def declare(L):
    """ctypes signatures of the entry points (called by the package's lib())."""
    L.teaser_hip_scene_create.argtypes = [C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_scene_destroy.argtypes = [_vp]
    L.teaser_hip_scene_last_error.argtypes = [_vp]
    L.teaser_hip_scene_last_error.restype = C.c_char_p
    L.teaser_hip_scene_fill_scratch.argtypes = [_vp, C.c_int32, _i64p]
    L.teaser_hip_scene_add_triangles.argtypes = [_vp, _fp, C.c_int64, _u32p, C.c_int64, _u32p]
    L.teaser_hip_scene_commit.argtypes = [_vp]
    L.teaser_hip_scene_triangle_count.argtypes = [_vp, _i64p]
    L.teaser_hip_scene_cast_rays.argtypes = [_vp, _fp, C.c_int64, _fp, _u32p, _u32p, _fp, _fp]
    L.teaser_hip_scene_test_occlusions.argtypes = [_vp, _fp, C.c_int64, C.c_double, C.c_double, _u8p]
    L.teaser_hip_scene_closest_points.argtypes = [_vp, _fp, C.c_int64, _fp, _fp, _u32p, _u32p, _fp, _fp]
    L.teaser_hip_scene_view_default.argtypes = [C.POINTER(SceneViewC)]
    L.teaser_hip_scene_cast_views.argtypes = [_vp, C.POINTER(SceneViewC), C.c_int32, C.POINTER(_fp), C.POINTER(_u32p),
                                              C.POINTER(_u32p), C.POINTER(_fp), C.POINTER(_fp)]


def create_rays_pinhole(intrinsic_matrix, extrinsic_matrix, width_px, height_px, pixel_offset=0.5):
    """Open3D's RaycastingScene.create_rays_pinhole on the host: ``height x width x 6`` float32 rays (origin, direction)
    of a pinhole camera, by the formulas of the header ("Views"), in double and rounded to float32.  The direction has
    z-depth 1, so the t of a hit is the depth.  ``pixel_offset`` 0.5 looks through pixel centres (Open3D's rays), 0 through
    the pixels' corners (the convention of the depth frames of this library)."""
    fx, fy, cx, cy = _fxfycxcy(intrinsic_matrix)
    E = np.array(extrinsic_matrix, dtype=np.float64)
    if E.shape != (4, 4):
        raise ValueError("extrinsic must be a 4 x 4 matrix")
    w, h, off = int(width_px), int(height_px), float(pixel_offset)
    if w < 0 or h < 0:
        raise ValueError("width and height must be >= 0")
    rays = np.zeros((h, w, 6), dtype=np.float32)
    with np.errstate(all="ignore"):
        a = ((np.arange(w, dtype=np.float64) + off) - cx) / fx
        b = ((np.arange(h, dtype=np.float64) + off) - cy) / fy
        for k in range(3):
            rays[..., k] = np.float32(-((E[0, k] * E[0, 3] + E[1, k] * E[1, 3]) + E[2, k] * E[2, 3]))
            rays[..., 3 + k] = ((E[0, k] * a[None, :] + E[1, k] * b[:, None]) + E[2, k]).astype(np.float32)
    return rays


def _ptr(a, ty):
    return None if a is None or a.size == 0 else a.ctypes.data_as(ty)


class RaycastingScene:
    """Open3D's t.geometry.RaycastingScene on ``device`` (-1: the current one)."""
    INVALID_ID = INVALID_ID

    def __init__(self, device=-1):
        from . import TeaserHipError, lib
        self._lib = lib()
        self._h = _vp()
        self._lock = threading.Lock()
        rc = self._lib.teaser_hip_scene_create(int(device), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise TeaserHipError(rc, "(no MI355X visible: the product has no CPU path)" if rc == 3 else "")

    # ---- the handle ---------------------------------------------------------------------------------------------
    def _call(self, fn, *args):
        from . import TeaserHipError
        if self._h is None:
            raise ValueError("the scene is closed")
        with self._lock:  # the handle serves one call at a time
            rc = fn(self._h, *args)
            err = self._lib.teaser_hip_scene_last_error(self._h).decode() if rc != 0 else ""
        if rc != 0:
            raise TeaserHipError(rc, err)

    def fill_scratch(self, byte):
        """DIAGNOSTIC (teaser_hip_scene_fill_scratch): sets every byte of the handle's scratch and staging buffers to
        `byte` (0 .. 255) and returns the device bytes filled.  The triangles and the tree are state and left alone."""
        filled = C.c_int64()
        self._call(self._lib.teaser_hip_scene_fill_scratch, int(byte), C.byref(filled))
        return filled.value

    def close(self):
        """Frees the scene; the object is unusable afterwards."""
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            self._lib.teaser_hip_scene_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- geometries ---------------------------------------------------------------------------------------------
    def add_triangles(self, vertices, triangles=None):
        """Adds a mesh and returns its geometry id (0, 1, 2, ...).  ``vertices`` n x 3 (converted to float32) with
        ``triangles`` m x 3 indices, or a mesh object with ``.vertices`` and ``.triangles`` (a TSDFTriangleMesh).  May
        follow queries: the next query rebuilds."""
        if triangles is None:
            vertices, triangles = vertices.vertices, vertices.triangles
        vert = np.asarray(vertices)
        tri = np.asarray(triangles)
        if vert.ndim != 2 or vert.shape[1] != 3:
            raise ValueError("vertices must be n x 3")
        if tri.ndim != 2 or tri.shape[1] != 3:
            raise ValueError("triangles must be m x 3")
        if tri.size and (tri.min() < 0 or tri.max() > 0xFFFFFFFF):
            raise ValueError("triangles must hold indices in [0, 2^32)")
        vert = np.ascontiguousarray(vert, dtype=np.float32)
        tri = np.ascontiguousarray(tri, dtype=np.uint32)
        gid = C.c_uint32()
        self._call(self._lib.teaser_hip_scene_add_triangles, _ptr(vert, _fp), len(vert), _ptr(tri, _u32p), len(tri), C.byref(gid))
        return gid.value

    def commit(self):
        """Builds the search structure now (a query on an uncommitted scene does it first)."""
        self._call(self._lib.teaser_hip_scene_commit)

    def triangle_count(self):
        n = C.c_int64()
        self._call(self._lib.teaser_hip_scene_triangle_count, C.byref(n))
        return n.value

    # ---- queries ------------------------------------------------------------------------------------------------
    @staticmethod
    def _rows(a, width, what):
        a = np.asarray(a)
        if a.ndim < 1 or a.shape[-1] != width:
            raise ValueError("%s must have a last dimension of %d" % (what, width))
        return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, width), a.shape[:-1]

    def cast_rays(self, rays):
        """The first surface every ray meets: a dict with Open3D's keys ``t_hit`` (float32, +inf for a miss),
        ``geometry_ids``, ``primitive_ids`` (uint32, INVALID_ID for a miss), ``primitive_uvs`` (the barycentric weights of
        the triangle's second and third vertex) and ``primitive_normals``; each shaped like ``rays`` without its last
        dimension."""
        r, shape = self._rows(rays, 6, "rays")
        n = len(r)
        out = {"t_hit": np.empty(n, np.float32), "geometry_ids": np.empty(n, np.uint32), "primitive_ids": np.empty(n, np.uint32),
               "primitive_uvs": np.empty((n, 2), np.float32), "primitive_normals": np.empty((n, 3), np.float32)}
        self._call(self._lib.teaser_hip_scene_cast_rays, _ptr(r, _fp), n, _ptr(out["t_hit"], _fp),
                   _ptr(out["geometry_ids"], _u32p), _ptr(out["primitive_ids"], _u32p), _ptr(out["primitive_uvs"], _fp),
                   _ptr(out["primitive_normals"], _fp))
        return {k: v.reshape(shape + v.shape[1:]) for k, v in out.items()}

    def test_occlusions(self, rays, tnear=0.0, tfar=float("inf")):
        """True where some triangle lies on the ray with tnear <= t <= tfar."""
        r, shape = self._rows(rays, 6, "rays")
        occ = np.zeros(len(r), dtype=np.uint8)
        self._call(self._lib.teaser_hip_scene_test_occlusions, _ptr(r, _fp), len(r), float(tnear), float(tfar), _ptr(occ, _u8p))
        return occ.astype(bool).reshape(shape)

    def compute_closest_points(self, query_points):
        """The closest point of the surface to every query point: a dict with Open3D's keys ``points``,
        ``geometry_ids``, ``primitive_ids``, ``primitive_uvs``, ``primitive_normals`` and, beyond Open3D's,
        ``distance`` (float32, +inf on a scene without a live triangle)."""
        p, shape = self._rows(query_points, 3, "query_points")
        n = len(p)
        out = {"points": np.empty((n, 3), np.float32), "distance": np.empty(n, np.float32),
               "geometry_ids": np.empty(n, np.uint32), "primitive_ids": np.empty(n, np.uint32),
               "primitive_uvs": np.empty((n, 2), np.float32), "primitive_normals": np.empty((n, 3), np.float32)}
        self._call(self._lib.teaser_hip_scene_closest_points, _ptr(p, _fp), n, _ptr(out["points"], _fp), _ptr(out["distance"], _fp),
                   _ptr(out["geometry_ids"], _u32p), _ptr(out["primitive_ids"], _u32p), _ptr(out["primitive_uvs"], _fp),
                   _ptr(out["primitive_normals"], _fp))
        return {k: v.reshape(shape + v.shape[1:]) for k, v in out.items()}

    def compute_distance(self, query_points):
        """The distance from every query point to the surface (float32); only this map is computed and copied."""
        p, shape = self._rows(query_points, 3, "query_points")
        d = np.empty(len(p), np.float32)
        self._call(self._lib.teaser_hip_scene_closest_points, _ptr(p, _fp), len(p), None, _ptr(d, _fp), None, None, None, None)
        return d.reshape(shape)

    def cast_views(self, intrinsic, extrinsics, width=None, height=None, pixel_offset=0.5, t_hit=True, ids=True, uvs=True,
                   normals=True):
        """One cast_rays dict per extrinsic with ``height x width`` maps, the rays generated on the device and all views in
        one call (one launch, one synchronisation); equal to cast_rays(create_rays_pinhole(...)) bit for bit.  intrinsic,
        width, height, pixel_offset: one for all views or a list with one per view; width and height default to the
        intrinsic's.  A map that is not asked for is absent from the dict and is neither computed nor copied."""
        ext = list(extrinsics)
        b = len(ext)
        if b == 0:
            return []
        intr = _each(intrinsic, b, "intrinsic", _is_intrinsic)
        W, H = _each(width, b, "width", _is_scalar), _each(height, b, "height", _is_scalar)
        off = _each(pixel_offset, b, "pixel_offset", _is_scalar)
        views = (SceneViewC * b)()
        want = {"t_hit": bool(t_hit), "geometry_ids": bool(ids), "primitive_ids": bool(ids), "primitive_uvs": bool(uvs),
                "primitive_normals": bool(normals)}
        tail = {"t_hit": (), "geometry_ids": (), "primitive_ids": (), "primitive_uvs": (2,), "primitive_normals": (3,)}
        res = []
        for k in range(b):
            v = views[k]
            self._lib.teaser_hip_scene_view_default(C.byref(v))
            E = np.array(np.eye(4) if ext[k] is None else ext[k], dtype=np.float64)
            if E.shape != (4, 4):
                raise ValueError("extrinsic must be a 4 x 4 matrix")
            w = W[k] if W[k] is not None else getattr(intr[k], "width", None)
            h = H[k] if H[k] is not None else getattr(intr[k], "height", None)
            if w is None or h is None:
                raise ValueError("width and height: the intrinsic carries none, so they must be given")
            v.width, v.height = int(w), int(h)
            v.fx, v.fy, v.cx, v.cy = _fxfycxcy(intr[k])
            v.extrinsic[:] = list(E.ravel())
            v.pixel_offset = float(off[k])
            shape = (max(v.height, 0), max(v.width, 0))
            res.append({key: np.zeros(shape + tail[key], dtype=np.uint32 if key.endswith("ids") else np.float32)
                        for key in tail if want[key]})

        def ptrs(key, ty):
            return (ty * b)(*[_ptr(r.get(key), ty) for r in res])
        self._call(self._lib.teaser_hip_scene_cast_views, views, b, ptrs("t_hit", _fp), ptrs("geometry_ids", _u32p),
                   ptrs("primitive_ids", _u32p), ptrs("primitive_uvs", _fp), ptrs("primitive_normals", _fp))
        return res

    def render_depth(self, intrinsic, extrinsic, width=None, height=None, depth_max=None):
        """The scene as a depth camera sees it: ``height x width`` float32 z-depth in metres, 0 where no surface was met
        (and, with ``depth_max``, where it lies beyond).  Rays go through the pixels' corners (pixel_offset 0), the
        convention of the depth frames, so compute_depth_odometry, track_frame_to_model and UniformTSDFVolume.integrate
        take the image as it is (with depth_scale 1)."""
        t = self.cast_views(intrinsic, [extrinsic], width, height, pixel_offset=0.0, ids=False, uvs=False, normals=False)[0]["t_hit"]
        miss = ~np.isfinite(t)
        if depth_max is not None:
            miss |= t > np.float32(depth_max)
        t[miss] = 0.0
        return t

    create_rays_pinhole = staticmethod(create_rays_pinhole)
