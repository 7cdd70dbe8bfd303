"""TSDF volume integration on the GPU with the surface of open3d.pipelines.integration.UniformTSDFVolume: depth frames
and their camera poses in, one fused cloud out.

    vol = UniformTSDFVolume(length=4.0, resolution=512, sdf_trunc=0.04, color_type=TSDFVolumeColorType.RGB8)
    vol.integrate_batch(depths, intrinsic, extrinsics, colors)     # any number of frames in one call
    cloud = vol.extract_point_cloud()                              # .points, .normals, .colors

The volume lives on the device from construction to ``close()`` (or garbage collection): frames go up at two bytes per
pixel, only the extracted surface comes back.  The arithmetic is written out in include/teaser_hip.h ("TSDF volume"):
float32 as Open3D forms it, frames applied in the order given, a voxel's bits the same for any split of the frames into
calls; bit parity with an Open3D binary is not claimed.  ``extrinsic`` is world-to-camera as in Open3D.

Images are numpy arrays: depth ``height x width`` uint16 or float32; colour ``height x width x 3`` uint8 for an RGB8
volume, ``height x width`` float32 for a Gray32 volume.  Rows may lie any distance apart.  Every volume has a handle of
its own (a lock serialises its calls).  Without a GPU the constructor raises TeaserHipError (NO_DEVICE): there is no CPU
path."""
import ctypes as C
import math
import threading

import numpy as np

from .rgbd import _each, _fxfycxcy, _image, _is_intrinsic, _is_matrix, _is_scalar

_vp, _dp, _fp, _i64p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int64)
_i32p, _i8p = C.POINTER(C.c_int32), C.POINTER(C.c_int8)


class TsdfVolumeC(C.Structure):
    """teaser_tsdf_volume_c (include/teaser_hip.h)."""
    _fields_ = [("length", C.c_double), ("sdf_trunc", C.c_double), ("origin", C.c_double * 3),
                ("resolution", C.c_int32), ("color_type", C.c_int32), ("reserved", C.c_int64)]


class TsdfFrameC(C.Structure):
    """teaser_tsdf_frame_c (include/teaser_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("depth_format", C.c_int32), ("color_format", C.c_int32),
                ("depth_row_bytes", C.c_int64), ("color_row_bytes", C.c_int64), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("extrinsic", C.c_double * 16), ("depth_scale", C.c_double),
                ("depth_trunc", C.c_double)]


class TsdfViewC(C.Structure):
    """teaser_tsdf_view_c (include/teaser_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("extrinsic", C.c_double * 16), ("depth_min", C.c_double), ("depth_max", C.c_double),
                ("weight_threshold", C.c_double), ("reserved", C.c_int64)]


class StsdfVolumeC(C.Structure):
    """teaser_stsdf_volume_c (include/teaser_hip.h)."""
    _fields_ = [("voxel_length", C.c_double), ("sdf_trunc", C.c_double), ("color_type", C.c_int32),
                ("volume_unit_resolution", C.c_int32), ("depth_sampling_stride", C.c_int32), ("initial_blocks", C.c_int32),
                ("slab_blocks", C.c_int32), ("reserved32", C.c_int32), ("max_blocks", C.c_int64), ("reserved", C.c_int64)]


assert C.sizeof(TsdfVolumeC) == 56 and C.sizeof(TsdfFrameC) == 208 and C.sizeof(TsdfViewC) == 200  # as the header asserts
assert C.sizeof(StsdfVolumeC) == 56


def declare(L):
    """ctypes signatures of the entry points (called by the package's lib())."""
    L.teaser_hip_tsdf_volume_default.argtypes = [C.POINTER(TsdfVolumeC)]
    L.teaser_hip_tsdf_create.argtypes = [C.POINTER(TsdfVolumeC), C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_tsdf_destroy.argtypes = [_vp]
    L.teaser_hip_tsdf_last_error.argtypes = [_vp]
    L.teaser_hip_tsdf_last_error.restype = C.c_char_p
    L.teaser_hip_tsdf_fill_scratch.argtypes = [_vp, C.c_int32, C.POINTER(C.c_int64)]
    L.teaser_hip_tsdf_reset.argtypes = [_vp]
    L.teaser_hip_tsdf_integrate_batch.argtypes = [_vp, C.c_int32, C.POINTER(TsdfFrameC), C.POINTER(_vp), C.POINTER(_vp)]
    L.teaser_hip_tsdf_extract_point_cloud.argtypes = [_vp, C.c_int64, _dp, _dp, _dp, _i64p]
    L.teaser_hip_tsdf_extract_voxel_point_cloud.argtypes = [_vp, C.c_int64, _dp, _dp, _i64p]
    L.teaser_hip_tsdf_download.argtypes = [_vp, _fp, _dp]
    L.teaser_hip_tsdf_upload.argtypes = [_vp, _fp, _dp]
    L.teaser_hip_tsdf_extract_triangle_mesh.argtypes = [_vp, C.c_int64, _dp, _dp, _dp, C.c_int64, _i32p, _i64p, _i64p]
    L.teaser_hip_tsdf_mesh_tables.argtypes = [_i32p, _i8p]
    L.teaser_hip_tsdf_view_default.argtypes = [C.POINTER(TsdfViewC)]
    L.teaser_hip_tsdf_ray_cast_views.argtypes = [_vp, C.c_int32, C.POINTER(TsdfViewC), C.POINTER(_fp), C.POINTER(_fp),
                                                 C.POINTER(_fp), C.POINTER(_fp), _i64p]
    L.teaser_hip_stsdf_volume_default.argtypes = [C.POINTER(StsdfVolumeC)]
    L.teaser_hip_stsdf_create.argtypes = [C.POINTER(StsdfVolumeC), C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_stsdf_destroy.argtypes = [_vp]
    L.teaser_hip_stsdf_last_error.argtypes = [_vp]
    L.teaser_hip_stsdf_last_error.restype = C.c_char_p
    L.teaser_hip_stsdf_fill_scratch.argtypes = [_vp, C.c_int32, C.POINTER(C.c_int64)]
    L.teaser_hip_stsdf_last_phases.argtypes = [_vp, _dp]
    L.teaser_hip_stsdf_reset.argtypes = [_vp]
    L.teaser_hip_stsdf_integrate_frames.argtypes = [_vp, C.c_int32, C.POINTER(TsdfFrameC), C.POINTER(_vp), C.POINTER(_vp),
                                                   _i64p, _i64p, _i64p]
    L.teaser_hip_stsdf_extract_point_cloud.argtypes = [_vp, C.c_int64, _dp, _dp, _dp, _i64p]
    L.teaser_hip_stsdf_extract_voxel_point_cloud.argtypes = [_vp, C.c_int64, _dp, _dp, _i64p]
    L.teaser_hip_stsdf_block_count.argtypes = [_vp, _i64p]
    L.teaser_hip_stsdf_block_keys.argtypes = [_vp, C.c_int64, _i32p, _i64p]
    L.teaser_hip_stsdf_download_blocks.argtypes = [_vp, C.c_int64, _fp, _dp, _i64p]
    L.teaser_hip_stsdf_upload_blocks.argtypes = [_vp, C.c_int64, _i32p, _fp, _dp]
    L.teaser_hip_stsdf_ray_cast_views.argtypes = [_vp, C.c_int32, C.POINTER(TsdfViewC), C.POINTER(_fp), C.POINTER(_fp),
                                                  C.POINTER(_fp), C.POINTER(_fp), _i64p]
    L.teaser_hip_stsdf_extract_triangle_mesh.argtypes = [_vp, C.c_int64, _dp, _dp, _dp, C.c_int64, _i32p, _i64p, _i64p]


class TSDFVolumeColorType:
    """Open3D's pipelines.integration.TSDFVolumeColorType."""
    NoColor, RGB8, Gray32 = 0, 1, 2


class TSDFPointCloud:
    """What the extractions return: ``points`` (count x 3 float64) and, where they exist, ``normals`` and ``colors``
    (count x 3 float64, else None)."""

    def __init__(self, points, normals=None, colors=None):
        self.points, self.normals, self.colors = points, normals, colors

    def __len__(self):
        return len(self.points)


class TSDFTriangleMesh:
    """What extract_triangle_mesh returns: ``vertices`` (n x 3 float64), ``triangles`` (m x 3 int32) and, where they
    exist, ``vertex_colors`` and ``vertex_normals`` (n x 3 float64, else None)."""

    def __init__(self, vertices, triangles, vertex_colors=None, vertex_normals=None):
        self.vertices, self.triangles = vertices, triangles
        self.vertex_colors, self.vertex_normals = vertex_colors, vertex_normals


class TSDFRayCastResult:
    """What ray_cast returns: ``depth`` (height x width float32, the z-depth in metres, 0 where no surface was met),
    ``vertex_map`` (world points), ``normal_map`` and ``color`` (height x width x 3 float32; None when not asked for, or
    for the colour of a volume without a colour type) and ``hits``, the number of pixels that met a surface."""

    def __init__(self, depth, vertex_map, normal_map, color, hits, color_type):
        self.depth, self.vertex_map, self.normal_map, self.color, self.hits = depth, vertex_map, normal_map, color, hits
        self._color_type = color_type

    def as_rgbd_image(self):
        """The frame as compute_rgbd_odometry takes it: the depth as it is (float32 metres) and a float32 intensity,
        (0.2990 R + 0.5870 G) + 0.1140 B of the colours in float32 -- the weights of "Depth frames" -- or, for a Gray32
        volume, the value itself."""
        from .odometry import RGBDImage
        if self.color is None:
            raise ValueError("the frame has no colour: the volume has no colour type, or color=False was given")
        c = self.color
        if self._color_type == TSDFVolumeColorType.Gray32:
            gray = np.ascontiguousarray(c[..., 0])
        else:
            f = np.float32
            gray = (f(0.2990) * c[..., 0] + f(0.5870) * c[..., 1]) + f(0.1140) * c[..., 2]
        return RGBDImage(gray, self.depth, depth_scale=1.0)  # float32 depth is taken as it is: neither parameter is applied


def write_triangle_mesh(path, mesh, binary=True):
    """The mesh as a PLY file, as teaser::PLYWriter::writeMesh (include/teaser/ply_io.h) writes it: vertex with double
    x, y, z and, with vertex colours, uchar red, green, blue (round(clamp(c, 0, 1) 255), a NaN as 0); face with
    ``list uchar int vertex_indices``.  binary: the host's byte order."""
    import sys
    vert = np.ascontiguousarray(mesh.vertices, dtype=np.float64).reshape(-1, 3)
    tri = np.ascontiguousarray(mesh.triangles, dtype=np.int32).reshape(-1, 3)
    rgb = None
    if mesh.vertex_colors is not None:
        c = np.nan_to_num(np.asarray(mesh.vertex_colors, dtype=np.float64).reshape(-1, 3), nan=0.0)
        rgb = np.floor(np.clip(c, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        if len(rgb) != len(vert):
            raise ValueError("vertex_colors: one row per vertex")
    fmt = "ascii" if not binary else "binary_%s_endian" % sys.byteorder
    head = "ply\nformat %s 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n" % (fmt, len(vert))
    if rgb is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(tri)
    with open(path, "wb") as f:
        f.write(head.encode())
        if binary:
            fields = [("xyz", np.float64, 3)] + ([("rgb", np.uint8, 3)] if rgb is not None else [])
            v = np.zeros(len(vert), dtype=np.dtype(fields, align=False))
            v["xyz"] = vert
            if rgb is not None:
                v["rgb"] = rgb
            f.write(v.tobytes())
            t = np.zeros(len(tri), dtype=np.dtype([("n", np.uint8), ("idx", np.int32, 3)], align=False))
            t["n"], t["idx"] = 3, tri
            f.write(t.tobytes())
        else:
            for k in range(len(vert)):
                row = " ".join("%.17g" % x for x in vert[k])
                if rgb is not None:
                    row += " %d %d %d" % tuple(rgb[k])
                f.write((row + "\n").encode())
            for a, b, c in tri:
                f.write(("3 %d %d %d\n" % (a, b, c)).encode())


class _TSDFHandle:
    """What the dense and the scalable volume share: the handle (``_prefix`` names its entry points), the frame records,
    integration, the two point-cloud extractions and the ray cast of any number of views."""
    _prefix = "teaser_hip_tsdf"

    def _fn(self, name):
        return getattr(self._lib, self._prefix + "_" + name)

    # ---- the handle ---------------------------------------------------------------------------------------------
    def _call(self, fn, *args):
        from . import TeaserHipError
        if self._h is None:
            raise ValueError("the volume is closed")
        with self._lock:  # the handle serves one call at a time
            rc = fn(self._h, *args)
            err = self._fn("last_error")(self._h).decode() if rc != 0 else ""
        if rc != 0:
            raise TeaserHipError(rc, err)

    def fill_scratch(self, byte):
        """DIAGNOSTIC (teaser_hip_*_fill_scratch): sets every byte of the handle's scratch and staging buffers to
        `byte` (0 .. 255) and returns the device bytes filled.  The volume itself is state and is left alone."""
        filled = C.c_int64()
        self._call(self._fn("fill_scratch"), int(byte), C.byref(filled))
        return filled.value

    def close(self):
        """Frees the volume; the object is unusable afterwards."""
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            self._fn("destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- integration --------------------------------------------------------------------------------------------
    def _frames(self, depths, intrinsic, extrinsics, colors, depth_scale, depth_trunc):
        b = len(depths)
        cols = list(colors) if colors is not None else [None] * b
        if len(cols) != b:
            raise ValueError("colors: one image per frame")
        K = [_fxfycxcy(k) for k in _each(intrinsic, b, "intrinsic", _is_intrinsic)]
        ext = _each(extrinsics, b, "extrinsics", _is_matrix)
        scale, trunc = _each(depth_scale, b, "depth_scale", _is_scalar), _each(depth_trunc, b, "depth_trunc", _is_scalar)
        frames = (TsdfFrameC * max(b, 1))()
        dimg, cimg = [], []
        for k in range(b):
            d, dpx = _image(depths[k], "depth", (np.uint16, np.float32), (1,))
            if d.ndim != 2:
                raise ValueError("depth has shape %s" % (d.shape,))
            E = np.array(np.eye(4) if ext[k] is None else ext[k], dtype=np.float64)
            if E.shape != (4, 4):
                raise ValueError("extrinsic must be a 4 x 4 matrix")
            f = frames[k]
            f.height, f.width = d.shape
            f.depth_format = 0 if d.dtype == np.uint16 else 1
            f.depth_row_bytes = d.strides[0] if d.size else d.shape[1] * dpx
            c = cols[k]
            if self.color_type == TSDFVolumeColorType.NoColor:
                c = None  # Open3D ignores the colour image of a frame here, too
            elif c is None:
                raise ValueError("color: a volume with a colour type needs a colour image per frame")
            else:
                want = (np.uint8,) if self.color_type == TSDFVolumeColorType.RGB8 else (np.float32,)
                c, cpx = _image(c, "color", want, (3,) if self.color_type == TSDFVolumeColorType.RGB8 else (1,))
                if c.shape[:2] != d.shape:
                    raise ValueError("color has shape %s beside a depth image of shape %s" % (c.shape, d.shape))
                f.color_format = 1 if self.color_type == TSDFVolumeColorType.RGB8 else 2
                f.color_row_bytes = c.strides[0] if c.size else c.shape[1] * cpx
            f.fx, f.fy, f.cx, f.cy = K[k]
            f.extrinsic[:] = list(E.ravel())
            f.depth_scale, f.depth_trunc = float(scale[k]), float(trunc[k])
            dimg.append(d)
            cimg.append(c)
        return b, frames, dimg, cimg

    def integrate_batch(self, depths, intrinsic, extrinsics, colors=None, depth_scale=1000.0, depth_trunc=3.0):
        """The frames, in the order given, in one call: a voxel ends with the bits that one integrate() per frame leaves.
        depths: a list of depth images; colors: a list of colour images (ignored by a volume without colour);
        intrinsic, extrinsics, depth_scale, depth_trunc: one for all frames or a list with one per frame."""
        if len(depths) == 0:
            return
        b, frames, dimg, cimg = self._frames(depths, intrinsic, extrinsics, colors, depth_scale, depth_trunc)

        def ptrs(arrs):
            return (_vp * b)(*[None if a is None or a.size == 0 else a.ctypes.data_as(_vp) for a in arrs])
        self._integrate_call(b, frames, ptrs(dimg), ptrs(cimg))

    def integrate(self, depth, intrinsic, extrinsic, color=None, depth_scale=1000.0, depth_trunc=3.0):
        """Open3D's integrate(rgbd, intrinsic, extrinsic) with the RGBD image given as its parts: the depth image, and
        for a volume with a colour type the colour image."""
        self.integrate_batch([depth], intrinsic, extrinsic, None if color is None else [color], depth_scale, depth_trunc)

    # ---- extraction ---------------------------------------------------------------------------------------------
    def _extract(self, fn, outputs):
        """The count first, then the rows into arrays of exactly that size; outputs: which optional arrays to ask for."""
        cnt = C.c_int64(0)
        none = [None] * (1 + len(outputs))
        self._call(fn, 0, *none, C.byref(cnt))
        n = int(cnt.value)
        pts = np.empty((n, 3))
        extra = [np.empty((n, 3)) if want else None for want in outputs]
        if n:
            self._call(fn, n, pts.ctypes.data_as(_dp), *[None if a is None else a.ctypes.data_as(_dp) for a in extra],
                       C.byref(cnt))
        return pts, extra

    def extract_point_cloud(self, normals=True):
        """Open3D's extract_point_cloud: the zero crossings between neighbouring voxels in Open3D's order, with their
        normals (unless normals=False) and, for a volume with a colour type, their colours."""
        pts, (nrm, col) = self._extract(self._fn("extract_point_cloud"),
                                        [bool(normals), self.color_type != TSDFVolumeColorType.NoColor])
        return TSDFPointCloud(pts, nrm, col)

    def extract_voxel_point_cloud(self):
        """Open3D's extract_voxel_point_cloud: the centre of every observed voxel with (tsdf + 1) / 2 as its colour."""
        pts, (col,) = self._extract(self._fn("extract_voxel_point_cloud"), [True])
        return TSDFPointCloud(pts, None, col)

    def _extract_mesh(self, vertex_normals):
        """The counts first, then the rows into arrays of exactly that size."""
        nv, nt = C.c_int64(0), C.c_int64(0)
        fn = self._fn("extract_triangle_mesh")
        self._call(fn, 0, None, None, None, 0, None, C.byref(nv), C.byref(nt))
        n, m = int(nv.value), int(nt.value)
        colored = self.color_type != TSDFVolumeColorType.NoColor
        vert, tri = np.empty((n, 3)), np.empty((m, 3), dtype=np.int32)
        col = np.empty((n, 3)) if colored else None
        nrm = np.empty((n, 3)) if vertex_normals else None
        if n or m:
            self._call(fn, n, vert.ctypes.data_as(_dp), None if col is None else col.ctypes.data_as(_dp),
                       None if nrm is None else nrm.ctypes.data_as(_dp), m, tri.ctypes.data_as(_i32p), C.byref(nv),
                       C.byref(nt))
        return TSDFTriangleMesh(vert, tri, col, nrm)

    # ---- ray casting --------------------------------------------------------------------------------------------
    def ray_cast_batch(self, intrinsic, extrinsics, width=None, height=None, depth_min=0.1, depth_max=3.0,
                       weight_threshold=3.0, vertex_map=True, normal_map=True, color=True):
        """One TSDFRayCastResult per extrinsic, all views in one call (one launch, one synchronisation).  intrinsic,
        width, height, depth_min, depth_max, weight_threshold: one for all views or a list with one per view; width
        and height default to the intrinsic's.  The rules: include/teaser_hip.h, "TSDF ray casting" for the dense volume
        and "Scalable TSDF ray casting" for the scalable one."""
        ext = list(extrinsics)
        b = len(ext)
        if b == 0:
            return []
        intr = _each(intrinsic, b, "intrinsic", _is_intrinsic)
        K = [_fxfycxcy(k) for k in intr]
        W, H = _each(width, b, "width", _is_scalar), _each(height, b, "height", _is_scalar)
        lo, hi = _each(depth_min, b, "depth_min", _is_scalar), _each(depth_max, b, "depth_max", _is_scalar)
        thr = _each(weight_threshold, b, "weight_threshold", _is_scalar)
        colored = bool(color) and self.color_type != TSDFVolumeColorType.NoColor
        views = (TsdfViewC * b)()
        maps = [[], [], [], []]
        for k in range(b):
            v = views[k]
            self._lib.teaser_hip_tsdf_view_default(C.byref(v))
            E = np.array(np.eye(4) if ext[k] is None else ext[k], dtype=np.float64)
            if E.shape != (4, 4):
                raise ValueError("extrinsic must be a 4 x 4 matrix")
            w = W[k] if W[k] is not None else getattr(intr[k], "width", None)
            h = H[k] if H[k] is not None else getattr(intr[k], "height", None)
            if w is None or h is None:
                raise ValueError("width and height: the intrinsic carries none, so they must be given")
            v.width, v.height = int(w), int(h)
            v.fx, v.fy, v.cx, v.cy = K[k]
            v.extrinsic[:] = list(E.ravel())
            v.depth_min, v.depth_max, v.weight_threshold = float(lo[k]), float(hi[k]), float(thr[k])
            shape = (max(v.height, 0), max(v.width, 0))
            for m, want in enumerate((True, bool(vertex_map), bool(normal_map), colored)):
                maps[m].append(np.zeros(shape + ((3,) if m else ()), dtype=np.float32) if want else None)

        def ptrs(arrs):
            return (_fp * b)(*[None if a is None or a.size == 0 else a.ctypes.data_as(_fp) for a in arrs])
        hits = (C.c_int64 * b)()
        self._call(self._fn("ray_cast_views"), b, views, ptrs(maps[0]), ptrs(maps[1]), ptrs(maps[2]),
                   ptrs(maps[3]), hits)
        return [TSDFRayCastResult(maps[0][k], maps[1][k], maps[2][k], maps[3][k], int(hits[k]), self.color_type)
                for k in range(b)]


class UniformTSDFVolume(_TSDFHandle):
    """Open3D's UniformTSDFVolume(length, resolution, sdf_trunc, color_type, origin): a cube of resolution^3 voxels with
    its corner at ``origin``, kept on ``device`` (-1: the current one)."""

    def __init__(self, length, resolution, sdf_trunc, color_type=TSDFVolumeColorType.NoColor, origin=(0.0, 0.0, 0.0),
                 device=-1):
        from . import TeaserHipError, lib
        if int(resolution) != resolution or not 1 <= int(resolution) <= 1024:
            raise ValueError("resolution must be an integer in [1, 1024]")
        if not (math.isfinite(float(length)) and float(length) > 0):
            raise ValueError("length must be finite and > 0")
        if not (math.isfinite(float(sdf_trunc)) and float(sdf_trunc) > 0):
            raise ValueError("sdf_trunc must be finite and > 0")
        if color_type not in (0, 1, 2):
            raise ValueError("color_type must be one of TSDFVolumeColorType.NoColor, RGB8, Gray32")
        o = np.asarray(origin, dtype=np.float64)
        if o.shape != (3,) or not np.isfinite(o).all():
            raise ValueError("origin must be three finite numbers")
        self.length, self.sdf_trunc, self.color_type = float(length), float(sdf_trunc), int(color_type)
        self._resolution, self.origin = int(resolution), o.copy()
        self._lib = lib()
        rec = TsdfVolumeC()
        self._lib.teaser_hip_tsdf_volume_default(C.byref(rec))
        rec.length, rec.sdf_trunc, rec.resolution, rec.color_type = self.length, self.sdf_trunc, self._resolution, self.color_type
        rec.origin[:] = list(o)
        self._h = _vp()
        self._lock = threading.Lock()
        rc = self._lib.teaser_hip_tsdf_create(C.byref(rec), int(device), C.byref(self._h))
        if rc != 0:
            self._h = None
            msg = self._lib.teaser_hip_tsdf_last_error(None).decode()
            raise TeaserHipError(rc, "(no MI355X visible: the product has no CPU path)" if rc == 3 else msg)

    @property
    def voxel_length(self):
        return self.length / self._resolution

    @property
    def resolution(self):
        return self._resolution

    def _integrate_call(self, b, frames, depth, color):
        self._call(self._lib.teaser_hip_tsdf_integrate_batch, b, frames, depth, color)

    # ---- extraction ---------------------------------------------------------------------------------------------
    def extract_triangle_mesh(self, vertex_normals=False):
        """Open3D's extract_triangle_mesh: marching cubes over the observed cubes, vertices and triangles in the order
        of Open3D's loop, with vertex colours for a volume with a colour type.  vertex_normals=True adds the TSDF
        gradient at every vertex (the normal rule of the point cloud), which Open3D's call does not give."""
        return self._extract_mesh(vertex_normals)

    def ray_cast(self, intrinsic, extrinsic, width=None, height=None, depth_min=0.1, depth_max=3.0, weight_threshold=3.0,
                 vertex_map=True, normal_map=True, color=True):
        """The fused model seen from a camera: per pixel the z-depth of the first surface its ray meets (Open3D's
        VoxelBlockGrid.ray_cast for the dense volume), with the world points, the normals and the colours.
        ``extrinsic`` is world-to-camera.  A voxel counts as surface only with a weight >= weight_threshold."""
        return self.ray_cast_batch(intrinsic, [extrinsic], width, height, depth_min, depth_max, weight_threshold, vertex_map,
                                   normal_map, color)[0]

    # ---- the voxels ---------------------------------------------------------------------------------------------
    def extract_volume_tsdf(self):
        """R^3 x 2 float32 (tsdf, weight) in Open3D's voxel order (x R + y) R + z."""
        out = np.empty((self._resolution ** 3, 2), dtype=np.float32)
        self._call(self._lib.teaser_hip_tsdf_download, out.ctypes.data_as(_fp), None)
        return out

    def extract_volume_color(self):
        """R^3 x 3 float64 in Open3D's voxel order (a volume with a colour type only)."""
        if self.color_type == TSDFVolumeColorType.NoColor:
            raise ValueError("the volume has no colour")
        out = np.empty((self._resolution ** 3, 3))
        self._call(self._lib.teaser_hip_tsdf_download, None, out.ctypes.data_as(_dp))
        return out

    def inject_volume_tsdf(self, tsdf_weight):
        a = np.ascontiguousarray(tsdf_weight, dtype=np.float32)
        if a.shape != (self._resolution ** 3, 2):
            raise ValueError("tsdf_weight must have shape %d x 2, got %s" % (self._resolution ** 3, a.shape))
        if not np.isfinite(a).all():
            raise ValueError("tsdf_weight has a non-finite value")
        self._call(self._lib.teaser_hip_tsdf_upload, a.ctypes.data_as(_fp), None)

    def inject_volume_color(self, color):
        if self.color_type == TSDFVolumeColorType.NoColor:
            raise ValueError("the volume has no colour")
        a = np.ascontiguousarray(color, dtype=np.float64)
        if a.shape != (self._resolution ** 3, 3):
            raise ValueError("color must have shape %d x 3, got %s" % (self._resolution ** 3, a.shape))
        if not (np.isfinite(a) | (np.isnan(a) if self.color_type == TSDFVolumeColorType.Gray32 else False)).all():
            raise ValueError("color has a non-finite value")
        self._call(self._lib.teaser_hip_tsdf_upload, None, a.ctypes.data_as(_dp))

    def reset(self):
        """Every voxel back to the empty state."""
        self._call(self._lib.teaser_hip_tsdf_reset)


class ScalableTSDFVolume(_TSDFHandle):
    """Open3D's ScalableTSDFVolume(voxel_length, sdf_trunc, color_type, volume_unit_resolution, depth_sampling_stride):
    only the blocks of 16^3 voxels that depth frames have come near are kept, so the scene needs no bounds.  The rules
    are written out in include/teaser_hip.h ("Scalable TSDF volume").  initial_blocks, slab_blocks and max_blocks (None:
    the library's defaults; max_blocks 0: no limit) size the memory the blocks lie in.  ``last_counts`` holds
    (touched, opened, out_of_range) of the last integrate call.  ray_cast_batch renders views of the open blocks
    (include/teaser_hip.h, "Scalable TSDF ray casting"); the single view is the module's ray_cast(volume, ...): Open3D's
    ScalableTSDFVolume has no method of that name, and this class keeps Open3D's surface.  The triangle mesh
    (include/teaser_hip.h, "Scalable TSDF triangle mesh") is extract_mesh(), or the module's
    extract_triangle_mesh(volume, ...), which serves either volume class."""
    _prefix = "teaser_hip_stsdf"

    def __init__(self, voxel_length, sdf_trunc, color_type=TSDFVolumeColorType.NoColor, volume_unit_resolution=16,
                 depth_sampling_stride=4, device=-1, initial_blocks=None, slab_blocks=None, max_blocks=None):
        from . import TeaserHipError, lib
        if color_type not in (0, 1, 2):
            raise ValueError("color_type must be one of TSDFVolumeColorType.NoColor, RGB8, Gray32")
        self.voxel_length, self.sdf_trunc, self.color_type = float(voxel_length), float(sdf_trunc), int(color_type)
        self.volume_unit_resolution, self.depth_sampling_stride = int(volume_unit_resolution), int(depth_sampling_stride)
        self.last_counts = (0, 0, 0)
        self._lib = lib()
        rec = StsdfVolumeC()
        self._lib.teaser_hip_stsdf_volume_default(C.byref(rec))
        rec.voxel_length, rec.sdf_trunc, rec.color_type = self.voxel_length, self.sdf_trunc, self.color_type
        rec.volume_unit_resolution, rec.depth_sampling_stride = self.volume_unit_resolution, self.depth_sampling_stride
        for name, v in (("initial_blocks", initial_blocks), ("slab_blocks", slab_blocks), ("max_blocks", max_blocks)):
            if v is not None:
                setattr(rec, name, int(v))
        self._h = _vp()
        self._lock = threading.Lock()
        rc = self._lib.teaser_hip_stsdf_create(C.byref(rec), int(device), C.byref(self._h))
        if rc != 0:
            self._h = None
            msg = self._lib.teaser_hip_stsdf_last_error(None).decode()
            raise TeaserHipError(rc, "(no MI355X visible: the product has no CPU path)" if rc == 3 else msg)

    def _integrate_call(self, b, frames, depth, color):
        t, o, r = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            self._call(self._lib.teaser_hip_stsdf_integrate_frames, b, frames, depth, color, C.byref(t), C.byref(o), C.byref(r))
        finally:
            self.last_counts = (int(t.value), int(o.value), int(r.value))

    def last_phases_ms(self):
        """DIAGNOSTIC (teaser_hip_stsdf_last_phases): the host's clock over the last integrate call, in milliseconds:
        (upload, touch pass and read-back; directory merge; zeroing and integration)."""
        ms = (C.c_double * 3)()
        self._call(self._lib.teaser_hip_stsdf_last_phases, ms)
        return tuple(ms)

    # ---- the blocks ---------------------------------------------------------------------------------------------
    @property
    def block_count(self):
        n = C.c_int64(0)
        self._call(self._lib.teaser_hip_stsdf_block_count, C.byref(n))
        return int(n.value)

    @property
    def block_bytes(self):
        """Device bytes of one block."""
        return (32 if self.color_type != TSDFVolumeColorType.NoColor else 8) * self.volume_unit_resolution ** 3

    def block_keys(self):
        """blocks x 3 int32: (bx, by, bz) of every open block in ascending order."""
        n = self.block_count
        keys, cnt = np.empty((n, 3), dtype=np.int32), C.c_int64(0)
        if n:
            self._call(self._lib.teaser_hip_stsdf_block_keys, n, keys.ctypes.data_as(_i32p), C.byref(cnt))
        return keys

    def extract_blocks(self):
        """(keys, tsdf_weight, color): blocks x 3 int32, blocks x 4096 x 2 float32 (tsdf, weight) and blocks x 4096 x 3
        float64 (None without a colour type), the blocks in ascending order and Open3D's voxel order inside."""
        keys = self.block_keys()
        n, v, cnt = len(keys), self.volume_unit_resolution ** 3, C.c_int64(0)
        tw = np.empty((n, v, 2), dtype=np.float32)
        col = np.empty((n, v, 3)) if self.color_type != TSDFVolumeColorType.NoColor else None
        if n:
            self._call(self._lib.teaser_hip_stsdf_download_blocks, n, tw.ctypes.data_as(_fp),
                       None if col is None else col.ctypes.data_as(_dp), C.byref(cnt))
        return keys, tw, col

    def inject_blocks(self, keys, tsdf_weight=None, color=None):
        """The voxels of the blocks ``keys`` (n x 3, any order, none twice); a block that is not open is opened first."""
        k = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 3)
        n, v = len(k), self.volume_unit_resolution ** 3
        tw = None if tsdf_weight is None else np.ascontiguousarray(tsdf_weight, dtype=np.float32)
        col = None if color is None else np.ascontiguousarray(color, dtype=np.float64)
        if tw is not None and tw.shape != (n, v, 2):
            raise ValueError("tsdf_weight must have shape %d x %d x 2, got %s" % (n, v, tw.shape))
        if col is not None and col.shape != (n, v, 3):
            raise ValueError("color must have shape %d x %d x 3, got %s" % (n, v, col.shape))
        self._call(self._lib.teaser_hip_stsdf_upload_blocks, n, k.ctypes.data_as(_i32p),
                   None if tw is None else tw.ctypes.data_as(_fp), None if col is None else col.ctypes.data_as(_dp))

    # ---- extraction ---------------------------------------------------------------------------------------------
    def extract_mesh(self, vertex_normals=False):
        """Open3D's ScalableTSDFVolume.extract_triangle_mesh: marching cubes over the open blocks, across their faces,
        blocks in ascending (bx, by, bz) and cubes in (x, y, z) order inside, with vertex colours for a volume with a
        colour type.  vertex_normals=True adds the TSDF gradient at every vertex (the normal rule of the point cloud).
        Returns a TSDFTriangleMesh."""
        return self._extract_mesh(vertex_normals)

    def reset(self):
        """Closes every block."""
        self._call(self._lib.teaser_hip_stsdf_reset)


def ray_cast_batch(volume, intrinsic, extrinsics, width=None, height=None, depth_min=0.1, depth_max=3.0, weight_threshold=3.0,
                   vertex_map=True, normal_map=True, color=True):
    """``volume.ray_cast_batch(...)`` for a UniformTSDFVolume or a ScalableTSDFVolume: one TSDFRayCastResult per
    extrinsic, all views in one call."""
    return volume.ray_cast_batch(intrinsic, extrinsics, width, height, depth_min, depth_max, weight_threshold, vertex_map,
                                 normal_map, color)


def ray_cast(volume, intrinsic, extrinsic, width=None, height=None, depth_min=0.1, depth_max=3.0, weight_threshold=3.0,
             vertex_map=True, normal_map=True, color=True):
    """The fused model of either volume class seen from one camera (UniformTSDFVolume.ray_cast says what comes back)."""
    return ray_cast_batch(volume, intrinsic, [extrinsic], width, height, depth_min, depth_max, weight_threshold, vertex_map,
                          normal_map, color)[0]


def extract_triangle_mesh(volume, vertex_normals=False):
    """The triangle mesh of either volume class: ``volume.extract_triangle_mesh(...)`` of a UniformTSDFVolume,
    ``volume.extract_mesh(...)`` of a ScalableTSDFVolume."""
    fn = getattr(volume, "extract_triangle_mesh", None)
    return (fn if fn is not None else volume.extract_mesh)(vertex_normals)


__all__ = ["UniformTSDFVolume", "ScalableTSDFVolume", "TSDFVolumeColorType", "TSDFPointCloud", "TSDFTriangleMesh", "TSDFRayCastResult",
           "write_triangle_mesh", "ray_cast", "ray_cast_batch", "extract_triangle_mesh"]
