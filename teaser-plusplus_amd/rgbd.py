"""Depth frames on the GPU: the step in front of everything else this package offers, and the look at its result.

``create_point_cloud_from_depth_image`` / ``create_point_cloud_from_rgbd_image`` are Open3D's
``PointCloud.create_from_depth_image`` / ``RGBDImage.create_from_color_and_depth`` followed by ``create_from_rgbd_image``;
``project_to_depth_image`` / ``project_to_rgbd_image`` are ``t.geometry.PointCloud.project_to_depth_image`` /
``project_to_rgbd_image`` with the winner of a pixel fixed (smallest depth, then smallest index) where Open3D leaves it to a
race.  The ``_batch`` forms take lists and run all frames in one launch sequence, every frame's result identical to the
frame run alone.  FP64; the arithmetic is written out in include/teaser_hip.h ("Depth frames"); bit parity with an Open3D
binary is not claimed.

Images are numpy arrays: depth ``height x width`` uint16 or float32, colour ``height x width x 3`` uint8, ``height x
width`` float32 or ``height x width x 3`` float32.  Rows may lie any distance apart (a cropped view is passed by its row
stride, never copied).  ``extrinsic`` is world-to-camera as in Open3D; the unprojection inverts it on the host (the C ABI
takes the camera pose, so that no inverse is part of the contract); ``camera_pose`` gives that matrix directly.

The calls run on the ICP handle of the device (one per device, shared with icp.py, calls serialised by its lock).
Without a GPU they raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from ._handles import _cloud
from .icp import _handle

_vp, _ip, _dp, _fp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)


class IcpFrameC(C.Structure):
    """teaser_icp_frame_c (include/teaser_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("depth_format", C.c_int32), ("color_format", C.c_int32),
                ("depth_row_bytes", C.c_int64), ("color_row_bytes", C.c_int64), ("intensity", C.c_int32),
                ("stride", C.c_int32), ("valid_only", C.c_int32), ("reserved", C.c_int32), ("fx", C.c_double),
                ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("camera_pose", C.c_double * 16),
                ("depth_scale", C.c_double), ("depth_trunc", C.c_double)]


class IcpProjectionC(C.Structure):
    """teaser_icp_projection_c (include/teaser_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("extrinsic", C.c_double * 16), ("depth_scale", C.c_double), ("depth_max", C.c_double)]


assert C.sizeof(IcpFrameC) == 224 and C.sizeof(IcpProjectionC) == 184  # the header asserts the same


def declare(L):
    """ctypes signatures of the entry points (called by the package's lib())."""
    L.teaser_hip_icp_frame_default.argtypes = [C.POINTER(IcpFrameC)]
    L.teaser_hip_icp_unproject_depth_batch.argtypes = [_vp, C.c_int32, C.POINTER(IcpFrameC), C.POINTER(_vp), C.POINTER(_vp),
                                                       _ip, C.POINTER(_dp), C.POINTER(_dp), C.POINTER(_ip)]
    L.teaser_hip_icp_project_depth_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), C.POINTER(_dp), _ip,
                                                     C.POINTER(IcpProjectionC), C.POINTER(_fp), C.POINTER(_fp),
                                                     C.POINTER(_ip), _ip]


class PinholeCameraIntrinsic:
    """Open3D's camera.PinholeCameraIntrinsic(width, height, fx, fy, cx, cy)."""

    def __init__(self, width, height, fx, fy, cx, cy):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)

    @property
    def intrinsic_matrix(self):
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])

    def get_focal_length(self):
        return self.fx, self.fy

    def get_principal_point(self):
        return self.cx, self.cy

    def __repr__(self):
        return "PinholeCameraIntrinsic(%d, %d, %r, %r, %r, %r)" % (self.width, self.height, self.fx, self.fy, self.cx,
                                                                  self.cy)


class DepthCloud:
    """One frame's cloud: ``points`` (count x 3 float64), and where they were asked for ``colors`` (count x 3 float64)
    and ``pixels`` (count int32: row width + column of every point's pixel)."""

    def __init__(self, points, colors=None, pixels=None):
        self.points, self.colors, self.pixels = points, colors, pixels

    def __len__(self):
        return len(self.points)


class DepthProjection:
    """One cloud's images: ``depth`` (height x width float32, 0 where empty), ``n_hit`` (the non-empty pixels, counted on
    the device), and where they were asked for ``color`` (height x width x 3 float32) and ``index`` (height x width
    int32: the point seen in every pixel, -1 where empty)."""

    def __init__(self, depth, n_hit, color=None, index=None):
        self.depth, self.n_hit, self.color, self.index = depth, n_hit, color, index


def _fxfycxcy(intrinsic):
    if isinstance(intrinsic, PinholeCameraIntrinsic):
        return intrinsic.fx, intrinsic.fy, intrinsic.cx, intrinsic.cy
    K = np.asarray(intrinsic, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("intrinsic must be a PinholeCameraIntrinsic or a 3 x 3 matrix")
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _each(v, b, what, is_one):
    """v as a list of b entries: one value for all (is_one(v)) or a list / tuple with one per frame."""
    if v is None or is_one(v):
        return [v] * b
    vs = list(v)
    if len(vs) != b:
        raise ValueError("%s: one for all or a list with one per frame" % what)
    return vs


def _matrix(m, what):
    if m is None:
        return np.eye(4)
    m = np.array(m, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError("%s must be a 4 x 4 matrix" % what)
    return m


_is_scalar = lambda v: np.ndim(v) == 0  # noqa: E731
_is_matrix = lambda v: not isinstance(v, (list, tuple)) and np.ndim(v) == 2  # noqa: E731
_is_intrinsic = lambda v: isinstance(v, PinholeCameraIntrinsic) or _is_matrix(v)  # noqa: E731


def _image(a, what, dtypes, channels):
    """`a` with rows of contiguous pixels (copied only when its pixels are not); returns (array, pixel bytes)."""
    a = np.asarray(a)
    if a.dtype not in dtypes:
        raise ValueError("%s must be of dtype %s, got %s" % (what, " or ".join(np.dtype(d).name for d in dtypes), a.dtype))
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in channels) or (a.ndim == 2 and 1 not in channels):
        raise ValueError("%s has shape %s" % (what, a.shape))
    px = a.itemsize * (a.shape[2] if a.ndim == 3 else 1)
    inner_ok = a.strides[1] == px and (a.ndim == 2 or a.strides[2] == a.itemsize)
    if a.size and (not inner_ok or a.strides[0] < px * a.shape[1]):
        a = np.ascontiguousarray(a)
    return a, px


def unproject_depth_batch(depths, intrinsics, colors=None, extrinsics=None, depth_scale=1000.0, depth_trunc=1000.0,
                          stride=1, convert_rgb_to_intensity=False, project_valid_depth_only=True, return_colors=None,
                          return_pixels=False, camera_poses=None, device=-1):
    """Per frame a DepthCloud (include/teaser_hip.h, "Depth frames").  depths: a list of depth images; colors: None, or a
    list with a colour image or None per frame; the other arguments one for all frames or a list with one per frame.
    return_colors: None means "where a colour image is given".  camera_poses: the camera-to-world matrices themselves,
    in place of extrinsics (which are inverted on the host)."""
    from . import lib
    b = len(depths)
    cols = list(colors) if colors is not None else [None] * b
    if len(cols) != b:
        raise ValueError("colors: one image (or None) per frame")
    if camera_poses is not None and extrinsics is not None:
        raise ValueError("give extrinsics or camera_poses, not both")
    if camera_poses is not None:
        poses = [_matrix(m, "camera_pose") for m in _each(camera_poses, b, "camera_poses", _is_matrix)]
    else:
        poses = [np.eye(4) if m is None else np.linalg.inv(_matrix(m, "extrinsic"))
                 for m in _each(extrinsics, b, "extrinsics", _is_matrix)]
    K = [_fxfycxcy(k) for k in _each(intrinsics, b, "intrinsics", _is_intrinsic)]
    scale, trunc = _each(depth_scale, b, "depth_scale", _is_scalar), _each(depth_trunc, b, "depth_trunc", _is_scalar)
    strides, inten = _each(stride, b, "stride", _is_scalar), _each(convert_rgb_to_intensity, b, "convert_rgb_to_intensity", _is_scalar)
    valid = _each(project_valid_depth_only, b, "project_valid_depth_only", _is_scalar)
    want_c = _each(return_colors, b, "return_colors", lambda v: v is None or _is_scalar(v))
    frames = (IcpFrameC * max(b, 1))()
    dimg, cimg, pts, cout, pout = [], [], [], [], []
    for k in range(b):
        d, dpx = _image(depths[k], "depth", (np.uint16, np.float32), (1,))
        if d.ndim != 2:
            raise ValueError("depth has shape %s" % (d.shape,))
        f = frames[k]
        lib().teaser_hip_icp_frame_default(C.byref(f))
        f.height, f.width = d.shape
        f.depth_format = 0 if d.dtype == np.uint16 else 1
        f.depth_row_bytes = d.strides[0] if d.size else d.shape[1] * dpx
        c = cols[k]
        if c is not None:
            c, cpx = _image(c, "color", (np.uint8, np.float32), (1, 3))
            if c.shape[:2] != d.shape or (c.dtype == np.uint8 and c.ndim != 3):
                raise ValueError("color has shape %s beside a depth image of shape %s" % (c.shape, d.shape))
            f.color_format = 1 if c.dtype == np.uint8 else (2 if c.ndim == 2 else 3)
            f.color_row_bytes = c.strides[0] if c.size else c.shape[1] * cpx
            f.intensity = 1 if (inten[k] and f.color_format == 1) else 0
        if int(strides[k]) < 1:
            raise ValueError("stride must be >= 1")
        f.stride, f.valid_only = int(strides[k]), 1 if valid[k] else 0
        f.fx, f.fy, f.cx, f.cy = K[k]
        f.camera_pose[:] = list(poses[k].ravel())
        f.depth_scale, f.depth_trunc = float(scale[k]), float(trunc[k])
        n_vis = -(-d.shape[0] // f.stride) * -(-d.shape[1] // f.stride)
        dimg.append(d)
        cimg.append(c)
        pts.append(np.empty((n_vis, 3)))
        with_c = (c is not None) if want_c[k] is None else bool(want_c[k])
        if with_c and c is None:
            raise ValueError("return_colors asks for the colours of a frame without a colour image")
        cout.append(np.empty((n_vis, 3)) if with_c else None)
        pout.append(np.empty(n_vis, dtype=np.int32) if return_pixels else None)
    count = np.zeros(max(b, 1), dtype=np.int32)
    if b:
        def ptrs(arrs, t):
            return (t * b)(*[None if a is None or a.size == 0 else a.ctypes.data_as(t) for a in arrs])
        _handle(device).call(lib().teaser_hip_icp_unproject_depth_batch, b, frames, ptrs(dimg, _vp), ptrs(cimg, _vp),
                             count.ctypes.data_as(_ip), ptrs(pts, _dp), ptrs(cout, _dp), ptrs(pout, _ip))
    cut = lambda a, k: None if a is None else (a if count[k] == len(a) else a[:count[k]].copy())  # noqa: E731
    return [DepthCloud(cut(pts[k], k), cut(cout[k], k), cut(pout[k], k)) for k in range(b)]


def project_depth_batch(clouds, widths, heights, intrinsics, colors=None, extrinsics=None, depth_scale=1000.0,
                        depth_max=3.0, return_index=False, device=-1):
    """Per cloud a DepthProjection (include/teaser_hip.h, "Depth frames").  clouds: a list of n x 3 arrays; colors: None,
    or a list with an n x 3 array or None per cloud (a cloud with colours gets its colour image); the other arguments
    one for all clouds or a list with one per cloud.  extrinsics are world-to-camera and used as given."""
    from . import lib
    pts = [_cloud(c, "points", kind="array of points") for c in clouds]
    b = len(pts)
    cols = list(colors) if colors is not None else [None] * b
    if len(cols) != b:
        raise ValueError("colors: one array (or None) per cloud")
    W, H = _each(widths, b, "widths", _is_scalar), _each(heights, b, "heights", _is_scalar)
    K = [_fxfycxcy(k) for k in _each(intrinsics, b, "intrinsics", _is_intrinsic)]
    E = [_matrix(m, "extrinsic") for m in _each(extrinsics, b, "extrinsics", _is_matrix)]
    scale, dmax = _each(depth_scale, b, "depth_scale", _is_scalar), _each(depth_max, b, "depth_max", _is_scalar)
    cams = (IcpProjectionC * max(b, 1))()
    depth, cimg, index = [], [], []
    for k in range(b):
        for arr, what in ((pts[k], "points"), (cols[k], "colors")):
            if arr is not None and not np.isfinite(np.asarray(arr, dtype=np.float64)).all():
                raise ValueError("%s: cloud %d has a non-finite component" % (what, k))
        if cols[k] is not None:
            cols[k] = _cloud(cols[k], "colors", kind="array of colours")
            if cols[k].shape != pts[k].shape:
                raise ValueError("colors: cloud %d has %d points and %d colours" % (k, len(pts[k]), len(cols[k])))
        w, h = int(W[k]), int(H[k])
        if w < 0 or h < 0:
            raise ValueError("width and height must be >= 0")
        cam = cams[k]
        cam.width, cam.height = w, h
        cam.fx, cam.fy, cam.cx, cam.cy = K[k]
        cam.extrinsic[:] = list(E[k].ravel())
        cam.depth_scale, cam.depth_max = float(scale[k]), float(dmax[k])
        depth.append(np.zeros((h, w), dtype=np.float32))
        cimg.append(np.zeros((h, w, 3), dtype=np.float32) if cols[k] is not None else None)
        index.append(np.full((h, w), -1, dtype=np.int32) if return_index else None)
    n = np.array([len(p) for p in pts] + ([0] if not b else []), dtype=np.int32)
    hit = np.zeros(max(b, 1), dtype=np.int32)
    if b:
        def ptrs(arrs, t):
            return (t * b)(*[None if a is None or a.size == 0 else a.ctypes.data_as(t) for a in arrs])
        _handle(device).call(lib().teaser_hip_icp_project_depth_batch, b, ptrs(pts, _dp), ptrs(cols, _dp),
                             n.ctypes.data_as(_ip), cams, ptrs(depth, _fp), ptrs(cimg, _fp), ptrs(index, _ip),
                             hit.ctypes.data_as(_ip))
    return [DepthProjection(depth[k], int(hit[k]), cimg[k], index[k]) for k in range(b)]


# ---- Open3D's names ---------------------------------------------------------------------------------------------------
def create_point_cloud_from_depth_image_batch(depths, intrinsics, extrinsics=None, depth_scale=1000.0, depth_trunc=1000.0,
                                              stride=1, project_valid_depth_only=True, return_pixels=False, device=-1):
    """create_point_cloud_from_depth_image for a list of depth images in one launch sequence: per frame the points, with
    return_pixels the pair (points, pixels)."""
    r = unproject_depth_batch(depths, intrinsics, None, extrinsics, depth_scale, depth_trunc, stride, False,
                              project_valid_depth_only, None, return_pixels, device=device)
    return [(x.points, x.pixels) if return_pixels else x.points for x in r]


def create_point_cloud_from_depth_image(depth, intrinsic, extrinsic=None, depth_scale=1000.0, depth_trunc=1000.0,
                                        stride=1, project_valid_depth_only=True, return_pixels=False, device=-1):
    """Open3D's PointCloud.create_from_depth_image: the count x 3 points of the valid pixels in row-major order (with
    project_valid_depth_only=False a row per visited pixel, NaN where the depth is invalid); with return_pixels also the
    int32 pixel index (row width + column) of every point."""
    return create_point_cloud_from_depth_image_batch([depth], intrinsic, extrinsic, depth_scale, depth_trunc, stride,
                                                     project_valid_depth_only, return_pixels, device)[0]


def create_point_cloud_from_rgbd_image_batch(colors, depths, intrinsics, extrinsics=None, depth_scale=1000.0,
                                             depth_trunc=3.0, convert_rgb_to_intensity=True,
                                             project_valid_depth_only=True, device=-1):
    """create_point_cloud_from_rgbd_image for lists of images in one launch sequence: per frame (points, colors)."""
    if any(c is None for c in colors):
        raise ValueError("colors: one colour image per frame")
    r = unproject_depth_batch(depths, intrinsics, colors, extrinsics, depth_scale, depth_trunc, 1, convert_rgb_to_intensity,
                              project_valid_depth_only, True, False, device=device)
    return [(x.points, x.colors) for x in r]


def create_point_cloud_from_rgbd_image(color, depth, intrinsic, extrinsic=None, depth_scale=1000.0, depth_trunc=3.0,
                                       convert_rgb_to_intensity=True, project_valid_depth_only=True, device=-1):
    """Open3D's RGBDImage.create_from_color_and_depth(color, depth, depth_scale, depth_trunc, convert_rgb_to_intensity)
    followed by PointCloud.create_from_rgbd_image: (points, colors), both count x 3 float64."""
    return create_point_cloud_from_rgbd_image_batch([color], [depth], intrinsic, extrinsic, depth_scale, depth_trunc,
                                                    convert_rgb_to_intensity, project_valid_depth_only, device)[0]


def project_to_depth_image_batch(clouds, widths, heights, intrinsics, extrinsics=None, depth_scale=1000.0, depth_max=3.0,
                                 device=-1):
    """project_to_depth_image for a list of clouds in one launch sequence: per cloud the height x width float32 image."""
    return [r.depth for r in project_depth_batch(clouds, widths, heights, intrinsics, None, extrinsics, depth_scale,
                                                 depth_max, device=device)]


def project_to_depth_image(points, width, height, intrinsic, extrinsic=None, depth_scale=1000.0, depth_max=3.0, device=-1):
    """Open3D's t.geometry.PointCloud.project_to_depth_image: the height x width float32 depth image of the cloud seen
    by the camera, 0 where no point lands; a pixel shows its nearest point."""
    return project_to_depth_image_batch([points], width, height, intrinsic, extrinsic, depth_scale, depth_max, device)[0]


def project_to_rgbd_image_batch(clouds, colors, widths, heights, intrinsics, extrinsics=None, depth_scale=1000.0,
                                depth_max=3.0, device=-1):
    """project_to_rgbd_image for lists of clouds and colours in one launch sequence: per cloud (depth, color)."""
    if any(c is None for c in colors):
        raise ValueError("colors: one array per cloud")
    return [(r.depth, r.color) for r in project_depth_batch(clouds, widths, heights, intrinsics, colors, extrinsics,
                                                            depth_scale, depth_max, device=device)]


def project_to_rgbd_image(points, colors, width, height, intrinsic, extrinsic=None, depth_scale=1000.0, depth_max=3.0,
                          device=-1):
    """Open3D's t.geometry.PointCloud.project_to_rgbd_image: (depth height x width float32, color height x width x 3
    float32), the colour of a pixel being that of the point its depth comes from."""
    return project_to_rgbd_image_batch([points], [colors], width, height, intrinsic, extrinsic, depth_scale, depth_max,
                                       device)[0]


__all__ = ["PinholeCameraIntrinsic", "DepthCloud", "DepthProjection", "unproject_depth_batch", "project_depth_batch",
           "create_point_cloud_from_depth_image", "create_point_cloud_from_depth_image_batch",
           "create_point_cloud_from_rgbd_image", "create_point_cloud_from_rgbd_image_batch", "project_to_depth_image",
           "project_to_depth_image_batch", "project_to_rgbd_image", "project_to_rgbd_image_batch"]
