"""The restatement of the depth-frame contract (tests/rgbd_reference.py) against what does not come from it: a frame
worked out by hand, the samples around the truncation, the pixels around a rounding boundary, the tie rule, a second
scalar form of the projection in Python floats, and a round trip that is exact by construction.  Also: the package exports
the new names (no device needed)."""
import importlib

import numpy as np
import pytest

import rgbd_reference as R

tp = importlib.import_module("teaser-plusplus_amd")


def test_worked_frame():
    """The 2 x 2 frame of the module docstring, both ways."""
    d = np.array([[1000, 0], [4000, 500]], dtype=np.uint16)
    f = R.Frame(2.0, 2.0, 0.5, 0.5, depth_scale=1000.0, depth_trunc=3.0)
    count, P, C, pix = R.unproject(d, None, f)
    assert count == 2 and C is None and pix.tolist() == [0, 3] and pix.dtype == np.int32
    assert P.tolist() == [[-0.25, -0.25, 1.0], [0.125, 0.125, 0.5]]
    count, P4, _, pix4 = R.unproject(d, None, f.but(valid_only=0))
    assert count == 4 and pix4.tolist() == [0, 1, 2, 3] and np.isnan(P4[1:3]).all() and P4[[0, 3]].tolist() == P.tolist()
    assert P4.view(np.uint64)[1, 0] == 0x7FF8000000000000
    depth, cimg, index, n_hit = R.project(P, None, R.Camera(2, 2, 2.0, 2.0, 0.5, 0.5, None, 1000.0, 3.0))
    assert depth.tolist() == [[1000.0, 0.0], [0.0, 500.0]] and index.tolist() == [[0, -1], [-1, 1]] and n_hit == 2
    assert cimg is None and depth.dtype == np.float32 and index.dtype == np.int32


def test_stride_visits_every_stride_th_row_and_column():
    d = np.arange(1, 36, dtype=np.uint16).reshape(5, 7)
    f = R.Frame(1.0, 1.0, 0.0, 0.0, depth_scale=1.0, depth_trunc=100.0)
    assert R.unproject(d, None, f.but(stride=2))[3].tolist() == [0, 2, 4, 6, 14, 16, 18, 20, 28, 30, 32, 34]
    assert R.unproject(d, None, f.but(stride=3))[3].tolist() == [0, 3, 6, 21, 24, 27]
    assert R.unproject(d, None, f.but(stride=8))[3].tolist() == [0]


def test_truncation_boundary():
    """depth_scale 1000, depth_trunc 3.0: 2999 is kept (2.999f < 3), 3000 gives exactly 3.0f and goes, like 3001 and
    65535; 0 is invalid.  A float32 frame is neither scaled nor truncated."""
    d = np.array([[0, 2999, 3000, 3001, 65535]], dtype=np.uint16)
    f = R.Frame(1.0, 1.0, 0.0, 0.0, depth_scale=1000.0, depth_trunc=3.0)
    assert R.depth_as_float(d, f).tolist() == [[0.0, float(np.float32(2999) / np.float32(1000)), 0.0, 0.0, 0.0]]
    assert R.unproject(d, None, f)[3].tolist() == [1]
    fl = np.array([[np.nan, -1.0, 1e-45, np.inf, 2.5, 3.0, 3000.0, 0.0, -0.0]], dtype=np.float32)
    count, P, _, pix = R.unproject(fl, None, f)
    assert pix.tolist() == [2, 3, 4, 5, 6] and P[4, 2] == 3000.0 and P[0, 2] == float(np.float32(1e-45)) and P[0, 2] > 0


def test_colour_formats():
    rgb = np.array([[[255, 0, 51], [10, 20, 30]]], dtype=np.uint8)
    d = np.array([[1, 1]], dtype=np.uint16)
    f = R.Frame(1.0, 1.0, 0.0, 0.0, depth_scale=1.0)
    assert R.unproject(d, rgb, f)[2].tolist() == [[1.0, 0.0, 0.2], [10 / 255.0, 20 / 255.0, 30 / 255.0]]
    inten = R.unproject(d, rgb, f.but(intensity=1))[2]
    w = [np.float32(x) for x in (0.2990, 0.5870, 0.1140)]
    want = ((w[0] * np.float32(10) + w[1] * np.float32(20)) + w[2] * np.float32(30)) / np.float32(255)
    assert inten[1].tolist() == [float(want)] * 3 and abs(inten[0, 0] - (0.299 + 0.114 * 0.2)) < 1e-6
    g = np.array([[0.25, 0.5]], dtype=np.float32)
    assert R.unproject(d, g, f)[2].tolist() == [[0.25] * 3, [0.5] * 3]
    c3 = np.array([[[0.25, 0.5, 0.75], [1.0, 0.0, 0.125]]], dtype=np.float32)
    assert R.unproject(d, c3, f)[2].tolist() == c3[0].astype(np.float64).tolist()


def test_rounding_boundary_and_tie_rule():
    """fx = 1, cx = 0.5, zc = 1: u = x + 0.5 exactly.  Halves round away from zero, so -0.5 leaves the image on the left
    and 2.5 on the right of a width of 3.  Equal depths: the smallest index wins; a smaller depth beats a smaller index."""
    assert R.round_half_away(np.array([-0.5, 0.5, 1.5, 2.5, 0.49999999999999994, -1.5, 2.0])).tolist() == [-1, 1, 2, 3, 0, -2, 2]
    cam = R.Camera(3, 2, 1.0, 1.0, 0.5, 0.5)
    P = np.array([[-1.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [2.0, 0.0, 1.0]])
    depth, _, index, n_hit = R.project(P, None, cam)
    assert index.tolist() == [[-1, -1, -1], [-1, 1, 2]] and n_hit == 2
    tie = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 1.5], [0.0, 0.0, 1.5], [0.0, 0.0, 1.5 + 1e-12]])
    depth, _, index, n_hit = R.project(tie, None, cam)
    assert n_hit == 1 and index[1, 1] == 1 and depth[1, 1] == np.float32(1500.0)
    depth, _, index, _ = R.project(tie[::-1], None, cam)
    assert index[1, 1] == 0  # 1.5 + 1e-12 rounds to the same float32 depth and now has the smallest index
    at_max = np.array([[0.0, 0.0, 3.0], [0.0, 0.0, np.nextafter(3.0, 4.0)], [0.0, 0.0, 0.0], [0.0, 0.0, -2.0], [0.0, 0.0, np.nan]])
    assert R.project(at_max, None, cam)[2][1, 1] == 0 and R.project(at_max, None, cam)[3] == 1


@pytest.mark.parametrize("case", [c for c in R.project_cases() if len(c[1]) <= 3000], ids=lambda c: c[0])
def test_the_two_forms_of_the_projection_agree(case):
    _, P, C, cam = case
    depth, cimg, index, n_hit = R.project(P, C, cam)
    sdepth, sindex = R.project_scalar(P, cam)
    assert depth.tobytes() == sdepth.tobytes() and np.array_equal(index, sindex) and n_hit == int((index >= 0).sum())
    if C is not None:
        hit = index >= 0
        assert np.array_equal(cimg[hit], np.asarray(C)[index[hit]].astype(np.float32)) and (cimg[~hit] == 0).all()


def test_unprojection_cases_are_what_their_names_say():
    by = {name: (d, c, f) for name, d, c, f in R.unproject_cases()}
    assert R.unproject(*by["64x4_one_tile"])[3].max() < 256 and by["64x4_one_tile"][0].size == 256
    assert by["257x1"][0].shape == (1, 257) and by["1x257"][0].shape == (257, 1)
    assert R.unproject(*by["65x9_all"])[0] == 585 and R.unproject(*by["65x9_none"])[0] == 0
    assert R.unproject(*by["65x9_last"])[3].tolist() == [584] and R.unproject(*by["65x9_none_every_pixel"])[0] == 585
    d, c, f = by["color1_intensity1_padded"]
    assert d.strides[0] > d.shape[1] * 2 and c.strides[0] > c.shape[1] * 3 and f.intensity == 1
    assert R.unproject(*by["0x5"])[0] == 0 and R.unproject(*by["5x0"])[0] == 0


def test_round_trip_is_exact_in_the_restatement():
    d, f, cam = R.round_trip_frame()
    count, P, _, pix = R.unproject(d, None, f)
    depth, _, index, n_hit = R.project(P, None, cam)
    valid = R.depth_as_float(d, f) > 0
    assert 0 < count < d.size and count == int(valid.sum()) == n_hit
    assert np.array_equal(depth[valid], d[valid].astype(np.float32)) and (depth[~valid] == 0).all()
    assert np.array_equal(index[valid], np.arange(count)) and np.array_equal(np.flatnonzero(valid.ravel()), pix)


def test_the_package_exports_the_names():
    names = ["PinholeCameraIntrinsic", "create_point_cloud_from_depth_image", "create_point_cloud_from_depth_image_batch",
             "create_point_cloud_from_rgbd_image", "create_point_cloud_from_rgbd_image_batch", "project_to_depth_image",
             "project_to_depth_image_batch", "project_to_rgbd_image", "project_to_rgbd_image_batch",
             "unproject_depth_batch", "project_depth_batch", "DepthCloud", "DepthProjection"]
    for name in names:
        assert name in tp.__all__ and getattr(tp, name) is not None, name
    for sym in ("teaser_hip_icp_frame_default", "teaser_hip_icp_unproject_depth_batch", "teaser_hip_icp_project_depth_batch"):
        assert sym in tp.EXPORTED_SYMBOLS
    K = tp.PinholeCameraIntrinsic(640, 480, 525.0, 520.0, 319.5, 239.5)
    assert K.intrinsic_matrix.tolist() == [[525.0, 0.0, 319.5], [0.0, 520.0, 239.5], [0.0, 0.0, 1.0]]
    assert (K.width, K.height) == (640, 480)
