"""The numpy restatement of RGB-D odometry (tests/odometry_reference.py) pinned by facts worked out by hand, not by
itself: the filters and the down-sampling of a 4 x 4 ramp, the correspondences of a plane shifted by whole pixels, one
pixel's hybrid Jacobian from the formulas in their cross-product form, the information matrix of three points, the
6 x 6 solve against numpy.linalg.solve, the recovery of a known motion, the properties the shared cases must have, and
the Python twin of fdet_sincos_d against the C++ function (through the host driver) and against libm."""
import importlib
import math
import subprocess

import numpy as np

import odometry_reference as R
from odometry_cxx import host_driver

f32 = np.float32
tp = importlib.import_module("teaser-plusplus_amd")


def test_filters_and_down_sampling_of_a_ramp():
    p = np.arange(16, dtype=f32).reshape(4, 4)            # p(y, x) = 4 y + x: every value below is exact in float32
    x0, x3, y0, y3 = (np.arange(4) == 0), (np.arange(4) == 3), (np.arange(4) == 0)[:, None], (np.arange(4) == 3)[:, None]
    # the Gaussian leaves a ramp alone except where a tap clamps: + a quarter step at the low edge, - at the high edge
    want = p + 0.25 * x0 - 0.25 * x3 + 1.0 * y0 - 1.0 * y3
    assert np.array_equal(R.gauss(p), want.astype(f32))
    assert np.array_equal(R.down(p), np.array([[2.5, 4.5], [10.5, 12.5]], dtype=f32))
    # Sobel dx: the difference is 2 inside and 1 at a clamped edge, the smoothing (1, 2, 1) sums to 4; dy likewise with
    # the row step 4
    dx = np.where(x0 | x3, 4.0, 8.0) * np.ones((4, 1))
    dy = np.where(y0 | y3, 16.0, 32.0) * np.ones((1, 4))
    assert np.array_equal(R.filter3(p, R.SOBEL_D, R.SOBEL_S), dx.astype(f32))
    assert np.array_equal(R.filter3(p, R.SOBEL_S, R.SOBEL_D), dy.astype(f32))
    # a NaN spreads to its 3 x 3 neighbourhood and is stored as THE quiet NaN; a 1 x 1 image clamps every tap
    q = p.copy()
    q[1, 2] = -np.nan
    g = R.gauss(q)
    assert np.isnan(g[0:3, 1:4]).all() and not np.isnan(g[:, 0]).any() and not np.isnan(g[3]).any()
    assert (g.view(np.uint32)[np.isnan(g)] == 0x7FC00000).all()
    assert np.array_equal(R.gauss(np.array([[3.0]], dtype=f32)), np.array([[3.0]], dtype=f32))
    assert R.down(np.zeros((5, 7), dtype=f32)).shape == (2, 3)   # floored halving drops a row and a column


def test_depth_and_intensity_conversion():
    d = np.array([[0, 1000, 2999, 3000, 4001]], dtype=np.uint16)
    z = R.convert_depth(d, 1000.0, 3.0, 0.0, 4.0)
    assert np.isnan(z[0, 0]) and z[0, 1] == f32(1.0) and z[0, 2] == f32(2999) / f32(1000) and np.isnan(z[0, 3]) and np.isnan(z[0, 4])
    fl = np.array([[0.0, -0.0, np.nan, -1.0, np.inf, 1.5, 4.0, 4.5]], dtype=f32)
    z = R.convert_depth(fl, 1000.0, 3.0, 0.0, 4.0)          # float32 samples: neither scale nor truncation
    assert np.isnan(z[0, :5]).all() and z[0, 5] == f32(1.5) and z[0, 6] == f32(4.0) and np.isnan(z[0, 7])
    rgb = np.array([[[255, 255, 255], [255, 0, 0], [0, 0, 0]]], dtype=np.uint8)
    i = R.convert_color(rgb)
    assert i[0, 2] == 0 and i[0, 1] == f32(0.2990) * f32(255) / f32(255) and abs(float(i[0, 0]) - 1.0) < 1e-6


def test_correspondences_of_a_plane_shifted_by_whole_pixels():
    """Constant depth 2, f = 4, a translation of 1 along x: u' = u + f t / d = u + 2 exactly."""
    h, w = 3, 7
    D = np.full((h, w), 2.0, dtype=f32)
    K = (4.0, 4.0, 3.0, 1.0)
    T = np.eye(4)
    T[0, 3] = 1.0
    tp_, src = R.correspondences(K, T, 0, D, D, 0.0)
    want_t = np.array([v * w + u + 2 for v in range(h) for u in range(w - 2)])
    assert np.array_equal(tp_, want_t) and np.array_equal(src, want_t - 2)
    # one level up the intrinsics are halved: the shift is one pixel
    tp_, src = R.correspondences(K, T, 1, D, D, 0.0)
    assert np.array_equal(src, tp_ - 1) and len(tp_) == h * (w - 1)
    # a target that is 0.02 off is kept at depth_diff_max 0.03 and rejected at 0.01; a NaN target is skipped
    D2 = D.copy()
    D2[1, 4] = f32(2.02)
    D2[2, 5] = np.nan
    assert len(R.correspondences(K, T, 0, D, D2, 0.03)[0]) == h * (w - 2) - 1
    assert len(R.correspondences(K, T, 0, D, D2, 0.01)[0]) == h * (w - 2) - 2
    # x = -0.3 + 0.5 truncates to pixel 0 (Open3D's int(u + 0.5)); x = -0.6 + 0.5 = -0.1 also truncates to 0
    T[0, 3] = -0.15                                             # a shift of -0.3 pixels
    tp_, src = R.correspondences(K, T, 0, D, D, 0.0)
    assert np.array_equal(tp_, src) and len(tp_) == h * w


def test_the_tie_case_really_ties_and_the_smallest_source_pixel_wins():
    cs = R.cases()["ties"]
    lev = R.result("ties").levels[0]
    tp_, src, (pix, bits, s) = R.correspondences(cs.pair.K, cs.pair.odo_init, 0, lev["D_s"], lev["D_t"], cs.opt.depth_diff_max, with_keys=True)
    ties = 0
    for p in np.unique(pix):
        m = pix == p
        best = bits[m].min()
        if (bits[m] == best).sum() > 1:
            ties += 1
            assert src[np.searchsorted(tp_, p)] == s[m][bits[m] == best].min()
    assert ties >= 1


def test_the_cases_have_what_they_are_there_for():
    c = R.cases()
    n0 = {name: c[name].pair.source_depth.size for name in c}
    assert (n0["block"], n0["block-1"], n0["block+1"], n0["group+1"]) == (R.BLOCK, R.BLOCK - 1, R.BLOCK + 1, R.GROUP * R.BLOCK + 1)
    assert [lev["D_s"].shape for lev in R.result("8x8").levels] == [(8, 8), (4, 4), (2, 2)]
    assert [lev["D_s"].shape for lev in R.result("4x4").levels] == [(4, 4), (2, 2), (1, 1)]
    assert [lev["D_s"].shape for lev in R.result("37x29").levels] == [(29, 37), (14, 18), (7, 9)]
    r = R.result("no_correspondence")
    assert not r.success and r.count == 0 and r.trace[0]["failed"] == 1 and np.array_equal(r.transformation, np.eye(4))
    r = R.result("singular")
    assert not r.success and r.count > 0 and not r.information.any() and np.array_equal(r.transformation, np.eye(4))
    r = R.result("no_iteration")
    assert r.success and r.iterations == 0 and np.array_equal(r.transformation, c["no_iteration"].pair.odo_init) and r.information[3, 3] == r.count > 0
    assert [t["level"] for t in R.result("skip_level").trace] == [0, 0, 0]
    # depth_diff rejections and the depth range: fewer correspondences than the same frames give without them
    cs = c["depth_diff"]
    lev = R.result("depth_diff").levels[0]
    tight = len(R.correspondences(cs.pair.K, np.eye(4), 0, lev["D_s"], lev["D_t"], cs.opt.depth_diff_max)[0])
    loose = len(R.correspondences(cs.pair.K, np.eye(4), 0, lev["D_s"], lev["D_t"], 10.0)[0])
    assert 0 < tight < loose
    lev = R.result("depth_range").levels[0]
    assert 0 < np.isnan(lev["D_s"]).sum() < lev["D_s"].size and np.isnan(R.result("f32_specials").levels[0]["D_s"]).any()
    assert c["37x29"].pair.source_depth.strides[0] > 37 * 2 and c["37x29"].pair.source_color.strides[0] > 37 * 3
    assert {c[n].pair.jacobian for n in c} == {0, 1} and not np.array_equal(c["big_init"].pair.odo_init, np.eye(4))


def test_one_pixel_of_the_hybrid_jacobian():
    """The rows in their cross-product form: with c = gradient (f / z, g / z, -(f x + g y) / z^2 weights) the photometric
    row is sqrt(1 - lambda) [p x c, c] and the geometric one sqrt(lambda) [p x (d - e_z), d - e_z]."""
    lev = {n: np.zeros((2, 2), dtype=f32) for n in R.PLANES}
    lev["X"][0, 1], lev["Y"][0, 1], lev["Z"][0, 1] = 0.25, -0.5, 2.0
    lev["I_s"][0, 1], lev["I_t"][1, 0], lev["D_t"][1, 0] = 0.25, 0.75, 2.5
    lev["I_t_dx"][1, 0], lev["I_t_dy"][1, 0], lev["D_t_dx"][1, 0], lev["D_t_dy"][1, 0] = 4.0, -8.0, 0.5, np.nan
    K, T = (8.0, 4.0, 0.5, 0.5), R.pose(0.1, -0.2, 0.3, (0.05, 0.1, -0.25))
    J, r = R.jacobian_rows(K, T, 1, lev, np.array([2]), np.array([1]), R.HYBRID)
    f, g = 4.0, 2.0                                            # level 1: the intrinsics halved
    p = T[:3, :3] @ np.array([0.25, -0.5, 2.0]) + T[:3, 3]
    grad_i, grad_d = np.array([0.125 * 4.0, 0.125 * -8.0]), np.array([0.125 * 0.5, 0.0])   # the NaN gradient counts as 0

    def chain(gr):
        return np.array([gr[0] * f / p[2], gr[1] * g / p[2], -(gr[0] * f * p[0] + gr[1] * g * p[1]) / p[2] ** 2])
    c, d = chain(grad_i), chain(grad_d) - np.array([0.0, 0.0, 1.0])
    sI, sD = math.sqrt(1 - 0.968), math.sqrt(0.968)
    assert np.allclose(J[0, 0], sI * np.concatenate([np.cross(p, c), c]), rtol=1e-13, atol=1e-15)
    assert np.allclose(J[0, 1], sD * np.concatenate([np.cross(p, d), d]), rtol=1e-13, atol=1e-15)
    assert np.allclose(r[0], [sI * 0.5, sD * (2.5 - p[2])], rtol=1e-13)
    Jc, rc = R.jacobian_rows(K, T, 1, lev, np.array([2]), np.array([1]), R.COLOR)
    assert Jc.shape == (1, 1, 6) and np.allclose(Jc[0, 0], np.concatenate([np.cross(p, c), c]), rtol=1e-13) and rc[0, 0] == 0.5
    v = R.pixel_values(J, r)[0]
    assert np.allclose(v[:21], [J[0, 0, i] * J[0, 0, j] + J[0, 1, i] * J[0, 1, j] for i in range(6) for j in range(i, 6)])
    assert np.allclose(v[21:27], J[0].T @ r[0]) and np.isclose(v[27], r[0] @ r[0]) and v[28] == 1.0


def test_the_information_matrix_of_three_points():
    """fx = fy = 1, cx = cy = 0: the point of pixel (v, u) with depth z is (u z, v z, z), all small integers here, so the
    sum of G^T G with G = [-[p]x | I] is exact in any order."""
    Dt = np.full((3, 3), np.nan, dtype=f32)
    Dt[1, 2], Dt[0, 1], Dt[2, 0] = 2.0, 3.0, 1.0
    tp_ = np.array([1, 5, 6])
    info, n = R.information((1.0, 1.0, 0.0, 0.0), Dt, tp_)
    want = np.zeros((6, 6))
    for p in ((3.0, 0.0, 3.0), (4.0, 2.0, 2.0), (0.0, 2.0, 1.0)):
        x, y, z = p
        G = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]])
        want += G.T @ G
    assert n == 3 and np.array_equal(info, want) and info[3, 3] == 3


def test_the_summation_order():
    """Three values whose sum depends on the order: 1e16 + 1 + 1 is 1e16 when the ones are added one at a time and
    1e16 + 2 when they meet first.  In a run's tree pixel 0 meets pixel 2 (o = 2) before pixel 1 (o = 1), which has met
    pixel 3 by then; run 0 meets run 1 before the sum of runs 2 and 3."""
    big = 1e16
    v = np.zeros((3, 1))
    v[:, 0] = [big, 1.0, 1.0]
    assert R.ordered_sum(R.BLOCK, np.array([0, 1, 3]), v)[0] == big + 2.0      # o = 2: v[1] + v[3] = 2; o = 1: big + 2
    assert R.ordered_sum(R.BLOCK, np.array([0, 2, 3]), v)[0] == big            # o = 2: v[0] + v[2] rounds to big; o = 1 again
    assert R.ordered_sum(R.BLOCK, np.array([0, 1, 2]), v)[0] == big            # (big + 1) rounds, then + 1 rounds
    assert R.ordered_sum(R.BLOCK, np.array([0, 64, 128]), v)[0] == big         # (run0 + run1) + (run2 + run3)
    assert R.ordered_sum(R.BLOCK, np.array([0, 128, 192]), v)[0] == big + 2.0
    # blocks of a group one at a time from 0.0; groups likewise
    assert R.ordered_sum(3 * R.BLOCK, np.array([0, R.BLOCK, 2 * R.BLOCK]), v)[0] == big
    n = (R.GROUP + 2) * R.BLOCK
    assert R.ordered_sum(n, np.array([0, R.GROUP * R.BLOCK, (R.GROUP + 1) * R.BLOCK]), v)[0] == big + 2.0


def test_the_solve_against_numpy_and_its_failures():
    """Not bit equality: LDL^T without pivoting against LAPACK's pivoted LU.  On 200 well-conditioned systems (J^T J of
    40 x 6 normal draws) the largest difference relative to the largest entry of the solution was measured as 5.433e-16;
    the assertion is that figure doubled."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(200):
        J = rng.normal(size=(40, 6))
        A, g = J.T @ J, rng.normal(size=6)
        tot = np.concatenate([[A[i, j] for i in range(6) for j in range(i, 6)], g])
        x, y = np.array(R.solve(tot)), np.linalg.solve(A, -g)
        worst = max(worst, np.abs(x - y).max() / np.abs(y).max())
    print("largest relative difference", worst)
    assert worst <= 2 * 5.433e-16
    eye = np.concatenate([[1.0 if i == j else 0.0 for i in range(6) for j in range(i, 6)], np.ones(6)])
    assert R.solve(eye) == [-1.0] * 6
    assert R.solve(np.zeros(27)) is None                       # a zero pivot
    small = eye.copy()
    small[0] = 1e-7                                            # |product of the pivots| < 1e-6
    assert R.solve(small) is None
    bad = eye.copy()
    bad[3] = np.nan
    assert R.solve(bad) is None
    neg = eye.copy()
    neg[0] = -1.0                                              # a negative pivot is no failure (Open3D tests |det| only)
    assert R.solve(neg) is not None


def test_the_pose_update():
    x = [0.01, -0.02, 0.03, 0.1, 0.2, -0.3]
    T = R.update(R.pose(0.3, 0.2, 0.1, (1.0, 2.0, 3.0)), x)
    assert np.allclose(T, R.pose(x[0], x[1], x[2], x[3:]) @ R.pose(0.3, 0.2, 0.1, (1.0, 2.0, 3.0)), atol=1e-15)
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])


def test_a_known_motion_is_recovered():
    """The analytic scene from two known poses, 160 x 120, hybrid term, the default options, from the identity guess.
    Measured on a CPU: rotation error 2.2440 -> 0.056007 degrees (a factor of 40.07), translation error 0.041231 ->
    0.00053513 m (a factor of 77.05); profiles/odometry/README.md.  The restatement is deterministic; half of each factor
    is asserted, the margin only covers numpy versions."""
    truth = R.pose(0.02, -0.03, 0.015, (0.03, -0.02, 0.02))
    r = R.compute(R.make_pair(160, 120, truth), R.option())

    def errors(T):
        E = T @ np.linalg.inv(truth)
        return np.degrees(np.arccos(min(1.0, (np.trace(E[:3, :3]) - 1.0) / 2.0))), np.linalg.norm(E[:3, 3])
    (r0, t0), (r1, t1) = errors(np.eye(4)), errors(r.transformation)
    print("rotation", r0, "->", r1, "factor", r0 / r1, "translation", t0, "->", t1, "factor", t0 / t1)
    assert r.success and r.iterations == 35 and r.count > 15000
    assert r0 / r1 >= 40.07 / 2 and t0 / t1 >= 77.05 / 2
    assert np.allclose(r.information, r.information.T) and np.all(np.linalg.eigvalsh(r.information) > 0)


SINCOS_ARGUMENTS = [0.0, -0.0, 1e-300, 0.5, -0.5, math.pi / 4, math.pi / 2, -math.pi / 2, math.pi, -math.pi, 3.0, 100.0, -1234.5678,
                    65535.999, 65536.0, -65536.0, 411774.0, 411775.0, 1e6, -1e9, 1e15, 2.0 ** 52, 1e22, -1e100, 1e300,
                    1.7976931348623157e308, 0.7853981633974484, 2.356194490192345, 1e-8, -3e-5]


def test_the_python_twin_of_fdet_sincos_equals_the_cxx_function():
    out = subprocess.run([host_driver(), "--sincos"] + [x.hex() for x in SINCOS_ARGUMENTS], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")[:len(SINCOS_ARGUMENTS)]
    for x, line in zip(SINCOS_ARGUMENTS, lines):
        s, c = (float.fromhex(t) for t in line.split())
        ps, pc = R.sincos(x)
        assert (s.hex(), c.hex()) == (float(ps).hex(), float(pc).hex()), (x, s, c, ps, pc)


def test_fdet_sincos_against_libm():
    """Measured here, not assumed.  Over the samples below -- [-pi, pi] and [-65536, 65536] -- the
    largest error was 2.00 ulp and 2.2204460492503131e-16 absolute (one ulp of 1).  Beyond 65536 the reduction rounds a
    remainder: over the sample up to 1e9 the largest error was 1.4498277578489649e-11 (1.6e-11 over a larger sample).
    The assertions are the two absolute figures doubled."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for x in np.concatenate([rng.uniform(-math.pi, math.pi, 20000), np.linspace(-math.pi, math.pi, 2001), rng.uniform(-65536, 65536, 5000)]):
        s, c = R.sincos(x)
        worst = max(worst, abs(s - math.sin(x)), abs(c - math.cos(x)))
    assert worst <= 2 * 2.2204460492503131e-16, worst
    worst = 0.0
    for x in np.exp(rng.uniform(math.log(65536.0), math.log(1e9), 5000)):
        s, c = R.sincos(x)
        worst = max(worst, abs(s - math.sin(x)), abs(c - math.cos(x)))
        assert abs(s * s + c * c - 1.0) < 1e-15
    assert worst <= 2 * 1.4498277578489649e-11, worst
    for x in (1e22, -1e100, 1.7976931348623157e308):           # every finite argument: a point of the unit circle
        s, c = R.sincos(x)
        assert abs(s * s + c * c - 1.0) < 1e-15
    assert R.sincos(0.0) == (0.0, 1.0)


def test_the_names_are_exported():
    for name in ("OdometryOption", "RGBDOdometryJacobianFromColorTerm", "RGBDOdometryJacobianFromHybridTerm", "RGBDImage",
                 "compute_rgbd_odometry", "compute_rgbd_odometry_batch", "rgbd_odometry_pyramid_batch"):
        assert name in tp.__all__ and getattr(tp, name) is not None, name
    header = open(tp.LIB_PATH.replace("teaser-plusplus_amd/libteaser_hip.so", "include/teaser_hip.h")).read()
    assert "#define TEASER_HIP_ODOMETRY_BLOCK %d\n" % R.BLOCK in header and "#define TEASER_HIP_ODOMETRY_GROUP %d\n" % R.GROUP in header
