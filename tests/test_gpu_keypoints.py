"""Batched ISS keypoint detection on the MI355X against the numpy restatement (tests/keypoints_reference.py), bit for
bit and without a tolerance: the mask, the saliency bits, both counts and the radii of every cloud.  (NaN equals NaN
for the resolution of a cloud with given radii: the contract only says NaN.)"""
import ctypes as C
import importlib

import numpy as np
import pytest

import keypoints_reference as RK
import normals_reference as RN
import outlier_reference as RO
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")
DEFAULTS = dict(salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def run(clouds, params):
    """One call for all clouds; params: one dict per cloud."""
    full = [dict(DEFAULTS, **p) for p in params]
    cols = {k: [p[k] for p in full] for k in DEFAULTS}
    return tp.compute_iss_keypoints_batch(clouds, return_saliency=True, **cols)


def check(got, X, p, what):
    ind, det = got
    ref = RK.iss_keypoints(X, **dict(DEFAULTS, **p))
    print("%s: n %d, keypoints %d, m up to %d, radii %s" % (what, len(X), ref["keep"].sum(),
                                                            ref["count"][:, 0].max() if len(X) else 0, ref["radii"]))
    assert np.array_equal(ind, np.flatnonzero(ref["keep"])), what + ": mask"
    assert RO.bits_equal(det["saliency"], ref["saliency"]), what + ": saliency"
    assert np.array_equal(det["count"], ref["count"]), what + ": counts"
    assert RO.bits_equal([det["resolution"], det["salient_radius"], det["non_max_radius"]], ref["radii"]), what + ": radii"
    return ref


def mixed_batch():
    """The clouds and parameters of the issue's list, in one batch (an empty cloud in the middle)."""
    far = RN.cube(129, 9) + np.array([1e6, -1e6, 1e6])
    items = [(RN.cube(n, 10 + n), dict(salient_radius=r, non_max_radius=r, gamma_21=2.0, gamma_32=2.0))
             for n in (1, 2, 4, 5, 6) for r in (0.0, 2.0)]
    items += [(RN.cube(n, n), dict()) for n in (63, 64, 65, 129)]
    items += [(RN.cube(n, n), dict(salient_radius=0.4, non_max_radius=0.3)) for n in (63, 64, 65, 129)]
    items += [(np.zeros((0, 3)), dict()),
              (RN.cube(257, 7), dict(salient_radius=0.3, min_neighbors=3, gamma_21=0.9, gamma_32=0.8)),  # r_n = 0: automatic
              (RN.planar(), dict(salient_radius=0.35, non_max_radius=0.2)), (RN.planar(), dict()),
              (RN.collinear(), dict()), (RN.collinear(), dict(salient_radius=0.6, non_max_radius=0.4, min_neighbors=2)),
              (RN.identical(), dict()), (RN.identical(), dict(salient_radius=0.1, non_max_radius=0.1)),
              (RN.tied_lattice(), dict()), (RN.tied_lattice(), dict(salient_radius=0.55, non_max_radius=0.3, gamma_21=2.0,
                                                                    gamma_32=2.0)),
              (far, dict(salient_radius=0.3, non_max_radius=0.2)), (far, dict()),
              (RN.cube(65, 5), dict(salient_radius=0.3, non_max_radius=0.45)),     # r_n > r_s
              (RN.cube(300, 6), dict(salient_radius=0.35, non_max_radius=0.02)),   # r_n << r_s
              (RN.cube(200, 8), dict(salient_radius=0.3, non_max_radius=0.2, min_neighbors=0, gamma_21=2.0, gamma_32=2.0)),
              (RN.cube(200, 8), dict(salient_radius=0.3, non_max_radius=0.2, gamma_21=0.0)),
              (RN.cube(200, 8), dict(salient_radius=0.3, non_max_radius=0.2, gamma_32=0.0)),
              (RN.cube(200, 8), dict(salient_radius=0.3, non_max_radius=0.2, gamma_21=2.0, gamma_32=2.0))]
    return [x for x, _ in items], [p for _, p in items]


def test_mixed_batch_against_the_restatement_and_each_cloud_alone():
    clouds, params = mixed_batch()
    got = run(clouds, params)
    keypoints = 0
    for c, (X, p, g) in enumerate(zip(clouds, params, got)):
        ref = check(g, X, p, "cloud %d" % c)
        keypoints += int(ref["keep"].sum())
        alone = run([X], [p])[0]
        assert alone[0].tobytes() == g[0].tobytes(), c
        assert all(np.asarray(alone[1][k]).tobytes() == np.asarray(g[1][k]).tobytes() for k in ("saliency", "count")), c
        assert RO.bits_equal([alone[1][k] for k in ("resolution", "salient_radius", "non_max_radius")],
                             [g[1][k] for k in ("resolution", "salient_radius", "non_max_radius")]), c
    assert keypoints > 50
    again = run(clouds, params)  # run after run
    assert all(a[0].tobytes() == b[0].tobytes() and a[1]["saliency"].tobytes() == b[1]["saliency"].tobytes()
               for a, b in zip(got, again))


def test_uncapped_neighbourhoods_beyond_the_capped_kernels():
    X = RN.cube(600, 21)
    p = dict(salient_radius=0.42, non_max_radius=0.2)
    ref = check(run([X], [p])[0], X, p, "600-point cube")
    assert (ref["count"][:, 0] > 100).mean() > 0.5 and ref["keep"].sum() > 0


def test_tied_lattice_permutes_with_the_cloud():
    X = RN.tied_lattice()
    perm = np.random.default_rng(6).permutation(len(X))
    for p in (dict(), dict(salient_radius=0.3, non_max_radius=0.6, gamma_21=2.0, gamma_32=2.0)):
        a, b = run([X, X[perm]], [p, p])
        check(a, X, p, "lattice")
        check(b, X[perm], p, "lattice permuted")
        mask_a, mask_b = np.zeros(len(X), bool), np.zeros(len(X), bool)
        mask_a[a[0]], mask_b[b[0]] = True, True
        assert np.array_equal(mask_a[perm], mask_b)  # every sum is exact: the same set gives the same bits
        assert a[1]["saliency"][perm].tobytes() == b[1]["saliency"].tobytes()
    assert len(a[0]) == 27  # the second parameter set: tied maxima inside each other's ball survive together


def test_down_sampled_config5_cloud():
    """The first 1500 points of a config-5 cloud (the fixture holds the clouds after voxel down-sampling, in voxel order:
    a contiguous part of the scene), so that the restatement's per-point loops stay within a second or two."""
    Z = np.load(ROOT + "/tests/golden/config5_clouds.npz")
    X = np.ascontiguousarray(Z["cloud_bin_0"][:1500], dtype=np.float64)
    ref = check(run([X], [dict()])[0], X, dict(), "config 5, down-sampled")
    assert ref["keep"].sum() > 0


WIDE = dict(salient_radius=0.4, non_max_radius=0.3, gamma_21=2.0, gamma_32=2.0, min_neighbors=3)
ORDINARY = dict(salient_radius=0.4, non_max_radius=0.3)


def width(clouds, params):
    return RK.key_bits(clouds, [p["salient_radius"] for p in params], [p["non_max_radius"] for p in params])


def in_a_batch(X):
    return [RN.cube(65, 65), X, np.zeros((0, 3)), RN.cube(129, 129)], [ORDINARY, WIDE, ORDINARY, ORDINARY]


def test_keys_wider_than_a_word_half_and_the_63_bit_boundary():
    """One cloud's key is 3 k + 1 bits when its box is a cube (k cell bits per axis and one bit of grid id), which 63
    is not: the single cloud of 63 bits has its z side halved (21 + 21 + 20 cell bits).  In the batch of four the id
    takes 3 bits, and a cube of 20 cell bits per axis gives 63."""
    a, b, b4 = RK.corner_clusters(512.0, 512.0, 512.0), RK.corner_clusters(393216.0, 393216.0, 196608.0), \
        RK.corner_clusters(196608.0, 196608.0, 196608.0)
    assert width([a], [WIDE]) == 34 and width(*in_a_batch(a)) == 36      # (a): above 32, the shifts leave the low half
    assert width([b], [WIDE]) == 63 and width(*in_a_batch(b4)) == 63     # (b): the widest key the call serves
    for X in (a, b, b4):
        ref = check(run([X], [WIDE])[0], X, WIDE, "clusters alone")
        assert ref["keep"].sum() > 0 and (ref["count"][:, 0] > 0).any()
    for X in (a, b4):
        clouds, params = in_a_batch(X)
        got = run(clouds, params)
        for c, (Y, p, g) in enumerate(zip(clouds, params, got)):
            check(g, Y, p, "clusters in a batch, cloud %d" % c)
        alone = run([X], [WIDE])[0]
        assert alone[0].tobytes() == got[1][0].tobytes() and alone[1]["saliency"].tobytes() == got[1][1]["saliency"].tobytes()
        assert alone[1]["count"].tobytes() == got[1][1]["count"].tobytes()


def test_a_64_bit_key_is_refused_naming_the_finer_grid():
    """One bit above the boundary, alone and at index 1 of a batch; the radius named is the one the predictor finds."""
    X = RK.corner_clusters(393216.0, 393216.0, 393216.0)  # 3 * 2^17: 21 cell bits per axis at r = 0.3, 20 at 0.4 and 0.45
    mirrored = dict(WIDE, salient_radius=0.3, non_max_radius=0.45)
    ok = RN.cube(65, 5)
    for p, named in ((WIDE, "non_max_radius"), (mirrored, "salient_radius")):
        assert width([X], [p]) == 64
        assert RK.refused_for_width([X], p["salient_radius"], p["non_max_radius"]) == (0, named)
        with pytest.raises(tp.TeaserHipError) as e:
            run([X], [p])
        assert named + " is too small" in str(e.value) and "problem 0" in str(e.value), str(e.value)
        assert width([ok, X], [ORDINARY, p]) == 65
        assert RK.refused_for_width([ok, X], [0.4, p["salient_radius"]], [0.3, p["non_max_radius"]]) == (1, named)
        with pytest.raises(tp.TeaserHipError) as e:
            run([ok, X], [ORDINARY, p])
        assert named + " is too small" in str(e.value) and "problem 1" in str(e.value), str(e.value)
        check(run([ok], [ORDINARY])[0], ok, ORDINARY, "after the refusal of " + named)


def test_keypoint_counts_equal_the_masks():
    """n_keypoints_out comes from a ballot and an atomicAdd per wave; the mask is written per point.  Straight through
    the C ABI for the mixed batch, next to the Python wrapper's own check of the same equality."""
    from importlib import import_module
    kp = import_module("teaser-plusplus_amd.keypoints")
    icp = import_module("teaser-plusplus_amd.icp")
    clouds, params = mixed_batch()
    clouds = [np.ascontiguousarray(X, dtype=np.float64) for X in clouds]
    b = len(clouds)
    rec = (kp.ISSParamsC * b)(*[kp.ISSParamsC(*[dict(DEFAULTS, **p)[k] for k in DEFAULTS], 0) for p in params])
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    n = np.array([len(X) for X in clouds], dtype=np.int32)
    keep = [np.full(len(X), 7, dtype=np.uint8) for X in clouds]
    kept = np.full(b, -1, dtype=np.int32)
    icp._handle(-1).call(tp.lib().teaser_hip_icp_iss_keypoints_batch, b, (dp * b)(*[X.ctypes.data_as(dp) for X in clouds]),
                         n.ctypes.data_as(ip), rec, (bp * b)(*[k.ctypes.data_as(bp) for k in keep]),
                         kept.ctypes.data_as(ip), None, None, None)
    assert kept.tolist() == [int(k.sum()) for k in keep] and kept.sum() > 50 and all(k.max(initial=0) <= 1 for k in keep)


def test_refusals_name_the_argument_and_the_cloud_and_leave_the_handle_usable():
    X = RN.cube(65, 5)
    bad = X.copy()
    bad[3, 1] = np.inf
    ok = dict(salient_radius=0.3, non_max_radius=0.2)
    for cloud, p, word in ((bad, ok, "points"), (X, dict(ok, salient_radius=-1.0), "salient_radius"),
                           (X, dict(ok, salient_radius=np.nan), "salient_radius"),
                           (X, dict(ok, salient_radius=1e200), "salient_radius"),
                           (X, dict(ok, non_max_radius=-1.0), "non_max_radius"),
                           (X, dict(ok, non_max_radius=np.inf), "non_max_radius"),
                           (X, dict(ok, gamma_21=np.nan), "gamma_21"), (X, dict(ok, gamma_32=np.inf), "gamma_32"),
                           (X, dict(ok, min_neighbors=-1), "min_neighbors"),
                           (X, dict(ok, salient_radius=1e-9), "salient_radius is too small")):
        with pytest.raises(tp.TeaserHipError) as e:
            run([X, cloud], [ok, p])
        assert word in str(e.value) and "problem 1" in str(e.value), str(e.value)
        check(run([X], [ok])[0], X, ok, "after the refusal of " + word)
    # NULL where n > 0, through the C ABI
    from importlib import import_module
    kp = import_module("teaser-plusplus_amd.keypoints")
    icp = import_module("teaser-plusplus_amd.icp")
    rec = (kp.ISSParamsC * 1)(kp.ISSParamsC(0.3, 0.2, 0.975, 0.975, 5, 0))
    n = np.array([len(X)], dtype=np.int32)
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    pp = (dp * 1)(X.ctypes.data_as(dp))
    kept = np.zeros(1, dtype=np.int32)
    with pytest.raises(tp.TeaserHipError) as e:
        icp._handle(-1).call(tp.lib().teaser_hip_icp_iss_keypoints_batch, 1, pp, n.ctypes.data_as(ip), rec,
                             (bp * 1)(None), kept.ctypes.data_as(ip), None, None, None)
    assert "keep_out" in str(e.value) and "problem 0" in str(e.value)
    check(run([X], [ok])[0], X, ok, "after the NULL refusal")
