"""Plane segmentation on the GPU against the contract of include/teaser_hip.h ("Plane segmentation"), stage by stage
through teaser_hip_plane_trials_batch and then as the full call.  Every comparison with the numpy restatement
(tests/plane_reference.py) is BIT FOR BIT: there is no SVD and no transcendental on the device.
  1  samples, flags and planes per trial, at trial counts around the tile and chunk edges and at a first trial above
     2^32, for ransac_n 3, 5 and 8; a three-point cloud (some trials degenerate) and a collinear one (all of them)
  2  count and E per trial at the block and group edges of the summation order
  3  the full call equals the restatement's loop and finish
  4  the bits do not depend on chunk_trials, on the partial budget, on the batch around a problem or on the run
  5  defaults and refusals"""
import ctypes as C
import importlib

import numpy as np
import pytest

import plane_reference as PR
import plane_scenes as SC

tp = importlib.import_module("teaser-plusplus_amd")

pytestmark = pytest.mark.gpu
D = 0.01
DEFAULT_CHUNK, DEFAULT_PARTIAL = 256, 64 << 20


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture
def options():
    """Sets plane options for a test and puts the defaults back."""
    def set_options(chunk=DEFAULT_CHUNK, partial=DEFAULT_PARTIAL):
        tp.set_plane_option("chunk_trials", chunk)
        tp.set_plane_option("partial_bytes", partial)
    try:
        yield set_options
    finally:
        set_options()


def same_trials(dev, ref):
    assert np.array_equal(dev["samples"], ref["samples"])
    assert np.array_equal(dev["flags"], ref["flags"])
    assert np.array_equal(bits(dev["plane"]), bits(ref["plane"]))
    assert np.array_equal(dev["count"], ref["count"])
    assert np.array_equal(bits(dev["E"]), bits(ref["E"]))


def same_result(dev, ref):
    assert (dev.best_trial, dev.trials, dev.valid_trials) == (ref["best_trial"], ref["trials"], ref["valid_trials"])
    assert np.array_equal(bits(dev.plane_model), bits(ref["plane"]))
    assert np.array_equal(dev.inliers, ref["inliers"]) and dev.inliers.dtype == np.int32
    assert np.array_equal(dev.mask, ref["mask"])
    assert bits([dev.fitness, dev.inlier_rmse]).tolist() == bits([ref["fitness"], ref["inlier_rmse"]]).tolist()


# ---- 1 ----
CLOUD = SC.planted(300, 0.5, 1)


@pytest.mark.parametrize("first,cnt", [(0, 63), (0, 64), (0, 65), (0, 255), (0, 256), (0, 257), (0, 2048),
                                       ((1 << 32) + 12345, 257)])
@pytest.mark.parametrize("ransac_n", [3, 5, 8])
def test_samples_flags_and_planes_equal_the_restatement(ransac_n, first, cnt):
    seed = 100 + ransac_n
    dev = tp.plane_trials_batch([CLOUD], D, first, cnt, ransac_n, seed)[0]
    ref = PR.trials(CLOUD, D, ransac_n, seed, first, cnt)
    same_trials(dev, ref)
    assert dev["flags"].any() and np.abs(np.linalg.norm(dev["plane"][dev["flags"] == 1, :3], axis=1) - 1).max() < 1e-15


def test_three_points_some_trials_degenerate():
    P3 = np.array([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])
    dev = tp.plane_trials_batch([P3], 0.1, 0, 256, 3, 41)[0]
    same_trials(dev, PR.trials(P3, 0.1, 3, 41, 0, 256))
    degenerate = int((dev["flags"] == 0).sum())
    assert 0 < degenerate < 256
    assert not dev["plane"][dev["flags"] == 0].any() and not dev["count"][dev["flags"] == 0].any()
    assert (dev["count"][dev["flags"] == 1] == 3).all()


def test_collinear_cloud_every_trial_degenerate():
    P = SC.collinear(50)
    dev = tp.plane_trials_batch([P], 0.1, 0, 64, 3, 42)[0]
    same_trials(dev, PR.trials(P, 0.1, 3, 42, 0, 64))
    assert not dev["flags"].any() and not dev["plane"].any() and not dev["count"].any() and not dev["E"].any()
    r = tp.segment_plane_batch([P], 0.1, 3, 64, 0.99, 42)[0]
    same_result(r, PR.segment(P, 0.1, 3, 64, 0.99, 42))
    assert r.best_trial == -1 and r.trials == 64 and r.valid_trials == 0
    assert not r.plane_model.any() and len(r.inliers) == 0 and not r.mask.any()


# ---- 2 ----
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 16383, 16384, 16385, 2 * 16384 + 1])
def test_count_and_E_at_the_edges_of_the_sum_order(n):
    P = SC.planted(n, 0.5, 200 + n % 97)
    if n >= 255:
        share = (np.abs(P @ SC.PLANTED_NORMAL[:3] + SC.PLANTED_NORMAL[3]) < D).mean()
        assert 0.1 < share < 0.9
    dev = tp.plane_trials_batch([P], D, 0, 65, 3, 300 + n)[0]
    ref = PR.trials(P, D, 3, 300 + n, 0, 65)
    same_trials(dev, ref)
    if n >= 255:
        assert dev["count"].max() > 0.1 * n and (dev["E"] >= 0).all() and (dev["E"] < D * np.maximum(dev["count"], 1)).all()
    else:
        assert not dev["flags"].any() and (dev["samples"] == -1).all()  # n < ransac_n: nothing is drawn


# ---- 3 ----
FULL = {
    "stops_early": dict(P=SC.planted(3000, 0.6, 31), d=D, ransac_n=3, num_iterations=1000, probability=0.99999999, seed=7),
    "never_stops": dict(P=SC.planted(700, 0.5, 32), d=D, ransac_n=5, num_iterations=300, probability=1.0, seed=8),
    "exact_plane": dict(P=SC.grid_plane(300), d=1e-9, ransac_n=3, num_iterations=1000, probability=0.99999999, seed=5),
    "too_few": dict(P=SC.planted(2, 0.5, 33), d=D, ransac_n=3, num_iterations=100, probability=0.99, seed=9),
    "no_iterations": dict(P=SC.planted(40, 0.5, 34), d=D, ransac_n=3, num_iterations=0, probability=0.99, seed=10),
}
_restated = {}


def restated(name):
    """The restatement's result, once per process."""
    if name not in _restated:
        c = FULL[name]
        _restated[name] = PR.segment(c["P"], c["d"], c["ransac_n"], c["num_iterations"], c["probability"], c["seed"])
    return _restated[name]


def run(name):
    c = FULL[name]
    return tp.segment_plane_batch([c["P"]], c["d"], c["ransac_n"], c["num_iterations"], c["probability"], c["seed"])[0]


@pytest.mark.parametrize("name", list(FULL))
def test_full_call_equals_the_restatements_loop_and_finish(name):
    ref, dev = restated(name), run(name)
    same_result(dev, ref)
    if name == "stops_early":
        assert 1 < dev.trials < 1000 and dev.best_trial >= 0 and 0.5 < dev.fitness < 0.7
    elif name == "never_stops":
        assert dev.trials == 300 and dev.best_trial >= 0
    elif name == "exact_plane":
        assert dev.trials == 1 and len(dev.inliers) == 300
        assert np.abs(dev.plane_model * np.sign(dev.plane_model[0]) - SC.GRID_PLANE).max() < 1e-12
    else:
        assert dev.trials == 0 and dev.best_trial == -1 and not dev.plane_model.any() and len(dev.inliers) == 0


# ---- 4 ----
def as_tuple(r):
    return (bits(r.plane_model).tolist(), r.inliers.tolist(), r.mask.tolist(), bits([r.fitness, r.inlier_rmse]).tolist(),
            r.best_trial, r.trials, r.valid_trials)


def test_bits_do_not_depend_on_the_chunk_the_budget_or_the_run(options):
    for name in ("stops_early", "never_stops"):
        want = as_tuple(run(name))
        assert as_tuple(run(name)) == want  # the run
        for chunk, partial in ((64, DEFAULT_PARTIAL), (4096, DEFAULT_PARTIAL), (64, 65536), (DEFAULT_CHUNK, 65536)):
            options(chunk, partial)
            assert as_tuple(run(name)) == want, (name, chunk, partial)
        options()


def test_bits_do_not_depend_on_the_batch(options):
    sizes = [0, 1, 257, 16385]
    clouds = [SC.planted(n, 0.5, 60 + k) for k, n in enumerate(sizes)]
    seeds = [70 + k for k in range(len(sizes))]
    alone = [as_tuple(tp.segment_plane_batch([c], D, 3, 150, 0.999, s)[0]) for c, s in zip(clouds, seeds)]
    assert alone[0][4:] == (-1, 0, 0) and alone[1][4:] == (-1, 0, 0) and alone[2][4] >= 0 and alone[3][4] >= 0
    ref = PR.segment(clouds[3], D, 3, 150, 0.999, seeds[3])
    assert alone[3][0] == bits(ref["plane"]).tolist() and alone[3][1] == ref["inliers"].tolist()
    for chunk, partial in ((DEFAULT_CHUNK, DEFAULT_PARTIAL), (64, 65536)):  # the second: two point waves for the largest
        options(chunk, partial)
        together = [as_tuple(r) for r in tp.segment_plane_batch(clouds, D, 3, 150, 0.999, seeds)]
        assert together == alone
        back = [as_tuple(r) for r in tp.segment_plane_batch(clouds[::-1], D, 3, 150, 0.999, seeds[::-1])]
        assert back == alone[::-1]
    t_alone = [tp.plane_trials_batch([c], D, 5, 70, 4, s)[0] for c, s in zip(clouds, seeds)]
    t_batch = tp.plane_trials_batch(clouds, D, 5, 70, 4, seeds)
    for a, b in zip(t_alone, t_batch):
        same_trials(a, b)


# ---- 5 ----
def raw_call(clouds, params):
    """teaser_hip_plane_segment_batch with parameters the Python layer would refuse: (status, message, results)."""
    L = tp.lib()
    h = tp.plane._cache.get(-1)
    b = len(clouds)
    pp = (tp.plane._dp * b)(*[c.ctypes.data_as(tp.plane._dp) if c is not None else None for c in clouds])
    n = (C.c_int32 * b)(*[len(c) if c is not None else 5 for c in clouds])
    out = (tp.plane.PlaneResultC * b)()
    C.memset(out, 0x5a, C.sizeof(out))
    with h.lock:
        rc = L.teaser_hip_plane_segment_batch(h.h, b, pp, n, params, out, None, None)
        msg = L.teaser_hip_plane_last_error(h.h).decode()
    return rc, msg, bytes(out)


def test_defaults_and_refusals(options):
    p = tp.plane.PlaneParamsC()
    assert tp.lib().teaser_hip_plane_params_default(p) == 0
    assert (p.ransac_n, p.num_iterations, p.probability, p.seed) == (3, 100, 0.99999999, 0)
    assert tp.get_plane_option("chunk_trials") == DEFAULT_CHUNK and tp.get_plane_option("partial_bytes") == DEFAULT_PARTIAL
    for name, v in (("chunk_trials", 63), ("chunk_trials", 4097), ("partial_bytes", 65535), ("no_such", 64)):
        with pytest.raises(tp.TeaserHipError):
            tp.set_plane_option(name, v)
    P = SC.planted(50, 0.5, 90)
    nan, inf = float("nan"), float("inf")
    bad_cloud = P.copy()
    bad_cloud[7, 1] = nan
    edits = [("distance_threshold", 0.0), ("distance_threshold", inf), ("distance_threshold", nan), ("ransac_n", 2),
             ("ransac_n", 9), ("probability", 0.0), ("probability", 1.5), ("probability", nan), ("num_iterations", -1)]
    untouched = b"\x5a" * (2 * C.sizeof(tp.plane.PlaneResultC))
    for field, value in edits:
        params = (tp.plane.PlaneParamsC * 2)(tp.plane._params(D, 3, 10, 0.99, 1), tp.plane._params(D, 3, 10, 0.99, 2))
        setattr(params[1], field, value)
        rc, msg, out = raw_call([P, P], params)
        assert rc == 1 and field in msg and "(problem 1)" in msg and out == untouched, (field, value, msg)
    params = (tp.plane.PlaneParamsC * 2)(tp.plane._params(D, 3, 10, 0.99, 1), tp.plane._params(D, 3, 10, 0.99, 2))
    rc, msg, out = raw_call([P, bad_cloud], params)
    assert rc == 1 and "points has non-finite" in msg and "(problem 1)" in msg and out == untouched
    rc, msg, out = raw_call([P, None], params)
    assert rc == 1 and "points is NULL" in msg and "(problem 1)" in msg and out == untouched
    # the handle is usable afterwards, and the clock seed gives a valid result
    rc, msg, out = raw_call([P, P], params)
    assert rc == 0 and msg == "" and out != untouched
    plane, inliers = tp.segment_plane(P, D)
    assert abs(np.linalg.norm(plane[:3]) - 1) < 1e-12 and len(inliers) >= 3
