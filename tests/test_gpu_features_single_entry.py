"""GPU tests of the single-cloud entry points of the correspondence front-end, teaser_hip_compute_fpfh and
teaser_hip_match_features (csrc/solver.hip): thin callers of the batched implementation (csrc/features.hip) with a
batch of one, on a features handle the solver handle owns.  What is pinned here is what the forwarding could get
wrong, at the smallest shapes that reach it: the block and chunk boundaries of one cloud / one pair, the arena
growing and being reused, the statuses the wrappers decide themselves, and the registration state of the same
handle.  Every result is compared with the CPU oracle (oracle/features_oracle.c); the contract is bit identity, so
no tolerance appears except the project's pose parity bar (1e-4) of the interleaving test."""
import ctypes as C
import importlib

import numpy as np
import pytest

from oracle import features as F
from oracle import oracle

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")
_fp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
OK, BAD_ARG = 0, 1

# 1, 2, 3: too few neighbours for a normal (NaN, as PCL); 65: two query blocks of 64; 513: two radius chunks of 512
SIZES = (1, 2, 3, 65, 513)
RN, RF = 0.03, 0.05


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def clouds():
    """Per size: (uniform points in a 0.2 box, the oracle's features, the oracle's normals)."""
    rng = np.random.default_rng(17)
    out = {}
    for n in SIZES:
        pts = rng.uniform(0, 0.2, size=(n, 3)).astype(np.float32)
        out[n] = (pts,) + F.fpfh_features(pts, RN, RF)
    return out


@pytest.fixture(scope="module")
def feats():
    """257 x 40 rows: two 1-NN data chunks of 256 one way, one the other.  dim 33 and the generic-dim 7."""
    rng = np.random.default_rng(23)
    return {dim: (rng.standard_normal((257, dim)).astype(np.float32), rng.standard_normal((40, dim)).astype(np.float32))
            for dim in (33, 7)}


@pytest.mark.parametrize("n", SIZES)
def test_fpfh_of_small_clouds_equals_the_oracle(clouds, n):
    pts, fo, no = clouds[n]
    est = tp.FPFHEstimation()
    f = est.computeFPFHFeatures(pts, RN, RF)
    assert same(f, fo) and same(est.getNormals(), no)
    if n <= 3:
        assert np.isnan(est.getNormals()).all()


def test_fpfh_arena_grows_and_is_reused(clouds):
    est = tp.FPFHEstimation()
    first = {}
    for n in SIZES:  # every call needs more than the one before it
        f = est.computeFPFHFeatures(clouds[n][0], RN, RF)
        first[n] = (f, est.getNormals())
        assert same(f, clouds[n][1]) and same(first[n][1], clouds[n][2]), n
    for n in reversed(SIZES):  # every call fits what is there
        f = est.computeFPFHFeatures(clouds[n][0], RN, RF)
        assert f.tobytes() == first[n][0].tobytes() and est.getNormals().tobytes() == first[n][1].tobytes(), n
        assert same(f, clouds[n][1]) and same(est.getNormals(), clouds[n][2]), n


@pytest.mark.parametrize("dim,crosscheck", [(33, True), (33, False), (7, True)])
def test_matching_equals_the_oracle_both_ways_round(feats, dim, crosscheck):
    a, b = feats[dim]
    m = tp.Matcher()
    for src, dst in ((a, b), (b, a)):  # (b, a): n_dst > n_src, the swapped roles of matcher.cc:123-133
        got = m.calculateCorrespondences(None, None, src, dst, False, crosscheck, False, 0)
        assert got == [tuple(r) for r in F.match(src, dst, crosscheck=crosscheck).tolist()]
        assert len(got) > 0


def _match(L, h, a, b, pairs, cap, crosscheck=1):
    cnt = C.c_int64(cap)
    rc = L.teaser_hip_match_features(h, None if a is None else a.ctypes.data_as(_fp), 0 if a is None else len(a),
                                     None if b is None else b.ctypes.data_as(_fp), 0 if b is None else len(b), 33,
                                     crosscheck, None if pairs is None else pairs.ctypes.data_as(_ip), C.byref(cnt))
    return rc, cnt.value


def test_statuses_of_the_wrappers(clouds, feats):
    L = tp.lib()
    s = tp.RobustRegistrationSolver()
    h = s._h
    pts = clouds[65][0]
    out = np.zeros((65, 33), dtype=np.float32)
    # compute_fpfh: n = 0 is nothing to do; a radius that is not > 0 is refused
    assert L.teaser_hip_compute_fpfh(h, None, 0, RN, RF, None, None) == OK
    for rn, rf in ((0.0, RF), (-1.0, RF), (RN, 0.0), (RN, -1.0)):
        assert L.teaser_hip_compute_fpfh(h, pts.ctypes.data_as(_fp), 65, rn, rf, out.ctypes.data_as(_fp), None) == BAD_ARG
    assert L.teaser_hip_compute_fpfh(h, pts.ctypes.data_as(_fp), 65, RN, RF, out.ctypes.data_as(_fp), None) == OK
    assert same(out, clouds[65][1])
    # match_features: an empty side gives zero pairs, whatever the other pointers are
    a, b = feats[33]
    assert _match(L, h, None, b, None, 5) == (OK, 0)
    assert _match(L, h, a, None, None, 5) == (OK, 0)
    # a capacity one short: BAD_ARG, the count needed, nothing written; the next valid call is correct
    want = F.match(a, b, crosscheck=True)
    needed = len(want)
    assert needed > 1
    pairs = np.full((needed, 2), -7, dtype=np.int32)
    assert _match(L, h, a, b, pairs, needed - 1) == (BAD_ARG, needed)
    assert (pairs == -7).all()
    assert _match(L, h, a, b, pairs, needed) == (OK, needed)
    assert pairs.tolist() == want.tolist()
    # a feature row of NaN has no nearest neighbour
    bad = a.copy()
    bad[5] = np.nan
    rc, _ = _match(L, h, bad, b, pairs, needed)
    assert rc == BAD_ARG
    assert L.teaser_hip_last_error(h).decode().startswith("teaser_hip_match_features:")
    assert _match(L, h, a, b, pairs, needed) == (OK, needed) and pairs.tolist() == want.tolist()
    s.close()


def test_front_end_calls_leave_the_registration_state_alone(clouds, feats):
    """solve, front-end calls, solve on ONE solver handle: both solutions are the oracle's."""
    pr = tp.synth_problem(20250523, 2000, 0.9, 0.01)
    kw = dict(noise_bound=0.01, cbar2=1.0, estimate_scaling=False, rotation_gnc_factor=1.4,
              rotation_max_iterations=100, rotation_cost_threshold=0.005)
    ref = oracle.solve(pr["src"], pr["dst"], **dict(kw, estimate_scaling=0))
    assert ref["valid"]
    est = tp.FPFHEstimation()
    est._solver = s = tp.RobustRegistrationSolver(tp.RobustRegistrationSolver.Params(**kw))
    matcher = tp.Matcher()
    matcher._solver = s

    def solve_equals_the_oracle():
        sol = s.solve(pr["src"], pr["dst"])
        assert sol.valid
        assert s.getInlierMaxClique() == ref["max_clique"].tolist()
        assert s.getRotationInliers() == ref["rotation_inliers"].tolist()
        assert s.getTranslationInliers() == ref["translation_inliers"].tolist()
        assert np.linalg.norm(sol.rotation - ref["rotation"]) < 1e-4
        assert np.linalg.norm(sol.translation - ref["translation"]) < 1e-4

    solve_equals_the_oracle()
    pts, fo, no = clouds[513]
    assert same(est.computeFPFHFeatures(pts, RN, RF), fo) and same(est.getNormals(), no)
    a, b = feats[33]
    assert matcher.calculateCorrespondences(None, None, a, b, False, True, False, 0) == \
        [tuple(r) for r in F.match(a, b, crosscheck=True).tolist()]
    solve_equals_the_oracle()
    s.close()
