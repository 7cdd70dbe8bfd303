"""GPU tests above 65 536 correspondences: the routes a problem (or a batch: the switches follow the batch's max_n)
takes on either side of that size, against the CPU oracle.  Run on a real MI355X with `pytest -m gpu`.

At n <= 65 536 the inlier graph comes from the matrix-core K1 filter (degrees accumulated by K1 itself), the degree
closure may decide the problem, and the colouring bound uses the colour-centric rounds from 8 192 vertices.  Above,
K1 is the all-FP64 kernel followed by the standalone degree kernel, the closure is off and the colouring bound takes
the vertex-centric rounds only; KCORE_HEU and rotation_tim_graph = COMPLETE are refused ("Problem-size
limits").  The fixtures (tests/golden/make_config_golden.py: long_65536, long_65537, long_100k) permute their
columns so that correspondences 0, 65 535, 65 536 and n - 1 are planted inliers: the largest 16-bit index and the
first index above it sit inside the maximum clique.
"""
import functools
import hashlib
import importlib

import numpy as np
import pytest

from oracle import oracle
from util import HipBuffers, check_against_fixture, config_golden, long_n_problem

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")
UNSUPPORTED = 4
LONG = ("long_65536", "long_65537", "long_100k")


def bench_params(**kw):
    p = dict(noise_bound=0.01, cbar2=1.0, estimate_scaling=False, rotation_gnc_factor=1.4,
             rotation_max_iterations=100, rotation_cost_threshold=0.005)
    p.update(kw)
    return p


def make_solver(**kw):
    return tp.RobustRegistrationSolver(tp.RobustRegistrationSolver.Params(**kw))


@functools.lru_cache(maxsize=None)
def fixture(name):
    return config_golden()[name]


@functools.lru_cache(maxsize=None)
def problem(name):
    fx = fixture(name)
    assert fx["long_n_permuted"]
    return long_n_problem(tp, fx["seed"], fx["n"], fx["outlier_ratio"], fx["noise_bound"])


@functools.lru_cache(maxsize=None)
def oracle_bitmap(name):
    pr = problem(name)
    _, bm = oracle.inlier_bitmap(pr["src"], pr["dst"], fixture(name)["noise_bound"], 1.0, False)
    return bm


@pytest.fixture(autouse=True, scope="module")
def _release_cached_problems():
    """The live oracle bitmaps (0.5 - 1.25 GB each) and the problems live as long as this module's tests only."""
    yield
    oracle_bitmap.cache_clear()
    problem.cache_clear()


def small_problem(k, n):
    return tp.synth_problem(20250523 + 70000 + k, n, 0.9, 0.01)


def result(s, sol, b=0):
    """Everything a solve returns for problem b, as comparable values."""
    return dict(valid=bool(sol.valid), R=np.array(sol.rotation[:]).reshape(3, 3), t=np.array(sol.translation[:]),
                clique=s.getInlierMaxClique(b), rot=s.getRotationInliers(b), trans=s.getTranslationInliers(b),
                deg=s.getDegrees(b).copy(), edges=int(s.raw_solution(b).num_edges))


def assert_same(a, b, what):
    assert a["valid"] == b["valid"], what
    assert a["clique"] == b["clique"], what
    assert (a["deg"] == b["deg"]).all(), what
    assert a["edges"] == b["edges"], what
    assert (a["R"] == b["R"]).all() and (a["t"] == b["t"]).all(), what
    assert a["rot"] == b["rot"] and a["trans"] == b["trans"], what


def assert_bitmap_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, "%d rows differ, first ones:" % bad.size, bad[:16].tolist())


def assert_clique_in_bitmap(bm, clique):
    c = np.asarray(clique)
    sub = np.unpackbits(np.ascontiguousarray(bm[c]).view(np.uint8), axis=1, bitorder="little")[:, c].astype(bool)
    assert (sub | np.eye(len(c), dtype=bool)).all()


def pinned_indices(n):
    return [i for i in (0, 65535, 65536, n - 1) if i < n]


def solve_with_options(pr, options, capfd=None, params=None):
    """One solve with tp.set_option(name, value) for each item of `options` (each restored to the value it had
    before); returns (solver, solution, profile, stderr)."""
    before = {k: tp.get_option(k) for k in options}
    try:
        for k, v in options.items():
            tp.set_option(k, v)
        s = make_solver(**(params or bench_params()))
        s.set_profiling(True)
        if capfd is not None:
            capfd.readouterr()
        sol = s.solve(pr["src"], pr["dst"])
        err = capfd.readouterr().err if capfd is not None else ""
        return s, sol, s.get_profile(), err
    finally:
        for k, v in before.items():
            tp.set_option(k, v)


# ---------------------------------------------------------------------------------------------
# each fixture on its own
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LONG)
def test_long_n_fixture_solved_alone(name, capfd):
    """The oracle's result (committed fixture), the WHOLE bitmap bit for bit against a live oracle.inlier_bitmap, the
    degrees = the row popcounts, the clique a clique of that bitmap -- and the route: at 65 536 the matrix-core K1 (no
    standalone degree launch) and the colour-centric colouring rounds (k4_debug names them when they run); above, the
    all-FP64 K1 + the degree kernel and the vertex-centric rounds.  (99 % outliers: the outliers' degrees are far above
    the clique's size, so the degree closure and the peel decline and the colouring bound proves the clique on both
    sides of the boundary.)"""
    fx, pr = fixture(name), problem(name)
    n = fx["n"]
    s, sol, prof, err = solve_with_options(pr, dict(k4_debug=1), capfd)
    check_against_fixture(s, sol, fx)
    assert fx["clique_unique"]
    clique = s.getInlierMaxClique()
    assert set(pinned_indices(n)) <= set(clique)
    bm = s.getInlierGraphBitmap()
    assert_bitmap_equal(bm, oracle_bitmap(name), name)
    deg = s.getDegrees().astype(np.int64)
    assert (deg == np.bitwise_count(bm).sum(axis=1)).all()
    assert int(deg.sum()) == fx["degree_sum"] == 2 * fx["num_edges"]
    assert_clique_in_bitmap(bm, clique)
    assert s.raw_solution().colour_uncoloured >= 0, s.raw_solution().colour_uncoloured  # the colouring bound ran
    assert prof["tim_graph_launches"] == 1, prof
    if n <= 65536:
        assert prof["degree_ms"] == 0.0, prof  # degrees from the matrix-core K1
        assert "colour_mis verify" in err and " 0 same-colour adjacencies" in err, err[-600:]
    else:
        assert prof["degree_ms"] > 0.0, prof  # the all-FP64 K1, then launch_degrees
        assert "colour_mis" not in err, err[-600:]


# ---------------------------------------------------------------------------------------------
# both sides of the boundary on the same problem
# ---------------------------------------------------------------------------------------------
def test_long_65536_routes_agree(capfd):
    """long_65536 through the routes n > 65 536 takes, one switch at a time and then all together: the all-FP64 K1
    (k1_fp64 = 1), no degree closure (deg_closure = 0), the vertex-centric colouring rounds (colour_mis = 0).
    Bitmap, degrees, clique, inlier lists, R and t identical to the default route, bit for bit; the profile and the
    k4_debug diagnostics show which K1 and which colouring rounds ran."""
    pr = problem("long_65536")
    s0, sol0, prof0, err0 = solve_with_options(pr, dict(k4_debug=1), capfd)
    want, bm0 = result(s0, sol0), s0.getInlierGraphBitmap().copy()
    check_against_fixture(s0, sol0, fixture("long_65536"))
    assert prof0["degree_ms"] == 0.0 and "colour_mis verify" in err0
    del s0
    variants = [dict(k1_fp64=1), dict(deg_closure=0), dict(colour_mis=0),
                dict(k1_fp64=1, deg_closure=0, colour_mis=0)]
    for opts in variants:
        s, sol, prof, err = solve_with_options(pr, dict(opts, k4_debug=1), capfd)
        assert_same(result(s, sol), want, opts)
        assert_bitmap_equal(s.getInlierGraphBitmap(), bm0, opts)
        assert s.raw_solution().colour_uncoloured >= 0, (opts, s.raw_solution().colour_uncoloured)
        assert (prof["degree_ms"] > 0.0) == ("k1_fp64" in opts), (opts, prof)
        if "colour_mis" in opts:
            assert "colour_mis" not in err, (opts, err[-600:])
        else:
            assert "colour_mis verify" in err and " 0 same-colour adjacencies" in err, (opts, err[-600:])
        del s


def test_degree_closure_gate_at_the_boundary(capfd):
    """The degree closure on both sides of the boundary, on problems it can decide: 98 % outliers and a noise bound of
    0.002, so the planted clique (1 311 vertices, within the closure's 2 048-vertex candidate set) is larger than any
    outlier's degree (at most about 1 220; the inliers' are at least about 1 700).  At n = 65 536 the closure decides
    the problem (colour_uncoloured = -2 / -3), and the route without it (deg_closure = 0) returns the same bitmap,
    degrees, clique, inlier lists, R and t; at n = 65 537 it is off.  Both: the bitmap is the oracle's, the clique is
    the planted inlier set (at most one consistent outlier more) and a clique of that bitmap."""
    nb = 0.002
    params = bench_params(noise_bound=nb)
    for n in (65536, 65537):
        pr = long_n_problem(tp, 20250523 + 90000 + n, n, 0.98, nb)
        s, sol, _, err = solve_with_options(pr, dict(k4_debug=1), capfd, params)
        got = result(s, sol)
        bm = s.getInlierGraphBitmap()
        _, ref = oracle.inlier_bitmap(pr["src"], pr["dst"], nb, 1.0, False)
        assert_bitmap_equal(bm, ref, n)
        del ref
        assert (got["deg"] == np.bitwise_count(bm).sum(axis=1)).all()
        inl = np.flatnonzero(pr["inliers"]).tolist()
        assert got["valid"] and set(inl) <= set(got["clique"]) and len(got["clique"]) <= len(inl) + 1
        assert set(pinned_indices(n)) <= set(got["clique"])
        assert_clique_in_bitmap(bm, got["clique"])
        unc = s.raw_solution().colour_uncoloured
        del s
        if n == 65536:
            assert unc in (-2, -3), (unc, err[:800])  # the closure decided it
            s1, sol1, _, _ = solve_with_options(pr, dict(deg_closure=0), params=params)
            assert s1.raw_solution().colour_uncoloured not in (-2, -3)
            assert_same(result(s1, sol1), got, "deg_closure = 0")
            assert_bitmap_equal(s1.getInlierGraphBitmap(), bm, "deg_closure = 0")
            del s1
        else:
            assert unc not in (-2, -3), unc  # no closure above 65 536
        del bm


# ---------------------------------------------------------------------------------------------
# batches whose max_n crosses the boundary
# ---------------------------------------------------------------------------------------------
def _packed(probs):
    src = np.ascontiguousarray(np.concatenate([p["src"].T for p in probs], axis=0))
    dst = np.ascontiguousarray(np.concatenate([p["dst"].T for p in probs], axis=0))
    n = np.array([p["src"].shape[1] for p in probs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    return src, dst, off, n


def test_mixed_batch_crossing_the_boundary():
    """15 problems of 1 000 - 5 000 points and long_65537 in the middle: the large member moves the whole batch onto
    the FP64 K1 / no-closure / vertex-centric routes.  Every small member must equal its own single solve (which
    takes the matrix-core K1 and the closure), the large one its fixture -- through solve_batch and through
    submit_batch / wait alike."""
    sizes = [1000 + 4000 * k // 14 for k in range(15)]
    small = [small_problem(k, n) for k, n in enumerate(sizes)]
    big = problem("long_65537")
    probs = small[:7] + [big] + small[7:]
    one = make_solver(**bench_params())
    want = {}
    closed_alone = 0
    for b, pr in enumerate(probs):
        if b != 7:
            want[b] = result(one, one.solve(pr["src"], pr["dst"]))
            closed_alone += one.raw_solution().colour_uncoloured in (-2, -3)
    del one
    assert closed_alone >= 3, closed_alone  # alone, the degree closure decides several of the small problems ...
    s = make_solver(**bench_params())
    s.set_profiling(True)
    sols = s.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
    assert s.get_profile()["degree_ms"] > 0.0  # the batch took the all-FP64 K1
    got = [result(s, o, b) for b, o in enumerate(sols)]
    for b, w in want.items():
        assert_same(got[b], w, b)
        assert s.raw_solution(b).colour_uncoloured not in (-2, -3), b  # ... in this batch it is off
    check_against_fixture(s, sols[7], fixture("long_65537"), problem=7)
    bm = np.ascontiguousarray(s.getInlierGraphBitmap(7))
    assert hashlib.sha256(bm.tobytes()).hexdigest() == fixture("long_65537")["bitmap_sha256"]
    del bm
    mem = HipBuffers()
    try:
        a = make_solver(**bench_params())
        src, dst, off, n = _packed(probs)
        out = a.wait(a.submit_batch(mem.device(src), mem.device(dst), off, n, host=False))
        for b in range(len(probs)):
            assert_same(result(a, out[b], b), got[b], ("async", b))
        del a
    finally:
        mem.free()


def test_bitmap_pool_beyond_4_gib():
    """long_100k four times, then a 2 000-point problem.  Each large member holds 100 000 x 1 563 words = 1.25 GB of
    bitmap: the fourth one spans byte 2^32 of the pool (3.75 -> 5.00 GB) and the small problem's rows start 5.0 GB in,
    past 2^32 bytes -- every bitmap offset is int64_t, and a byte or word offset cut to 32 bits (signed or unsigned)
    would fold these rows onto the first members'.  The four large members match the oracle (bitmaps against the live
    oracle bitmap), the small one its single solve, bitmap included."""
    big = problem("long_100k")
    fx = fixture("long_100k")
    words = fx["n"] * ((fx["n"] + 63) // 64)
    assert 3 * words * 8 < 2 ** 32 < 4 * words * 8
    ref = oracle_bitmap("long_100k")
    sm = small_problem(99, 2000)
    one = make_solver(**bench_params())
    want = result(one, one.solve(sm["src"], sm["dst"]))
    want_bm = one.getInlierGraphBitmap().copy()
    del one
    _, sm_ref = oracle.inlier_bitmap(sm["src"], sm["dst"], 0.01, 1.0, False)
    assert (want_bm == sm_ref).all()
    probs = [big, big, big, big, sm]
    s = make_solver(**bench_params())
    sols = s.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
    for b in range(4):
        check_against_fixture(s, sols[b], fx, problem=b)
        assert_bitmap_equal(s.getInlierGraphBitmap(b), ref, b)
        assert (s.getDegrees(b) == s.getDegrees(0)).all(), b
    assert_same(result(s, sols[4], 4), want, "small member")
    assert_bitmap_equal(s.getInlierGraphBitmap(4), want_bm, "small member")


# ---------------------------------------------------------------------------------------------
# clique search on a supplied graph above 65 536 vertices
# ---------------------------------------------------------------------------------------------
def test_max_clique_on_a_70k_vertex_graph_whose_bounds_do_not_close():
    """maxClique(bm, n) at n = 70 000: G(n, 90 / n) with a planted 22-clique -- the palette (the heuristic clique's
    size) is a few colours short of what the graph needs, so survivors stay uncoloured and the exact search runs from
    them, at W = 1 094 words per row.  Against oracle.max_clique: same size, a valid clique, the same content when the
    maximum is unique."""
    n, avg_deg, k = 70000, 90, 22
    rng = np.random.default_rng(1000 + n)
    m = int(n * avg_deg / 2)
    e = rng.integers(0, n, size=(m, 2))
    e = e[e[:, 0] != e[:, 1]]
    members = np.sort(rng.choice(n, size=k, replace=False))
    ii, jj = np.triu_indices(k, 1)
    e = np.concatenate([e, np.stack([members[ii], members[jj]], 1)])
    bm = np.zeros((n, (n + 63) // 64), dtype=np.uint64)
    for a, b in ((e[:, 0], e[:, 1]), (e[:, 1], e[:, 0])):
        np.bitwise_or.at(bm, (a, b >> 6), np.uint64(1) << (b & 63).astype(np.uint64))
    o = oracle.max_clique(bm, n)
    s = make_solver()
    c, exact_run = s.maxClique(bm, n)
    assert exact_run  # the bounds did not close: the exact search ran at this size
    assert len(c) == len(o["clique"]) >= k
    assert c == sorted(c)
    assert_clique_in_bitmap(bm, c)
    if o["unique"]:
        assert c == o["clique"].tolist()
    if len(c) == k:
        assert c == members.tolist()


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def _check_handle_still_solves(s, params):
    """After a refusal the same handle solves (a single problem and a batch) exactly as a fresh handle does."""
    pr = small_problem(500, 1500)
    fresh = make_solver(**params)
    want = result(fresh, fresh.solve(pr["src"], pr["dst"]))
    assert want["valid"]
    assert_same(result(s, s.solve(pr["src"], pr["dst"])), want, "single solve after a refusal")
    sols = s.solve_batch([pr["src"], pr["src"]], [pr["dst"], pr["dst"]])
    for b in range(2):
        assert_same(result(s, sols[b], b), want, ("batch after a refusal", b))


def test_refusals_above_the_limits_leave_the_handle_usable():
    """KCORE_HEU above 65 536 (solve and the standalone maxClique), estimate_scaling above 46 341 and
    rotation_tim_graph = COMPLETE above sum n(n-1)/2 + 2 = 2^31: TEASER_HIP_ERR_UNSUPPORTED with its message; the
    same handle then solves small problems as a fresh one does."""
    big = tp.synth_problem(20250523 + 65537, 65537, 0.99, 0.01)
    kc = bench_params(inlier_selection_mode=tp.InlierSelectionMode.KCORE_HEU)
    s = make_solver(**kc)
    with pytest.raises(tp.TeaserHipError) as ei:
        s.solve(big["src"], big["dst"])
    assert ei.value.status == UNSUPPORTED and "KCORE_HEU" in str(ei.value) and "65536" in str(ei.value)
    _check_handle_still_solves(s, kc)
    with pytest.raises(tp.TeaserHipError) as ei:
        s.maxClique(np.zeros((65537, 1025), dtype=np.uint64), 65537)
    assert ei.value.status == UNSUPPORTED and "KCORE_HEU" in str(ei.value) and "65536" in str(ei.value)
    c, _ = s.maxClique(oracle.bitmap_from_edges(5, np.array([[0, 1], [0, 2], [1, 2], [3, 4]])), 5)
    assert c == [0, 1, 2]
    _check_handle_still_solves(s, kc)
    del s

    sc = bench_params(estimate_scaling=True)
    s = make_solver(**sc)
    pr = tp.synth_problem(20250523 + 46342, 46342, 0.99, 0.01)
    with pytest.raises(tp.TeaserHipError) as ei:
        s.solve(pr["src"], pr["dst"])
    assert ei.value.status == UNSUPPORTED and "estimate_scaling" in str(ei.value) and "46341" in str(ei.value)
    _check_handle_still_solves(s, sc)
    del s

    cp = bench_params(rotation_tim_graph=tp.InlierGraphFormulation.COMPLETE)
    s = make_solver(**cp)
    with pytest.raises(tp.TeaserHipError) as ei:
        s.solve(big["src"], big["dst"])
    assert ei.value.status == UNSUPPORTED and "COMPLETE" in str(ei.value)
    _check_handle_still_solves(s, cp)
