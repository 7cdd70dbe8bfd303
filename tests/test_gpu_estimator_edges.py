"""The rotation and translation estimators (csrc/kernels_estimate.hip) at every clique-size edge, against the oracle.

With use_max_clique = False the clique is 0 .. n - 1, so K = n exactly (tests/estimator_cases.py, whose table says what
each size of SIZES exercises: the register slots of the fast route at 256 / 257, its sort padding and the p1[K] line at
511 / 512, the general route from 513, the endpoint sort in global scratch from 1025, ...).

Tolerances.  tests/test_estimator_cases.py holds the oracle alone, on exactly the solves below, to an order sensitivity
of 1e-14 in R and 1e-15 max(1, |t|) in t (measured: 5e-15, 8e-16) and to an iteration count that does not move with the
threshold.  The bounds here are 1000 times that, rounded up, and far below the suite's 1e-4:
    || R - R_oracle ||_F   <= 1e-11
    max | t - t_oracle |   <= 1e-12 max(1, |t|_inf)   (+ |s - s_oracle| max ||src|| where the scale is estimated)
    gnc_iterations         equal
    gnc_cost               equal if infinite, else 1e-9 relative
    both inlier lists      equal
The only exemption is R at K = 2, which one TIM does not determine; test_k2 replaces it by invariants.

FGR solves a linear system per iteration, and the device's solver need not round like the oracle's: FGR_R_TOL below."""
import importlib

import numpy as np
import pytest

import estimator_cases as EC
from oracle import oracle

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")

R_TOL = 1e-11
T_TOL = 1e-12
COST_RTOL = 1e-9
SCALE_RTOL = 1e-9
# || R - R_oracle ||_F of the FGR cases.  Measured on the MI355X: K = 3: 3.7e-16, 255: 6.5e-16, 256: 1.1e-15, 257: 9.0e-16,
# 513: 1.1e-15 -- the general bound holds, nothing is widened (and it may never go above 1e-9, the bound of
# test_fgr_rotation_known_answer)
FGR_R_TOL = R_TOL

CASES = {cid: (ck, pk) for cid, ck, pk in EC.solve_cases()}
ROUTE_IDS = [cid for cid in CASES if cid.split("-")[0] in ("route", "bench", "offset", "scaled")]
OTHER_IDS = [cid for cid in CASES if cid.split("-")[0] in ("fgr", "quatro", "complete")]


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


_solvers = {}


def solver_for(p):
    key = tuple(sorted(p.items()))
    if key not in _solvers:
        _solvers[key] = tp.RobustRegistrationSolver(tp.RobustRegistrationSolver.Params(**p))
    return _solvers[key]


def record(s, sol, problem=0):
    raw = s.raw_solution(problem)
    return dict(valid=bool(sol.valid), scale=float(sol.scale), R=sol.rotation.copy(), t=sol.translation.copy(),
                cost=float(raw.gnc_cost), iters=int(raw.gnc_iterations), clique=s.getInlierMaxClique(problem),
                rot=s.getRotationInliers(problem), trans=s.getTranslationInliers(problem))


def device_solve(c, p):
    s = solver_for(p)
    return record(s, s.solve(c["src"], c["dst"]))


_oracle_solves = {}


def oracle_solve(cid):
    """(case, parameters, oracle solution) of a case of EC.solve_cases(), computed once"""
    if cid not in _oracle_solves:
        ck, pk = CASES[cid]
        c, p = EC.case(**ck), EC.params(**pk)
        _oracle_solves[cid] = (c, p, oracle.solve(c["src"], c["dst"], **EC.oracle_kw(p)))
    return _oracle_solves[cid]


def same_bits(a, b):
    return (a["valid"] == b["valid"] and a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes()
            and np.float64(a["cost"]).tobytes() == np.float64(b["cost"]).tobytes() and a["iters"] == b["iters"]
            and a["rot"] == b["rot"] and a["trans"] == b["trans"])


def check_against_oracle(tag, d, o, c, r_tol=R_TOL, compare_rotation=True):
    K = c["src"].shape[1]
    assert d["valid"] and o["valid"]
    assert d["clique"] == list(range(K))
    ds = abs(d["scale"] - o["scale"])
    dR = np.linalg.norm(d["R"] - o["rotation"])
    dt = np.abs(d["t"] - o["translation"]).max()
    t_tol = T_TOL * max(1.0, np.abs(o["translation"]).max()) + ds * np.linalg.norm(c["src"], axis=0).max()
    if r_tol > R_TOL:   # (a rotation held to a wider bound reaches t through R src: that term and nothing else)
        t_tol += r_tol * np.linalg.norm(c["src"], axis=0).max()
    print("%s: dR %.3g dt %.3g (bound %.3g) ds %.3g iterations %d / %d cost %.17g / %.17g"
          % (tag, dR, dt, t_tol, ds, d["iters"], o["gnc_iterations"], d["cost"], o["gnc_cost"]))
    assert ds <= SCALE_RTOL * max(1.0, abs(o["scale"]))
    if compare_rotation:
        assert dR <= r_tol
        assert dt <= t_tol
    assert d["iters"] == o["gnc_iterations"]
    if np.isinf(o["gnc_cost"]):
        assert d["cost"] == o["gnc_cost"]
    else:
        assert abs(d["cost"] - o["gnc_cost"]) <= COST_RTOL * abs(o["gnc_cost"])
    assert d["rot"] == o["rotation_inliers"].tolist()
    assert d["trans"] == o["translation_inliers"].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# a. the fast and the general route in a solve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ROUTE_IDS)
def test_solve_at_the_size_edges_vs_oracle(cid):
    """GNC-TLS on CHAIN TIMs: every K >= 3 of SIZES on `clean`, `outliers` and `dups` (from K = 8), K in {3, 257, 512,
    513} also at the benchmark's cost threshold 0.005, 1000 units from the origin (cancellation in the window sums)
    and with an estimated scale of 1.7 (inv_scale, the rotation bound nb 2 / scale, scale R in the raw translation)."""
    c, p, o = oracle_solve(cid)
    check_against_oracle(cid, device_solve(c, p), o, c)


# ---------------------------------------------------------------------------------------------------------------------
# b. K = 2
# ---------------------------------------------------------------------------------------------------------------------
def test_k2():
    """One distinct TIM does not determine R: the oracle and the device may legitimately differ (the only case exempt
    from the comparison of R and, through R, of t).  Instead: a proper rotation that turns the src TIM onto the dst TIM,
    a translation that leaves both points within beta, both inlier lists complete."""
    c, p = EC.case(2, "clean", EC.SEED), EC.params()
    d = device_solve(c, p)
    o = oracle.solve(c["src"], c["dst"], **EC.oracle_kw(p))
    check_against_oracle("k2", d, o, c, compare_rotation=False)
    R, t = d["R"], d["t"]
    assert d["valid"]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12
    a = R @ (c["src"][:, 1] - c["src"][:, 0])
    b = c["dst"][:, 1] - c["dst"][:, 0]
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    assert np.linalg.norm(np.cross(a, b)) <= 1e-12 and a @ b > 0
    assert np.abs(c["dst"] - R @ c["src"] - t[:, None]).max() <= EC.NB
    assert d["rot"] == [0, 1] and d["trans"] == [0, 1]


# ---------------------------------------------------------------------------------------------------------------------
# c. fused against separate, at the edges
# ---------------------------------------------------------------------------------------------------------------------
def both_settings(fn):
    """fn() under fused_estimators = 0 and 1 -> {0: ..., 1: ...}; the option is restored"""
    got = {}
    try:
        for mode in (0, 1):
            tp.set_option("fused_estimators", mode)
            got[mode] = fn()
    finally:
        tp.set_option("fused_estimators", 1)
    return got


@pytest.mark.parametrize("K", EC.SIZES)
def test_fused_matches_the_separate_kernels_at_the_size_edges(K):
    """The assertions of test_fused_estimators_match_the_separate_kernels (tests/test_gpu_parity.py) at the sizes it
    lacks: R, cost, iterations and rotation inliers bit-identical, t within 1e-13 relative, same translation inliers."""
    p = EC.params()
    for kind in ("outliers", "dups") if K >= 8 else ("clean",):
        c = EC.case(K, kind, EC.SEED)
        got = both_settings(lambda: device_solve(c, p))
        a, b = got[0], got[1]
        assert a["valid"] and b["valid"] and a["clique"] == b["clique"] == list(range(K))
        assert a["R"].tobytes() == b["R"].tobytes(), (K, kind, a["R"], b["R"])
        assert np.float64(a["cost"]).tobytes() == np.float64(b["cost"]).tobytes() and a["iters"] == b["iters"]
        assert a["rot"] == b["rot"]
        assert np.abs(a["t"] - b["t"]).max() <= 1e-13 * max(1.0, np.abs(a["t"]).max()), (K, kind, a["t"], b["t"])
        assert a["trans"] == b["trans"]


# ---------------------------------------------------------------------------------------------------------------------
# d. one batch of everything
# ---------------------------------------------------------------------------------------------------------------------
def test_one_batch_of_every_size():
    """Every size in one solve_batch, with one single-point problem in the middle (valid = 0: the K <= 1 branch of the
    kernel runs beside live workgroups): every problem equals its own single solve bit for bit."""
    p = EC.params()
    cs = [EC.case(K, EC.kind_at(K, "outliers"), EC.SEED) for K in EC.SIZES]
    mid = len(cs) // 2
    one = dict(src=np.array([[0.1], [0.2], [0.3]]), dst=np.array([[0.5], [0.1], [-0.3]]))
    batch = cs[:mid] + [one] + cs[mid:]
    s = solver_for(p)
    single = [record(s, s.solve(c["src"], c["dst"])) for c in batch]
    sols = s.solve_batch([c["src"] for c in batch], [c["dst"] for c in batch])
    got = [record(s, sol, b) for b, sol in enumerate(sols)]
    for b, c in enumerate(batch):
        if b == mid:
            for r in (single[b], got[b]):
                assert not r["valid"] and r["rot"] == [] and r["trans"] == []
        else:
            assert got[b]["valid"] and got[b]["clique"] == list(range(c["src"].shape[1]))
            assert same_bits(got[b], single[b]), (b, c["src"].shape[1], got[b], single[b])


# ---------------------------------------------------------------------------------------------------------------------
# e. the other estimators and COMPLETE TIMs: the general route inside the fused kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", OTHER_IDS)
def test_other_estimators_and_complete_tims_vs_oracle(cid):
    """FGR and QUATRO (yaw-only motion) at K in {3, 255, 256, 257, 513}; GNC-TLS on COMPLETE TIMs at K in {3, 23, 24, 65}
    (KT = 3, 253, 276, 2080: the pair-index inversion of TimSource::get on both sides of one block of TIMs).  `outliers`
    from K = 8, `clean` at K = 3."""
    c, p, o = oracle_solve(cid)
    check_against_oracle(cid, device_solve(c, p), o, c, r_tol=FGR_R_TOL if cid.startswith("fgr") else R_TOL)


# ---------------------------------------------------------------------------------------------------------------------
# f. stage entry points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", [0, EC.FGR, EC.QUATRO])
@pytest.mark.parametrize("k", EC.OTHER_SIZES)
def test_solve_for_rotation_at_the_size_edges_vs_oracle(k, alg):
    """gnc_tls_raw_kernel (raw TIM columns) and the FGR / QUATRO blocks on the chain TIMs of the `outliers` case."""
    c = EC.case(k, EC.kind_at(k, "outliers"), EC.SEED + 7, yaw_only=(alg == EC.QUATRO))
    src, dst = EC.chain_tims(c["src"]), EC.chain_tims(c["dst"])
    nb = 2 * EC.NB   # the bound of a TIM is twice the bound of a point (registration.cc:702-704)
    s = solver_for(EC.params(rotation_estimation_algorithm=alg))
    R = s.solveForRotation(src, dst, noise_bound=nb)
    fn = (oracle.gnc_tls_rotation, oracle.fgr_rotation, oracle.quatro_rotation)[alg]
    o = fn(src, dst, nb, 1.4, 100, 1e-12)
    last = s._last_rotation
    dR = np.linalg.norm(R - o["R"])
    print("solveForRotation k %d alg %d: dR %.3g iterations %d / %d cost %.17g / %.17g"
          % (k, alg, dR, last["iterations"], o["iterations"], last["cost"], o["cost"]))
    assert dR <= (FGR_R_TOL if alg == EC.FGR else R_TOL)
    assert (last["inliers"] == o["inliers"]).all()
    assert last["iterations"] == o["iterations"]
    if np.isinf(o["cost"]):
        assert last["cost"] == o["cost"]
    else:
        assert abs(last["cost"] - o["cost"]) <= COST_RTOL * abs(o["cost"])


@pytest.mark.parametrize("kind", ["outliers", "dups"])
@pytest.mark.parametrize("k", [2, 3, 255, 256, 257, 1024, 1025])
def test_solve_for_translation_at_the_size_edges_vs_oracle(k, kind):
    """tls_translation_kernel: three workgroups and the last-arriver AND; the endpoint sort in LDS up to k = 1024, in
    global scratch from 1025.  (`clean` below k = 8, where the two kinds do not exist.)"""
    c = EC.case(k, EC.kind_at(k, kind), EC.SEED + 8)
    v1, v2 = c["R"] @ c["src"], c["dst"]
    s = solver_for(EC.params())
    t = s.solveForTranslation(v1, v2)
    ot, om = oracle.tls_translation(v1, v2, EC.NB)
    print("solveForTranslation k %d %s: dt %.3g inliers %d" % (k, kind, np.abs(t - ot).max(), om.sum()))
    assert np.abs(t - ot).max() <= T_TOL * max(1.0, np.abs(ot).max())
    assert (s._last_translation["inliers"] == om).all()
    if k >= 8:
        assert 0 < om.sum() < k


# ---------------------------------------------------------------------------------------------------------------------
# g. singletons
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", EC.SINGLETON_STAGE_SIZES)
def test_singletons_through_solve_for_translation(k):
    """Residuals pairwise more than 2 beta apart on every axis: the reference returns the smallest (its first minimum
    among singletons that all cost exactly beta (k - 1)), and column 0 is the only inlier."""
    c = EC.case(k, "singletons", EC.SEED)
    s = solver_for(EC.params())
    t = s.solveForTranslation(c["src"], c["dst"])
    ot, om = oracle.tls_translation(c["src"], c["dst"], EC.NB)
    x = c["dst"] - c["src"]
    assert np.abs(t - ot).max() <= T_TOL * max(1.0, np.abs(ot).max())
    assert np.abs(t - x.min(axis=1)).max() <= T_TOL * max(1.0, np.abs(x).max())
    assert (s._last_translation["inliers"] == om).all() and np.flatnonzero(om).tolist() == [0]


@pytest.mark.parametrize("K", EC.SINGLETON_SOLVE_SIZES)
def test_singletons_through_a_solve(K):
    """The same through a solve (R = I, K = n), under both settings of fused_estimators.  The window form of the fast
    route gets a singleton's sums as prefix differences (a + b) - a, which are not b in general: it evaluates a window
    of one value exactly, or an arbitrary singleton wins by 1e-17 and t is off by a multiple of the spacing (seen on the
    MI355X before that rule, fused_estimators = 1: K = 3 and K = 5 failed, at K = 5 t = (4.138, 4.133, 4.045) against
    the smallest residuals (4.048, 4.043, 4.015) -- three, three and one steps of 0.03 off -- with no translation inlier).
    Every TIM of this case is an outlier, so R is whatever GNC-TLS leaves; the expectation is taken with the device's own
    R (the residuals are singletons under any rotation: tests/estimator_cases.py), the oracle's t is compared with its
    distance in R propagated."""
    c, p = EC.case(K, "singletons", EC.SEED), EC.params()
    o = oracle.solve(c["src"], c["dst"], **EC.oracle_kw(p))
    assert o["translation_inliers"].tolist() == [0]
    got = both_settings(lambda: device_solve(c, p))
    for mode in (0, 1):
        d = got[mode]
        assert d["valid"] and d["clique"] == list(range(K))
        x = c["dst"] - d["R"] @ c["src"]
        gaps = np.diff(np.sort(x, axis=1), axis=1).min()
        dR = np.linalg.norm(d["R"] - o["rotation"])
        print("singletons K %d fused %d: t %s smallest residual %s dR %.3g" % (K, mode, d["t"], x.min(axis=1), dR))
        assert gaps > 2 * EC.NB and (np.argmin(x, axis=1) == 0).all()
        assert np.abs(d["t"] - x.min(axis=1)).max() <= T_TOL * max(1.0, np.abs(x).max()), (mode, d["t"], x)
        assert np.abs(d["t"] - o["translation"]).max() <= (T_TOL * max(1.0, np.abs(o["translation"]).max())
                                                           + dR * np.linalg.norm(c["src"], axis=0).max())
        assert d["trans"] == o["translation_inliers"].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# exact endpoint ties where the reference is pinned all the same
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_endpoint_ties_that_are_pinned():
    """EC.TIE_DST (src = 0, beta = 1): the optimal window follows a closing and has a member whose opening ties with it.
    Either order of the two evaluates that window, so the oracle, the sweep and the window form agree; a closing search
    that drops the tied opening does not (tests/test_fused_translation_model.py)."""
    c = dict(src=np.zeros((3, 4)), dst=EC.TIE_DST)
    p = EC.params(noise_bound=EC.TIE_NB)
    o = oracle.solve(c["src"], c["dst"], **EC.oracle_kw(p))
    got = both_settings(lambda: device_solve(c, p))
    for mode in (0, 1):
        check_against_oracle("ties fused %d" % mode, got[mode], o, c)
