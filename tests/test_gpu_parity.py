"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the committed
golden vectors.  Run on a real MI355X with `pytest -m gpu`.

Parity bar (BASELINE.json north_star): bit-exact adjacency bitmap / clique / inlier index sets,
rotation within 1e-4 Frobenius, translation within 1e-4 m.
"""
import hashlib
import importlib

import numpy as np
import pytest

from oracle import oracle
from util import (R_TOL, T_TOL, angular_error, check_against_fixture, config_golden, golden, is_clique,
                  numpy_rows_predicate)

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")
G = golden()


def make_solver(**kw):
    return tp.RobustRegistrationSolver(tp.RobustRegistrationSolver.Params(**kw))


def bench_params(**kw):
    """SURVEY.md 8(d) synthetic-config parameters (example values teaser_cpp_ply.cc:79-87)."""
    p = dict(noise_bound=0.01, cbar2=1.0, estimate_scaling=False, rotation_gnc_factor=1.4,
             rotation_max_iterations=100, rotation_cost_threshold=0.005)
    p.update(kw)
    return p


def oracle_params(p):
    q = dict(p)
    q["estimate_scaling"] = int(q.get("estimate_scaling", True))
    return q


def check_solution_parity(solver, sol, o, problem=0, check_clique=True):
    assert sol.valid == o["valid"]
    clique = solver.getInlierMaxClique(problem)
    assert len(clique) == len(o["max_clique"])
    if check_clique and o["clique_unique"]:
        assert clique == o["max_clique"].tolist()
    if not o["valid"]:
        return
    if o["clique_unique"]:
        assert abs(sol.scale - o["scale"]) <= 1e-9 * max(1, abs(o["scale"]))
        assert np.linalg.norm(sol.rotation - o["rotation"]) <= R_TOL
        assert np.linalg.norm(sol.translation - o["translation"]) <= T_TOL
        assert solver.getRotationInliers(problem) == o["rotation_inliers"].tolist()
        assert solver.getTranslationInliers(problem) == o["translation_inliers"].tolist()


# ---------------------------------------------------------------------------------------------
# K1: adjacency bitmap, bit-exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rho,seed", [(64, 0.5, 1), (65, 0.3, 2), (200, 0.9, 3), (1000, 0.9, 4),
                                        (3000, 0.95, 5), (4097, 0.8, 6)])
def test_k1_bitmap_bit_exact_synthetic(n, rho, seed):
    pr = tp.synth_problem(20250523 + seed, n, rho, 0.01)
    s = make_solver(**bench_params())
    s.solve(pr["src"], pr["dst"])
    bm = s.getInlierGraphBitmap()
    _, ref = oracle.inlier_bitmap(pr["src"], pr["dst"], 0.01, 1.0, False)
    assert bm.shape == ref.shape
    assert (bm == ref).all()
    deg = s.getDegrees()
    assert (deg == oracle.bitmap_to_dense(ref, n).sum(1)).all()


def test_k1_bitmap_bit_exact_fixtures():
    for src, dst, nb in [(G["object_in"], G["scene_in"], float(G["object_noise_bound"])),
                         (G["model1000"].astype(np.float64).T, G["scene1000"].astype(np.float64).T, 0.0067364)]:
        s = make_solver(**bench_params(noise_bound=nb))
        s.solve(src, dst)
        _, ref = oracle.inlier_bitmap(src, dst, nb, 1.0, False)
        assert (s.getInlierGraphBitmap() == ref).all()


def test_k1_guard_band_exact_path():
    """Pairs sitting exactly on the pruning boundary force the in-band (IEEE sqrt) path:
    src on a line at distance a, dst at a + beta (+- a few ulps)."""
    rng = np.random.default_rng(11)
    nb = 0.01
    beta = 2 * nb
    n = 512
    a = rng.uniform(0.1, 3.0, size=n)
    src = np.zeros((3, n))
    dst = np.zeros((3, n))
    src[0] = np.cumsum(a)
    gaps = a + beta
    # perturb a quarter of the gaps by a few ulps either way
    k = rng.integers(-3, 4, size=n)
    gaps = np.where(rng.uniform(size=n) < 0.5, gaps, np.nextafter(gaps, gaps + k))
    dst[0] = np.cumsum(gaps)
    s = make_solver(**bench_params(noise_bound=nb))
    s.solve(src, dst)
    _, ref = oracle.inlier_bitmap(src, dst, nb, 1.0, False)
    assert (s.getInlierGraphBitmap() == ref).all()
    # duplicates / zero-length TIMs (A = 0 or B = 0)
    src2 = np.repeat(rng.uniform(size=(3, 40)), 4, axis=1)
    dst2 = src2 + rng.uniform(-0.03, 0.03, size=src2.shape)
    s.solve(src2, dst2)
    _, ref2 = oracle.inlier_bitmap(src2, dst2, nb, 1.0, False)
    assert (s.getInlierGraphBitmap() == ref2).all()


def k1_only_params(nb):
    """Only the bitmap is under test: heuristic clique mode + a short time limit keep the stages
    behind K1 bounded on these deliberately degenerate graphs."""
    return bench_params(noise_bound=nb, inlier_selection_mode=tp.InlierSelectionMode.PMC_HEU,
                        max_clique_time_limit=5.0)


def test_k1_filter_fallbacks():
    """The matrix-core K1 is a filter; these inputs exercise every way out of it, all of which must
    still give the oracle's bitmap bit for bit:
      * a fix-up worklist overflow (duplicated points: every pair is a short pair) -> the host
        reruns the batch on the all-FP64 K1;
      * beta far below the filter's resolution (kappa > 1/4) -> FP64 kernel body chosen on the device;
      * huge coordinate offsets (centring must absorb them) and non-finite coordinates."""
    rng = np.random.default_rng(14)
    nb = 0.01
    # overflow: 3000 points drawn from 6 distinct locations -> ~750k zero-length pairs + short pairs
    base = rng.uniform(size=(3, 6))
    idx = rng.integers(0, 6, size=3000)
    src = base[:, idx] + rng.uniform(-1e-4, 1e-4, size=(3, 3000))
    dst = src + rng.uniform(-2e-3, 2e-3, size=src.shape)
    s = make_solver(**k1_only_params(nb))
    s.solve(src, dst)
    _, ref = oracle.inlier_bitmap(src, dst, nb, 1.0, False)
    assert (s.getInlierGraphBitmap() == ref).all()
    # the worklist is shared by a batch: an overflowing problem must not leave its neighbour unresolved
    prn = tp.synth_problem(20250523 + 18, 2000, 0.9, nb)
    s.solve_batch([src, prn["src"]], [dst, prn["dst"]])
    assert (s.getInlierGraphBitmap(0) == ref).all()
    _, refn = oracle.inlier_bitmap(prn["src"], prn["dst"], nb, 1.0, False)
    assert (s.getInlierGraphBitmap(1) == refn).all()
    # beta tiny relative to the cloud: the f32 filter cannot resolve it
    pr = tp.synth_problem(20250523 + 15, 700, 0.5, 1e-7)
    s2 = make_solver(**k1_only_params(1e-7))
    s2.solve(pr["src"], pr["dst"])
    _, ref2 = oracle.inlier_bitmap(pr["src"], pr["dst"], 1e-7, 1.0, False)
    assert (s2.getInlierGraphBitmap() == ref2).all()
    # large offsets: src near (1e4, -2e4, 3e4), dst near (-5e3, 7e3, 1e3)
    pr = tp.synth_problem(20250523 + 16, 1500, 0.8, nb)
    src3 = pr["src"] + np.array([[1e4], [-2e4], [3e4]])
    dst3 = pr["dst"] + np.array([[-5e3], [7e3], [1e3]])
    s.solve(src3, dst3)
    _, ref3 = oracle.inlier_bitmap(src3, dst3, nb, 1.0, False)
    assert (s.getInlierGraphBitmap() == ref3).all()
    # a non-finite coordinate: NaN/inf comparisons are false in the reference -> no edges there
    src4, dst4 = pr["src"].copy(), pr["dst"].copy()
    src4[0, 3] = np.inf
    dst4[1, 7] = np.nan
    s.solve(src4, dst4)
    _, ref4 = oracle.inlier_bitmap(src4, dst4, nb, 1.0, False)
    assert (s.getInlierGraphBitmap() == ref4).all()


def test_k1_filter_adversarial_band():
    """Pairs engineered to sit at every distance from the decision boundary (ulps to 1e-3 beta), at
    several scales: whatever the filter cannot decide must be resolved by the FP64 fix-up."""
    rng = np.random.default_rng(17)
    for scale, nb in ((1.0, 0.01), (250.0, 0.05), (0.02, 1e-4)):
        beta = 2 * nb
        n = 2048
        src = rng.uniform(-1, 1, size=(3, n)) * scale
        # dst = src moved radially from a common origin so that many pair length differences land
        # within a few 1e-k beta of +-beta
        R0 = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        dst = R0 @ src
        off = rng.choice([0, 1, -1], size=n) * beta * (1 + rng.choice([0, 1e-15, 1e-12, 1e-9, 1e-7, 1e-5, 1e-3], size=n))
        d = dst / np.linalg.norm(dst, axis=0)
        dst = dst + d * off * rng.uniform(0.3, 1.0, size=n)
        s = make_solver(**k1_only_params(nb))
        s.solve(src, dst)
        _, ref = oracle.inlier_bitmap(src, dst, nb, 1.0, False)
        assert (s.getInlierGraphBitmap() == ref).all()


# ---------------------------------------------------------------------------------------------
# stage solvers: the reference's own known answers (through the HIP kernels)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [1, 2, 3])
def test_scalar_tls_known_answers(case):
    s = make_solver()
    est, mask = s.scalarTLS(G["tls%d_x" % case], G["tls%d_r" % case])
    assert abs(est - float(G["tls%d_est" % case])) < float(G["tls_tol"])
    assert (mask == G["tls%d_mask" % case].astype(bool)).all()
    oe, om = oracle.scalar_tls(G["tls%d_x" % case], G["tls%d_r" % case])
    assert abs(est - oe) < 1e-12 and (mask == om).all()


def test_scalar_tls_random_vs_oracle():
    rng = np.random.default_rng(12)
    s = make_solver()
    for n in (2, 3, 17, 100, 500, 1023, 1025, 5000):
        x = np.concatenate([rng.normal(0.7, 0.01, size=n // 2), rng.uniform(-5, 5, size=n - n // 2)])
        r = rng.uniform(0.01, 0.05, size=n)
        est, mask = s.scalarTLS(x, r)
        oe, om = oracle.scalar_tls(x, r)
        assert abs(est - oe) < 1e-10
        assert (mask == om).all()


def test_scalar_tls_large_vs_oracle():
    """n > 2^18 measurements: device radix sort + three-pass blocked sweep (kernels_scale.hip)
    against the oracle's sequential sweep.  The running sums associate differently (~1e-16
    relative), hence 1e-9 on the estimate; the consensus mask is identical."""
    rng = np.random.default_rng(13)
    s = make_solver()
    for n in ((1 << 18) + 1, 400000, 1000003):
        x = np.concatenate([rng.normal(1.3, 0.004, size=n // 10), rng.uniform(0.2, 4.0, size=n - n // 10)])
        r = rng.uniform(0.005, 0.05, size=n)
        est, mask = s.scalarTLS(x, r)
        oe, om = oracle.scalar_tls(x, r)
        assert abs(est - oe) < 1e-9
        assert (mask == om).all()
    # heavy ties: the stable sort must order tied endpoints like the oracle (insertion order)
    n = 300000
    x = np.round(rng.uniform(0, 2, size=n), 2)
    r = np.full(n, 0.25)
    est, mask = s.scalarTLS(x, r)
    oe, om = oracle.scalar_tls(x, r)
    assert abs(est - oe) < 1e-9 and (mask == om).all()


def test_scale_float_key_sort_matches_the_64_bit_sort():
    """The scale stage sorts FLOAT-rounded endpoint keys (4 radix passes over 8-byte items) and restores the exact
    FP64 order inside runs of equal float keys (tls_order_fix_kernel); runs too long to fix fall back to the 64-bit
    sort.  Both paths must produce the SAME order, hence bit-identical estimates (the sums then associate
    identically): random data, clusters of doubles that collide as floats (in-run reordering does the work), exact
    duplicates (ties keep insertion order), and whole solves, single and batched (the `scale_sort64` option flips the
    path inside this process)."""
    rng = np.random.default_rng(14)
    s = make_solver()

    def both(fn):
        tp.set_option("scale_sort64", 0)
        a = fn()
        tp.set_option("scale_sort64", 1)
        try:
            b = fn()
        finally:
            tp.set_option("scale_sort64", 0)
        return a, b

    n = 400000
    cases = []
    cases.append((np.concatenate([rng.normal(1.3, 0.004, size=n // 10), rng.uniform(0.2, 4.0, size=n - n // 10)]),
                  rng.uniform(0.005, 0.05, size=n)))
    # clusters of 24 values 1e-9 apart (one float at this magnitude spans 6e-8 .. 2.4e-7), shuffled; equal ranges
    # inside a cluster so that the endpoint keys collide as floats too
    base = np.repeat(rng.uniform(0.5, 3.0, size=n // 24 + 1), 24)[:n]
    x = base + 1e-9 * (rng.permutation(n) % 24)
    rr = np.repeat(rng.uniform(0.01, 0.05, size=n // 24 + 1), 24)[:n]
    cases.append((x, rr))
    # exact duplicates in runs of 8 (ties: insertion order) mixed with near-duplicates
    x2 = np.repeat(rng.uniform(0.5, 3.0, size=n // 8 + 1), 8)[:n]
    x2[::3] += 3e-10
    cases.append((x2, np.repeat(rng.uniform(0.01, 0.05, size=n // 8 + 1), 8)[:n]))
    for x, r in cases:
        (ea, ma), (eb, mb) = both(lambda: s.scalarTLS(x, r))
        assert np.float64(ea).tobytes() == np.float64(eb).tobytes()
        assert (ma == mb).all()
        oe, om = oracle.scalar_tls(x, r)
        assert abs(ea - oe) < 1e-9 and (ma == om).all()
    # whole solves: one large problem, one mid-size batch (the hull path off: it sums the state in front of the hull
    # in its own order, see test_scale_hull_matches_the_full_sort)
    p = bench_params(estimate_scaling=True, noise_bound=0.02)
    pr = tp.synth_problem(4242, 3000, 0.8, 0.01)
    sv = make_solver(**p)
    tp.set_option("scale_hull", 0)
    try:
        a, b = both(lambda: sv.solve(pr["src"], pr["dst"] * 1.5).scale)
        assert np.float64(a).tobytes() == np.float64(b).tobytes() and abs(a - 1.5) < 0.05
        probs = [tp.synth_problem(4300 + i, m, 0.7, 0.01) for i, m in enumerate([900, 1500, 800, 2000])]
        srcs, dsts = [q["src"] for q in probs], [q["dst"] * (1.0 + 0.2 * i) for i, q in enumerate(probs)]
        a, b = both(lambda: [o.scale for o in sv.solve_batch(srcs, dsts)])
        assert [np.float64(v).tobytes() for v in a] == [np.float64(v).tobytes() for v in b]
    finally:
        tp.set_option("scale_hull", 60)


@pytest.mark.parametrize("n,rho,k,nb,seed", [(4500, 0.8, 1.5, 0.02, 4242), (4200, 0.95, 1.3, 0.013, 4243),
                                             (6000, 0.6, 0.8, 0.008, 4244), (5000, 0.99, 1.0, 0.01, 4245)])
def test_scale_hull_matches_the_full_sort(n, rho, k, nb, seed):
    """Large problems sort only the HULL of the arg-min (kernels_scale.hip: value bins with exact prefix sums, a lower
    bound of the cost per bin against one achieved cost; the endpoints outside the hull enter as an exactly summed
    state).  Same arg-min as the sweep over everything: the estimate agrees to the last few ulps (the state in front
    of the hull is summed in another order), the consensus graph is the same graph -- with the host sizing the
    compacted arrays (one more sync) and with the fixed capacity of the option -- and the oracle agrees with both.
    Cases: an inlier peak (a hull of a per cent of the endpoints), almost no inliers (a flat top: a third of them)."""
    pr = tp.synth_problem(seed, n, rho, 0.01)
    src, dst = pr["src"], pr["dst"] * k
    p = bench_params(estimate_scaling=True, noise_bound=nb)
    got = {}
    try:
        for name, hull, sync in (("full", 0, 1), ("hull", 60, 1), ("hull_fixed", 60, 0), ("hull_tiny", 1, 1)):
            tp.set_option("scale_hull", hull)
            tp.set_option("scale_hull_sync", sync)
            s = make_solver(**p)
            sol = s.solve(src, dst)
            raw = s.raw_solution()
            # (the clique's SIZE: with almost no inliers there are many maximum cliques, and which one the parallel
            # search meets first is not pinned)
            got[name] = (sol.scale, int(raw.num_edges), len(s.getInlierMaxClique()),
                         hashlib.sha256(s.getInlierGraphBitmap().tobytes()).hexdigest())
    finally:
        tp.set_option("scale_hull", 60)
        tp.set_option("scale_hull_sync", 1)
    full = got["full"]
    for name in ("hull", "hull_fixed", "hull_tiny"):
        g = got[name]
        assert abs(g[0] - full[0]) <= 1e-13 * abs(full[0]), (name, g[0], full[0])
        assert g[1:] == full[1:], name
    if n <= 4500:  # (the oracle's sort of 2 x 1e7 endpoints: seconds)
        o = oracle.solve(src, dst, **oracle_params(p))
        assert abs(full[0] - o["scale"]) <= 1e-9




def test_estimate_scaling_degenerate_ties_fall_back_to_the_64_bit_sort():
    """A lattice cloud and its exact double: every TRIM has the same raw scale (2.0) and the ranges take a few dozen
    distinct values, so the endpoint keys form runs of tens of thousands of EQUAL float keys -- far beyond what the
    order-fix kernel repairs in place.  The stage must notice (scale_overflow), the solve must repeat itself with the
    64-bit sort, and the result must be the one the 64-bit path gives directly (and the oracle's)."""
    import os
    g = np.arange(12, dtype=np.float64)
    src = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=0).reshape(3, -1) * 0.1   # 1728 points
    dst = 2.0 * src
    p = bench_params(estimate_scaling=True, noise_bound=0.01)
    s = make_solver(**p)
    tp.set_option("scale_sort64", 0)
    a = s.solve(src, dst)
    tp.set_option("scale_sort64", 1)
    try:
        b = s.solve(src, dst)
    finally:
        tp.set_option("scale_sort64", 0)
    assert a.valid and b.valid
    assert np.float64(a.scale).tobytes() == np.float64(b.scale).tobytes()
    assert abs(a.scale - 2.0) < 1e-9
    o = oracle.solve(src, dst, **oracle_params(p))
    assert abs(a.scale - o["scale"]) <= 1e-9
    # the same inside a batch (mid-size path: composite keys), next to an ordinary problem
    pr = tp.synth_problem(4711, 1500, 0.7, 0.01)
    sols = s.solve_batch([src, pr["src"]], [dst, pr["dst"] * 1.25])
    assert np.float64(sols[0].scale).tobytes() == np.float64(a.scale).tobytes()
    assert abs(sols[1].scale - 1.25) < 0.05


SCALE_DIFF_LOG = []


@pytest.mark.parametrize("n,rho,scale,seed", [(725, 0.8, 1.7, 31), (1500, 0.9, 0.6, 32), (2500, 0.9, 2.25, 33),
                                              (1000, 0.7, 1.0, 34), (2000, 0.85, 3.5, 35), (3000, 0.9, 0.25, 36)])
def test_solve_estimate_scaling_large_vs_oracle(n, rho, scale, seed):
    """estimate_scaling = true (the Params default) beyond the single-workgroup range
    (registration.cc:410-425 with M = n(n-1)/2 up to 3.1e6 TRIMs here)."""
    pr = tp.synth_problem(20250523 + seed, n, rho, 0.01)
    dst = pr["dst"] * scale
    nb = 0.01 * scale  # the generator's noise (within 0.01) is scaled with the cloud
    p = bench_params(estimate_scaling=True, noise_bound=nb)
    s = make_solver(**p)
    sol = s.solve(pr["src"], dst)
    o = oracle.solve(pr["src"], dst, **oracle_params(p))
    assert sol.valid and o["valid"]
    assert abs(sol.scale - o["scale"]) <= 1e-9
    assert abs(sol.scale - scale) < 0.05 * scale
    _, ref = oracle.inlier_bitmap(pr["src"], dst, nb, 1.0, True)
    bm = s.getInlierGraphBitmap()
    # The consensus test |s_k - s_hat| <= alpha_k uses s_hat.  The sweep's prefix sums are associated
    # differently from the reference's sequential loop, so s_hat may differ in its last ulps.  Bar: a
    # bit-identical s_hat must give a bit-identical bitmap; otherwise every differing pair must sit ON the
    # boundary (| |s_k - s_hat| - alpha_k | within 1e-9 for both estimates), at most two of them.
    x = bm ^ ref
    diff = int(np.unpackbits(x.view(np.uint8)).sum())
    same_scale = np.float64(sol.scale).tobytes() == np.float64(o["scale"]).tobytes()
    SCALE_DIFF_LOG.append(dict(n=n, scale_bitwise_equal=bool(same_scale), scale_abs_diff=abs(sol.scale - o["scale"]),
                               bitmap_bits_differing=diff))
    if same_scale:
        assert diff == 0, diff
    else:
        assert diff <= 2, diff
        W = x.shape[1]
        beta = 2 * nb
        for i, w in zip(*np.nonzero(x)):
            for b in range(64):
                if (int(x[i, w]) >> b) & 1:
                    j = w * 64 + b
                    va = np.linalg.norm(pr["src"][:, j] - pr["src"][:, i])
                    vb = np.linalg.norm(dst[:, j] - dst[:, i])
                    for sh in (sol.scale, o["scale"]):
                        assert abs(abs(vb / va - sh) - beta / va) <= 1e-9
        assert W == (n + 63) // 64
    if diff == 0:
        check_solution_parity(s, sol, o)


def test_estimate_scaling_bitmap_differences_over_many_seeds():
    """the bitmap-difference log over >= 50 seeds.  Fifty more problems on the device-wide-sort
    path (725..1400 points, 50..90 % outliers, scales 0.3..3): scale within 1e-9 of the oracle's, and every bit of the
    consensus bitmap compared; a difference is only tolerated ON the boundary, as above."""
    rng = np.random.default_rng(20250923)
    for k in range(50):
        n = int(rng.integers(725, 1401))
        rho = float(rng.uniform(0.5, 0.9))
        scale = float(np.exp(rng.uniform(np.log(0.3), np.log(3.0))))
        pr = tp.synth_problem(777000 + k, n, rho, 0.01)
        dst = pr["dst"] * scale
        nb = 0.01 * scale
        p = bench_params(estimate_scaling=True, noise_bound=nb)
        s = make_solver(**p)
        sol = s.solve(pr["src"], dst)
        o = oracle.solve(pr["src"], dst, **oracle_params(p))
        assert sol.valid and o["valid"] and abs(sol.scale - o["scale"]) <= 1e-9, (k, n, sol.scale, o["scale"])
        _, ref = oracle.inlier_bitmap(pr["src"], dst, nb, 1.0, True)
        x = s.getInlierGraphBitmap() ^ ref
        diff = int(np.unpackbits(x.view(np.uint8)).sum())
        same_scale = np.float64(sol.scale).tobytes() == np.float64(o["scale"]).tobytes()
        SCALE_DIFF_LOG.append(dict(n=n, seed=777000 + k, outlier_ratio=round(rho, 3), scale_bitwise_equal=bool(same_scale),
                                   scale_abs_diff=abs(sol.scale - o["scale"]), bitmap_bits_differing=diff))
        assert diff == 0 if same_scale else diff <= 2, (k, n, diff)
        if diff:
            beta = 2 * nb
            for i, w in zip(*np.nonzero(x)):
                for b in range(64):
                    if (int(x[i, w]) >> b) & 1:
                        j = w * 64 + b
                        va = np.linalg.norm(pr["src"][:, j] - pr["src"][:, i])
                        vb = np.linalg.norm(dst[:, j] - dst[:, i])
                        for sh in (sol.scale, o["scale"]):
                            assert abs(abs(vb / va - sh) - beta / va) <= 1e-9


def test_estimate_scaling_bitmap_difference_log():
    """How often the large-n estimate_scaling bitmap differs from the oracle's: the cases
    above are summarised into gpurun_out/scale_bitmap_diff.json (copied to profiles/ by the round's scripts)."""
    import json
    import os

    from util import ROOT
    assert len(SCALE_DIFF_LOG) >= 3  # (runs after the cases above, same module, same process: 56 in a full run)
    out = os.path.join(ROOT, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    doc = dict(cases=SCALE_DIFF_LOG, cases_with_differing_bits=sum(1 for c in SCALE_DIFF_LOG if c["bitmap_bits_differing"]))
    json.dump(doc, open(os.path.join(out, "scale_bitmap_diff.json"), "w"), indent=1)
    assert doc["cases_with_differing_bits"] <= max(1, len(SCALE_DIFF_LOG) // 10)


def test_estimate_scaling_batch_small_problems():
    """estimate_scaling = true over a ragged batch: the problems of up to 724 points share two launches (all
    TRIMs, all scalar TLS problems), larger ones keep the radix-sort path; every problem is bit-identical to
    its own single solve, and two of them are checked against the oracle."""
    nb = 0.01
    sizes = [60, 300, 724, 2, 511, 900, 128, 725, 1]
    probs = []
    for i, n in enumerate(sizes):
        q = tp.synth_problem(500 + i, n, 0.5, nb)
        sc = 1.0 + 0.25 * i
        probs.append((q["src"], q["dst"] * sc))
    p = bench_params(estimate_scaling=True, noise_bound=nb * 3.25)  # (covers the largest scaled noise)
    s = make_solver(**p)
    sols = s.solve_batch([q[0] for q in probs], [q[1] for q in probs])
    batch = [(bool(o.valid), o.scale, o.rotation.copy(), o.translation.copy(), s.getInlierMaxClique(b))
             for b, o in enumerate(sols)]
    one = make_solver(**p)
    for b, q in enumerate(probs):
        o = one.solve(q[0], q[1])
        assert bool(o.valid) == batch[b][0]
        assert one.getInlierMaxClique() == batch[b][4], sizes[b]
        if o.valid:
            assert o.scale == batch[b][1], sizes[b]
            assert (o.rotation == batch[b][2]).all() and (o.translation == batch[b][3]).all()
    for b in (1, 4):
        ref = oracle.solve(probs[b][0], probs[b][1], **oracle_params(p))
        assert abs(batch[b][1] - ref["scale"]) <= 1e-9 * max(1.0, abs(ref["scale"]))
        assert batch[b][4] == ref["max_clique"].tolist() or not ref["clique_unique"]


def test_estimate_scaling_batch_mid_size_problems():
    """estimate_scaling = true, problems of 725 .. 4096 points: ONE value sort for the whole batch, a stable
    gathering pass by problem, one sweep over all segments (kernels_scale.hip).  Bit-identical to the problems
    solved one at a time (the sweep chunks are cut from each segment's own start); one against the oracle."""
    nb = 0.01
    sizes = [800, 1500, 2000, 900, 1000, 3000, 725]
    probs = []
    for i, n in enumerate(sizes):
        q = tp.synth_problem(700 + i, n, 0.6, nb)
        probs.append((q["src"], q["dst"] * (0.5 + 0.3 * i)))
    p = bench_params(estimate_scaling=True, noise_bound=nb * 2.5)
    s = make_solver(**p)
    sols = s.solve_batch([q[0] for q in probs], [q[1] for q in probs])
    batch = [(bool(o.valid), o.scale, o.rotation.copy(), o.translation.copy(), s.getInlierMaxClique(b))
             for b, o in enumerate(sols)]
    one = make_solver(**p)
    for b, q in enumerate(probs):
        o = one.solve(q[0], q[1])
        assert bool(o.valid) == batch[b][0]
        assert o.scale == batch[b][1], sizes[b]
        assert one.getInlierMaxClique() == batch[b][4], sizes[b]
        if o.valid:
            assert (o.rotation == batch[b][2]).all() and (o.translation == batch[b][3]).all()
    ref = oracle.solve(probs[0][0], probs[0][1], **oracle_params(p))
    assert abs(batch[0][1] - ref["scale"]) <= 1e-9 * max(1.0, abs(ref["scale"]))
    assert batch[0][4] == ref["max_clique"].tolist() or not ref["clique_unique"]


def test_solve_estimate_scaling_full_size_vs_oracle_fixture():
    """Full-size estimate_scaling = true (N = 10 000: M = 5e7 TRIMs, 1e8 endpoints through the
    radix sort) against the oracle's result committed in tests/golden/scale_golden.json (made by
    tests/golden/make_scale_golden.py; 43 s of CPU there).  At 95 % outliers the reference's TLS
    scale estimate does not recover the true scale -- parity is with the algorithm, not the truth."""
    import json
    import os

    from util import ROOT
    for g in json.load(open(os.path.join(ROOT, "tests", "golden", "scale_golden.json"))):
        pr = tp.synth_problem(g["seed"], g["n"], g["outlier_ratio"], 0.01)
        dst = pr["dst"] * g["dst_scale"]
        s = make_solver(**bench_params(estimate_scaling=True, noise_bound=g["noise_bound"]))
        sol = s.solve(pr["src"], dst)
        assert abs(sol.scale - g["oracle_scale"]) <= 1e-9
        assert abs(int(s.raw_solution().num_edges) - g["oracle_edges"]) <= 2
        if g["outlier_ratio"] <= 0.6:  # here the estimate is good: the pose is the planted one
            assert abs(sol.scale - g["dst_scale"]) < 5e-3
            assert angular_error(pr["R"], sol.rotation) < 0.02
            assert np.linalg.norm(sol.translation - g["dst_scale"] * pr["t"]) < 0.05


def test_solve_for_scale_stage_vs_oracle():
    """solveForScale(v1, v2) (registration.h:584) on caller-supplied TIMs, both scale solvers, against the
    oracle's restatement of registration.cc:410-443; scale-solver-test.cc:71-130's all-in / one-out masks."""
    src = G["object_in"].astype(np.float64)  # 3 x 168, scale-solver-test.cc uses objectIn.csv
    rng = np.random.default_rng(7)
    tims, _ = oracle.compute_tims(src)
    tims = np.asarray(tims if tims.shape[0] == 3 else tims.T)
    # fixed scale (ScaleInliersSelector): identical TIMs -> all in; one TIM stretched -> exactly that one out
    s = make_solver(noise_bound=0.01, estimate_scaling=False)
    assert s.solveForScale(tims, tims) == 1.0 and s.scale_inliers_mask_of_last_stage.all()
    t2 = tims.copy()
    t2[:, 5] *= 3.0
    assert s.solveForScale(tims, t2) == 1.0
    want = np.ones(tims.shape[1], dtype=bool)
    want[5] = np.abs(np.linalg.norm(tims[:, 5]) - np.linalg.norm(t2[:, 5])) <= 0.02
    assert (s.scale_inliers_mask_of_last_stage == want).all() and not want[5]
    # TLS scale: random scale with noise, vs the oracle (scale to 1e-9, identical masks)
    for scale in (1.0, 0.73, 2.5):
        noisy = scale * tims + rng.uniform(-0.004, 0.004, size=tims.shape)
        s = make_solver(noise_bound=0.01, estimate_scaling=True)
        got = s.solveForScale(tims, noisy)
        ref_scale, ref_mask = oracle.scale_inliers_mask(tims, noisy, 0.01, 1.0, True)
        assert abs(got - ref_scale) <= 1e-9 * max(1.0, ref_scale) and abs(got - scale) < 0.05 * scale
        assert (s.scale_inliers_mask_of_last_stage == ref_mask).all()


def _large_route_tims(case):
    """2^18 + 1 TIM pairs, the smallest count the single-workgroup sort does not take."""
    m = (1 << 18) + 1
    rng = np.random.default_rng(31)
    if case == "random":
        v1 = rng.uniform(-1, 1, size=(3, m))
        v2 = 1.7 * v1 + rng.uniform(-0.004, 0.004, size=(3, m))
        out = rng.permutation(m)[:m // 2]
        v2[:, out] = rng.uniform(-3, 3, size=(3, out.size))
        return v1, v2, None
    # heavy ties: 64 distinct lengths, eight distinct ratios, 1.5 for two thirds of the pairs -- the endpoint keys fall
    # into runs of thousands of equal keys, far beyond what the order-fix kernel repairs in place (kFxHalo = 64): the
    # float-key attempt must hand over to the 64-bit sort
    v1 = np.zeros((3, m))
    v2 = np.zeros((3, m))
    v1[0] = rng.integers(32, 96, size=m) / 64.0
    k = np.where(rng.uniform(size=m) < 0.6, 1.5, rng.integers(1, 8, size=m) / 2.0)
    v2[0] = v1[0] * k
    return v1, v2, 1.5


@pytest.mark.parametrize("case", ["random", "ties"])
def test_solve_for_scale_large_route_vs_oracle(case):
    """solveForScale with estimate_scaling on more TIMs than one workgroup sorts (radix sort + blocked sweep, float keys
    first): the oracle's scale to 1e-9 and its mask, and the same bytes whichever sort the `scale_sort64` option picks."""
    v1, v2, exact = _large_route_tims(case)
    ref_scale, ref_mask = oracle.scale_inliers_mask(v1, v2, 0.01, 1.0, True)
    print(case, "oracle scale %.17g, %d of %d in the mask" % (ref_scale, int(np.sum(ref_mask)), v1.shape[1]))
    if exact is not None:
        assert ref_scale == exact
    s = make_solver(noise_bound=0.01, estimate_scaling=True)
    got = {}
    try:
        for sort64 in (0, 1):
            tp.set_option("scale_sort64", sort64)
            scale = s.solveForScale(v1, v2)
            got[sort64] = (np.float64(scale).tobytes(), s.scale_inliers_mask_of_last_stage.copy())
            print(case, "scale_sort64 =", sort64, "scale %.17g" % scale)
            assert abs(scale - ref_scale) <= 1e-9 * max(1.0, scale)
            assert (got[sort64][1] == np.asarray(ref_mask).ravel()).all()
    finally:
        tp.set_option("scale_sort64", 0)
    assert got[0][0] == got[1][0] and (got[0][1] == got[1][1]).all()


def test_stage_calls_between_two_solves_on_one_handle():
    """One handle, in order: a solve, maxClique, the getters (refused: the stage call holds no batch), scalarTLS,
    solveForTranslation, the same solve again.  The stage calls replace the solve's views into the header block
    (descriptors, states, peel counters) by buffers of their own and the next solve takes them back: both solves must
    equal a fresh handle's bit for bit."""
    pr = tp.synth_problem(20250523 + 1, 64, 0.5, 0.01)

    def solve(s):
        sol = s.solve(pr["src"], pr["dst"])
        return (sol.valid, np.float64(sol.scale).tobytes(), sol.rotation.tobytes(), sol.translation.tobytes(),
                s.getInlierMaxClique(), s.getRotationInliers(), s.getTranslationInliers(),
                s.getInlierGraphBitmap().tobytes(), s.getDegrees().tobytes())

    fresh = solve(make_solver(**bench_params()))
    s = make_solver(**bench_params())
    first = solve(s)
    c, _ = s.maxClique(oracle.bitmap_from_edges(5, G["graph_k5_edges"]), 5)
    assert c == [0, 1, 2, 3, 4]
    for getter in (s.getInlierMaxClique, s.getRotationInliers, s.getTranslationInliers, s.getInlierGraphBitmap, s.getDegrees):
        with pytest.raises(tp.TeaserHipError):
            getter(0)
    rng = np.random.default_rng(12)
    x = np.concatenate([rng.normal(0.7, 0.01, size=8), rng.uniform(-5, 5, size=9)])
    r = rng.uniform(0.01, 0.05, size=17)
    est, mask = s.scalarTLS(x, r)
    oe, om = oracle.scalar_tls(x, r)
    assert abs(est - oe) < 1e-10 and (mask == om).all()
    t = s.solveForTranslation(G["trans_v1"], G["trans_v2"])
    ot, om = oracle.tls_translation(G["trans_v1"], G["trans_v2"], 0.01)
    assert np.linalg.norm(t - ot) < 1e-12 and (s._last_translation["inliers"] == om).all()
    again = solve(s)
    assert first == fresh and again == fresh


def test_translation_known_answer():
    s = make_solver(noise_bound=float(G["trans_noise_bound"]))
    t = s.solveForTranslation(G["trans_v1"], G["trans_v2"])
    assert np.linalg.norm(t - G["trans_expected_t"]) < float(G["trans_tol"])
    ot, om = oracle.tls_translation(G["trans_v1"], G["trans_v2"], float(G["trans_noise_bound"]))
    assert np.linalg.norm(t - ot) < 1e-12
    assert (s._last_translation["inliers"] == om).all()


def test_rotation_known_answer():
    src = G["rot_src"].T
    R_exp = G["rot_expected_R"]
    dst = R_exp @ src
    mi, thr, fac, nb = G["rot_params"]
    s = make_solver(rotation_max_iterations=int(mi), rotation_cost_threshold=float(thr),
                    rotation_gnc_factor=float(fac))
    R = s.solveForRotation(src, dst, noise_bound=float(nb))
    assert angular_error(R_exp, R) < float(G["rot_tol"])
    assert np.linalg.norm(R - R_exp) < 1e-9


def test_rotation_with_outliers_vs_oracle():
    rng = np.random.default_rng(13)
    for trial in range(5):
        k = 300
        src = rng.normal(size=(3, k))
        R0 = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        if np.linalg.det(R0) < 0:
            R0[:, 0] *= -1
        dst = R0 @ src + 0.005 * rng.normal(size=(3, k))
        bad = rng.choice(k, size=60, replace=False)
        dst[:, bad] = rng.normal(size=(3, 60))
        s = make_solver(rotation_cost_threshold=1e-12)
        R = s.solveForRotation(src, dst, noise_bound=0.02)
        o = oracle.gnc_tls_rotation(src, dst, 0.02, 1.4, 100, 1e-12)
        assert np.linalg.norm(R - o["R"]) < 1e-8
        assert (s._last_rotation["inliers"] == o["inliers"]).all()
        assert s._last_rotation["iterations"] == o["iterations"]
        assert abs(s._last_rotation["cost"] - o["cost"]) <= 1e-9 * max(1.0, abs(o["cost"]))


# ---------------------------------------------------------------------------------------------
# clique stage
# ---------------------------------------------------------------------------------------------
def test_toy_graph_cliques():
    s = make_solver()
    c, _ = s.maxClique(oracle.bitmap_from_edges(5, G["graph_k5_edges"]), 5)
    assert c == [0, 1, 2, 3, 4]
    c, _ = s.maxClique(oracle.bitmap_from_edges(4, G["graph_4node_edges"]), 4)
    assert c == [0, 2, 3]
    c, _ = s.maxClique(oracle.bitmap_from_edges(4, []), 4)
    assert len(c) == 1


def test_random_graph_cliques_vs_oracle():
    rng = np.random.default_rng(14)
    s = make_solver()
    n_exact = 0
    for trial in range(30):
        n = int(rng.integers(5, 300))
        p = float(rng.uniform(0.05, 0.8))
        if n > 150:
            p = min(p, 0.5)
        A = np.triu(rng.uniform(size=(n, n)) < p, 1)
        bm = oracle.bitmap_from_edges(n, np.argwhere(A))
        c, er = s.maxClique(bm, n)
        o = oracle.max_clique(bm, n)
        n_exact += int(er)
        assert len(c) == len(o["clique"])
        assert is_clique(A | A.T, c)
        assert c == sorted(c)
        if o["unique"]:
            assert c == o["clique"].tolist()
    assert n_exact > 0  # the device B&B was actually exercised


def test_mid_size_graph_cliques_vs_oracle():
    """Compact graphs of 9 .. 16 bit-set words (513 .. 1024 vertices: adjacency staged in LDS, colouring with one word
    per lane and the four-step DPP maximum) and just beyond (17 words: the generic colouring): sparse enough for the
    oracle's search to finish in seconds, dense enough that the device search runs."""
    rng = np.random.default_rng(16)
    s = make_solver()
    n_exact = 0
    # (768 and 769: the last size the all-starts greedy serves, kSmallCap, and the first it does not)
    for n, p in ((600, 0.12), (760, 0.10), (900, 0.08), (1020, 0.08), (1080, 0.07), (768, 0.10), (769, 0.10)):
        A = np.triu(rng.uniform(size=(n, n)) < p, 1)
        members = np.sort(rng.choice(n, size=9, replace=False))  # a planted 9-clique above the random graph's 5 - 6
        A[np.ix_(members, members)] |= np.triu(np.ones((9, 9), dtype=bool), 1)
        bm = oracle.bitmap_from_edges(n, np.argwhere(A))
        c, er = s.maxClique(bm, n)
        o = oracle.max_clique(bm, n)
        n_exact += int(er)
        assert len(c) == len(o["clique"]) >= 9, (n, len(c), len(o["clique"]))
        assert is_clique(A | A.T, c) and c == sorted(c)
        if o["unique"]:
            assert c == o["clique"].tolist()
    assert n_exact > 0


def test_planted_clique_needs_exact():
    """A planted clique hidden among higher-degree decoys: greedy start vertices miss it, the
    exact stage must find it."""
    rng = np.random.default_rng(15)
    n, k = 400, 30
    A = np.triu(rng.uniform(size=(n, n)) < 0.35, 1)
    members = np.sort(rng.choice(n, size=k, replace=False))
    for i in members:
        for j in members:
            if i < j:
                A[i, j] = True
    bm = oracle.bitmap_from_edges(n, np.argwhere(A))
    s = make_solver()
    c, er = s.maxClique(bm, n)
    o = oracle.max_clique(bm, n)
    assert len(c) == len(o["clique"]) >= k
    assert is_clique(A | A.T, c)
    if o["unique"]:
        assert c == o["clique"].tolist()


def test_max_clique_time_limit_returns_the_incumbent():
    """graph.cc:44: pmc's time limit ends the search and the incumbent is returned.  A dense random graph whose exact
    search takes far longer than the limit: status TIME_LIMIT, and what comes back is a valid clique at least as
    large as the heuristic's.  The limit covers the whole exact stage of the call (every launch gets what is left of
    it), so the call returns promptly."""
    import time
    rng = np.random.default_rng(23)
    n = 900
    A = np.triu(rng.uniform(size=(n, n)) < 0.6, 1)
    bm = oracle.bitmap_from_edges(n, np.argwhere(A))
    heu = make_solver(inlier_selection_mode=tp.InlierSelectionMode.PMC_HEU)
    ch, _ = heu.maxClique(bm, n)
    s = make_solver(max_clique_time_limit=2e-4)
    t0 = time.perf_counter()
    c, er = s.maxClique(bm, n)
    dt = time.perf_counter() - t0
    assert s.last_status == 5, tp.STATUS_NAMES.get(s.last_status)
    assert er and len(c) >= len(ch) and is_clique(A | A.T, c)
    assert dt < 5.0


def test_colouring_bound_and_restricted_roots_vs_oracle():
    """Graphs built so the greedy bound is NOT the maximum (several planted cliques of mixed size
    among dense noise): the global colouring bound must leave the larger cliques' vertices
    uncoloured and the B&B restricted to those roots must still return a maximum clique."""
    rng = np.random.default_rng(77)
    s = make_solver()
    n_exact = 0
    for trial in range(24):
        n = int(rng.integers(120, 700))
        p = float(rng.uniform(0.1, 0.45))
        A = np.triu(rng.uniform(size=(n, n)) < p, 1)
        for _ in range(int(rng.integers(1, 5))):
            k = int(rng.integers(8, 40))
            members = rng.choice(n, size=k, replace=False)
            for i in members:
                for j in members:
                    if i < j:
                        A[i, j] = True
        bm = oracle.bitmap_from_edges(n, np.argwhere(A))
        c, er = s.maxClique(bm, n)
        o = oracle.max_clique(bm, n)
        n_exact += int(er)
        assert len(c) == len(o["clique"]), (trial, n, p, len(c), len(o["clique"]))
        assert is_clique(A | A.T, c)
        if o["unique"]:
            assert c == o["clique"].tolist()
    assert n_exact > 0


@pytest.mark.parametrize("n,rho,seed", [(20000, 0.985, 41), (30000, 0.99, 42), (50000, 0.99, 43)])
def test_colouring_rounds_in_one_launch_match_the_launch_per_round_route(n, rho, seed):
    """colour_persistent_kernel (option colour_persistent = n0 > 0: problems of at least n0 vertices; off by default --
    measured slower) runs every colouring round inside one launch, rounds separated by a grid barrier, the
    colour table in LDS.  Same hashes, same rule: the uncoloured set, the clique and the estimate must be those of the
    launch-per-round kernels, bit for bit.  (Outlier degrees far above the clique size: the peel closes nothing and the
    colouring bound is what proves the greedy clique.)"""
    pr = tp.synth_problem(20250523 + seed, n, rho, 0.01)
    got = {}
    try:
        for mode in (0, 8192):
            tp.set_option("colour_persistent", mode)
            s = make_solver(**bench_params())
            sol = s.solve(pr["src"], pr["dst"])
            raw = s.raw_solution()
            got[mode] = (bool(sol.valid), sol.rotation.copy(), sol.translation.copy(), s.getInlierMaxClique(),
                         int(raw.colour_uncoloured), int(raw.clique_exact_run), int(raw.heuristic_size))
    finally:
        tp.set_option("colour_persistent", 0)
    a, b = got[0], got[8192]
    assert a[0] and b[0] and a[4] >= 0, a[4:]  # the colouring stage ran
    assert a[3] == b[3] and a[4:] == b[4:] and (a[1] == b[1]).all() and (a[2] == b[2]).all()
    assert set(np.flatnonzero(pr["inliers"]).tolist()) <= set(a[3])


@pytest.mark.parametrize("n,rho,seed", [(20000, 0.985, 41), (30000, 0.99, 42), (50000, 0.99, 43), (60000, 0.98, 44)])
def test_colour_centric_bound_matches_the_vertex_centric_route(n, rho, seed, capfd):
    """Option colour_mis = n0 (default 8192): problems of at least n0 vertices prove the greedy clique with the
    colour-centric rounds (a bit set per colour = the union of its members' rows; bidders accepted in priority order as
    the lexicographically first maximal independent set: kernels_clique.hip, mis_*).  Another proper colouring with the
    same palette: the verdict, the clique and the estimate must be those of the vertex-centric rounds; the diagnostics
    pass of k4_debug checks every coloured vertex against its whole row (no two adjacent vertices share a colour).
    (The last case has 1 200 inliers: more than the 1 024 colours the route keeps bit sets for -- the other vertices use
    the first 1 024 only.)"""
    pr = tp.synth_problem(20250523 + seed, n, rho, 0.01)
    got = {}
    try:
        for mode in (0, 4096):
            tp.set_option("colour_mis", mode)
            tp.set_option("k4_debug", 1 if mode else 0)
            s = make_solver(**bench_params())
            capfd.readouterr()
            sol = s.solve(pr["src"], pr["dst"])
            err = capfd.readouterr().err
            raw = s.raw_solution()
            got[mode] = (bool(sol.valid), sol.rotation.copy(), sol.translation.copy(), s.getInlierMaxClique(),
                         int(raw.colour_uncoloured), int(raw.clique_exact_run), int(raw.heuristic_size), err)
    finally:
        tp.set_option("colour_mis", 8192)
        tp.set_option("k4_debug", 0)
    a, b = got[0], got[4096]
    assert a[0] and b[0] and a[4] >= 0 and b[4] >= 0, (a[4:7], b[4:7])  # the colouring stage ran on both routes
    assert a[3] == b[3] and a[5:7] == b[5:7] and (a[1] == b[1]).all() and (a[2] == b[2]).all()
    assert "colour_mis verify" in b[7] and " 0 same-colour adjacencies" in b[7], b[7][-600:]
    assert b[4] <= max(64, 4 * a[4]), (a[4], b[4])  # (as good a colouring: a handful of survivors without a colour)
    assert set(np.flatnonzero(pr["inliers"]).tolist()) <= set(a[3])


def _sparse_graph_with_planted_clique(rng, n, avg_deg, k):
    """G(n, avg_deg / n) as an edge list + a planted k-clique (members spread over the index range)."""
    m = int(n * avg_deg / 2)
    e = rng.integers(0, n, size=(m, 2))
    e = e[e[:, 0] != e[:, 1]]
    members = np.sort(rng.choice(n, size=k, replace=False))
    ii, jj = np.triu_indices(k, 1)
    e = np.concatenate([e, np.stack([members[ii], members[jj]], 1)])
    return e, members


@pytest.mark.parametrize("n,avg_deg,k", [(9000, 40, 24), (12000, 90, 22), (20000, 60, 12)])
def test_colour_centric_bound_on_supplied_graphs(n, avg_deg, k, capfd):
    """The colour-centric bound through findMaxClique on graphs whose colouring is NOT a formality: (a) palette ample, the
    bound closes; (b) palette short by a few colours, the survivors without a colour are the roots of the exact search;
    (c) palette far too small, most survivors are roots.  Both routes must return a maximum clique of the same size
    (a valid clique containing the planted one when that is the unique maximum).  These graphs have far more vertices
    than 128 x clique size, where the product keeps the vertex-centric rounds (a round then admits a fraction of the
    vertices only): colour_mis_any = 1 sends them through the colour-centric ones all the same, and the diagnostics
    pass must have seen a proper colouring."""
    rng = np.random.default_rng(1000 + n)
    e, members = _sparse_graph_with_planted_clique(rng, n, avg_deg, k)
    bm = np.zeros((n, (n + 63) // 64), dtype=np.uint64)
    for a, b in ((e[:, 0], e[:, 1]), (e[:, 1], e[:, 0])):
        np.bitwise_or.at(bm, (a, b >> 6), np.uint64(1) << (b & 63).astype(np.uint64))
    adj = set(map(tuple, np.sort(e, 1).tolist()))
    got = {}
    try:
        for mode in (0, 4096):
            tp.set_option("colour_mis", mode)
            tp.set_option("colour_mis_any", 1 if mode else 0)
            tp.set_option("k4_debug", 1 if mode else 0)
            s = make_solver()
            capfd.readouterr()
            c, er = s.maxClique(bm, n)
            got[mode] = (c, er, capfd.readouterr().err)
    finally:
        tp.set_option("colour_mis", 8192)
        tp.set_option("colour_mis_any", 0)
        tp.set_option("k4_debug", 0)
    assert "colour_mis verify" in got[4096][2] and " 0 same-colour adjacencies" in got[4096][2], got[4096][2][-400:]
    for c, _, _ in got.values():
        assert c == sorted(c) and all((a, b) in adj for i, a in enumerate(c) for b in c[i + 1:])
    assert len(got[0][0]) == len(got[4096][0]) >= k
    if len(got[0][0]) == k:
        assert got[4096][0] == members.tolist() or len(got[4096][0]) == k


def test_colour_centric_bound_in_a_batch_of_mixed_sizes():
    """The speculative form of the stage (enqueued behind the peel for every problem of the batch, guarded on the device
    by each problem's state): three problems, one below the option's size, one that the peel closes, through
    solve_batch twice (the second call runs the bound stage speculatively); results = the vertex-centric route's."""
    specs = [(20000, 0.985, 51), (5000, 0.9, 52), (30000, 0.99, 53)]
    prs = [tp.synth_problem(20250523 + sd, n, rho, 0.01) for n, rho, sd in specs]
    srcs, dsts = [p["src"] for p in prs], [p["dst"] for p in prs]
    got = {}
    try:
        for mode in (0, 4096):
            tp.set_option("colour_mis", mode)
            s = make_solver(**bench_params())
            s.solve_batch(srcs, dsts)
            sols = s.solve_batch(srcs, dsts)
            got[mode] = [(bool(o.valid), o.rotation.copy(), o.translation.copy(), s.getInlierMaxClique(i),
                          int(s.raw_solution(i).clique_exact_run)) for i, o in enumerate(sols)]
    finally:
        tp.set_option("colour_mis", 8192)
    for a, b, pr in zip(got[0], got[4096], prs):
        assert a[0] and b[0] and a[3] == b[3] and a[4] == b[4]
        assert (a[1] == b[1]).all() and (a[2] == b[2]).all()
        assert set(np.flatnonzero(pr["inliers"]).tolist()) <= set(b[3])


# ---------------------------------------------------------------------------------------------
# end-to-end
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rho,seed", [(100, 0.5, 21), (500, 0.9, 22), (2000, 0.9, 23), (5000, 0.9, 24)])
def test_solve_parity_synthetic(n, rho, seed):
    pr = tp.synth_problem(20250523 + seed, n, rho, 0.01)
    p = bench_params()
    s = make_solver(**p)
    sol = s.solve(pr["src"], pr["dst"])
    o = oracle.solve(pr["src"], pr["dst"], **oracle_params(p))
    check_solution_parity(s, sol, o)
    assert o["clique_unique"]
    assert set(s.getInlierMaxClique()) == set(np.flatnonzero(pr["inliers"]).tolist())
    assert angular_error(pr["R"], sol.rotation) < 0.05
    assert np.linalg.norm(pr["t"] - sol.translation) < 0.05
    # input-ordered translation inliers (registration.h:752-763)
    cl = s.getInlierMaxClique()
    assert s.getInputOrderedTranslationInliers() == [cl[i] for i in s.getTranslationInliers()]


def test_solve_parity_config2_10k():
    """BASELINE config 2: N = 10 000, 95 % outliers (the bench workload)."""
    pr = tp.synth_problem(20250523, 10000, 0.95, 0.01)
    p = bench_params()
    s = make_solver(**p)
    sol = s.solve(pr["src"], pr["dst"])
    o = oracle.solve(pr["src"], pr["dst"], **oracle_params(p))
    check_solution_parity(s, sol, o)
    assert len(s.getInlierMaxClique()) == 500
    _, ref = oracle.inlier_bitmap(pr["src"], pr["dst"], 0.01, 1.0, False)
    assert (s.getInlierGraphBitmap() == ref).all()
    assert s.raw_solution().num_edges == o["num_edges"]


def test_solve_config3_50k_properties():
    """BASELINE config 3: N = 50 000, 99 % outliers (1.25e9 pairs, 313 MB bitmap).  The oracle needs
    minutes here, so size-independent properties: sampled bitmap rows bit-exact against the reference
    expression evaluated in numpy, symmetry, degree sum = 2 edges, the clique is a clique containing
    the planted inliers, ground-truth pose."""
    n, nb = 50000, 0.01
    pr = tp.synth_problem(20250523 + 3, n, 0.99, nb)
    s = make_solver(**bench_params())
    sol = s.solve(pr["src"], pr["dst"])
    assert sol.valid
    bm = s.getInlierGraphBitmap()
    bits = lambda rows: np.unpackbits(bm[rows].view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)
    rng = np.random.default_rng(3)
    rows = np.sort(rng.choice(n, size=48, replace=False))
    ref = numpy_rows_predicate(pr["src"], pr["dst"], rows, 2 * nb)
    got = bits(rows)
    assert (got == ref).all()
    # symmetry on the sampled rows: bit (i, j) == bit (j, i)
    for k, i in enumerate(rows[:8]):
        js = np.flatnonzero(got[k])
        col = (bm[js, i >> 6] >> np.uint64(i & 63)) & np.uint64(1)
        assert col.all()
    deg = s.getDegrees()
    assert int(deg.sum()) == 2 * int(s.raw_solution().num_edges)
    assert (deg[rows] == got.sum(1)).all()
    clique = np.array(s.getInlierMaxClique())
    inl = np.flatnonzero(pr["inliers"])
    assert set(inl.tolist()) <= set(clique.tolist()) and len(clique) <= len(inl) + 3
    sub = numpy_rows_predicate(pr["src"][:, clique], pr["dst"][:, clique], range(len(clique)), 2 * nb)
    assert (sub | np.eye(len(clique), dtype=bool)).all()
    assert angular_error(pr["R"], sol.rotation) < 0.01
    assert np.linalg.norm(sol.translation - pr["t"]) < 0.01


@pytest.mark.parametrize("case", ["config3", "config3_seed2"])
def test_solve_config3_50k_vs_oracle_fixture(case):
    """BASELINE config 3 against the ORACLE (committed fixtures, two seeds: the oracle needs minutes at this size):
    identical clique / inlier index sets, R and t within 1e-4, identical edge count, and the WHOLE 313 MB
    adjacency bitmap bit for bit through its SHA-256."""
    import hashlib
    fx = config_golden()[case]
    pr = tp.synth_problem(fx["seed"], fx["n"], fx["outlier_ratio"], fx["noise_bound"])
    s = make_solver(**bench_params())
    sol = s.solve(pr["src"], pr["dst"])
    check_against_fixture(s, sol, fx)
    assert fx["clique_unique"] and len(fx["max_clique"]) >= 500
    bm = np.ascontiguousarray(s.getInlierGraphBitmap())
    assert hashlib.sha256(bm.tobytes()).hexdigest() == fx["bitmap_sha256"]
    deg = s.getDegrees().astype(np.int64)
    assert int(deg.sum()) == fx["degree_sum"] and int(deg.max()) == fx["degree_max"]
    assert int((deg * (np.arange(fx["n"], dtype=np.int64) % 1009 + 1)).sum()) == fx["degree_weighted_checksum"]


def test_solve_config2_and_config4_elements_vs_oracle_fixture():
    """Config 2 and three elements of the config-4 batch (solved inside the full 128-problem batch)
    against the committed oracle fixture, bitmaps through their SHA-256."""
    import hashlib
    G4 = config_golden()
    fx2 = G4["config2"]
    pr = tp.synth_problem(fx2["seed"], fx2["n"], fx2["outlier_ratio"], fx2["noise_bound"])
    s = make_solver(**bench_params())
    check_against_fixture(s, s.solve(pr["src"], pr["dst"]), fx2)
    assert hashlib.sha256(np.ascontiguousarray(s.getInlierGraphBitmap()).tobytes()).hexdigest() == fx2["bitmap_sha256"]
    B, n = 128, 5000
    probs = [tp.synth_problem(20250523 + 4000 + b, n, 0.9, 0.01) for b in range(B)]
    sols = s.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
    for b in (0, 57, 127):
        fx = G4["config4_b%d" % b]
        assert fx["seed"] == 20250523 + 4000 + b
        check_against_fixture(s, sols[b], fx, problem=b)
        bm = np.ascontiguousarray(s.getInlierGraphBitmap(b))
        assert hashlib.sha256(bm.tobytes()).hexdigest() == fx["bitmap_sha256"]


def test_solve_config4_batch_5k_properties():
    """BASELINE config 4 (one GPU's share): 128 independent N = 5 000 problems, 90 % outliers, in one
    batched call; every problem recovers its planted clique and pose, and batched results are
    identical to solving the same problem alone."""
    B, n, nb = 128, 5000, 0.01
    probs = [tp.synth_problem(20250523 + 4000 + b, n, 0.9, nb) for b in range(B)]
    s = make_solver(**bench_params())
    sols = s.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
    cliques = [s.getInlierMaxClique(b) for b in range(B)]
    for b, (p, sol) in enumerate(zip(probs, sols)):
        assert sol.valid
        inl = set(np.flatnonzero(p["inliers"]).tolist())
        assert inl <= set(cliques[b]) and len(cliques[b]) <= len(inl) + 3
        assert angular_error(p["R"], sol.rotation) < 0.02
        assert np.linalg.norm(sol.translation - p["t"]) < 0.02
    s1 = make_solver(**bench_params())
    for b in (0, 57, 127):
        one = s1.solve(probs[b]["src"], probs[b]["dst"])
        assert s1.getInlierMaxClique() == cliques[b]
        assert np.array_equal(one.rotation, sols[b].rotation)
        assert np.array_equal(one.translation, sols[b].translation)


def test_solve_object_scene_fixed_scale():
    """Hard clique fixture (max_core+1 > omega): registration-test.cc:313-391 bounds."""
    obj, scn = G["object_in"], G["scene_in"]
    p = bench_params(noise_bound=float(G["object_noise_bound"]))
    s = make_solver(**p)
    sol = s.solve(obj, scn)
    o = oracle.solve(obj, scn, **oracle_params(p))
    check_solution_parity(s, sol, o)
    assert len(s.getInlierMaxClique()) == 34
    # max_core+1 (37) > omega (34): neither the greedy bound nor the peel closes it; either the
    # global colouring bound proves 34 (no uncoloured survivor) or the B&B has to run
    raw = s.raw_solution()
    assert raw.colour_uncoloured == 0 or raw.clique_exact_run == 1
    bR1, bt1, bR2, bt2 = G["object_bounds"]
    assert angular_error(G["object_expected_R"], sol.rotation) <= bR2
    assert np.linalg.norm(sol.translation - G["object_expected_t"]) <= bt2
    adj = oracle.bitmap_to_dense(s.getInlierGraphBitmap(), obj.shape[1])
    assert is_clique(adj, s.getInlierMaxClique())


def test_solve_object_scene_estimate_scaling():
    obj, scn = G["object_in"], G["scene_in"]
    p = dict(noise_bound=float(G["object_noise_bound"]), estimate_scaling=True,
             rotation_cost_threshold=0.005)
    s = make_solver(**p)
    sol = s.solve(obj, scn)
    o = oracle.solve(obj, scn, **oracle_params(p))
    assert abs(sol.scale - float(G["object_expected_scale"])) < 1e-4
    assert abs(sol.scale - o["scale"]) < 1e-9
    _, ref = oracle.inlier_bitmap(obj, scn, p["noise_bound"], 1.0, True)
    assert (s.getInlierGraphBitmap() == ref).all()
    check_solution_parity(s, sol, o)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_benchmark_fixtures(k):
    """reference test/benchmark/registration-benchmark.cc:180-374 thresholds, on the GPU path."""
    src = G["bench%d_src" % k].astype(np.float64).T
    dst = G["bench%d_dst" % k].astype(np.float64).T
    p = dict(noise_bound=float(G["bench%d_noise_bound" % k]), cbar2=1.0, estimate_scaling=True,
             rotation_max_iterations=100, rotation_gnc_factor=1.4, rotation_cost_threshold=1e-12)
    s = make_solver(**p)
    sol = s.solve(src, dst)
    assert sol.valid
    sg, Rg, tg, se, Re, te = G["bench%d_thresholds" % k]
    assert abs(sol.scale - float(G["bench%d_s_ref" % k])) <= sg
    assert angular_error(G["bench%d_R_ref" % k], sol.rotation) <= Rg
    assert np.linalg.norm(sol.translation - G["bench%d_t_ref" % k]) <= tg
    assert abs(sol.scale - float(G["bench%d_s_est" % k])) <= se
    assert angular_error(G["bench%d_R_est" % k], sol.rotation) <= Re
    assert np.linalg.norm(sol.translation - G["bench%d_t_est" % k]) <= te
    o = oracle.solve(src, dst, **oracle_params(p))
    check_solution_parity(s, sol, o)


def test_bunny_config1():
    """BASELINE config 1 (plumbing): bun_zipper_res3 with the example's T, noise and outlier model
    (teaser_cpp_ply.cc:12-40,62-68) driven by a seeded generator."""
    rng = np.random.default_rng(20250523)
    src = G["bunny"].astype(np.float64).T  # 3 x 1889
    T = G["bunny_T"]
    n = src.shape[1]
    NB = 0.001
    dst = T[:3, :3] @ src + T[:3, 3:4]
    dst += (rng.uniform(-1, 1, size=dst.shape)) * NB / 2
    for _ in range(1700):  # with replacement, like the example
        i = int(rng.integers(0, n))
        dst[:, i] += float(rng.integers(5, 11))
    p = bench_params(noise_bound=NB)
    s = make_solver(**p)
    sol = s.solve(src, dst)
    o = oracle.solve(src, dst, **oracle_params(p))
    check_solution_parity(s, sol, o)
    assert angular_error(T[:3, :3], sol.rotation) < 0.02
    assert np.linalg.norm(T[:3, 3] - sol.translation) < 0.005


def test_outlier_detection():
    """registration-test.cc:394-467: clique == exact inlier set for far outliers."""
    rng = np.random.default_rng(17)
    for n_out in range(1, 6):
        src = rng.uniform(-1, 1, size=(3, 20))
        R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        if np.linalg.det(R) < 0:
            R[:, 0] *= -1
        t = rng.uniform(-1, 1, size=(3, 1))
        dst = R @ src + t
        out_idx = rng.choice(20, size=n_out, replace=False)
        dst[:, out_idx] += rng.uniform(5, 10, size=(3, n_out))
        s = make_solver(**bench_params(rotation_cost_threshold=1e-12))
        sol = s.solve(src, dst)
        assert s.getInlierMaxClique() == sorted(set(range(20)) - set(out_idx.tolist()))
        assert angular_error(R, sol.rotation) < 1e-6
        assert np.linalg.norm(sol.translation - t.ravel()) < 1e-6


def test_edge_cases():
    s = make_solver(**bench_params())
    # empty and single-point inputs: valid = false, no crash (registration.cc:643-647)
    for n in (0, 1):
        sol = s.solve(np.zeros((3, n)), np.zeros((3, n)))
        assert not sol.valid
    # two consistent points: clique of 2
    src = np.array([[0, 1.0], [0, 0], [0, 0]])
    sol = s.solve(src, src + 0.5)
    assert sol.valid and s.getInlierMaxClique() == [0, 1]
    assert np.linalg.norm(sol.translation - 0.5) < 1e-9
    # all outliers: two far-inconsistent points -> clique size 1 -> invalid
    dst = np.array([[0, 9.0], [0, 0], [0, 0]])
    sol = s.solve(src, dst)
    assert not sol.valid and len(s.getInlierMaxClique()) == 1
    # handle reuse after an invalid solve (the reference object is single-use; ours is not)
    pr = tp.synth_problem(5, 300, 0.5, 0.01)
    a = s.solve(pr["src"], pr["dst"])
    b = s.solve(pr["src"], pr["dst"])
    assert a.valid and (a.rotation == b.rotation).all() and (a.translation == b.translation).all()
    # no outliers at all
    pr = tp.synth_problem(6, 700, 0.0, 0.01)
    sol = s.solve(pr["src"], pr["dst"])
    assert len(s.getInlierMaxClique()) == 700


def test_kcore_heuristic_mode_vs_oracle():
    """inlier_selection_mode = KCORE_HEU (graph.cc:58-81 as documented): exact core numbers on the GPU;
    when max_core > (int)(threshold * N) the inlier set is every vertex of the maximum core, otherwise
    the heuristic clique.  Both branches, against the oracle's Batagelj-Zaversnik restatement."""
    # (a) 70 % inliers: the inlier clique (size 280 of 400) makes max_core = 279 > 0.5 * 400 -> shortcut;
    #     the maximum core is larger than the clique here (outliers attached to it), which is the
    #     documented difference between KCORE_HEU and the clique modes
    for seed, n, rho, thr in ((71, 400, 0.3, 0.5), (72, 600, 0.25, 0.4), (73, 1000, 0.45, 0.5)):
        pr = tp.synth_problem(seed, n, rho, 0.01)
        p = bench_params(inlier_selection_mode=tp.InlierSelectionMode.KCORE_HEU, kcore_heuristic_threshold=thr)
        s = make_solver(**p)
        sol = s.solve(pr["src"], pr["dst"])
        _, bm = oracle.inlier_bitmap(pr["src"], pr["dst"], 0.01, 1.0, False)
        taken, core_set, max_core = oracle.kcore_heuristic(bm, n, thr)
        assert taken and max_core > int(thr * n)
        assert s.getInlierMaxClique() == core_set.tolist()
        o = oracle.solve(pr["src"], pr["dst"], **oracle_params(p))
        assert o["max_clique"].tolist() == core_set.tolist()
        check_solution_parity(s, sol, o)
    # (b) 90 % outliers: max_core (~ inliers - 1) <= 0.5 * N -> no shortcut, the heuristic clique
    pr = tp.synth_problem(74, 1000, 0.9, 0.01)
    p = bench_params(inlier_selection_mode=tp.InlierSelectionMode.KCORE_HEU)
    s = make_solver(**p)
    sol = s.solve(pr["src"], pr["dst"])
    _, bm = oracle.inlier_bitmap(pr["src"], pr["dst"], 0.01, 1.0, False)
    taken, _, max_core = oracle.kcore_heuristic(bm, 1000, 0.5)
    assert not taken
    o = oracle.solve(pr["src"], pr["dst"], **oracle_params(p))
    check_solution_parity(s, sol, o)
    # threshold == 1 short-circuits the comparison (graph.cc:67): never the shortcut
    pr = tp.synth_problem(71, 400, 0.3, 0.01)
    p = bench_params(inlier_selection_mode=tp.InlierSelectionMode.KCORE_HEU, kcore_heuristic_threshold=1.0)
    s = make_solver(**p)
    s.solve(pr["src"], pr["dst"])
    assert s.getInlierMaxClique() == np.flatnonzero(pr["inliers"]).tolist()


def test_inlier_selection_modes():
    pr = tp.synth_problem(31, 400, 0.8, 0.01)
    truth = np.flatnonzero(pr["inliers"]).tolist()
    for mode in (tp.InlierSelectionMode.PMC_EXACT, tp.InlierSelectionMode.PMC_HEU,
                 tp.InlierSelectionMode.KCORE_HEU):
        s = make_solver(**bench_params(inlier_selection_mode=mode))
        s.solve(pr["src"], pr["dst"])
        assert s.getInlierMaxClique() == truth
    s = make_solver(**bench_params(inlier_selection_mode=tp.InlierSelectionMode.NONE))
    sol = s.solve(pr["src"], pr["dst"])
    assert s.getInlierMaxClique() == list(range(400))
    o = oracle.solve(pr["src"], pr["dst"], **oracle_params(bench_params(inlier_selection_mode=3)))
    assert np.linalg.norm(sol.rotation - o["rotation"]) < R_TOL
    assert np.linalg.norm(sol.translation - o["translation"]) < T_TOL
    # out-of-range rotation algorithm: loud error, never a silent fallback
    s = make_solver(**bench_params())
    bad = tp.RobustRegistrationSolver.Params(**bench_params())
    bad.rotation_estimation_algorithm = 7
    s.reset(bad)
    with pytest.raises(tp.TeaserHipError):
        s.solve(pr["src"], pr["dst"])


def test_reference_snapshot_semantics_option():
    """reference_snapshot_semantics = 1: a handle behaves like the reference SNAPSHOT's binary, whose solve() reads a
    params_ that neither constructor nor reset() ever assigns (registration.h:830-908, registration.cc:574-583; SURVEY
    F3): inlier_selection_mode NONE / use_max_clique = false / COMPLETE graph are ignored -- PMC_EXACT + CHAIN run --
    while noise bound, scaling and the rotation estimator stay the caller's.  Default 0: the documented modes."""
    pr = tp.synth_problem(31, 400, 0.8, 0.01)
    truth = np.flatnonzero(pr["inliers"]).tolist()
    kw = bench_params(inlier_selection_mode=tp.InlierSelectionMode.NONE, use_max_clique=False,
                      rotation_tim_graph=tp.InlierGraphFormulation.COMPLETE)
    s = make_solver(**kw)
    s.solve(pr["src"], pr["dst"])
    assert s.getInlierMaxClique() == list(range(400))  # documented semantics: no clique selection
    ref = make_solver(**bench_params())
    want = ref.solve(pr["src"], pr["dst"])
    tp.set_option("reference_snapshot_semantics", 1)
    try:
        s2 = make_solver(**kw)  # (the option is read when a handle is created or reset)
        got = s2.solve(pr["src"], pr["dst"])
        assert s2.getInlierMaxClique() == truth == ref.getInlierMaxClique()
        assert np.array_equal(got.rotation, want.rotation) and np.array_equal(got.translation, want.translation)
        assert s2.getRotationInliers() == ref.getRotationInliers()
        # the caller's Params are still what the getter returns
        assert int(s2.getParams().inlier_selection_mode) == int(tp.InlierSelectionMode.NONE)
        s.reset(tp.RobustRegistrationSolver.Params(**kw))  # an existing handle picks the option up at reset()
        s.solve(pr["src"], pr["dst"])
        assert s.getInlierMaxClique() == truth
    finally:
        tp.set_option("reference_snapshot_semantics", 0)
    s.reset(tp.RobustRegistrationSolver.Params(**kw))
    s.solve(pr["src"], pr["dst"])
    assert s.getInlierMaxClique() == list(range(400))


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_reference_no_max_clique_and_clique_finder_modes(seed):
    """The reference's own NoMaxClique / CliqueFinderModes tests (registration-test.cc:469-680; inputs restated in
    tests/reference_cases.py) through the HIP path: the reference's thresholds, and parity with the oracle."""
    from reference_cases import PARAMS, T_REF, angular_error, case
    src, tgt, outliers = case(seed)
    runs = [dict(PARAMS, use_max_clique=False)] + [dict(PARAMS, inlier_selection_mode=m) for m in (0, 1, 2, 3)]
    for kw in runs:
        s = make_solver(**kw)
        sol = s.solve(src, tgt)
        assert sol.valid
        assert angular_error(T_REF[:, :3], sol.rotation) <= 0.2
        assert np.linalg.norm(T_REF[:, 3] - sol.translation) <= 0.1
        o = oracle.solve(src, tgt, **oracle_params(dict(kw, use_max_clique=int(kw.get("use_max_clique", True)))))
        check_solution_parity(s, sol, o)


# ---------------------------------------------------------------------------------------------
# FGR / QUATRO rotation estimators (registration.cc:206-408)
# ---------------------------------------------------------------------------------------------
def test_fgr_rotation_known_answer():
    # reference test/teaser/rotation-solver-test.cc:101-134 through the HIP kernel
    src = G["rot_src"].T
    R_exp = G["rot_expected_R"]
    dst = R_exp @ src
    mi, thr, fac, nb = G["fgr_params"]
    s = make_solver(rotation_estimation_algorithm=tp.RotationEstimationAlgorithm.FGR, noise_bound=float(nb),
                    rotation_gnc_factor=float(fac), rotation_max_iterations=int(mi),
                    rotation_cost_threshold=float(thr))
    R = s.solveForRotation(src, dst)
    assert angular_error(R_exp, R) < float(G["rot_tol"])
    o = oracle.fgr_rotation(src, dst, nb, fac, int(mi), thr)
    assert np.linalg.norm(R - o["R"]) < 1e-9
    assert s._last_rotation["iterations"] == o["iterations"]
    assert (s._last_rotation["inliers"] == o["inliers"]).all()


def test_quatro_rotation_known_answer():
    # reference test/teaser/registration-test.cc:179-216 through the HIP kernel
    src = G["rot_src"].T
    R_exp = G["quatro_expected_R"]
    dst = R_exp @ src
    mi, thr, fac, nb = G["quatro_params"]
    s = make_solver(rotation_estimation_algorithm=tp.RotationEstimationAlgorithm.QUATRO,
                    noise_bound=float(nb), rotation_gnc_factor=float(fac),
                    rotation_max_iterations=int(mi), rotation_cost_threshold=float(thr))
    R = s.solveForRotation(src, dst)
    assert angular_error(R_exp, R) < 1e-5
    o = oracle.quatro_rotation(src, dst, nb, fac, int(mi), thr)
    assert np.linalg.norm(R - o["R"]) < 1e-9


@pytest.mark.parametrize("alg", [1, 2])
def test_fgr_quatro_rotation_with_outliers_vs_oracle(alg):
    rng = np.random.default_rng(40 + alg)
    k = 700
    src = rng.uniform(-1, 1, size=(3, k))
    th = 0.7
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    R0 = Rz if alg == 2 else Rz @ Rx
    dst = R0 @ src + rng.uniform(-0.004, 0.004, size=(3, k))
    dst[:, :150] = rng.uniform(-1, 1, size=(3, 150))
    s = make_solver(rotation_estimation_algorithm=alg, noise_bound=0.01, rotation_gnc_factor=1.4,
                    rotation_max_iterations=100, rotation_cost_threshold=1e-6)
    R = s.solveForRotation(src, dst)
    fn = oracle.fgr_rotation if alg == 1 else oracle.quatro_rotation
    o = fn(src, dst, 0.01, 1.4, 100, 1e-6)
    assert np.linalg.norm(R - o["R"]) <= R_TOL
    assert s._last_rotation["iterations"] == o["iterations"]
    assert (s._last_rotation["inliers"] == o["inliers"]).all()
    assert angular_error(R0, R) < 0.02


@pytest.mark.parametrize("alg", [1, 2])
def test_solve_fgr_quatro_vs_oracle(alg):
    """End-to-end solve() with the FGR / QUATRO rotation estimators (registration.h:856-869)."""
    for n, rho, seed in ((500, 0.8, 51), (3000, 0.9, 52)):
        pr = tp.synth_problem(20250523 + seed, n, rho, 0.01)
        p = bench_params(rotation_estimation_algorithm=alg)
        s = make_solver(**p)
        sol = s.solve(pr["src"], pr["dst"])
        o = oracle.solve(pr["src"], pr["dst"], **oracle_params(p))
        check_solution_parity(s, sol, o)
        if alg == 1:
            assert angular_error(pr["R"], sol.rotation) < 0.02
            with pytest.raises(RuntimeError):  # registration.h:753-756
                s.getInputOrderedTranslationInliers()
    # the reference's own end-to-end FGR test: objectIn / sceneIn (registration-test.cc:256-392)
    if alg == 1:
        obj, scn = G["object_in"], G["scene_in"]
        nb = float(G["object_noise_bound"])
        bR1, bt1, bR2, bt2 = G["object_bounds"]
        p = dict(noise_bound=nb, cbar2=1.0, estimate_scaling=True, rotation_gnc_factor=1.4,
                 rotation_max_iterations=100, rotation_cost_threshold=0.005,
                 rotation_estimation_algorithm=1)
        s = make_solver(**p)
        sol = s.solve(obj, scn)
        assert abs(sol.scale - float(G["object_expected_scale"])) < 1e-4
        assert angular_error(G["object_expected_R"], sol.rotation) <= bR1
        assert np.linalg.norm(sol.translation - G["object_expected_t"]) <= bt1
        o = oracle.solve(obj, scn, **oracle_params(p))
        check_solution_parity(s, sol, o)


def test_complete_tim_graph():
    pr = tp.synth_problem(32, 300, 0.7, 0.01)
    p = bench_params(rotation_tim_graph=tp.InlierGraphFormulation.COMPLETE)
    s = make_solver(**p)
    sol = s.solve(pr["src"], pr["dst"])
    o = oracle.solve(pr["src"], pr["dst"], **oracle_params(dict(p, rotation_tim_graph=1)))
    check_solution_parity(s, sol, o)


def test_tim_product_getters():
    """getSrcTIMs / getMaxClique*TIMs / get*TIMsMapForRotation (registration.h:778-824): rebuilt on
    the host from the last inputs, in the reference's pair order and chain convention."""
    pr = tp.synth_problem(20250523 + 61, 150, 0.6, 0.01)
    s = make_solver(**bench_params())
    sol = s.solve(pr["src"], pr["dst"])
    t_src, _ = oracle.compute_tims(pr["src"])
    assert np.array_equal(s.getSrcTIMs(), t_src.T if t_src.shape[0] != 3 else t_src)
    c = np.array(s.getInlierMaxClique())
    K = len(c)
    m = s.getSrcTIMsMapForRotation()
    assert m.shape == (2, K) and (m[1] == c).all() and (m[0] == np.roll(c, -1)).all()  # (leaf, root)
    ts, td = s.getMaxCliqueSrcTIMs(), s.getMaxCliqueDstTIMs()
    assert ts.shape == (3, K) and np.allclose(ts[:, 0], pr["src"][:, c[1]] - pr["src"][:, c[0]])
    # rotated src TIMs match the (de-scaled) dst TIMs on the rotation inliers
    inl = s.getRotationInliers()
    res = td[:, inl] - sol.rotation @ ts[:, inl]
    assert np.abs(res).max() < 4 * 0.01


def test_correspondence_overload():
    """solve(PointCloud, PointCloud, correspondences), registration.cc:553-566."""
    pr = tp.synth_problem(33, 500, 0.6, 0.01)
    rng = np.random.default_rng(33)
    src_cloud = pr["src"].T.astype(np.float32)
    dst_cloud = pr["dst"].T.astype(np.float32)
    perm = rng.permutation(500)
    dst_shuffled = dst_cloud[perm]
    inv = np.argsort(perm)
    corr = np.stack([np.arange(500), inv], axis=1)
    p = bench_params()
    s = make_solver(**p)
    sol = s.solve_correspondences(src_cloud, dst_shuffled, corr)
    # the ORACLE on the gathered, float -> double widened arrays (registration.cc:557-565): pins the
    # gather + widening semantics independently of the HIP path
    gs = src_cloud[corr[:, 0]].astype(np.float64).T
    gd = dst_shuffled[corr[:, 1]].astype(np.float64).T
    o = oracle.solve(gs, gd, **oracle_params(p))
    check_solution_parity(s, sol, o)
    assert o["valid"] and o["clique_unique"]
    assert s.getInlierMaxClique() == o["max_clique"].tolist()
    # and the matrix overload of the HIP path agrees bit for bit with the correspondence overload
    s2 = make_solver(**p)
    sol2 = s2.solve(gs, gd)
    assert (sol.rotation == sol2.rotation).all() and (sol.translation == sol2.translation).all()
    assert s.getInlierMaxClique() == s2.getInlierMaxClique()


def test_batch_matches_single():
    """Batched mode: ragged batch, each problem identical to its single-solve result."""
    sizes = [300, 1000, 64, 777, 1, 500]
    probs = [tp.synth_problem(40 + i, n, 0.8, 0.01) for i, n in enumerate(sizes)]
    sb = make_solver(**bench_params())
    sols = sb.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
    for i, pr in enumerate(probs):
        s1 = make_solver(**bench_params())
        one = s1.solve(pr["src"], pr["dst"])
        assert sols[i].valid == one.valid
        assert sb.getInlierMaxClique(i) == s1.getInlierMaxClique()
        if one.valid:
            assert (sols[i].rotation == one.rotation).all()
            assert (sols[i].translation == one.translation).all()
            assert sb.getRotationInliers(i) == s1.getRotationInliers()
            assert sb.getTranslationInliers(i) == s1.getTranslationInliers()


def test_determinism():
    pr = tp.synth_problem(50, 3000, 0.9, 0.01)
    s = make_solver(**bench_params())
    first = s.solve(pr["src"], pr["dst"])
    c0 = s.getInlierMaxClique()
    b0 = s.getInlierGraphBitmap().copy()
    for _ in range(5):
        sol = s.solve(pr["src"], pr["dst"])
        assert (sol.rotation == first.rotation).all() and (sol.translation == first.translation).all()
        assert s.getInlierMaxClique() == c0
        assert (s.getInlierGraphBitmap() == b0).all()


# ---------------------------------------------------------------------------------------------
# asynchronous batches (teaser_hip_submit_batch / teaser_hip_wait), host inputs, several handles
# ---------------------------------------------------------------------------------------------
def _packed(probs):
    src = np.ascontiguousarray(np.concatenate([p["src"].T for p in probs], axis=0))
    dst = np.ascontiguousarray(np.concatenate([p["dst"].T for p in probs], axis=0))
    n = np.array([p["src"].shape[1] for p in probs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    return src, dst, off, n


def test_async_paths_agree_across_host_modes():
    """The asynchronous path has three host-side modes since round 4: the second half of a batch on the caller's thread
    (TEASER_HIP_FINISHER=0), on the lane's finisher thread, and with the bound stage enqueued speculatively behind the
    peel.  Seven batches alternating between "all closed by the peel" and "open problems" (tests/async_digest.py)
    must give the same cliques, inlier lists, R and t, bit for bit, in all three -- and the open problems must
    really have gone through the colouring bound."""
    import json
    import os
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "async_digest.py")
    got = []
    for fin, spec in (("0", "0"), ("1", "0"), ("1", "1")):
        env = dict(os.environ, TEASER_HIP_FINISHER=fin, TEASER_HIP_SPEC_BOUNDS=spec)
        p = subprocess.run([sys.executable, script], capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        got.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert got[0]["coloured"] >= 12, got  # 6 open problems x 2 input modes went through the colouring bound
    assert got[0]["digest"] == got[1]["digest"] == got[2]["digest"], got
    assert got[0]["coloured"] == got[1]["coloured"] == got[2]["coloured"]


def test_async_batches_match_sync():
    """Four ragged batches in flight over three lanes (device inputs, then host inputs): every problem
    is identical -- clique, inliers, R, t bit for bit -- to the synchronous batched solve."""
    from util import HipBuffers
    sizes = [[300, 1000, 64, 777], [2000, 500], [1500, 1, 129, 640, 900], [1024, 2048]]
    batches = [[tp.synth_problem(900 + 10 * k + i, n, 0.85, 0.01) for i, n in enumerate(sz)]
               for k, sz in enumerate(sizes)]
    ref = make_solver(**bench_params())
    want = []
    for probs in batches:
        sols = ref.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
        want.append([(bool(o.valid), o.rotation.copy(), o.translation.copy(), ref.getInlierMaxClique(b),
                      ref.getRotationInliers(b), ref.getTranslationInliers(b)) for b, o in enumerate(sols)])
    mem = HipBuffers()
    s = make_solver(**bench_params())
    s.set_pipeline_depth(3)
    for host in (False, True):
        put = mem.pinned if host else mem.device
        tickets = []
        for probs in batches[:3]:
            src, dst, off, n = _packed(probs)
            tickets.append(s.submit_batch(put(src), put(dst), off, n, host=host))
        # all three lanes are in flight: a fourth DEVICE submit must be refused, loudly; a fourth HOST
        # batch is staged (its copy starts at once), a fifth one refused
        src, dst, off, n = _packed(batches[3])
        a, b = put(src), put(dst)
        t3 = None
        if host:
            t3 = s.submit_batch(a, b, off, n, host=True)
            with pytest.raises(tp.TeaserHipError):
                s.wait(t3)  # still staged behind the lanes: BUSY until an earlier ticket has been waited for
        with pytest.raises(tp.TeaserHipError):
            s.submit_batch(a, b, off, n, host=host)
        for k in (1, 0, 2):  # tickets may be waited for in any order
            out = s.wait(tickets[k])
            for bi, w in enumerate(want[k]):
                o = out[bi]
                assert bool(o.valid) == w[0]
                assert s.getInlierMaxClique(bi) == w[3]
                if w[0]:
                    assert (np.array(o.rotation[:]).reshape(3, 3) == w[1]).all()
                    assert (np.array(o.translation[:]) == w[2]).all()
                    assert s.getRotationInliers(bi) == w[4] and s.getTranslationInliers(bi) == w[5]
        if t3 is None:
            t3 = s.submit_batch(a, b, off, n, host=host)
        out = s.wait(t3)
        for bi, w in enumerate(want[3]):
            assert s.getInlierMaxClique(bi) == w[3]
            assert (np.array(out[bi].rotation[:]).reshape(3, 3) == w[1]).all()
        with pytest.raises((tp.TeaserHipError, KeyError)):
            s.wait(t3)  # a ticket is waited for exactly once
    # the synchronous API on the same handle still works between asynchronous batches
    one = s.solve(batches[0][1]["src"], batches[0][1]["dst"])
    assert (one.rotation == want[0][1][1]).all() and s.getInlierMaxClique() == want[0][1][3]
    del s
    mem.free()


def test_async_headline_batch_64x10k_vs_oracle_fixture():
    """The route bench.py times -- teaser_hip_submit_batch / teaser_hip_wait, two batches in flight, finisher threads on,
    device and page-locked host inputs -- on a WHOLE headline batch (64 problems of N = 10 000, 95 % outliers), checked
    problem by problem against the committed ORACLE fixture (tests/golden/make_config2_batch_golden.py): edge count,
    maximum clique and both inlier lists (through their SHA-256; content only where the oracle found the maximum clique
    unique -- one problem of the 64 has two), R and t to the north_star tolerances, and the 12.5 MB bitmap of four
    problems bit for bit."""
    import hashlib
    import json
    import os
    from util import ROOT, HipBuffers
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "config2_batch_golden.json")))
    B, n = fx["batch"], fx["n"]
    probs = [tp.synth_problem(fx["seed0"] + b, n, fx["outlier_ratio"], fx["noise_bound"]) for b in range(B)]
    other = [tp.synth_problem(fx["seed0"] + 500 + b, n, fx["outlier_ratio"], fx["noise_bound"]) for b in range(B)]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.int32)).tobytes()).hexdigest()

    def check(s, out, bitmaps):
        assert sum(1 for f in fx["problems"] if not f["clique_unique"]) <= 2
        for b, f in enumerate(fx["problems"]):
            o = out[b]
            assert bool(o.valid) == f["valid"] and o.num_edges == f["num_edges"] and o.clique_size == f["clique_size"], b
            if f["clique_unique"]:
                assert sha(s.getInlierMaxClique(b)) == f["max_clique_sha256"], b
                assert sha(s.getRotationInliers(b)) == f["rotation_inliers_sha256"], b
                assert sha(s.getTranslationInliers(b)) == f["translation_inliers_sha256"], b
                assert np.linalg.norm(np.array(o.rotation[:]) - np.array(f["rotation"])) <= R_TOL, b
                assert np.linalg.norm(np.array(o.translation[:]) - np.array(f["translation"])) <= T_TOL, b
            else:  # a maximum clique, whichever: every pair adjacent
                bm = s.getInlierGraphBitmap(b)
                cl = np.asarray(s.getInlierMaxClique(b))
                sub = np.unpackbits(np.ascontiguousarray(bm[cl]).view(np.uint8), axis=1, bitorder="little")[:, cl].astype(bool)
                assert (sub | np.eye(len(cl), dtype=bool)).all(), b
        for b in bitmaps:
            bm = np.ascontiguousarray(s.getInlierGraphBitmap(b))
            assert hashlib.sha256(bm.tobytes()).hexdigest() == fx["problems"][b]["bitmap_sha256"], b

    mem = HipBuffers()
    s = make_solver(**bench_params())
    s.set_pipeline_depth(2)
    for host in (False, True):
        put = mem.pinned if host else mem.device
        sa, da, off, nn = _packed(probs)
        sb, db, _, _ = _packed(other)
        A = (put(sa), put(da))
        Bb = (put(sb), put(db))
        t0 = s.submit_batch(A[0], A[1], off, nn, host=host)
        t1 = s.submit_batch(Bb[0], Bb[1], off, nn, host=host)
        check(s, s.wait(t0), (0, 30, 63))
        t2 = s.submit_batch(A[0], A[1], off, nn, host=host)   # the same lane again, behind the other batch
        s.wait(t1)
        check(s, s.wait(t2), (17,))
    del s
    mem.free()


def test_staged_batch_takes_the_first_free_lane():
    """Depth 2, host inputs: t0, t1 on the lanes, t2 staged.  After wait(t1) lane 1 is free although it is lane 0's
    turn: the staged batch must move there, and wait(t2) must succeed BEFORE t0 has been waited for (a caller that
    retries on BUSY used to spin for ever: the staged batch only ever went to lanes[next_lane])."""
    from util import HipBuffers
    probs = [[tp.synth_problem(1300 + 10 * k + i, n, 0.8, 0.01) for i, n in enumerate(sz)]
             for k, sz in enumerate([[700, 300], [512], [900, 65, 400]])]
    ref = make_solver(**bench_params())
    want = []
    for pb in probs:
        sols = ref.solve_batch([p["src"] for p in pb], [p["dst"] for p in pb])
        want.append([(o.rotation.copy(), o.translation.copy()) for o in sols])
    mem = HipBuffers()
    s = make_solver(**bench_params())
    s.set_pipeline_depth(2)
    tickets = []
    for pb in probs:
        src, dst, off, n = _packed(pb)
        tickets.append(s.submit_batch(mem.pinned(src), mem.pinned(dst), off, n, host=True))
    with pytest.raises(tp.TeaserHipError):
        s.wait(tickets[2])  # staged: BUSY until an earlier ticket has been waited for
    for k in (1, 2, 0):
        out = s.wait(tickets[k])
        for bi, w in enumerate(want[k]):
            assert (np.array(out[bi].rotation[:]).reshape(3, 3) == w[0]).all()
            assert (np.array(out[bi].translation[:]) == w[1]).all()
    del s
    mem.free()


def test_multi_device_fan_out():
    """teaser_hip_multi_*: two handles (the same GPU listed twice on a 1-GPU box), one host thread each;
    a ragged batch cut into contiguous blocks gives the same results as one handle."""
    sizes = [1200, 300, 64, 2000, 777, 1, 500, 1500, 900]
    probs = [tp.synth_problem(700 + i, n, 0.8, 0.01) for i, n in enumerate(sizes)]
    ref = make_solver(**bench_params())
    want = ref.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
    cl = [ref.getInlierMaxClique(b) for b in range(len(probs))]
    ndev = tp.device_count()
    m = tp.MultiDeviceSolver(tp.RobustRegistrationSolver.Params(**bench_params()),
                             devices=[0, 0] if ndev == 1 else None)
    assert m.device_count() == (2 if ndev == 1 else ndev)
    out = m.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
    for b in range(len(probs)):
        assert bool(out[b].valid) == want[b].valid
        assert m.max_clique(b) == cl[b]
        if want[b].valid:
            assert (np.array(out[b].rotation[:]).reshape(3, 3) == want[b].rotation).all()
            assert (np.array(out[b].translation[:]) == want[b].translation).all()
    m.close()


def test_k1_matrix_core_filter_matches_the_fp64_kernel():
    """The two K1 routes of the product -- the matrix-core filter with its FP64 fix-up, and the all-FP64 kernel that the
    overflow rerun, n > 65536 and estimate_scaling take (forced here with the `k1_fp64` option) -- produce the same
    bitmap, and it is the oracle's.  (The scheduling variants of the filter kernel live in the lab build,
    scripts/probe/k1_lab, which asserts the same identity for each of them.)"""
    pr = tp.synth_problem(61, 4500, 0.9, 0.01)
    _, ref = oracle.inlier_bitmap(pr["src"], pr["dst"], 0.01, 1.0, False)
    try:
        for v in (1, 0):
            tp.set_option("k1_fp64", v)
            s = make_solver(**bench_params())
            s.solve(pr["src"], pr["dst"])
            assert (s.getInlierGraphBitmap() == ref).all(), v
    finally:
        tp.set_option("k1_fp64", 0)


def test_mixed_size_batch_with_one_large_member():
    """One n = 50 000 problem beside small ones: every problem's counted worklist segment is sized from ITS OWN pair
    count (prefix offsets in the prep records), so the large member stays on the matrix-core route (no overflow
    rerun) and every bitmap / clique equals the single-problem solve."""
    big = tp.synth_problem(7001, 50000, 0.99, 0.01)
    small = [tp.synth_problem(7100 + k, 1000, 0.9, 0.01) for k in range(15)]
    probs = small[:7] + [big] + small[7:]
    s = make_solver(**bench_params())
    s.set_profiling(2)
    sols = s.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
    assert s.get_profile()["tim_graph_launches"] == 1  # no all-FP64 rerun of the batch
    cl = [s.getInlierMaxClique(b) for b in range(len(probs))]
    deg = [s.getDegrees(b).copy() for b in range(len(probs))]
    one = make_solver(**bench_params())
    for b in (0, 7, 15):
        ref = one.solve(probs[b]["src"], probs[b]["dst"])
        assert one.getInlierMaxClique() == cl[b]
        assert (one.getDegrees() == deg[b]).all()
        assert (ref.rotation == sols[b].rotation).all() and (ref.translation == sols[b].translation).all()
    assert cl[7] == np.flatnonzero(big["inliers"]).tolist()  # 500 inliers, 99 % outliers: the clique is the inlier set


def test_fused_estimators_match_the_separate_kernels():
    """estimate_fused_kernel (rotation + translation + inlier lists + state hand-over in one launch) against the three
    separate launches (option fused_estimators = 0): the GNC-TLS arithmetic is ordered identically, so R, the GNC cost, the
    iteration count and the rotation inliers are bit-identical; the translation comes from the window form of the scalar
    TLS (sorted values + prefix sums instead of the endpoint sweep): same estimate to ~1e-15, same inlier list.  Cliques of
    2 .. 512 vertices take the fast route, larger ones (and FGR / QUATRO / COMPLETE) the general route inside the kernel.
    The cliques here have roughly 5, 64, 150, 250, 360, 513 and 576 vertices; the size edges of both routes (2, 3, 255 ..
    258, 511, 512, 513, 1024, 1025) are in tests/test_gpu_estimator_edges.py, against the oracle too."""
    cases = [(300, 0.5, 31), (1200, 0.7, 32), (2500, 0.9, 33), (640, 0.1, 34), (9, 0.4, 35), (64, 0.0, 36), (513, 0.0, 37)]
    probs = [tp.synth_problem(9000 + seed, n, rho, 0.01) for n, rho, seed in cases]
    try:
        _fused_estimators_cases(cases, probs)
    finally:
        tp.set_option("fused_estimators", 1)


def _fused_estimators_cases(cases, probs):
    res = {}
    for mode in ("0", "1"):
        tp.set_option("fused_estimators", int(mode))
        s = make_solver(**bench_params())
        out = []
        for pr in probs:
            sol = s.solve(pr["src"], pr["dst"])
            raw = s.raw_solution()
            out.append((sol.rotation.copy(), sol.translation.copy(), s.getRotationInliers(), s.getTranslationInliers(),
                        raw.gnc_cost, raw.gnc_iterations, s.getInlierMaxClique()))
        sols = s.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
        out.append([(o.rotation.copy(), o.translation.copy()) for o in sols])
        res[mode] = out
    for k in range(len(probs)):
        a, b = res["0"][k], res["1"][k]
        assert a[6] == b[6]
        assert (a[0] == b[0]).all(), cases[k]
        assert a[2] == b[2] and a[4] == b[4] and a[5] == b[5]
        assert np.abs(a[1] - b[1]).max() <= 1e-13 * max(1.0, np.abs(a[1]).max()), (cases[k], a[1], b[1])
        assert a[3] == b[3]
        # batched = single, within a route
        for mode in ("0", "1"):
            assert (res[mode][-1][k][0] == res[mode][k][0]).all() and (res[mode][-1][k][1] == res[mode][k][1]).all()
    # FGR, QUATRO and COMPLETE TIMs: the general route
    for kw in (dict(rotation_estimation_algorithm=tp.RotationEstimationAlgorithm.FGR),
               dict(rotation_estimation_algorithm=tp.RotationEstimationAlgorithm.QUATRO),
               dict(rotation_tim_graph=tp.InlierGraphFormulation.COMPLETE)):
        got = {}
        for mode in ("0", "1"):
            tp.set_option("fused_estimators", int(mode))
            s = make_solver(**bench_params(**kw))
            sol = s.solve(probs[0]["src"], probs[0]["dst"])
            got[mode] = (sol.rotation.copy(), sol.translation.copy(), s.getRotationInliers(), s.getTranslationInliers())
        assert (got["0"][0] == got["1"][0]).all() and (got["0"][1] == got["1"][1]).all()
        assert got["0"][2] == got["1"][2] and got["0"][3] == got["1"][3]
    tp.set_option("fused_estimators", 1)


# ---------------------------------------------------------------------------------------------
# degree closure in front of the heuristic (kernels_heuristic.hip: degree_closure_kernel)
# ---------------------------------------------------------------------------------------------
def _solve_both_routes(probs, params):
    """Every problem alone and the whole list as one batch, with and without the degree closure."""
    got = {}
    try:
        for on in (1, 0):
            tp.set_option("deg_closure", on)
            s = make_solver(**params)
            single = []
            for pr in probs:
                sol = s.solve(pr["src"], pr["dst"])
                raw = s.raw_solution()
                single.append((bool(sol.valid), sol.rotation.copy(), sol.translation.copy(), s.getInlierMaxClique(),
                               s.getRotationInliers(), s.getTranslationInliers(), int(raw.colour_uncoloured),
                               int(raw.num_edges), int(raw.heuristic_size)))
            sols = s.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
            batch = [(bool(o.valid), o.rotation.copy(), o.translation.copy(), s.getInlierMaxClique(b),
                      s.getRotationInliers(b), s.getTranslationInliers(b), int(s.raw_solution(b).colour_uncoloured),
                      int(s.raw_solution(b).num_edges), int(s.raw_solution(b).heuristic_size))
                     for b, o in enumerate(sols)]
            got[on] = (single, batch)
    finally:
        tp.set_option("deg_closure", 1)
    return got


def test_degree_closure_matches_the_greedy_route_on_50_seeds():
    """The closure (omega <= h1 = max{k : #{H >= k - 1} >= k} with H the h-index of a vertex's neighbours' degrees; a
    (k - 1)-core of exactly k vertices IS the unique maximum clique: lb = ub as graph.cc:83-102) against the route without
    it (greedy starts, selection, peel, colouring bound, exact search): identical cliques, inlier lists, R and t, bit for
    bit -- on workloads it decides (marker colour_uncoloured = -2) and on workloads where it must decline: noise bounds
    at which the outliers' degrees exceed the clique's size, random graphs whose maximum clique is not unique, graphs
    without edges.  Where it decides, the oracle must agree that the maximum clique is unique, and on its content."""
    cases = []
    for k in range(30):   # the metric's regime at small sizes, several outlier rates
        # (at 95 % outliers and these sizes the degree bound h0 is far above the clique: R, cut at 7/8 of h0, misses it)
        cases.append((100 + 97 * k, [0.5, 0.8, 0.9, 0.95][k % 4], 0.01, True if k % 4 != 3 else None))
    for k in range(12):   # declined: every outlier's degree is above the clique size (the clique is not inside R)
        cases.append((1500 + 100 * k, 0.92, 0.05, False))
    for k in range(8):    # tiny problems, all-outlier problems (cliques of 2 .. 4 among random edges: seldom unique)
        cases.append(([2, 3, 5, 17, 64, 65, 128, 400][k], [0.0, 0.0, 0.4, 0.5, 1.0, 1.0, 1.0, 1.0][k], 0.01, None))
    assert len(cases) == 50
    probs = [tp.synth_problem(31000 + i, n, rho, nb) for i, (n, rho, nb, _) in enumerate(cases)]
    decided = 0
    for nb in (0.01, 0.05):
        idx = [i for i, c in enumerate(cases) if c[2] == nb]
        params = bench_params(noise_bound=nb)
        got = _solve_both_routes([probs[i] for i in idx], params)
        for j, i in enumerate(idx):
            for kind in (0, 1):  # single, batched
                a, b = got[1][kind][j], got[0][kind][j]
                assert b[6] != -2  # switched off means off
                assert a[0] == b[0] and len(a[3]) == len(b[3]) and a[7] == b[7], (cases[i], kind)
                if cases[i][3] is True:
                    assert a[6] == -2 and a[8] == len(a[3]), cases[i]
                elif cases[i][3] is False:
                    assert a[6] != -2, cases[i]
                if a[6] == -3:  # decided among several maximum cliques: the size is pinned (above), the content is not
                    assert cases[i][3] is not True and a[8] == len(a[3]), cases[i]
                elif a[6] == -2 or cases[i][3] is not None:  # (a maximum clique that is not unique is not pinned)
                    assert a[3] == b[3], (cases[i], kind)
                    if a[0]:
                        assert (a[1] == b[1]).all() and (a[2] == b[2]).all() and a[4] == b[4] and a[5] == b[5], (cases[i], kind)
                decided += int(a[6] == -2)
            a = got[1][0][j]
            if a[6] in (-2, -3) and cases[i][0] <= 1500:
                o = oracle.solve(probs[i]["src"], probs[i]["dst"], **oracle_params(params))
                if a[6] == -2:
                    assert o["clique_unique"] and o["max_clique"].tolist() == a[3], cases[i]
                else:
                    assert not o["clique_unique"] and len(o["max_clique"]) == len(a[3]), cases[i]
    assert decided >= 44


def test_degree_closure_decides_a_tie_between_maximum_cliques():
    """Headline shape, the one problem in ~200 the closure used to leave open: the (k - 1)-core has k + 1 vertices (an
    outlier consistent with every inlier but one), so there are two maximum cliques.  The closure now drops a minimum
    vertex cover of the core's missing edges (marker colour_uncoloured = -3): a maximum clique of the oracle's size,
    every pair of it an edge of the graph, the other route (closure off) agreeing on the size, and the oracle on the
    clique not being unique."""
    pr = tp.synth_problem(20250523 + 30, 10000, 0.95, 0.01)
    params = bench_params()
    got = _solve_both_routes([pr], params)
    a, b = got[1][0][0], got[0][0][0]
    assert a[6] == -3 and b[6] != -3 and b[6] != -2
    assert a[0] and b[0] and len(a[3]) == len(b[3]) == a[8] and a[7] == b[7]
    assert got[1][1][0][3] == a[3]  # batched = single
    s = make_solver(**params)
    s.solve(pr["src"], pr["dst"])
    bm = s.getInlierGraphBitmap()  # every pair of the clique is an edge of the graph
    members = np.array(a[3])
    for v in a[3]:
        bits = (bm[v, members >> 6] >> (members & 63).astype(np.uint64)) & np.uint64(1)
        assert int(bits.sum()) == len(a[3]) - 1
    o = oracle.solve(pr["src"], pr["dst"], **oracle_params(params))
    assert len(o["max_clique"]) == len(a[3]) and not o["clique_unique"]
    # the estimate is as good as the other route's: both cliques hold 499 of the same inliers
    assert np.linalg.norm(a[1] - b[1]) < 1e-3 and np.linalg.norm(a[2] - b[2]) < 1e-3


@pytest.mark.parametrize("skip_closed", [0, 1])
def test_degree_closure_switches_the_heuristic_launches_off_and_on(skip_closed):
    """Default (heu_skip_closed = 0): greedy / select / peel are always enqueued behind the closure (their workgroups
    return at once for a decided problem), with every start of an open problem in a workgroup of its own once the
    previous batch had few open problems.  heu_skip_closed = 1: a handle whose previous batch was decided entirely by
    the closure does not enqueue them for the next one; a problem the closure then leaves open is served by the finish
    half (one more round trip) and switches the launches back on.  Whatever the history and the setting, results equal
    those of a fresh handle."""
    easy = [tp.synth_problem(32000 + i, 900 + 50 * i, 0.3, 0.05) for i in range(4)]
    hard = [tp.synth_problem(32100 + i, 1800, 0.92, 0.05) for i in range(2)]
    params = bench_params(noise_bound=0.05)

    def solve(s, probs):
        sols = s.solve_batch([p["src"] for p in probs], [p["dst"] for p in probs])
        return [(o.rotation.copy(), o.translation.copy(), s.getInlierMaxClique(b), int(s.raw_solution(b).colour_uncoloured))
                for b, o in enumerate(sols)]

    def same(a, b):
        return all((x[0] == y[0]).all() and (x[1] == y[1]).all() and x[2] == y[2] and x[3] == y[3] for x, y in zip(a, b))

    want_easy = solve(make_solver(**params), easy)
    want_mixed = solve(make_solver(**params), easy[:2] + hard)
    assert all(w[3] == -2 for w in want_easy) and [w[3] == -2 for w in want_mixed] == [True, True, False, False]
    tp.set_option("heu_skip_closed", skip_closed)
    try:
        s = make_solver(**params)
        s.set_profiling(1)
        assert same(solve(s, easy), want_easy)             # first batch: launches enqueued (nothing known yet), all skipped
        assert same(solve(s, easy), want_easy)             # second: not enqueued at all when skip_closed
        t_skip = s.get_profile()["peel_ms"]
        assert (t_skip == 0.0) == bool(skip_closed)
        assert same(solve(s, easy[:2] + hard), want_mixed)  # open problems (skip_closed: the finish half runs the stage)
        assert s.get_profile()["peel_ms"] > 0.0
        assert same(solve(s, easy[:2] + hard), want_mixed)  # enqueued up front again
        assert same(solve(s, easy), want_easy)
    finally:
        tp.set_option("heu_skip_closed", 0)
