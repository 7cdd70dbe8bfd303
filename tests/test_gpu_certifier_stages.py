"""The certifier's device kernels (csrc/kernels_certify.hip) stage by stage against the oracle (oracle/certifier.py) and
the longdouble restatement of tests/certifier_reference.py:
  * the projection onto the affine dual subspace (teaser_hip_certify_dual_projection: the five launches of the loop)
    elementwise, with forward error bounds gamma_k sum|terms| whose operation counts k stand beside the assertions;
  * the matrices of one iteration of the loop itself (teaser_hip_certify_stages), each kernel's output recomputed from
    the GPU's own captured inputs;
  * whole sub-optimality trajectories at the launch-geometry edges (N + 1 = 64, 65, 128, 129, 130; N = 1, 2, 3), with
    mislabelled theta, one iteration, gamma_tau = 1 and a threshold that decides the stop index.
Not covered: the branch for an eigendecomposition that does not converge (info != 0 -> gap = +inf); reaching it needs
input that makes the solver fail."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import certifier_reference as CR
from oracle import certifier as CO

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "certifier_golden.npz"))
TOL = 1e-7  # certification-test.cc:29, the CSV precision of the fixtures
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


@pytest.fixture(scope="module")
def cert():
    return tp.DRSCertifier()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def thetas(N, rng):
    one = -np.ones(N)
    one[rng.integers(N)] = 1.0
    return dict(random=rng.choice([-1.0, 1.0], size=N), inliers=np.ones(N), outliers=-np.ones(N), single=one)


def random_instance(rng, n, out_frac=0.25, nb=0.02):
    """As test_gpu_certifier.py::test_certify_random_instances_vs_oracle (certification-test.cc:527-584) builds them."""
    src = rng.uniform(-1, 1, size=(3, n))
    Rm = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    if np.linalg.det(Rm) < 0:
        Rm[:, 0] = -Rm[:, 0]
    dst = Rm @ src + rng.uniform(-nb / 2, nb / 2, size=(3, n))
    mask = rng.uniform(size=n) >= out_frac
    dst[:, ~mask] = rng.uniform(-1, 1, size=(3, int((~mask).sum())))
    return dict(R=Rm, src=src, dst=dst, theta=np.where(mask, 1.0, -1.0), nb=nb, cbar2=1.0, iters=40)


def fixture_instance(kind, c):
    g = lambda n: G["%s%d_%s" % (kind, c, n)]
    nb, cbar2, iters = g("params")
    return dict(R=g("R_est"), src=g("v1"), dst=g("v2"), theta=g("theta_est").reshape(-1), nb=float(nb),
                cbar2=float(cbar2), iters=int(iters))


def stage_instance(name):
    if name.startswith("random"):
        n = int(name[6:])
        return random_instance(np.random.default_rng(500 + n), n)
    return fixture_instance(name[:5], int(name[5:]))


# ---- the dual projection: kernels against the reference ------------------------------------------------------------

def check_projection(got, ref, terms, N, tag):
    """|gpu - ref| <= gamma_k sum|terms| elementwise; k = the floating-point operations on the path to the element."""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD)).astype(np.float64)
    t = np.asarray(terms, dtype=np.float64)
    cls = CR.element_classes(N)
    worst = {k: float((err[m] / np.maximum(t[m], 1e-300)).max() / (EPS / 2)) for k, m in cls.items()}
    print("dual projection %s N=%d: largest |gpu - ref| / (u sum|terms|) per class: %s" % (tag, N, worst))
    # 3 x 3 parts and corners of the off-diagonal blocks, (W_rc - W_cr) / 2: one subtraction (the halving is exact); k = 2
    assert (err[cls["off33"]] <= CR.gamma(2) * t[cls["off33"]]).all(), worst
    # their last rows / columns, the 3-vectors of A_inv b_W: the four sums of cert_ainv_apply_kernel hold at most 2N terms,
    # each with a three-multiply factor, on the four-term b_W; k = 4N + 12
    assert (err[cls["offborder"]] <= CR.gamma(4 * N + 12) * t[cls["offborder"]]).all(), worst
    # last rows / columns of the diagonal blocks: the row sum over N + 1 of those 3-vectors and the product with theta_i;
    # k = (4N + 12) + (N + 2)
    assert (err[cls["diagborder"]] <= CR.gamma(4 * N + 12 + N + 2) * t[cls["diagborder"]]).all(), worst
    # 3 x 3 parts of the diagonal blocks, W_ii - mean: N additions, one division, one subtraction (N + 2 <= 2N + 2);
    # k = 2N + 2
    assert (err[cls["diag33"]] <= CR.gamma(2 * N + 2) * t[cls["diag33"]]).all(), worst


def check_structure(cert, got, W, theta, N):
    """What needs no tolerance (and the diagonal blocks' sum, whose bound is (N + 1) eps sum|entries|)."""
    n = 4 * N + 4
    cls = CR.element_classes(N)
    # symmetric bit for bit: block (j, i) is written as the transpose of block (i, j) from the same register, and the
    # last row / column of a diagonal block from one expression.  (The diagonal blocks' 3 x 3 parts are W's own minus the
    # mean: as symmetric as W is -- test_dual_projection_of_a_symmetric_w.)
    m = ~cls["diag33"]
    assert np.array_equal(bits(got)[m], bits(got.T)[m])
    B = np.asarray(got).reshape(N + 1, 4, N + 1, 4).transpose(0, 2, 1, 3)  # [block row, block column, r, c]
    off = ~np.eye(N + 1, dtype=bool)
    blk = B[off]
    # every off-diagonal block: antisymmetric 3 x 3 part, border [y; -y^T], zero corner (certification.cc:381-419)
    assert np.array_equal(blk[:, :3, :3], -blk[:, :3, :3].transpose(0, 2, 1))
    assert np.array_equal(blk[:, :3, 3], -blk[:, 3, :3])
    assert (blk[:, 3, 3] == 0).all()
    assert N < 2 or np.abs(blk[:, :3, 3]).min() > 0  # (not vacuous: the borders are filled)
    # the diagonal blocks' 3 x 3 parts sum to zero (the mean was subtracted) within (N + 1) eps sum|entries|, the entries
    # being those the mean is taken of, W's: the sum and the division are N + 1 operations on them (the division is exact
    # for N = 1), each subtraction one more on |W_ii - mean| <= |W_ii| + |mean|: at most (N + 4) u sum|W_ii| <=
    # (2N + 2) u sum|W_ii| from N = 2 on, 3 u sum|W_ii| for N = 1.  (Measured in W_dual's own entries the bound is missed
    # by the oracle's FP64 output itself at N = 1: where W_ii nearly equals the mean, the mean's rounding is all that is left.)
    d = np.arange(N + 1)
    d33 = B[d, d][:, :3, :3].astype(LD)
    w33 = np.asarray(W).reshape(N + 1, 4, N + 1, 4).transpose(0, 2, 1, 3)[d, d][:, :3, :3].astype(LD)
    assert (np.abs(d33.sum(axis=0)) <= (N + 1) * EPS * np.abs(w33).sum(axis=0)).all()
    # two calls give the same bytes
    again = cert.dual_projection(W, theta)
    assert np.array_equal(bits(again), bits(got))
    assert got.shape == (n, n)


@pytest.mark.parametrize("c", [1, 2, 3])
def test_dual_projection_reference_fixtures(cert, c):
    """getOptimalDualProjection of the reference's own W_1st_iter (certification-test.cc's check, its tolerance)."""
    g = lambda n: G["small%d_%s" % (c, n)]
    got = cert.dual_projection(g("W_1st_iter"), g("theta_est").reshape(-1))
    assert np.abs(got - g("W_dual_1st_iter")).max() < TOL


@pytest.mark.parametrize("N", [1, 2, 3, 62, 63, 64, 65, 127, 128, 129])
def test_dual_projection_vs_dense_oracle(cert, N):
    rng = np.random.default_rng(2000 + N)
    n = 4 * N + 4
    W = rng.normal(size=(n, n))  # not symmetric: the blocks below the diagonal must not be read
    theta = rng.choice([-1.0, 1.0], size=N)
    got = cert.dual_projection(W, theta)
    ref, terms = CR.dual_projection_dense(W, np.concatenate([[1.0], theta]))
    check_projection(got, ref, terms, N, "dense")
    check_structure(cert, got, W, theta, N)


@pytest.mark.parametrize("N", [300, 1000])
def test_dual_projection_vs_structured_restatement(cert, N):
    rng = np.random.default_rng(3000 + N)
    n = 4 * N + 4
    W = rng.normal(size=(n, n))
    theta = rng.choice([-1.0, 1.0], size=N)
    got = cert.dual_projection(W, theta)
    ref, terms = CR.dual_projection_structured(W, np.concatenate([[1.0], theta]))
    check_projection(got, ref, terms, N, "structured")
    del ref, terms
    check_structure(cert, got, W, theta, N)


@pytest.mark.parametrize("kind", ["inliers", "outliers", "single"])
@pytest.mark.parametrize("N", [64, 129])
def test_dual_projection_theta_edges(cert, N, kind):
    rng = np.random.default_rng(4000 + N)
    n = 4 * N + 4
    theta = thetas(N, rng)[kind]
    W = rng.normal(size=(n, n))
    got = cert.dual_projection(W, theta)
    ref, terms = CR.dual_projection_dense(W, np.concatenate([[1.0], theta]))
    check_projection(got, ref, terms, N, kind)
    check_structure(cert, got, W, theta, N)


def test_dual_projection_of_a_symmetric_w(cert):
    """With an exactly symmetric W (what the loop feeds it up to rounding) all of W_dual is symmetric bit for bit: the
    mean's entries (r, c) and (c, r) are the same sums in the same order."""
    N = 65
    rng = np.random.default_rng(5)
    W = rng.normal(size=(4 * N + 4, 4 * N + 4))
    W = W + W.T
    got = cert.dual_projection(W, rng.choice([-1.0, 1.0], size=N))
    assert np.array_equal(bits(got), bits(got.T)) and np.abs(got).max() > 0


def test_dual_projection_refusals(cert):
    """Null pointers, n < 1, n > 8000, a non-finite W and a theta that is not +-1 are refused with a message that names
    the argument; the handle works afterwards."""
    s = cert._solver
    L, h = s._lib, s._h
    W = np.zeros((8, 8))
    th = np.ones(1)
    out = np.zeros((8, 8))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    err = lambda: L.teaser_hip_last_error(h).decode()
    assert L.teaser_hip_certify_dual_projection(None, p(W), p(th), 1, p(out)) == 1
    assert L.teaser_hip_certify_dual_projection(h, None, p(th), 1, p(out)) == 1 and "W is NULL" in err()
    assert L.teaser_hip_certify_dual_projection(h, p(W), None, 1, p(out)) == 1 and "theta is NULL" in err()
    assert L.teaser_hip_certify_dual_projection(h, p(W), p(th), 1, None) == 1 and "W_dual is NULL" in err()
    assert L.teaser_hip_certify_dual_projection(h, p(W), p(th), 0, p(out)) == 1 and "n must be >= 1" in err()
    assert L.teaser_hip_certify_dual_projection(h, p(W), p(th), 8001, p(out)) == 4 and "more than 8000" in err()  # (n is checked before W is read)
    for bad in (np.nan, np.inf):
        Wb = W.copy()
        Wb[5, 2] = bad
        with pytest.raises(tp.TeaserHipError, match="W has a non-finite entry"):
            cert.dual_projection(Wb, th)
    for bad in (0.0, 0.5, np.nan, 2.0):
        with pytest.raises(tp.TeaserHipError, match="theta has an entry"):
            cert.dual_projection(W, np.array([bad]))
    with pytest.raises(ValueError):
        cert.dual_projection(np.zeros((8, 9)), th)
    rng = np.random.default_rng(1)
    W = rng.normal(size=(8, 8))
    ref, terms = CR.dual_projection_dense(W, np.array([1.0, 1.0]))
    check_projection(cert.dual_projection(W, th), ref, terms, 1, "after refusals")


# ---- the matrices of one iteration of the loop -----------------------------------------------------------------------

# numpy's eigh with UPLO="L" against UPLO="U" in nearest_psd: the largest elementwise difference over the M entering the
# first and the last iteration of every case below (the oracle's own M); measured on the CPU, see test_stages
PSD_SPREAD = 3.98e-13
STAGE_CASES = ["small1", "small3", "large1", "random1", "random63", "random64", "random65", "random129"]


def nearest_psd_uplo(A, uplo):
    """oracle.certifier.nearest_psd with the triangle numpy's eigh reads made explicit."""
    w, V = np.linalg.eigh((A + A.T) / 2, UPLO=uplo)
    return (V * np.where(w < 0, 0.0, w)) @ V.T


def check_stage(cert, inst, st, traj, it, M_init_gpu, mu, stopped):
    N = inst["src"].shape[1]
    n = 4 * N + 4
    M, P, W, Wd, Ma, Mo = (np.ascontiguousarray(st[k]) for k in ("M_in", "M_psd", "W", "W_dual", "M_affine", "M_out"))
    Ml, Pl, Wl, Wdl, Mal, Il = (a.astype(LD) for a in (M, P, W, Wd, Ma, M_init_gpu))
    # cert_w_kernel: W = 2 M_psd - M - M_init, at most three rounded operations (contraction allowed): 4 eps sum|operands|
    assert (np.abs(Wl - (2 * Pl - Ml - Il)) <= 4 * EPS * (2 * np.abs(Pl) + np.abs(Ml) + np.abs(Il))).all()
    # cert_affine_kernel: M_affine = M_init + W_dual
    assert (np.abs(Mal - (Il + Wdl)) <= 4 * EPS * (np.abs(Il) + np.abs(Wdl))).all()
    # cert_update_kernel: M += gamma (M_affine - M_psd); not launched where the loop stopped
    if stopped:
        assert np.array_equal(bits(Mo), bits(M))
    else:
        g = LD(cert.params.gamma_tau)
        assert (np.abs(Mo.astype(LD) - (Ml + g * (Mal - Pl))) <= 4 * EPS * (np.abs(Ml) + g * (np.abs(Mal) + np.abs(Pl)))).all()
        assert not np.array_equal(Mo, M)
    # the projection inside the loop is the projection entry: same launches, same bytes
    assert np.array_equal(bits(cert.dual_projection(W, inst["theta"])), bits(Wd))
    # nearest PSD matrix (cert_sym_kernel, rocSOLVER dsyevd, cert_scale_kernel, rocBLAS dgemm) against the oracle's
    ref = CO.nearest_psd(M)
    norm2 = float(np.linalg.norm(M, 2))
    bar = max(10 * PSD_SPREAD, n * EPS * norm2)
    psd_err = float(np.abs(P - ref).max())
    asym = float(np.abs(P - P.T).max())
    S = (Ml + Ml.T) / 2
    inner = float(abs((Pl * (S - Pl)).sum()))
    normF = float(np.linalg.norm(M))
    print("stage it=%d n=%d: |M_psd - oracle| %.3g (bar %.3g, ||M||_2 %.3g); asymmetry %.3g (bar %.3g); <M_psd, sym(M) - M_psd> "
          "%.3g (bar %.3g)" % (it, n, psd_err, bar, norm2, asym, 2 * EPS * np.abs(P).max(), inner, bar * normF))
    assert psd_err <= bar
    assert asym <= 2 * EPS * np.abs(P).max()
    assert inner <= bar * normF
    # the gap of the trajectory is that of the captured M_affine: D[0], (N + 1) / mu and the clamp to zero
    assert abs(CO.suboptimality_gap(Ma, mu, N) - traj[it]) < TOL


@pytest.mark.parametrize("name", STAGE_CASES)
def test_stages(cert, name):
    """The matrices of iteration 0 and of the last executed iteration, out of the launches of the run itself.

    Derived bars stand beside their assertions in check_stage.  Measured, against the reference side only: M_psd
    against the oracle's nearest_psd of the captured M involves two eigensolvers.  Two CPU evaluations of nearest_psd
    of the same M (numpy's eigh with UPLO="L" and UPLO="U"), on the M entering the first and the last iteration of the
    oracle's run of each of the eight cases, differ elementwise by at most 3.98e-13 (random129, iteration 0, ||M||_2 =
    94; 1.1e-14 for small1); relative to ||M||_2 by at most 4.2e-15.  The bar is ten times that, 3.98e-12 (the factor
    allows for a third solver, rocSOLVER), and not below n eps ||M||_2 (1.1e-11 for random129, 6.1e-12 for large1).
    The orthogonality check <M_psd, sym(M) - M_psd> uses that bar times ||M||_F; 2 eps max|M_psd| ||M||_F in its place
    is missed by numpy's own nearest_psd (2.7e-11 against 5.7e-12 for random129), so it cannot be meant."""
    inst = stage_instance(name)
    N = inst["src"].shape[1]
    c = tp.DRSCertifier(noise_bound=inst["nb"], cbar2=inst["cbar2"], max_iterations=inst["iters"])
    args = (inst["R"], inst["src"], inst["dst"], inst["theta"])
    plain = c.certify(*args)
    traj = plain.suboptimality_traj
    last = len(traj) - 1
    assert last >= 0
    M_init, mu = CR.dense_minit(inst["R"], inst["src"], inst["dst"], inst["theta"], inst["nb"], inst["cbar2"])
    res0, st0 = c.certify_stages(*args, 0)
    # with and without capture: the same trajectory, bit for bit
    assert np.array_equal(bits(res0.suboptimality_traj), bits(traj))
    assert res0.is_optimal == plain.is_optimal and res0.best_suboptimality == plain.best_suboptimality
    # cert_init_kernel / minit(): M entering iteration 0 is M_init (the bar of test_cert_setup_blocks_vs_oracle), and
    # exactly zero outside the first block row, the first block column and the diagonal blocks
    M0 = np.ascontiguousarray(st0["M_in"])
    assert np.abs(M0 - M_init).max() <= 1e-11 * max(1.0, np.abs(M_init).max())
    blk = np.arange(4 * N + 4) // 4
    outside = (blk[:, None] != blk[None, :]) & (blk[:, None] != 0) & (blk[None, :] != 0)
    assert (M0[outside] == 0).all() and (M0 != 0).sum() >= 16 * (N + 1)
    stopped = traj[last] < c.params.sub_optimality
    check_stage(c, inst, st0, traj, 0, M0, mu, stopped and last == 0)
    if last > 0:
        res1, st1 = c.certify_stages(*args, last)
        assert np.array_equal(bits(res1.suboptimality_traj), bits(traj))
        check_stage(c, inst, st1, traj, last, M0, mu, stopped)
    # an iteration the run never reaches is refused, naming the argument; the handle works afterwards
    with pytest.raises(tp.TeaserHipError, match="iteration %d was not reached" % (last + 1)) as e:
        c.certify_stages(*args, last + 1)
    assert e.value.status == 1
    with pytest.raises(tp.TeaserHipError, match="iteration must be >= 0"):
        c.certify_stages(*args, -1)
    assert np.array_equal(bits(c.certify(*args).suboptimality_traj), bits(traj))


# ---- whole trajectories at the shapes the suite lacked ------------------------------------------------------------------

def check_trajectory(inst, theta=None, **params):
    theta = inst["theta"] if theta is None else theta
    kw = dict(noise_bound=inst["nb"], cbar2=inst["cbar2"], max_iterations=inst["iters"])
    kw.update(params)
    got = tp.DRSCertifier(**kw).certify(inst["R"], inst["src"], inst["dst"], theta)
    ref = CO.certify(inst["R"], inst["src"], inst["dst"], theta, **kw)
    assert got.suboptimality_traj.shape == ref["suboptimality_traj"].shape
    assert np.abs(got.suboptimality_traj - ref["suboptimality_traj"]).max() < TOL
    assert got.is_optimal == ref["is_optimal"]
    return got, ref


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 128, 129])
def test_trajectory_at_geometry_edges(N):
    check_trajectory(random_instance(np.random.default_rng(600 + N), N))


@pytest.mark.parametrize("kind", ["inliers", "outliers", "wrong"])
def test_trajectory_with_mislabelled_theta(kind):
    """theta all +1, all -1, and wrong on purpose (every label flipped: inliers called outliers), which does not certify
    and runs cert_update_kernel max_iterations - 1 times."""
    inst = random_instance(np.random.default_rng(664), 64)
    theta = dict(inliers=np.ones(64), outliers=-np.ones(64), wrong=-inst["theta"])[kind]
    got, _ = check_trajectory(inst, theta)
    if kind == "wrong":
        assert len(got.suboptimality_traj) == inst["iters"] and not got.is_optimal


@pytest.mark.parametrize("gamma_tau", [1.0, 1.999999])
@pytest.mark.parametrize("max_iterations", [1, 25])
def test_trajectory_params(max_iterations, gamma_tau):
    inst = fixture_instance("small", 2)
    got, _ = check_trajectory(inst, max_iterations=max_iterations, gamma_tau=gamma_tau)
    assert len(got.suboptimality_traj) <= max_iterations


def test_threshold_decides_the_stop_index():
    """sub_optimality between two consecutive values of the oracle's trajectory, both at least 1e-5 away from it: the
    1e-7 agreement cannot move the stop."""
    inst = fixture_instance("small", 1)
    full = CO.certify(inst["R"], inst["src"], inst["dst"], inst["theta"], noise_bound=inst["nb"], cbar2=inst["cbar2"],
                      max_iterations=inst["iters"])["suboptimality_traj"]
    k = len(full) // 2
    thr = (full[k - 1] + full[k]) / 2
    assert k >= 2 and full[:k].min() >= thr + 1e-5 and full[k] <= thr - 1e-5 and thr > 1e-3
    got, ref = check_trajectory(inst, sub_optimality=thr)
    assert len(ref["suboptimality_traj"]) == k + 1 and len(got.suboptimality_traj) == k + 1 and got.is_optimal


def test_no_correspondences_and_too_many():
    c = tp.DRSCertifier()
    got = c.certify(np.eye(3), np.zeros((3, 0)), np.zeros((3, 0)), np.zeros(0))
    assert len(got.suboptimality_traj) == 0 and got.is_optimal is False
    z = np.zeros((3, 8001))
    with pytest.raises(tp.TeaserHipError, match="teaser_hip_certify: more than 8000 correspondences") as e:
        c.certify(np.eye(3), z, z, np.ones(8001))
    assert e.value.status == 4
    with pytest.raises(tp.TeaserHipError, match="teaser_hip_certify_stages: more than 8000 correspondences"):
        c.certify_stages(np.eye(3), z, z, np.ones(8001), 0)
    with pytest.raises(tp.TeaserHipError, match="iteration 0 was not reached"):
        c.certify_stages(np.eye(3), np.zeros((3, 0)), np.zeros((3, 0)), np.zeros(0), 0)
