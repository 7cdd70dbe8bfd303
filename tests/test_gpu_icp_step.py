"""One ICP step of every estimation method on the MI355X against the 50-digit reference (tests/icp_step_reference.py,
fixture tests/golden/icp_step_golden.npz): with max_iteration = 1 and forced correspondences the result's
transformation is U init, so Umeyama through svd_rot3, the 6 x 6 LDL^T and Generalized ICP's per-pair W are seen one
step at a time, at degenerate inputs and at the sums' own granularity (256 source points per block, the 4-wave block
sum, the finalize loop that strides the block partials by 256).  Every input is a small dyadic rational, so the sums
are exact in any order and an exactly singular system is exactly singular on the device.

Bars.  For a case with a unique answer ||T_gpu - T_golden||_F <= 16 max(A, B): A the error of the project's FP64 CPU
restatement against the 50-digit step on that case (measured on the CPU, stored in the fixture), B = 2^-52 times the
case's condition (s0 / (s1 + d s2) for Umeyama, cond(A) for the 6 x 6 solves; every one asserted <= 1e3 by the
reference); 16 covers a different, equally valid operation order (Jacobi against LAPACK).  Per case, as the fixture's
generator prints them (A; condition; bar):
  pt_3_triangle 8.1e-16 4.0 1.4e-14    pt_4_coplanar 4.6e-16 4.1 1.5e-14    pt_64 4.1e-16 0.50 6.5e-15
  pt_mirror_slab 6.6e-16 2.3 1.1e-14   pt_isotropic 0 0.50 1.8e-15
  pl_patch 9.9e-17 119 4.2e-13         pl_zero_residuals 0 119 4.2e-13      pl_huber_edge 1.2e-16 115 4.1e-13
  pl_tukey_edge 1.7e-16 213 7.6e-13    pl_cauchy 3.9e-16 114 4.1e-13        pl_gm 2.7e-16 112 4.0e-13
  gi_regular 1.7e-16 2.7 9.6e-15       gi_mixed_singular 1.9e-16 2.8 9.9e-15
  gpt_255 6.0e-16 0.82 9.7e-15         gpt_256 1.2e-15 0.81 1.8e-14         gpt_257 8.5e-16 0.82 1.4e-14
  gpt_513 4.6e-16 0.51 7.3e-15         gpt_768_gap 1.4e-15 0.96 2.2e-14     gpt_65793 6.5e-16 0.53 1.0e-14
  gpl_255 4.6e-16 71 2.5e-13           gpl_256 1.2e-16 71 2.5e-13           gpl_257 2.2e-16 72 2.5e-13
  gpl_513 1.2e-16 79 2.8e-13           gpl_768_gap 1.0e-16 279 9.9e-13      gpl_65793 8.6e-17 281 1.0e-12
  ggi_255 2.0e-16 10 3.7e-14           ggi_256 2.1e-16 11 3.7e-14           ggi_257 1.5e-16 11 3.9e-14
  ggi_513 9.3e-17 11 3.9e-14           ggi_768_gap 1.4e-16 43 1.5e-13
Exact-identity, bit-equality and scaling checks take no tolerance.  Where R is not unique (rank(H) <= 1) the test
asserts a maximiser: R^T R = I and det R = 1 to 1e-12, R H symmetric and tr(R H) = s0 to 1e-12 s0 (the asymmetry of
R H is first order in the angle between R u0 and v0, so the same 1e-12 holds it), t = mu_Q - R mu_P, and R = I exactly
for H = 0.

Not built: the header's remark that W = n n^T gives the point-to-plane step cannot be reached through the API, because
W = adj(M) / det(M) has full rank whenever the pair contributes at all."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import icp_step_reference as S
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")

G = np.load(os.path.join(ROOT, "tests", "golden", "icp_step_golden.npz"))
NAMES = [str(n) for n in G["names"]]
KIND = dict(zip(NAMES, [str(k) for k in G["kinds"]]))
UNIQUE = [n for n in NAMES if KIND[n] == "unique"]
IDENTITY = [n for n in NAMES if KIND[n] == "identity"]
MAXIMISER = [n for n in NAMES if KIND[n] == "maximiser"]
GRANULARITY = [n for n in NAMES if n[0] == "g" and n[:3] != "gi_"]
BIG = {"gpt_65793": S.POINT, "gpl_65793": S.PLANE}
assert sorted(UNIQUE + IDENTITY + MAXIMISER) == sorted(NAMES) and set(BIG) <= set(UNIQUE)  # no case left out
LOSS = (None, tp.HuberLoss, tp.CauchyLoss, tp.GMLoss, tp.TukeyLoss)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


_cases, _results = {}, {}


def case(name):
    """The case's inputs: from the fixture, or regenerated from its formula (the two 65 793-point cases)."""
    if name not in _cases:
        if name in BIG:
            c = S.big_case(BIG[name])
        else:
            method, kernel, stored = (int(v) for v in G[name + "/meta"])
            assert stored
            get = lambda key: G[name + "/" + key] if name + "/" + key in G.files else None
            c = dict(name=name, method=method, kernel=kernel, P=G[name + "/P"], Q=G[name + "/Q"],
                     init=G[name + "/init"], N=get("N"), Cs=get("Cs"), Ct=get("Ct"), r=float(G[name + "/rk"][0]),
                     k=float(G[name + "/rk"][1]))
        _cases[name] = c
    return _cases[name]


def estimation(c):
    if c["method"] == S.POINT:
        return tp.TransformationEstimationPointToPoint()
    if c["method"] == S.PLANE:
        return tp.TransformationEstimationPointToPlane(None if c["kernel"] == 0 else LOSS[c["kernel"]](c["k"]))
    return tp.TransformationEstimationForGeneralizedICP()


ONE = tp.ICPConvergenceCriteria(max_iteration=1)


def run(c, scale=1.0):
    init = c["init"].copy()
    init[:3, 3] *= scale
    out = tp.registration_icp(c["P"] * scale, c["Q"] * scale, c["r"] * scale, init, estimation(c), ONE,
                              target_normals=c["N"], source_covariances=c["Cs"], target_covariances=c["Ct"])
    assert out.iterations == 1
    return out


def result(name):
    """One single run per case, shared by the tests that need it."""
    if name not in _results:
        _results[name] = run(case(name))
    return _results[name]


def matches(name):
    if name in BIG:
        return np.arange(S.BIG_N, dtype=np.int32)
    return G[name + "/match"]


def check_pass(name, out):
    """Fitness, RMSE and the correspondence set of the pass after the step, where the reference showed that it sees the
    correspondences of the pass before it."""
    if not bool(G[name + "/keeps"]):
        return
    j = matches(name)
    src = np.nonzero(j >= 0)[0]
    assert out.fitness == float(G[name + "/fitness"])
    assert np.array_equal(out.correspondence_set, np.stack([src, j[src]], 1))


def check_rigid(T):
    assert np.isfinite(T).all()
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    Rm = T[:3, :3]
    assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rm) - 1.0) <= 1e-12


def bar_of(name):
    a, cond = float(G[name + "/err_fp64"]), float(G[name + "/cond"])
    assert np.isfinite(a) and cond <= S.COND_MAX
    return 16.0 * max(a, 2.0 ** -52 * cond)


def check_unique(name, out):
    err, bar = np.linalg.norm(out.transformation - G[name + "/T"]), bar_of(name)
    print("%s: |dT| %.3g  bar %.3g  (A %.3g, condition %.3g)" % (name, err, bar, float(G[name + "/err_fp64"]),
                                                                float(G[name + "/cond"])))
    check_rigid(out.transformation)
    assert err <= bar
    check_pass(name, out)


@pytest.mark.parametrize("name", UNIQUE)
def test_step_matches_the_50_digit_reference(name):
    out = result(name)
    check_unique(name, out)
    if name == "pl_zero_residuals":  # g = 0: xi = 0 and the step is the identity, exactly
        assert np.array_equal(out.transformation, np.eye(4))
    if name == "pt_isotropic":  # H = 2 I
        assert np.array_equal(out.transformation[:3, :3], np.eye(3))
    if name == "pt_mirror_slab":
        assert int(G[name + "/d"]) == -1 and G[name + "/sv"][1] > G[name + "/sv"][2] > 0
    if name == "gi_mixed_singular":  # the singular pairs count for fitness and RMSE and add nothing to U
        assert int(G[name + "/skipped"]) == 21 and out.fitness == 1.0 and len(out.correspondence_set) == 64


@pytest.mark.parametrize("name", IDENTITY)
def test_exactly_singular_systems_give_the_exact_identity(name):
    c, out = case(name), result(name)
    assert bool(G[name + "/exact"])
    assert np.array_equal(out.transformation, c["init"])
    check_pass(name, out)  # U = I: the pass after the step IS the pass before it
    assert bool(G[name + "/keeps"])
    rmse = float(G[name + "/rmse"])
    assert abs(out.inlier_rmse - rmse) <= 2 * np.spacing(rmse)
    if name == "gi_all_singular":
        assert int(G[name + "/skipped"]) == 64 and out.fitness == 1.0


def check_maximiser(name, T, scale=1.0):
    """rank(H) <= 1: any proper rotation that maximises tr(R H), and the translation that goes with it."""
    check_rigid(T)
    H, s0 = G[name + "/H"] * scale * scale, float(G[name + "/sv"][0]) * scale * scale
    mu_p, mu_q = G[name + "/mu_p"] * scale, G[name + "/mu_q"] * scale
    Rm = T[:3, :3]
    RH = Rm @ H
    assert int(G[name + "/rank"]) <= 1
    assert np.abs(RH - RH.T).max() <= 1e-12 * s0 and abs(np.trace(RH) - s0) <= 1e-12 * s0
    size = max(np.abs(mu_p).max(), np.abs(mu_q).max(), scale)
    assert np.abs(T[:3, 3] - (mu_q - Rm @ mu_p)).max() <= 1e-12 * size
    if int(G[name + "/rank"]) == 0:
        assert np.array_equal(Rm, np.eye(3))


@pytest.mark.parametrize("name", MAXIMISER)
def test_rank_deficient_cross_covariance_gives_a_maximiser(name):
    check_maximiser(name, result(name).transformation)


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("pt_")])
@pytest.mark.parametrize("exponent", [60, -60])
def test_point_to_point_scales_exactly_with_a_power_of_two(name, exponent):
    base = result(name).transformation
    s = 2.0 ** exponent
    T = run(case(name), s).transformation
    assert T[:3, :3].tobytes() == base[:3, :3].tobytes()
    assert np.array_equal(T[:3, 3], base[:3, 3] * s) and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])


def test_granularity_cases_keep_their_bits_inside_one_mixed_batch():
    names = GRANULARITY
    assert len(names) == 23 and set(BIG) <= set(names)
    cs = [case(n) for n in names]
    batch = tp.registration_icp_batch([c["P"] for c in cs], [c["Q"] for c in cs], [c["r"] for c in cs],
                                      np.array([c["init"] for c in cs]), ONE,
                                      estimation_methods=[estimation(c) for c in cs],
                                      target_normals=[c["N"] for c in cs],
                                      source_covariances=[c["Cs"] for c in cs],
                                      target_covariances=[c["Ct"] for c in cs])
    for n, got in zip(names, batch):
        alone = result(n)
        assert got.transformation.tobytes() == alone.transformation.tobytes(), n
        assert got.fitness == alone.fitness and got.inlier_rmse == alone.inlier_rmse, n
        assert np.array_equal(got.correspondence_set, alone.correspondence_set), n


def solve_cov(cs):
    """teaser_hip_icp_batch_cov directly on a list of cases: the transformations."""
    L = tp.lib()
    h, lock = tp.icp._handle(-1)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    b = len(cs)
    keep = [{k: None if c[k] is None else np.ascontiguousarray(c[k], dtype=np.float64)
             for k in ("P", "Q", "N", "Cs", "Ct")} for c in cs]
    n_s = np.array([len(c["P"]) for c in cs], dtype=np.int32)
    n_t = np.array([len(c["Q"]) for c in cs], dtype=np.int32)
    init = np.ascontiguousarray(np.array([c["init"] for c in cs]))
    par = (tp.icp.IcpParamsC * b)(*[tp.icp.IcpParamsC(c["r"], 1, 1e-6, 1e-6) for c in cs])
    est = (tp.icp.IcpEstimationC * b)(*[tp.icp.IcpEstimationC(c["method"], c["kernel"], c["k"]) for c in cs])
    out = (tp.icp.IcpResultC * b)()
    with lock:
        rc = L.teaser_hip_icp_batch_cov(h, b, ptrs_of(keep, "P"), n_s.ctypes.data_as(ip), ptrs_of(keep, "Q"),
                                        n_t.ctypes.data_as(ip), init.ctypes.data_as(dp), par, out, None,
                                        ptrs_of(keep, "N"), est, ptrs_of(keep, "Cs"), ptrs_of(keep, "Ct"))
        msg = L.teaser_hip_icp_last_error(h).decode()
    assert rc == 0, msg
    return [np.array(o.transformation[:]).reshape(4, 4) for o in out]


def ptrs_of(keep, key):
    dp = C.POINTER(C.c_double)
    return (dp * len(keep))(*[None if k[key] is None else k[key].ctypes.data_as(dp) for k in keep])


def test_cov_entry_serves_a_mixed_batch_of_degenerate_and_regular_steps():
    """The three methods, singular and regular, through teaser_hip_icp_batch_cov in one call: the single runs' bits."""
    names = ["gi_mixed_singular", "pt_mirror_slab", "pl_parallel_normals", "gi_all_singular", "pl_tukey_edge",
             "pt_all_to_one", "gi_regular", "pl_one", "pt_5_collinear"]
    for n, T in zip(names, solve_cov([case(n) for n in names])):
        assert T.tobytes() == result(n).transformation.tobytes(), n


@pytest.mark.parametrize("near, then", [("near_pt", "pt_64"), ("near_pl", "pl_patch"), ("near_gi", "gi_regular")])
def test_near_singular_input_gives_a_rigid_transform_and_leaves_the_handle_sound(near, then):
    """Roughness of the order 2^-30 on a planar input: ill-conditioned by right, so only what must hold is asserted --
    a finite, proper rigid transform (the step or the identity) -- and the next well-posed call is unharmed."""
    c = {x["name"]: x for x in S.near_singular_cases()}[near]
    out = run(c)
    check_rigid(out.transformation)
    assert np.isfinite(out.fitness) and np.isfinite(out.inlier_rmse)
    check_unique(then, run(case(then)))
