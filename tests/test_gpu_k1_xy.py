"""GPU tests of the K1 filter in its X / Y formulation (two chained MFMAs per quarter tile, w from the chain's first
link): bitmap and degrees equal the oracle's bit for bit at the tile, quarter-tile and block-row edges of the kernel,
under exact power-of-two rescalings, with low pieces in the fp16 subnormal range, on pairs engineered onto the decision
boundary, at both ends of the admission range and just outside it, with an admitted and a refused problem in one batch
and with large point offsets.  Every case that has to run the FILTER is checked against the admission code itself
(k1c::consts_xy through the host program of test_k1_xy_consts_host.py): a case that fell back to the FP64 body would
prove nothing."""
import importlib

import numpy as np
import pytest

from oracle import oracle
from test_k1_f16_band_model import adversarial
from test_k1_xy_band_model import admitted_interval, operands_xy
from test_k1_xy_consts_host import host_consts_xy

pytestmark = pytest.mark.gpu

tp = importlib.import_module("teaser-plusplus_amd")


def k1_only_solver(nb):
    """Only the bitmap is under test: heuristic clique mode + a short time limit keep the stages behind K1 bounded."""
    return tp.RobustRegistrationSolver(tp.RobustRegistrationSolver.Params(
        noise_bound=nb, cbar2=1.0, estimate_scaling=False, rotation_gnc_factor=1.4, rotation_max_iterations=100,
        rotation_cost_threshold=0.005, inlier_selection_mode=tp.InlierSelectionMode.PMC_HEU, max_clique_time_limit=5.0))


def admitted(src, dst, nb):
    """src, dst [3, n]: the admission test of the pre-pass (beta = 2 nb at cbar2 = 1), evaluated by the device's code"""
    op = operands_xy(np.ascontiguousarray(src.T), np.ascontiguousarray(dst.T), 2 * nb)
    return host_consts_xy([(2 * nb, op["s"], op["r2"])])[0]["use_mfma"] == 1


def check_problem(solver, problem, src, dst, nb):
    n = src.shape[1]
    _, ref = oracle.inlier_bitmap(src, dst, nb, 1.0, False)
    assert (solver.getInlierGraphBitmap(problem) == ref).all()
    assert (solver.getDegrees(problem) == oracle.bitmap_to_dense(ref, n).sum(1)).all()


def check(src, dst, nb, expect_admitted=True):
    assert admitted(src, dst, nb) == expect_admitted
    s = k1_only_solver(nb)
    s.solve(src, dst)
    check_problem(s, 0, src, dst, nb)


@pytest.mark.parametrize("n", [2, 63, 64, 65, 129, 257, 513])
def test_tile_edges(n):
    """two points, one short of a tile, the diagonal tile and its padding (64, 65), a third tile (129), the edge of a
    four-row-tile block (257) and of an eight-tile column group (513)"""
    pr = tp.synth_problem(20251001 + n, n, 0.8, 0.01)
    check(pr["src"], pr["dst"], 0.01)


@pytest.mark.parametrize("k", [-6, 6])
def test_power_of_two_rescaling(k):
    pr = tp.synth_problem(20251002, 512, 0.8, 0.01)
    f = 2.0 ** k
    check(pr["src"] * f, pr["dst"] * f, 0.01 * f)


def test_anisotropic_cloud_with_subnormal_low_pieces():
    rng = np.random.default_rng(31)
    src, dst = adversarial(rng, 512, 1.0, 0.02, axes=(1.0, 1.0, 1e-4))
    check(np.ascontiguousarray(src.T), np.ascontiguousarray(dst.T), 0.01)


@pytest.mark.parametrize("scale,nb", [(1.0, 0.01), (250.0, 0.05)])
def test_adversarial_band(scale, nb):
    rng = np.random.default_rng(32)
    src, dst = adversarial(rng, 1024, scale, 2 * nb)
    check(np.ascontiguousarray(src.T), np.ascontiguousarray(dst.T), nb)


@pytest.fixture(scope="module")
def ends():
    """a cloud and the ends of the interval of beta the admission test admits on it: ((admitted, refused neighbour)
    at the lower end -- eta <= 1/8 --, the same at the upper end -- the short-pair limit)"""
    rng = np.random.default_rng(33)
    src, dst = adversarial(rng, 400, 1.0, 0.02)
    return src, dst, admitted_interval(src, dst)


@pytest.mark.parametrize("end,inside", [(0, True), (0, False), (1, True), (1, False)])
def test_ends_of_the_admission_range(ends, end, inside):
    """kappa at both ends of the admission range (the filter runs), and just outside each (the FP64 body runs and the
    result is the oracle's all the same); the boundary pairs of the cloud sit at beta = 0.02, the ends' own are the
    short pairs and whatever lies near them"""
    src, dst, iv = ends
    beta = iv[end][0 if inside else 1]
    check(np.ascontiguousarray(src.T), np.ascontiguousarray(dst.T), beta / 2, expect_admitted=inside)


def test_boundary_pairs_at_the_upper_end():
    """pairs engineered onto the boundary at the largest admitted beta of their own cloud"""
    rng = np.random.default_rng(34)
    probe = adversarial(np.random.default_rng(35), 400, 1.0, 0.02)
    beta = admitted_interval(*probe)[1][0] * 0.9
    src, dst = adversarial(rng, 400, 1.0, beta)
    check(np.ascontiguousarray(src.T), np.ascontiguousarray(dst.T), beta / 2)


def test_batch_of_an_admitted_and_a_refused_problem():
    """beta = 2e-7: far below the filter's resolution on a unit cloud (FP64 body, chosen per problem on the device),
    within it on the same cloud shrunk by 2^-13"""
    nb = 1e-7
    a = tp.synth_problem(20251003, 700, 0.5, nb)
    b = tp.synth_problem(20251004, 900, 0.5, nb * 2.0 ** 13)
    srcs, dsts = [a["src"], b["src"] * 2.0 ** -13], [a["dst"], b["dst"] * 2.0 ** -13]
    assert not admitted(srcs[0], dsts[0], nb) and admitted(srcs[1], dsts[1], nb)
    s = k1_only_solver(nb)
    s.solve_batch(srcs, dsts)
    for p in range(2):
        check_problem(s, p, srcs[p], dsts[p], nb)


def test_large_offsets():
    pr = tp.synth_problem(20251005, 1000, 0.8, 0.01)
    check(pr["src"] + np.array([[1e4], [-2e4], [3e4]]), pr["dst"] + np.array([[-5e3], [7e3], [1e3]]), 0.01)
