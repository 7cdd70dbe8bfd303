"""tests/fused_translation_model.py (the window form of the scalar TLS, as the fast route of estimate_fused_kernel computes
it) against the oracle's sweep (oracle.scalar_tls, registration.cc:21-88), on the CPU.

Where the reference is pinned the two are the same algorithm: same estimate to 1e-13, same inlier mask.  Two families are
recorded apart, so that the GPU tests' expectations (tests/test_gpu_estimator_edges.py) are explicit:
 (a) an opening and a closing of exactly equal value: the reference's std::sort leaves their order unspecified, the oracle
     keeps insertion order, the kernel puts the opening first -- they may differ, each returns a cost-minimal candidate
     of its own order;
 (b) values pairwise more than 2 beta apart: every consensus set is a singleton and the reference IS pinned -- its
     running sums return to exactly 0, every singleton costs exactly beta (K - 1), the first minimum is the smallest
     value.  A window sum (a + b) - a is not b in general, so singletons are evaluated exactly (x_hat = the value,
     residual = 0); the rule before that let an arbitrary singleton win by 1e-17.
     The pin has a limit of the reference's own making: its x_hat is (x w) / w with w = 1 / beta^2, which is x only where
     that division rounds back (always for beta a power of two; for beta = 0.01 always where the mantissa of x is below
     1.6).  Elsewhere its singleton residual is +-1e-17 too and its choice a matter of rounding; the `singletons` case
     keeps its values where the reference is pinned."""
import numpy as np
import pytest

import estimator_cases as EC
import fused_translation_model as M
from oracle import oracle

BETA = EC.NB
FAST_SIZES = [K for K in EC.SIZES if K <= M.MAX_K]


def _agree(x, beta):
    est = M.fused_tls(x, beta)
    oe, om = oracle.scalar_tls(x, np.full(len(x), beta))
    assert abs(est - oe) <= 1e-13, (est, oe)
    assert (M.inliers(x, est, beta) == om).all()


@pytest.mark.parametrize("K", FAST_SIZES)
def test_window_form_is_the_reference_sweep_on_random_data(K):
    """three quarters of the values clustered within the noise, one quarter uniform"""
    rng = np.random.default_rng(500 + K)
    for trial in range(6):
        n_cl = (3 * K) // 4
        x = np.concatenate([rng.uniform(-1, 1) + rng.uniform(-0.6 * BETA, 0.6 * BETA, size=n_cl),
                            rng.uniform(-1, 1, size=K - n_cl)])
        _agree(rng.permutation(x), BETA)


@pytest.mark.parametrize("K", [K for K in FAST_SIZES if K >= 8])
def test_window_form_is_the_reference_sweep_on_duplicated_values(K):
    """the translation residuals of the `dups` case: exactly equal values in the sort"""
    c = EC.case(K, "dups", EC.SEED)
    x = c["dst"] - c["R"] @ c["src"]
    h = K // 2
    assert (x[:, h:2 * h] == x[:, :h]).all()
    for a in range(3):
        _agree(x[a], BETA)


def test_prefix_sums_at_the_size_edges():
    """p1[i] is the sum of the first i sorted values at every size, the K = 512 entry p1[K] included"""
    rng = np.random.default_rng(77)
    for K in FAST_SIZES:
        sx = np.sort(rng.uniform(-1, 1, size=K))
        p1, p2 = M.prefix_sums(sx, K)
        assert p1.shape == (K + 1,) and p1[0] == 0 and p2[0] == 0
        for p, w in ((p1, sx), (p2, sx * sx)):   # any order of K additions: K eps max|partial sum|
            ref = np.concatenate([[0], np.cumsum(w)])
            assert np.abs(p - ref).max() <= K * np.finfo(float).eps * max(1.0, np.abs(ref).max())


def _order_costs(x, beta, opening_first):
    """[(cost, x_hat)] after every endpoint, in exact arithmetic, with equal endpoint values ordered as the oracle does
    (insertion order: x_i - beta, x_i + beta, x_{i+1} - beta, ...) or as the kernel does (an opening before a closing)"""
    from fractions import Fraction as F
    K = len(x)
    eps = [(F(x[i]) - F(beta), (0, i) if opening_first else (2 * i,), i, 1) for i in range(K)]
    eps += [(F(x[i]) + F(beta), (1, i) if opening_first else (2 * i + 1,), i, -1) for i in range(K)]
    card, s1, s2 = 0, F(0), F(0)
    out = []
    for _, _, i, e in sorted(eps):
        card += e
        s1 += e * F(x[i])
        s2 += e * F(x[i]) ** 2
        if card > 0:
            xh = s1 / card
            out.append((float(card * xh * xh + s2 - 2 * s1 * xh + F(beta) * (K - card)), float(xh)))
    return out


def test_exact_endpoint_ties_are_unpinned():
    """(a) values on a grid of 2^-6 with beta = 2^-7: x_i + beta == x_j - beta exactly for grid neighbours.  No equality
    between the two orders is asserted -- only that each returns a candidate of minimal cost in its own order (to the
    rounding of a cost, 1e-15: distinct windows can cost the same in exact arithmetic)."""
    beta = 2.0 ** -7
    rng = np.random.default_rng(5)
    differ = 0
    for trial in range(200):
        K = int(rng.integers(2, 12))
        x = rng.integers(-8, 8, size=K) * 2.0 ** -6
        est = M.fused_tls(x, beta)
        oe, _ = oracle.scalar_tls(x, np.full(K, beta))
        for got, opening_first in ((est, True), (oe, False)):
            costs = _order_costs(x.tolist(), beta, opening_first)
            least = min(c for c, _ in costs)
            assert any(abs(got - xh) <= 1e-15 for c, xh in costs if c <= least + 1e-15), (x, got, opening_first)
        differ += abs(est - oe) > 1e-13
    print("estimates that differ between the two tie orders: %d of 200" % differ)


SINGLETON_EXAMPLE = [0.29054346092738864, 0.3104011775136786]   # more than 2 beta = 2^-6 apart


def test_singletons_the_reference_returns_the_smallest_value():
    """(b) the reference is pinned on singletons, and the model follows it"""
    beta = 2.0 ** -7
    oe, om = oracle.scalar_tls(SINGLETON_EXAMPLE, np.full(2, beta))
    assert oe == min(SINGLETON_EXAMPLE) and om.tolist() == [True, False]
    assert M.fused_tls(SINGLETON_EXAMPLE, beta) == oe
    # the rule before: the second singleton's window sum is (a + b) - a, its residual -1e-17 instead of 0, and it wins
    assert M.fused_tls(SINGLETON_EXAMPLE, beta, exact_singletons=False) == max(SINGLETON_EXAMPLE)


def test_singletons_random():
    """(b) K in 2 .. 5, spacing just above 2 beta: oracle = smallest value = model, bit for bit"""
    beta = 2.0 ** -7
    rng = np.random.default_rng(6)
    old_rule_misses = 0
    for trial in range(2000):
        K = int(rng.integers(2, 6))
        x = rng.uniform(-1, 1) + np.cumsum(2 * beta + rng.uniform(1e-3, 6e-3, size=K))
        x = rng.permutation(x)
        oe, om = oracle.scalar_tls(x, np.full(K, beta))
        assert oe == x.min()
        assert M.fused_tls(x, beta) == oe
        old_rule_misses += M.fused_tls(x, beta, exact_singletons=False) != oe
    print("the prefix-difference rule picked another singleton in %d of 2000" % old_rule_misses)
    assert old_rule_misses > 0   # (the discrepancy this rule was replaced for is real)


def test_singletons_limit_of_the_pin():
    """beta = 0.01: values in [4, 6.4) (mantissa below 1.6) -- the reference returns the smallest; values in [6.4, 8) --
    the reference itself picks another singleton now and then"""
    rng = np.random.default_rng(8)
    other = {4.0: 0, 6.5: 0}
    for base in other:
        for trial in range(1500):
            K = int(rng.integers(2, 8))
            x = rng.permutation(base + rng.uniform(0, 0.02) + np.cumsum(rng.uniform(0.03, 0.04, size=K)))
            assert x.max() < (6.4 if base == 4.0 else 8.0)
            oe, _ = oracle.scalar_tls(x, np.full(K, BETA))
            other[base] += abs(oe - x.min()) > BETA
            assert M.fused_tls(x, BETA) == x.min()
    print("the reference returned another singleton than the smallest:", other)
    assert other[4.0] == 0 and other[6.5] > 0


@pytest.mark.parametrize("K", EC.SINGLETON_STAGE_SIZES)
def test_singletons_case(K):
    c = EC.case(K, "singletons", EC.SEED)
    x = c["dst"] - c["src"]
    for a in range(3):
        oe, _ = oracle.scalar_tls(x[a], np.full(K, BETA))
        # (x_hat = (x w) / w in the reference: up to an ulp off x where w = 1 / beta^2 is not a power of two)
        assert abs(oe - x[a].min()) <= 2 * np.finfo(float).eps * abs(oe) and M.fused_tls(x[a], BETA) == x[a].min()


def test_tie_cases_are_pinned_and_tell_a_dropped_tied_opening():
    """EC.TIE_DST: exact ties, yet oracle = model; the closing search with < for <= gives another estimate on every axis"""
    for a in range(3):
        x = EC.TIE_DST[a]
        assert (np.abs(np.subtract.outer(x, x)) == 2 * EC.TIE_NB).any()
        oe, om = oracle.scalar_tls(x, np.full(x.size, EC.TIE_NB))
        est = M.fused_tls(x, EC.TIE_NB)
        assert abs(est - oe) <= 1e-13 and (M.inliers(x, est, EC.TIE_NB) == om).all()
        assert abs(M.fused_tls(x, EC.TIE_NB, opening_first=False) - oe) > 0.04
