"""The structured restatement of the certifier's dual projection (tests/certifier_reference.py, the reference of the GPU
stage tests above N = 129) pinned on the CPU against the oracle's dense route (oracle/certifier.py: linear_projection +
optimal_dual_projection).  Nothing is measured here: the structured route runs in longdouble, the dense one in FP64, so
they may differ by the dense route's own rounding, k eps sum|terms| per element with k the operation count of that
element's path (as in tests/test_gpu_certifier_stages.py)."""
import numpy as np
import pytest

import certifier_reference as CR

EPS = float(np.finfo(np.float64).eps)


def thetas(N, rng):
    one = -np.ones(N)
    one[rng.integers(N)] = 1.0
    return dict(random=rng.choice([-1.0, 1.0], size=N), inliers=np.ones(N), outliers=-np.ones(N), single=one)


@pytest.mark.parametrize("N", range(1, 41))
def test_structured_projection_matches_the_dense_oracle(N):
    assert np.finfo(np.longdouble).eps < 1e-18  # the reference needs a real extended type
    rng = np.random.default_rng(1000 + N)
    n = 4 * N + 4
    cls = CR.element_classes(N)
    assert sum(m.sum() for m in cls.values()) == n * n
    for kind, theta in thetas(N, rng).items():
        thp = np.concatenate([[1.0], theta])
        W = rng.normal(size=(n, n))  # not symmetric: the blocks below the diagonal must not be read
        dense, terms = CR.dual_projection_dense(W, thp)
        got, terms_s = CR.dual_projection_structured(W, thp)
        # the two routes' term sums are the same quantity
        assert np.abs(terms_s - terms).max() <= 1e-12 * float(terms.max()), kind
        err = np.abs(got - dense).astype(np.float64)
        t = terms.astype(np.float64)
        # operation counts per path: see test_gpu_certifier_stages.py
        for name, k in (("off33", 2), ("offborder", 4 * N + 12), ("diagborder", 4 * N + 12 + N + 2), ("diag33", 2 * N + 2)):
            m = cls[name]
            assert (err[m] <= k * EPS * t[m]).all(), (kind, name, float((err[m] / np.maximum(t[m], 1e-300)).max() / EPS))
        assert (got != 0).sum() >= (dense != 0).sum()  # (not vacuous: the structured route fills what the dense one fills)
