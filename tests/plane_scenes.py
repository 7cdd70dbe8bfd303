"""Inputs shared by the plane-segmentation tests: np.random.default_rng with fixed seeds, plus integer grids.  TEST
INFRASTRUCTURE ONLY."""
import numpy as np

GRID_PLANE = np.array([1.0, 2.0, 2.0, -6.0]) / 3.0  # x + 2 y + 2 z = 6


def grid_plane(n):
    """n integer points exactly on x + 2 y + 2 z = 6: (2 u, v, 3 - u - v) over a square of (u, v)."""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    u, v = k % side - side // 2, k // side - side // 2
    return np.stack([2.0 * u, 1.0 * v, 3.0 - u - v], axis=1)


def collinear(n):
    """n integer points on one line: every cross product is exactly zero."""
    k = np.arange(n, dtype=np.float64) - n // 3
    return np.stack([k, 2.0 * k, 3.0 * k], axis=1)


def planted(n, ratio, seed, noise=0.004):
    """A noisy plane z = 0.1 x - 0.2 y + 0.3 holding about `ratio` of the n points, shuffled among uniform clutter in
    [-1, 1]^3."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-1.0, 1.0, size=(n, 3))
    on = rng.uniform(size=n) < ratio
    P[on, 2] = 0.1 * P[on, 0] - 0.2 * P[on, 1] + 0.3 + rng.uniform(-noise, noise, size=int(on.sum()))
    return P


PLANTED_NORMAL = np.array([-0.1, 0.2, 1.0, -0.3]) / np.sqrt(0.01 + 0.04 + 1.0)
