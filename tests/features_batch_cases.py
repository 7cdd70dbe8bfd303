"""Inputs shared by the batched front-end's tests and scripts/bench_features.py."""
import os

import numpy as np

from util import ROOT


def config5_pairs(count, seed=555):
    """`count` perturbed copies of the 3DMatch pair of tests/golden/config5_clouds.npz, generated as bench.py's
    config-5 workload generates them: the source cloud moved by a seeded random rigid transform, both clouds jittered
    by N(0, (0.1 voxel)^2) noise.  Returns (list of source clouds, list of target clouds, voxel size), float32."""
    C5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    A0, B0, vox = C5["cloud_bin_0"].astype(np.float64), C5["cloud_bin_4"].astype(np.float64), float(C5["voxel_size"])
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for _ in range(count):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                       [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        tv = rng.uniform(-1, 1, 3)
        src.append(((A0 + 0.1 * vox * rng.standard_normal(A0.shape) - tv) @ Rm).astype(np.float32))
        dst.append((B0 + 0.1 * vox * rng.standard_normal(B0.shape)).astype(np.float32))
    return src, dst, vox


def sparse_cloud():
    """The 302-point cloud with isolated points of test_gpu_features.test_fpfh_sparse_points_and_limits."""
    rng = np.random.default_rng(5)
    return np.concatenate([rng.uniform(0, 0.2, size=(300, 3)), [[5, 5, 5], [9, 9, 9]]]).astype(np.float32)


def ball_cloud():
    """The 5 000-point ball of test_gpu_features.test_fpfh_more_than_4096_neighbours (radii 0.2, 1.1)."""
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(5000, 3))
    return (pts / np.linalg.norm(pts, axis=1, keepdims=True) * rng.uniform(0, 0.5, size=(5000, 1)) ** (1 / 3)).astype(np.float32)
