#!/usr/bin/env python3
"""Generates tests/golden/voxel_crop.npz: a spatial crop of the raw 3DMatch cloud cloud_bin_0.ply of the reference's
examples/teaser_python_fpfh_icp (float32 xyz at the scan's real density, about 40 k points) and the voxel
down-sampling restatement's output for it (tests/voxel_reference.py) at the tutorial's VOXEL_SIZE = 0.05:
means (float64), counts and trace (the output voxel of every input point).

Run from the repo root (needs /root/reference):  python tests/golden/make_voxel_golden.py
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import voxel_reference as R  # noqa: E402

REF = "/root/reference/examples/teaser_python_fpfh_icp/data/"
VOXEL = 0.05
TARGET = 40000


def read_xyz(path):
    """float32 xyz of a PLY, read by the example that consumes the tutorial's clouds."""
    spec = importlib.util.spec_from_file_location("fpfh_example", os.path.join(ROOT, "examples", "teaser_python_fpfh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex.read_ply_xyz(path)


def main():
    raw = read_xyz(REF + "cloud_bin_0.ply")
    centre = np.median(raw, axis=0)
    # the smallest cube around the median point that holds TARGET points (Chebyshev distance)
    d = np.max(np.abs(raw - centre), axis=1)
    half = np.sort(d)[TARGET - 1]
    crop = raw[d <= half]
    means, counts, trace = R.voxel_down_sample(crop.astype(np.float64), VOXEL)
    print("crop", crop.shape, "half-edge %.3f" % half, "->", means.shape, "max count", counts.max())
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "voxel_crop.npz"), points=crop,
                        voxel_size=np.float64(VOXEL), means=means, counts=counts, trace=trace)


if __name__ == "__main__":
    main()
