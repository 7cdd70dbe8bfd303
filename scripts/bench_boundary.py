#!/usr/bin/env python3
"""Boundary-point detection (compute_boundary_points on the ICP handle) on the MI355X: what a call costs.

  (1) the two config-5 clouds (5 208 and 5 034 points, tests/golden/config5_clouds.npz) at the tutorial's normal
      neighbourhood -- Hybrid(2 voxels, 30), threshold 90 degrees, normals estimated inside the call -- as ONE call and
      as two calls; the same with the normals given (estimated once, outside the timing);
  (2) 64 such clouds (the two clouds, each jittered by a hundredth of a voxel from a seed) in one call and as 64 calls;
  (3) one cloud of 300 000 points, uniform in a cube whose density gives a 2-voxel ball about 30 points, with the
      default "fpfh_list_bytes" (one pass) and with a bound that forces several passes;
  (4) the numpy restatement (tests/boundary_reference.py) on one config-5 cloud, on the device's own normals, and whether
      the device's mask and gaps equal it.

With --profile-workload the script only runs three calls of workload (2) and writes nothing: it is what
`rocprofv3 --kernel-trace --stats` is pointed at for the split between the list search and the boundary kernel.

Every timing is a host clock around a Python call that ends in a device synchronise, after `--warmup` untimed calls:
median, minimum and maximum of `--reps` (at least nine; the numpy restatement: two).  Needs an MI355X: there is no CPU
path.

    python scripts/bench_boundary.py --reps 9 --warmup 2 --out profiles/boundary/bench_boundary.json"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
tp = importlib.import_module("teaser-plusplus_amd")
import boundary_reference as R  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--profile-workload", action="store_true", help="three calls of the 64-cloud workload, nothing else")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary", "bench_boundary.json"))
    a = ap.parse_args()
    if a.reps < 9:
        sys.exit("at least nine runs")
    if tp.device_count() < 1:
        sys.exit("bench_boundary.py needs an MI355X")
    c5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    A, B, vox = c5["cloud_bin_0"].astype(np.float64), c5["cloud_bin_4"].astype(np.float64), float(c5["voxel_size"])
    sp = tp.KDTreeSearchParamHybrid(2 * vox, 30)
    inside = lambda clouds: tp.compute_boundary_points_batch(clouds, None, sp, 90.0, normal_search=sp)  # noqa: E731
    rng = np.random.default_rng(2024)
    many = [(A if k % 2 == 0 else B) + 0.01 * vox * rng.standard_normal((len(A) if k % 2 == 0 else len(B), 3))
            for k in range(64)]
    if a.profile_workload:
        for _ in range(3):
            inside(many)
        return
    out = dict(reps=a.reps, warmup=a.warmup, voxel=vox, points=[len(A), len(B)], max_nn=30, angle_threshold=90.0,
               fpfh_list_bytes=tp.get_icp_option("fpfh_list_bytes"))

    pair = [A, B]
    normals = tp.estimate_normals_batch(pair, sp)
    res = inside(pair)
    out["config5_pair"] = dict(
        boundary_points=[r.n_boundary for r in res],
        one_call=timed(lambda: inside(pair), a.reps, a.warmup),
        two_calls=timed(lambda: [inside([c]) for c in pair], a.reps, a.warmup),
        one_call_normals_given=timed(lambda: tp.compute_boundary_points_batch(pair, normals, sp, 90.0), a.reps, a.warmup),
        normals_alone_one_call=timed(lambda: tp.estimate_normals_batch(pair, sp), a.reps, a.warmup))
    print("pair", out["config5_pair"], file=sys.stderr, flush=True)

    out["config5_x64"] = dict(
        clouds=64, points=int(sum(map(len, many))),
        one_call=timed(lambda: inside(many), a.reps, a.warmup),
        single_calls=timed(lambda: [inside([c]) for c in many], a.reps, a.warmup))
    print("x64", out["config5_x64"], file=sys.stderr, flush=True)

    n_big = 300000
    edge = (n_big * 4.0 / 3.0 * np.pi * (2 * vox) ** 3 / 30.0) ** (1.0 / 3.0)  # about 30 points in a 2-voxel ball
    big = np.random.default_rng(9).random((n_big, 3)) * edge
    default = tp.get_icp_option("fpfh_list_bytes")
    gaps = lambda: tp.compute_boundary_points_batch([big], None, sp, 90.0, normal_search=sp, return_max_gap=True)[0]  # noqa: E731
    row = dict(points=n_big, cube_edge=float(edge), list_bytes_needed=12 * 30 * n_big,
               one_pass=timed(lambda: inside([big]), a.reps, a.warmup))
    try:
        tp.set_icp_option("fpfh_list_bytes", 16 << 20)
        row["bound_16MiB_several_passes"] = timed(lambda: inside([big]), a.reps, a.warmup)
        few = gaps()
    finally:
        tp.set_icp_option("fpfh_list_bytes", default)
    row["passes_at_16MiB"] = -(-12 * 30 * n_big // (16 << 20))
    full = gaps()
    row["boundary_points"] = full.n_boundary
    row["same_bits_at_both_bounds"] = bool(few.max_gap.tobytes() == full.max_gap.tobytes() and
                                           np.array_equal(few.mask, full.mask))
    out["big_300k"] = row
    print("big", row, file=sys.stderr, flush=True)

    if not a.no_host:
        r = tp.compute_boundary_points_batch([A], None, sp, 90.0, normal_search=sp, return_max_gap=True,
                                             return_normals=True)[0]
        host = lambda: R.boundary_points(A, r.normals, R.HYBRID, 2 * vox, 30, 90.0)  # noqa: E731
        mask, gap, _ = host()
        out["numpy_restatement_cloud_bin_0"] = dict(
            timed(host, 2, 0), equal_to_device=bool(gap.tobytes() == r.max_gap.tobytes() and np.array_equal(mask, r.mask)))
        print("numpy", out["numpy_restatement_cloud_bin_0"], file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
