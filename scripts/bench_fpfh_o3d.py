#!/usr/bin/env python3
"""The Open3D-form FPFH (compute_fpfh_feature on the ICP handle) on the MI355X: what a call costs.

  (1) the two config-5 clouds (5 208 and 5 034 points, tests/golden/config5_clouds.npz) at the tutorial's parameters --
      normals Hybrid(2 voxels, 30), features Hybrid(5 voxels, 100), normals estimated inside the call -- as ONE call and
      as two calls; the same with the normals given (estimated once, outside the timing);
  (2) 64 such clouds (the two clouds, each jittered by a hundredth of a voxel from a seed) in one call and as 64 calls;
  (3) one cloud of 300 000 points, uniform in a cube whose density matches config 5's neighbour counts roughly (edge
      chosen so that a 5-voxel ball holds about 100 points), with the default "fpfh_list_bytes" (one pass) and with a
      bound that forces several passes (the lists computed twice);
  (4) the numpy restatement (tests/fpfh_o3d_reference.py) on one config-5 cloud, on the device's own normals, and whether
      the device's rows equal it;
  (5) for orientation only: compute_fpfh_batch, the PCL form (float32, uncapped radius, its own normals), on the clouds of
      (1) and (2).  It is another descriptor: the two are not interchangeable, and the times are not a ranking.

Every timing is a host clock around a Python call that ends in a device synchronise, after `--warmup` untimed calls:
median, minimum and maximum of `--reps` (at least nine; the numpy restatement: two).  Needs an MI355X: there is no CPU
path.

    python scripts/bench_fpfh_o3d.py --reps 9 --warmup 2 --out profiles/fpfh_o3d/bench_fpfh_o3d.json"""
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
import fpfh_o3d_reference as R  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_o3d", "bench_fpfh_o3d.json"))
    a = ap.parse_args()
    if a.reps < 9:
        sys.exit("at least nine runs")
    if tp.device_count() < 1:
        sys.exit("bench_fpfh_o3d.py needs an MI355X")
    c5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    A, B, vox = c5["cloud_bin_0"].astype(np.float64), c5["cloud_bin_4"].astype(np.float64), float(c5["voxel_size"])
    nsp, fsp = tp.KDTreeSearchParamHybrid(2 * vox, 30), tp.KDTreeSearchParamHybrid(5 * vox, 100)
    inside = lambda clouds: tp.compute_fpfh_feature_batch(clouds, None, fsp, normal_search=nsp)  # noqa: E731
    out = dict(reps=a.reps, warmup=a.warmup, voxel=vox, points=[len(A), len(B)],
               fpfh_list_bytes=tp.get_icp_option("fpfh_list_bytes"))

    pair = [A, B]
    normals = tp.estimate_normals_batch(pair, nsp)
    lists = R.neighbour_lists(A, R.HYBRID, 5 * vox, 100)[2] if not a.no_host else None
    out["config5_pair"] = dict(
        one_call=timed(lambda: inside(pair), a.reps, a.warmup),
        two_calls=timed(lambda: [inside([c]) for c in pair], a.reps, a.warmup),
        one_call_normals_given=timed(lambda: tp.compute_fpfh_feature_batch(pair, normals, fsp), a.reps, a.warmup),
        normals_alone_one_call=timed(lambda: tp.estimate_normals_batch(pair, nsp), a.reps, a.warmup),
        pcl_form_one_call=timed(lambda: tp.compute_fpfh_batch(pair, 2 * vox, 5 * vox), a.reps, a.warmup))
    if lists is not None:
        out["config5_pair"]["neighbours_cloud_bin_0"] = dict(mean=float(lists.mean()), capped_at_100=int((lists == 100).sum()))
    print("pair", out["config5_pair"], file=sys.stderr, flush=True)

    rng = np.random.default_rng(2024)
    many = [(A if k % 2 == 0 else B) + 0.01 * vox * rng.standard_normal((len(A) if k % 2 == 0 else len(B), 3))
            for k in range(64)]
    out["config5_x64"] = dict(
        clouds=64, points=int(sum(map(len, many))),
        one_call=timed(lambda: inside(many), a.reps, a.warmup),
        single_calls=timed(lambda: [inside([c]) for c in many], a.reps, a.warmup),
        pcl_form_one_call=timed(lambda: tp.compute_fpfh_batch(many, 2 * vox, 5 * vox), a.reps, a.warmup))
    print("x64", out["config5_x64"], file=sys.stderr, flush=True)

    n_big = 300000
    edge = (n_big * 4.0 / 3.0 * np.pi * (5 * vox) ** 3 / 100.0) ** (1.0 / 3.0)  # about 100 points in a 5-voxel ball
    big = np.random.default_rng(9).random((n_big, 3)) * edge
    default = tp.get_icp_option("fpfh_list_bytes")
    row = dict(points=n_big, cube_edge=float(edge), list_bytes_needed=12 * 100 * n_big,
               one_pass=timed(lambda: inside([big]), a.reps, a.warmup))
    try:
        tp.set_icp_option("fpfh_list_bytes", 64 << 20)
        row["bound_64MiB_several_passes"] = timed(lambda: inside([big]), a.reps, a.warmup)
        few = inside([big])[0]
    finally:
        tp.set_icp_option("fpfh_list_bytes", default)
    row["passes_at_64MiB"] = -(-12 * 100 * n_big // (64 << 20))
    row["same_bits_at_both_bounds"] = bool(few.tobytes() == inside([big])[0].tobytes())
    out["big_300k"] = row
    print("big", row, file=sys.stderr, flush=True)

    if not a.no_host:
        F, N = tp.compute_fpfh_feature_batch([A], None, fsp, normal_search=nsp, return_normals=True)[0]
        host = lambda: R.compute_fpfh_feature(A, N, R.HYBRID, 5 * vox, 100)  # noqa: E731
        out["numpy_restatement_cloud_bin_0"] = dict(timed(host, 2, 0), equal_to_device=bool(host()[0].tobytes() == F.tobytes()))
        print("numpy", out["numpy_restatement_cloud_bin_0"], file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
