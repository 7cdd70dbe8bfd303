#!/usr/bin/env python3
"""Measures the batched outlier removal and the self k-NN under it (teaser-plusplus_amd.remove_statistical_outlier_batch /
remove_radius_outlier_batch / self_knn_batch) and prints ONE JSON object (and writes it to --out when given):
  config5     the two config-5 clouds (tests/golden/config5_clouds.npz, about 5 k points each): batch = 1 (one cloud
              per call) and batch = 64 (32 copies of the pair with seeded jitter in one call, against the same 64 as
              sequential single calls); statistical removal (20, 2.0), radius removal (16 points inside 3 voxels) and
              self k-NN (k = 20)
  single      one 313 395-point scan-like cloud (tests/voxel_reference.py scan_like): the same three calls
  host_ref    the same work on the same host with scipy.spatial.cKDTree (query k = 20 / query_ball_point with
              return_length), workers = 1 and workers = -1; it computes the distances in another order, so it is a
              speed baseline and a near-equality check (masks compared, differences counted), not the bit reference
Wall-clock medians over --reps calls after --warmup calls (every call is synchronous).  "fallbacks" is the number of
queries the whole-cloud scan served in the last call.  Usage:
    python scripts/bench_outliers.py [--reps 10] [--warmup 2] [--no-host-ref] [--out profiles/outliers/bench_outliers.json]"""
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
import voxel_reference as VR  # noqa: E402

tp = importlib.import_module("teaser-plusplus_amd")
NB, RATIO, K = 20, 2.0, 20


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def kdtree_statistical(P, nb, ratio, workers):
    from scipy.spatial import cKDTree
    d, _ = cKDTree(P).query(P, k=min(nb, len(P)), workers=workers)
    avg = d.reshape(len(P), -1).mean(axis=1)
    use = avg > 0
    mean = avg[use].sum() / len(P)
    std = np.sqrt(((avg[use] - mean) ** 2).sum() / (len(P) - 1))
    return use & (avg < mean + ratio * std)


def kdtree_radius(P, nb, r, workers):
    from scipy.spatial import cKDTree
    return cKDTree(P).query_ball_point(P, r * (1 - 1e-15), return_length=True, workers=workers) > nb


def workload(name, clouds, radius, nb_points, reps, warmup, host_ref):
    one = clouds[:1]
    res = dict(clouds=len(clouds), points=int(sum(len(c) for c in clouds)))
    calls = dict(statistical=lambda cs: tp.remove_statistical_outlier_batch(cs, NB, RATIO),
                 radius=lambda cs: tp.remove_radius_outlier_batch(cs, nb_points, radius),
                 self_knn=lambda cs: tp.self_knn_batch(cs, K, return_distance=True))
    for key, fn in calls.items():
        t1, o1 = timed(lambda: fn(one), reps, warmup)
        row = dict(batch1_ms=1e3 * t1)
        if key != "radius":
            row["fallbacks_batch1"] = tp.get_icp_option("knn_fallbacks")
        if len(clouds) > 1:
            tb, ob = timed(lambda: fn(clouds), reps, warmup)
            ts, _ = timed(lambda: [fn([c]) for c in clouds], max(reps // 4, 2), 1)
            row.update(batch_ms=1e3 * tb, sequential_ms=1e3 * ts, speedup=ts / tb)
        if key != "self_knn":
            row["kept_first_cloud"] = int(len(o1[0][1]))
        res[key] = row
    if host_ref:
        P = clouds[0]
        gpu_s = np.zeros(len(P), dtype=bool)
        gpu_s[tp.remove_statistical_outlier(P, NB, RATIO)[1]] = True
        gpu_r = np.zeros(len(P), dtype=bool)
        gpu_r[tp.remove_radius_outlier(P, nb_points, radius)[1]] = True
        ref = {}
        for workers in (1, -1):
            ts, ms = timed(lambda: kdtree_statistical(P, NB, RATIO, workers), 3, 1)
            tr, mr = timed(lambda: kdtree_radius(P, nb_points, radius, workers), 3, 1)
            ref["workers_%s" % ("all" if workers < 0 else workers)] = dict(
                statistical_ms=1e3 * ts, radius_ms=1e3 * tr, statistical_mask_differences=int((ms != gpu_s).sum()),
                radius_mask_differences=int((mr != gpu_r).sum()))
        ref["cores_available"] = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
        ref["first_cloud_points"] = len(P)
        res["host_ref_ckdtree_first_cloud"] = ref
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host-ref", action="store_true")
    ap.add_argument("--no-large", action="store_true", help="skip the 313 395-point cloud")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_outliers.py needs an MI355X")
    c5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    vox = float(c5["voxel_size"])
    pair = [c5["cloud_bin_0"].astype(np.float64), c5["cloud_bin_4"].astype(np.float64)]
    rng = np.random.default_rng(64)
    clouds = [pair[k % 2] + (0.0 if k < 2 else 0.05 * vox) * rng.standard_normal(pair[k % 2].shape) for k in range(64)]
    res = {"workload": "statistical (%d, %g) / radius / self k-NN (k = %d): config-5 clouds, batch 1 and 64; one "
                       "313 395-point cloud" % (NB, RATIO, K)}
    res["config5"] = workload("config5", clouds, 3 * vox, 16, a.reps, a.warmup, not a.no_host_ref)
    if not a.no_large:
        P = VR.scan_like()
        res["single"] = workload("single", [P], 0.05, 16, max(a.reps // 2, 3), 1, not a.no_host_ref)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
