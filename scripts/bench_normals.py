#!/usr/bin/env python3
"""Measures batched normal estimation and the point-to-plane ICP that estimates its own target normals, and prints ONE
JSON object (and writes it to --out when given).  Every timing is a wall-clock median over --reps calls after --warmup
calls; every call ends with the library's own stream synchronisation, so the synchronisation is inside the timer.
"spread" is (max - min) / median of the repeats.

  hybrid      normals of the config-5 target at radius 2 voxels, max_nn 30, one cloud per call and 64 clouds per call,
              next to estimate_covariances_batch with the same radius and max_nn (the same search; 24 against 72 bytes
              written per point)
  knn         normals with k-NN search, k = 30, next to self_knn_batch at k = 30, the same two batch sizes
  auto        registration_icp(target_normals=KDTreeSearchParamHybrid(2 voxels, 30)) against estimate_normals followed
              by registration_icp(target_normals=array) on the dense ~250 k-point pair of scripts/bench_icp.py
  touched     estimate_covariances_batch, remove_statistical_outlier and self_knn on the config-5 target: the calls
              whose kernels share device code with normal estimation

Comparison with another commit: run the script on both with --only parent (the calls that exist on both: the
covariance, self k-NN and statistical-removal rows) and --out to two files, alternating the two runs several times;
--compare A.json B.json prints the ratio of the medians of every row both files have, next to both spreads.
Usage:
    python scripts/bench_normals.py [--reps 15] [--warmup 3] [--only all|parent] [--no-dense]
                                    [--out profiles/normals/bench_normals.json]
    python scripts/bench_normals.py --compare parent.json this.json"""
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
import icp_reference as R  # noqa: E402

tp = importlib.import_module("teaser-plusplus_amd")
MAX_NN = 30


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    med = float(np.median(ts))
    return dict(ms=1e3 * med, spread=(max(ts) - min(ts)) / med, reps=reps)


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    rows = {}
    for group in a:
        if not isinstance(a[group], dict) or group not in b:
            continue
        for name, ra in a[group].items():
            rb = b[group].get(name)
            if isinstance(ra, dict) and isinstance(rb, dict) and "ms" in ra and "ms" in rb:
                rows["%s.%s" % (group, name)] = dict(a_ms=ra["ms"], b_ms=rb["ms"], b_over_a=rb["ms"] / ra["ms"],
                                                     a_spread=ra["spread"], b_spread=rb["spread"])
    print(json.dumps(rows, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["all", "parent"], default="all")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if tp.device_count() < 1:
        sys.exit("bench_normals.py needs an MI355X")
    P, Q, vox, init = R.config5_problem()
    radius = 2 * vox
    rng = np.random.default_rng(31)
    many = [Q + rng.normal(0, 1e-4, size=Q.shape) for _ in range(64)]
    new = a.only == "all"
    res = {"workload": "config-5 target (%d points), radius %.4f, max_nn %d; 64 jittered copies per batched call"
                       % (len(Q), radius, MAX_NN)}
    t = lambda fn, few=False: timed(fn, max(a.reps // 3, 3) if few else a.reps, 1 if few else a.warmup)  # noqa: E731

    hy = {"covariances_single": t(lambda: tp.estimate_covariances_batch([Q], radius, MAX_NN)),
          "covariances_batch64": t(lambda: tp.estimate_covariances_batch(many, radius, MAX_NN), True)}
    kn = {"self_knn_single": t(lambda: tp.self_knn_batch([Q], MAX_NN)),
          "self_knn_batch64": t(lambda: tp.self_knn_batch(many, MAX_NN), True)}
    if new:
        sp, kp = tp.KDTreeSearchParamHybrid(radius, MAX_NN), tp.KDTreeSearchParamKNN(MAX_NN)
        hy["normals_single"] = t(lambda: tp.estimate_normals_batch([Q], sp))
        hy["normals_batch64"] = t(lambda: tp.estimate_normals_batch(many, sp), True)
        hy["normals_with_cov_and_eig_single"] = t(
            lambda: tp.estimate_normals_batch([Q], sp, covariances=True, eigenvalues=True))
        kn["normals_single"] = t(lambda: tp.estimate_normals_batch([Q], kp))
        kn["normals_batch64"] = t(lambda: tp.estimate_normals_batch(many, kp), True)
        kn["fallbacks_last_call"] = int(tp.get_icp_option("knn_fallbacks"))
        for g in (hy, kn):
            for size in ("single", "batch64"):
                base = g["covariances_" + size] if g is hy else g["self_knn_" + size]
                g["normals_over_base_" + size] = g["normals_" + size]["ms"] / base["ms"]
    res["hybrid"], res["knn"] = hy, kn
    res["touched"] = {"estimate_covariances_batch": hy["covariances_single"],
                      "self_knn": t(lambda: tp.self_knn(Q, 20)),
                      "remove_statistical_outlier": t(lambda: tp.remove_statistical_outlier(Q, 20, 2.0))}
    if new and not a.no_dense:
        drng = np.random.default_rng(5)  # the dense pair of scripts/bench_icp.py
        A = np.repeat(P, 48, axis=0) + drng.normal(0, 0.01, size=(48 * len(P), 3))
        B = np.repeat(Q, 50, axis=0) + drng.normal(0, 0.01, size=(50 * len(Q), 3))
        sp = tp.KDTreeSearchParamHybrid(radius, MAX_NN)
        est = tp.TransformationEstimationPointToPlane(tp.TukeyLoss(vox / 2))
        crit = tp.ICPConvergenceCriteria(max_iteration=100)
        one = lambda: tp.registration_icp(A, B, vox, init, est, crit, target_normals=sp)  # noqa: E731
        two = lambda: tp.registration_icp(A, B, vox, init, est, crit,  # noqa: E731
                                          target_normals=tp.estimate_normals(B, sp))
        r1, r2 = one(), two()
        res["auto"] = {"points": [len(A), len(B)], "iterations": r1.iterations,
                       "same_bits": bool(r1.transformation.tobytes() == r2.transformation.tobytes()),
                       "self_estimating_call": timed(one, 5, 1), "two_call_form": timed(two, 5, 1)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
