#!/usr/bin/env python3
"""DBSCAN clustering on the MI355X: what a call costs.

  (a) a synthetic indoor scene with its plane removed (a handful of blobs plus sparse uniform noise, generated from a
      seed) at 10^5 and 10^6 points;
  (b) tests/golden/bun_zipper_res3.ply;
  (c) 64 clouds of 20 000 points in one call against the same 64 as single calls;
  (d) the same scenes through sklearn's DBSCAN(algorithm="kd_tree", n_jobs=16) on the host, where sklearn is importable:
      a DIFFERENT implementation (it tests d <= eps and stores every neighbourhood), not a parity target.

Every timing is a host clock around a Python call that ends in a device synchronise, after `--warmup` untimed calls:
median, minimum and maximum of `--reps` (at least nine).  Needs an MI355X: there is no CPU path.  `--only NAME` runs one
workload a few times without timing it, as the program of a kernel trace.

    python scripts/bench_dbscan.py --reps 9 --warmup 2 --out profiles/dbscan/bench_dbscan.json"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
tp = importlib.import_module("teaser-plusplus_amd")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def indoor_scene(n, seed):
    """What is left of a 6 x 6 x 2.5 room once its floor is gone: eight Gaussian blobs (sigma 0.15 .. 0.3) holding 95 %
    of the points, and 5 % uniform noise.  The point density grows with n; eps is chosen per n by the caller."""
    rng = np.random.default_rng(seed)
    blobs = 8
    centres = np.stack([rng.uniform(0.5, 5.5, blobs), rng.uniform(0.5, 5.5, blobs), rng.uniform(0.3, 2.0, blobs)], 1)
    sigma = rng.uniform(0.15, 0.3, blobs)
    n_noise = n // 20
    which = rng.integers(0, blobs, n - n_noise)
    P = centres[which] + sigma[which, None] * rng.standard_normal((n - n_noise, 3))
    noise = np.stack([rng.uniform(0, 6, n_noise), rng.uniform(0, 6, n_noise), rng.uniform(0, 2.5, n_noise)], 1)
    return np.ascontiguousarray(np.concatenate([P, noise])[rng.permutation(n)])


def read_ply_xyz(path):
    with open(path, "rb") as f:
        header = []
        while True:
            line = f.readline().decode("ascii", "replace").strip()
            header.append(line)
            if line == "end_header":
                break
        n = int([h.split()[2] for h in header if h.startswith("element vertex")][0])
        props = [h.split()[2] for h in header if h.startswith("property")]
        data = np.loadtxt(f, max_rows=n, dtype=np.float64)
        return np.ascontiguousarray(data[:, [props.index("x"), props.index("y"), props.index("z")]])


def summary(labels, counts, c):
    return dict(points=int(len(labels)), clusters=int(c), noise=int((labels < 0).sum()),
                mean_neighbours=float(counts.mean()) if len(counts) else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--only", default="", help="run this workload five times without timing it (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan", "bench_dbscan.json"))
    a = ap.parse_args()
    if a.reps < 9 and not a.only:
        sys.exit("at least nine runs")
    if tp.device_count() < 1:
        sys.exit("bench_dbscan.py needs an MI355X")
    # eps follows the density: on the order of a hundred neighbours at a blob's centre
    scenes = {"indoor_1e5": (indoor_scene(100000, 1), 0.08, 10), "indoor_1e6": (indoor_scene(1000000, 2), 0.04, 10),
              "bunny": (read_ply_xyz(os.path.join(ROOT, "tests", "golden", "bun_zipper_res3.ply")), 0.01, 5)}
    batch = [indoor_scene(20000, 100 + k) for k in range(64)]
    if a.only:
        for _ in range(5):
            if a.only == "batch64":
                tp.cluster_dbscan_batch(batch, 0.14, 10)
            else:
                P, eps, mp = scenes[a.only]
                tp.cluster_dbscan(P, eps, mp)
        return
    out = dict(reps=a.reps, warmup=a.warmup, scenes={})
    for name, (P, eps, mp) in scenes.items():
        labels, counts = tp.cluster_dbscan(P, eps, mp, return_counts=True)
        row = dict(eps=eps, min_points=mp, result=summary(labels, counts, labels.max() + 1),
                   device=timed(lambda: tp.cluster_dbscan(P, eps, mp), a.reps, a.warmup))
        out["scenes"][name] = row
        print(name, row, file=sys.stderr, flush=True)
    labels, ncl, counts = tp.cluster_dbscan_batch(batch, 0.14, 10, return_counts=True)
    out["batch64"] = dict(eps=0.14, min_points=10, points_per_cloud=20000,
                          clusters=[int(ncl.min()), int(ncl.max())],
                          mean_neighbours=float(np.mean([c.mean() for c in counts])),
                          one_call=timed(lambda: tp.cluster_dbscan_batch(batch, 0.14, 10), a.reps, a.warmup),
                          single_calls=timed(lambda: [tp.cluster_dbscan(c, 0.14, 10) for c in batch], a.reps, a.warmup))
    print("batch64", out["batch64"], file=sys.stderr, flush=True)
    if not a.no_sklearn:
        try:
            from sklearn.cluster import DBSCAN
        except ImportError:
            out["sklearn"] = "not importable: not run"
        else:
            out["sklearn"] = dict(note="a different implementation on the host (kd_tree, n_jobs=16, d <= eps): not a parity target")
            for name, (P, eps, mp) in scenes.items():
                fit = lambda: DBSCAN(eps=eps, min_samples=mp, algorithm="kd_tree", n_jobs=16).fit(P)  # noqa: E731
                t = time.perf_counter()
                sk = fit()
                first = time.perf_counter() - t
                reps = 9 if first < 4.0 else 3  # a fit of many seconds is run three times, and the file says so
                out["sklearn"][name] = dict(clusters=int(sk.labels_.max() + 1), noise=int((sk.labels_ < 0).sum()),
                                            host=timed(fit, reps, 0))
                print("sklearn", name, out["sklearn"][name], file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
