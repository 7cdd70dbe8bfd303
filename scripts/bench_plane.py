#!/usr/bin/env python3
"""Plane segmentation on the MI355X: what a call costs at lidar sizes, what the early stop saves, what one batched call
buys, and which chunk_trials serves them.

The scenes are synthetic and generated here from a seed: a noisy ground plane (half of the points, noise 0.02) under
uniform clutter in a 20 x 20 x 4 box; distance_threshold 0.05, ransac_n 3.
  (a) one cloud of 10^5 points and one of 10^6 at `--iterations` trials (default 1 000), once with probability = 1 (no
      early stop: every trial is scored over every point) and once with the default 0.99999999; for the run without
      early stop also the rate of (hypothesis, point) evaluations per second of the WHOLE call (uploads, finish and
      host walk included: an end-to-end figure, not the score kernel's share of peak);
  (b) the 10^5 cloud without early stop at chunk_trials 64, 256, 1024 and 4096 (the knob's sweep);
  (c) `--clouds` clouds (default 64) of 20 000 points in ONE call against the same clouds one call after the other,
      default probability;
  (d) the numpy restatement (tests/plane_reference.py) of the first `--host-trials` trials of the 10^5 cloud on the same
      host -- the only baseline there is -- as time per trial.

Every timing is a host clock around a call that ends in a device synchronise, after `--warmup` untimed calls, median and
spread of `--reps`.  Needs an MI355X: there is no CPU path.

    python scripts/bench_plane.py --reps 5 --warmup 1 --out profiles/plane/bench_plane.json"""
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


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def scene(n, seed):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-1.0, 1.0, size=(n, 3)) * [10.0, 10.0, 2.0]
    on = rng.uniform(size=n) < 0.5
    P[on, 2] = 0.03 * P[on, 0] - 0.02 * P[on, 1] - 1.5 + rng.normal(0.0, 0.02, size=int(on.sum()))
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--host-trials", type=int, default=32)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane", "bench_plane.json"))
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_plane.py needs an MI355X")
    d, default_p = 0.05, 0.99999999
    res = dict(distance_threshold=d, iterations=a.iterations, chunk_trials=tp.get_plane_option("chunk_trials"),
               partial_bytes=tp.get_plane_option("partial_bytes"), single=[], chunk_sweep=[])
    sizes = [int(v) for v in a.sizes.split(",")]
    clouds = {n: scene(n, 1000 + k) for k, n in enumerate(sizes)}
    for n, P in clouds.items():
        for p in (1.0, default_p):
            last = []
            t = timed(lambda: last.append(tp.segment_plane_batch([P], d, 3, a.iterations, p, 5)[0]), a.reps, a.warmup)
            r = last[-1]
            row = dict(points=n, probability=p, trials=r.trials, inliers=len(r.inliers), fitness=r.fitness, **t)
            if p == 1.0:
                row["evaluations_per_s_whole_call"] = r.trials * n / (1e-3 * t["median_ms"])
            res["single"].append(row)
            print(json.dumps(row))
    P = clouds[sizes[0]]
    for chunk in (64, 256, 1024, 4096):
        tp.set_plane_option("chunk_trials", chunk)
        row = dict(points=len(P), chunk_trials=chunk,
                   **timed(lambda: tp.segment_plane_batch([P], d, 3, a.iterations, 1.0, 5), a.reps, a.warmup))
        res["chunk_sweep"].append(row)
        print(json.dumps(row))
    tp.set_plane_option("chunk_trials", res["chunk_trials"])
    small = [scene(20000, 2000 + k) for k in range(a.clouds)]
    seeds = [7 + k for k in range(a.clouds)]
    one = timed(lambda: tp.segment_plane_batch(small, d, 3, a.iterations, default_p, seeds), a.reps, a.warmup)
    each = timed(lambda: [tp.segment_plane_batch([c], d, 3, a.iterations, default_p, s) for c, s in zip(small, seeds)],
                 a.reps, a.warmup)
    got = tp.segment_plane_batch(small, d, 3, a.iterations, default_p, seeds)
    res["batch"] = dict(clouds=a.clouds, points=20000, one_call=one, one_call_each=each,
                        trials_min=min(r.trials for r in got), trials_max=max(r.trials for r in got))
    print(json.dumps(res["batch"]))
    import plane_reference as PR
    t = time.perf_counter()
    ref = PR.trials(P, d, 3, 5, 0, a.host_trials)
    host_ms = 1e3 * (time.perf_counter() - t)
    dev = tp.plane_trials_batch([P], d, 0, a.host_trials, 3, 5)[0]
    res["numpy_restatement"] = dict(points=len(P), trials=a.host_trials, ms_per_trial=host_ms / a.host_trials,
                                    equal_bits=bool(np.array_equal(ref["count"], dev["count"]) and
                                                    np.array_equal(ref["E"].view(np.uint64), dev["E"].view(np.uint64))))
    print(json.dumps(res["numpy_restatement"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
