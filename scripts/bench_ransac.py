#!/usr/bin/env python3
"""RANSAC registration on correspondences on the MI355X: what one batched call buys, and what a long run costs.

The correspondences come from the config-5 fixture pair (tests/golden/config5_clouds.npz: FPFH + one-directional nearest
neighbours on the device, about 5 k pairs); every problem of the batch is that pair with its source moved by its own
seeded rigid transform, and has its own RANSAC seed.  Edge-length checker 0.9, distance checker and
max_correspondence_distance 1.5 voxels, ransac_n 3.
  (a) `--pairs` problems (default 64) at `--iterations` trials (default 10 000, confidence 0.999) in ONE call, and the
      same problems one call after the other;
  (a') the same batch without checkers, so that every one of the 64 x 10 000 hypotheses is scored over all pairs (the
      score kernel's workload: with the checkers on, a few dozen trials per problem survive them);
  (b) one pair at 100 000 trials with confidence 1 (no early stop), at chunk_trials 4096 and 65536;
  (c) the numpy restatement (tests/ransac_reference.py) of the first `--host-trials` trials of one pair on the same
      host -- the only baseline there is -- as time per trial.

Every timing is a host clock around a call that ends in a device synchronise, after `--warmup` untimed calls, median and
spread of `--reps`.  Needs an MI355X: there is no CPU path.

    python scripts/bench_ransac.py --reps 5 --warmup 1 --out profiles/ransac/bench_ransac.json"""
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


def rigid(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return Rm, rng.uniform(-1, 1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=10000)
    ap.add_argument("--host-trials", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac", "bench_ransac.json"))
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_ransac.py needs an MI355X")
    c5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    A, B, vox = c5["cloud_bin_0"], c5["cloud_bin_4"], float(c5["voxel_size"])
    fa, fb = tp.compute_fpfh_batch([A, B], 2 * vox, 5 * vox)
    pairs = tp.feature_matching_correspondences(fa, fb, False)
    A, B = A.astype(np.float64), B.astype(np.float64)
    rng = np.random.default_rng(2024)
    srcs = []
    for _ in range(a.pairs):
        Rm, t = rigid(rng)
        srcs.append((A - t) @ Rm)
    dsts, cors = [B] * a.pairs, [pairs] * a.pairs
    r = 1.5 * vox
    checkers = [tp.CorrespondenceCheckerBasedOnEdgeLength(0.9), tp.CorrespondenceCheckerBasedOnDistance(r)]
    kw = dict(max_correspondence_distance=r, ransac_n=3, checkers=checkers)
    crit = tp.RANSACConvergenceCriteria(a.iterations, 0.999)
    seeds = list(range(1, a.pairs + 1))
    out = dict(points=[len(A), len(B)], correspondences=len(pairs), pairs=a.pairs, iterations=a.iterations)

    def batch():
        return tp.registration_ransac_based_on_correspondence_batch(srcs, dsts, cors, criteria=crit, seed=seeds, **kw)

    res = batch()
    out["batch_results"] = dict(trials=[min(x.trials for x in res), max(x.trials for x in res)],
                                valid_trials=[min(x.valid_trials for x in res), max(x.valid_trials for x in res)],
                                fitness=[min(x.fitness for x in res), max(x.fitness for x in res)])
    out["batch_one_call"] = timed(batch, a.reps, a.warmup)
    out["single_calls"] = timed(lambda: [tp.registration_ransac_based_on_correspondence(
        srcs[k], dsts[k], cors[k], criteria=crit, seed=seeds[k], **kw) for k in range(a.pairs)], a.reps, a.warmup)
    loose = dict(kw, checkers=[])
    one = tp.registration_ransac_based_on_correspondence_batch(srcs, dsts, cors, criteria=tp.RANSACConvergenceCriteria(
        a.iterations, 1.0), seed=seeds, **loose)
    out["batch_no_checkers"] = timed(lambda: tp.registration_ransac_based_on_correspondence_batch(
        srcs, dsts, cors, criteria=tp.RANSACConvergenceCriteria(a.iterations, 1.0), seed=seeds, **loose), a.reps, a.warmup)
    out["batch_no_checkers"].update(trials=[min(x.trials for x in one), max(x.trials for x in one)],
                                    valid_trials=[min(x.valid_trials for x in one), max(x.valid_trials for x in one)],
                                    scored_pairs=int(sum(x.valid_trials for x in one)) * len(pairs))
    print(json.dumps({k: out[k] for k in ("batch_results", "batch_one_call", "single_calls", "batch_no_checkers")}),
          flush=True)
    long_crit = tp.RANSACConvergenceCriteria(100000, 1.0)
    before = tp.get_ransac_option("chunk_trials")
    out["one_pair_100k"] = {}
    try:
        for chunk in (4096, 65536):
            tp.set_ransac_option("chunk_trials", chunk)
            one = tp.registration_ransac_based_on_correspondence(srcs[0], B, pairs, criteria=long_crit, seed=1, **kw)
            row = timed(lambda: tp.registration_ransac_based_on_correspondence(srcs[0], B, pairs, criteria=long_crit,
                                                                               seed=1, **kw), a.reps, a.warmup)
            row.update(trials=one.trials, valid_trials=one.valid_trials, fitness=one.fitness)
            out["one_pair_100k"][str(chunk)] = row
    finally:
        tp.set_ransac_option("chunk_trials", before)
    print(json.dumps(dict(one_pair_100k=out["one_pair_100k"])), flush=True)
    if a.host_trials > 0:
        import ransac_reference as RR
        t = time.perf_counter()
        ref = RR.trial_records(srcs[0], B, pairs, r, 0, a.host_trials, 3, 0.9, r, 1)
        ms = 1e3 * (time.perf_counter() - t)
        dev = tp.ransac_trials_batch([srcs[0]], [B], [pairs], r, 0, a.host_trials, None, 3, checkers, 1)[0]
        out["numpy_restatement"] = dict(trials=a.host_trials, ms=ms, ms_per_trial=ms / a.host_trials,
                                        valid_trials=int((ref["flags"] & 4).astype(bool).sum()),
                                        samples_agree=bool(np.array_equal(ref["samples"], dev["samples"])),
                                        edge_flags_agree=bool(np.array_equal(ref["flags"] & 1, dev["flags"] & 1)))
        print(json.dumps(dict(numpy_restatement=out["numpy_restatement"])), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
