#!/usr/bin/env python3
"""Fast Global Registration on correspondences on the MI355X: what one batched call buys, and the two routes.

The correspondences come from the config-5 fixture pair (tests/golden/config5_clouds.npz: FPFH + one-directional nearest
neighbours on the device, about 5 k pairs); every problem of the batch is that pair with its source moved by its own
seeded rigid transform.  Options at Open3D's defaults, maximum_correspondence_distance 0.5 voxels, no tuple test (the
solve is what is timed); the timed call is teaser_hip_fgr_correspondence_batch alone, that is
registration_fgr_based_on_correspondence_batch WITHOUT its evaluate_registration step (timed apart, once).
  (a) `--pairs` problems (default 64) in ONE call and the same problems one call after the other, on the streamed route
      (about 5 k pairs exceed the resident bound) and, cut to their first 3 000, 1 000 and 250 pairs, on the resident
      route (resident_max_corr 3072 for 3 000, 1024 below) and on the streamed route (0);
  (b) one pair at about 10^5 correspondences (the pairs repeated) on the streamed route, and one pair at 3 000 on both;
  (c) the numpy restatement (tests/fgr_reference.py, float64) of one 3 000-pair problem on the same host -- the only
      baseline there is.

Every timing is a host clock around a call that ends in a device synchronise, after `--warmup` untimed calls, median and
spread of `--reps`.  Needs an MI355X: there is no CPU path.

    python scripts/bench_fgr.py --reps 5 --warmup 1 --out profiles/fgr/bench_fgr.json"""
import argparse
import ctypes as C
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


def solve_only(srcs, dsts, cors, opt):
    """teaser_hip_fgr_correspondence_batch alone (no evaluation): the list of poses."""
    F = tp.fgr
    b, src, dst, cor, opts, params = F._gather(srcs, dsts, cors, opt)
    args, keep = F._args(src, dst, cor, params)
    out = (F.FgrResultC * b)()
    h = F._cache.get(-1)
    h.call(h._lib.teaser_hip_fgr_correspondence_batch, b, *args, out)
    return [np.array(out[k].transformation[:]).reshape(4, 4) for k in range(b)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fgr", "bench_fgr.json"))
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_fgr.py needs an MI355X")
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
    dsts = [B] * a.pairs
    opt = tp.FastGlobalRegistrationOption(maximum_correspondence_distance=0.5 * vox, tuple_test=False)
    out = dict(points=[len(A), len(B)], correspondences=len(pairs), pairs=a.pairs)
    before = tp.get_fgr_option("resident_max_corr")
    try:
        for label, cor, knob in (("streamed_all_pairs", pairs, 0), ("resident_3000_pairs", pairs[:3000], 3072),
                                 ("streamed_3000_pairs", pairs[:3000], 0), ("resident_1000_pairs", pairs[:1000], 1024),
                                 ("streamed_1000_pairs", pairs[:1000], 0), ("resident_250_pairs", pairs[:250], 1024),
                                 ("streamed_250_pairs", pairs[:250], 0)):
            tp.set_fgr_option("resident_max_corr", knob)
            cors = [cor] * a.pairs
            row = dict(correspondences=len(cor), resident_max_corr=knob)
            row["one_call"] = timed(lambda: solve_only(srcs, dsts, cors, opt), a.reps, a.warmup)
            row["single_calls"] = timed(lambda: [solve_only([srcs[k]], [B], [cor], opt) for k in range(a.pairs)],
                                        a.reps, a.warmup)
            row["one_pair"] = timed(lambda: solve_only([srcs[0]], [B], [cor], opt), a.reps, a.warmup)
            out[label] = row
            print(json.dumps({label: row}), flush=True)
        big = np.concatenate([pairs] * (100000 // len(pairs) + 1))[:100000]
        tp.set_fgr_option("resident_max_corr", 0)
        out["one_pair_100k_streamed"] = timed(lambda: solve_only([srcs[0]], [B], [big], opt), a.reps, a.warmup)
        out["one_pair_100k_streamed"]["correspondences"] = len(big)
        print(json.dumps(dict(one_pair_100k_streamed=out["one_pair_100k_streamed"])), flush=True)
        tp.set_fgr_option("resident_max_corr", before)
        full = tp.registration_fgr_based_on_correspondence_batch(srcs, dsts, [pairs] * a.pairs, opt)
        out["with_evaluation_one_call"] = timed(
            lambda: tp.registration_fgr_based_on_correspondence_batch(srcs, dsts, [pairs] * a.pairs, opt), a.reps, a.warmup)
        out["fitness"] = [min(r.fitness for r in full), max(r.fitness for r in full)]
    finally:
        tp.set_fgr_option("resident_max_corr", before)
    import fgr_reference as FR
    t = time.perf_counter()
    ref = FR.fgr(srcs[0], B, pairs[:3000], maximum_correspondence_distance=0.5 * vox)
    ms = 1e3 * (time.perf_counter() - t)
    dev = solve_only([srcs[0]], [B], [pairs[:3000]], opt)[0]
    out["numpy_restatement"] = dict(correspondences=3000, ms=ms,
                                    max_abs_difference_from_device=float(np.abs(ref["transformation"] - dev).max()))
    print(json.dumps(dict(numpy_restatement=out["numpy_restatement"], with_evaluation=out["with_evaluation_one_call"],
                          fitness=out["fitness"])), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
