#!/usr/bin/env python3
"""RGB-D odometry (compute_rgbd_odometry_batch on the ICP handle) on the MI355X: what a pair costs alone, what a batch
buys, and where the time goes.

  (1) one 640 x 480 pair per call (uint16 depth, float32 intensity, the hybrid term, the default options: 35 iterations
      on three levels);
  (2) 64 such pairs (consecutive frames of the trajectory of examples/teaser_python_odometry.py, eight frames eight
      times over) in ONE call against 64 calls; the two must give the same bits;
  (3) the preprocessing and pyramid stage alone, for one pair and for 64.

Call times are a host clock around a Python call that ends in a device synchronise, after `--warmup` untimed calls:
median, minimum and maximum of `--reps` (at least nine).  A call includes the host's checks, the packing of the rows, the
upload, the launches, the copy back and the synchronisation.

Kernel time comes from a run of its own: `--profile-workload one_call` (or `pair`) runs the calls and writes nothing;
`rocprofv3 --kernel-trace --stats` is pointed at it, and its kernel_stats.csv is kept beside the JSON.  Needs an MI355X:
there is no CPU path.

    python scripts/bench_odometry.py --reps 9 --warmup 1 --out profiles/odometry/bench_odometry.json"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
tp = importlib.import_module("teaser-plusplus_amd")
ex = importlib.import_module("teaser_python_odometry")

W, H, PAIRS, FRAMES = 640, 480, 64, 9


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def workload():
    """(K, 64 sources, 64 targets, the true motions)."""
    K, poses, depths, paints = ex.sequence(W, H, FRAMES)
    frames = [tp.RGBDImage.create_from_color_and_depth(c, d, depth_scale=1000.0, depth_trunc=6.0) for c, d in zip(paints, depths)]
    rep = PAIRS // (FRAMES - 1)
    return K, frames[:-1] * rep, frames[1:] * rep, [ex.true_motion(poses, k) for k in range(FRAMES - 1)] * rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-workload", choices=["one_call", "pair"], default=None)
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_odometry.py needs an MI355X: no HIP device visible")
    K, src, tgt, truth = workload()
    option = tp.OdometryOption(depth_max=6.0)

    def one_call(n=PAIRS):
        return tp.compute_rgbd_odometry_batch(src[:n], tgt[:n], K, option=option)

    def many_calls():
        return [tp.compute_rgbd_odometry_batch(src[k:k + 1], tgt[k:k + 1], K, option=option)[0] for k in range(PAIRS)]

    if a.profile_workload:
        for _ in range(3):
            one_call(PAIRS if a.profile_workload == "one_call" else 1)
        return
    batch, single = one_call(), many_calls()
    same = all(x.success == y.success and x.count == y.count and x.transformation.tobytes() == y.transformation.tobytes()
               and x.information.tobytes() == y.information.tobytes() for x, y in zip(batch, single))
    errs = [ex.pose_error(r.transformation, t) for r, t in zip(batch, truth)]
    n_iter = sum(option.iteration_number_per_pyramid_level)
    out = dict(workload=dict(width=W, height=H, pairs=PAIRS, iterations=option.iteration_number_per_pyramid_level,
                             launches_per_call=3 * len(option.iteration_number_per_pyramid_level) + 4 + 3 * n_iter + 3),
               same_bits_one_call_and_64_calls=bool(same), successes=int(sum(r.success for r in batch)),
               correspondences=[int(r.count) for r in batch[:FRAMES - 1]],
               max_rotation_error_deg=float(max(e[0] for e in errs)), max_translation_error_m=float(max(e[1] for e in errs)))
    out["one_pair_per_call"] = timed(lambda: one_call(1), a.reps, a.warmup)
    out["one_call_64_pairs"] = timed(one_call, a.reps, a.warmup)
    out["calls_64"] = timed(many_calls, a.reps, a.warmup)
    out["pyramid_one_pair"] = timed(lambda: tp.rgbd_odometry_pyramid_batch(src[:1], tgt[:1], K, option=option), a.reps, a.warmup)
    out["pyramid_one_call_8_pairs"] = timed(lambda: tp.rgbd_odometry_pyramid_batch(src[:8], tgt[:8], K, option=option), a.reps, a.warmup)
    for key in ("one_call_64_pairs", "calls_64"):
        out[key]["ms_per_pair"] = out[key]["median_ms"] / PAIRS
    out["batch_speedup"] = out["calls_64"]["median_ms"] / out["one_call_64_pairs"]["median_ms"]
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
