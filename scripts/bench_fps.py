#!/usr/bin/env python3
"""Farthest-point down-sampling on the MI355X: what a call costs.

  (a) 64 clouds of 10 000 points, K = 1 000, in ONE call against the same 64 as single calls (resident route);
  (b) the same call with "fps_resident_max" = 0: the streamed route on identical work, and the time per round of both;
  (c) one cloud of 300 000 points, K = 5 000 (streamed): the call and the time per round;
  (d) the numpy restatement (tests/fps_reference.py) on the same host for one cloud of (a) and for (c).

The clouds are uniform in the unit cube, generated from seeds.  Every timing is a host clock around a Python call that
ends in a device synchronise, after `--warmup` untimed calls: median, minimum and maximum of `--reps` (at least nine).
The results of (a) and (b) are compared byte for byte in the same run.  Needs an MI355X: there is no CPU path.

    python scripts/bench_fps.py --reps 9 --warmup 2 --out profiles/fps/bench_fps.json"""
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
import fps_reference as RF  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps", "bench_fps.json"))
    a = ap.parse_args()
    if a.reps < 9:
        sys.exit("at least nine runs")
    if tp.device_count() < 1:
        sys.exit("bench_fps.py needs an MI355X")
    B, N, K = 64, 10000, 1000
    batch = [np.random.default_rng(100 + b).random((N, 3)) for b in range(B)]
    big, big_k = np.random.default_rng(7).random((300000, 3)), 5000
    cap = tp.get_icp_option("fps_resident_max")
    out = dict(reps=a.reps, warmup=a.warmup, fps_resident_max=cap)

    def per_round(row, k):
        row["us_per_round"] = 1e3 * row["median_ms"] / k
        return row

    try:
        resident = tp.farthest_point_down_sample_batch(batch, K)
        one = per_round(timed(lambda: tp.farthest_point_down_sample_batch(batch, K), a.reps, a.warmup), K)
        single = timed(lambda: [tp.farthest_point_indices(c, K) for c in batch], a.reps, a.warmup)
        alone = per_round(timed(lambda: tp.farthest_point_indices(batch[0], K), a.reps, a.warmup), K)
        tp.set_icp_option("fps_resident_max", 0)
        streamed = tp.farthest_point_down_sample_batch(batch, K)
        one_s = per_round(timed(lambda: tp.farthest_point_down_sample_batch(batch, K), a.reps, a.warmup), K)
        alone_s = per_round(timed(lambda: tp.farthest_point_indices(batch[0], K), a.reps, a.warmup), K)
    finally:
        tp.set_icp_option("fps_resident_max", cap)
    out["batch64"] = dict(clouds=B, points_per_cloud=N, num_samples=K,
                          routes_identical=all(r.tobytes() == s.tobytes() for r, s in zip(resident, streamed)),
                          resident_one_call=one, resident_single_calls=single, resident_one_cloud=alone,
                          streamed_one_call=one_s, streamed_one_cloud=alone_s)
    print("batch64", out["batch64"], file=sys.stderr, flush=True)
    out["big"] = dict(points=len(big), num_samples=big_k,
                      streamed=per_round(timed(lambda: tp.farthest_point_indices(big, big_k), a.reps, a.warmup), big_k))
    print("big", out["big"], file=sys.stderr, flush=True)
    if not a.no_host:
        ref = RF.fps(batch[0], K)[0]
        ref_big = RF.fps(big, big_k)[0]
        out["numpy"] = dict(note="tests/fps_reference.py on the same host, one thread of numpy",
                            one_cloud_of_batch64=timed(lambda: RF.fps(batch[0], K), 9, 0),
                            all_64_clouds_ms_extrapolated=None,
                            big=timed(lambda: RF.fps(big, big_k), 3, 0),
                            equal_to_device=bool(np.array_equal(ref, resident[0]) and
                                                 np.array_equal(ref_big, tp.farthest_point_indices(big, big_k))))
        out["numpy"]["all_64_clouds_ms_extrapolated"] = 64 * out["numpy"]["one_cloud_of_batch64"]["median_ms"]
        print("numpy", out["numpy"], file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
