#!/usr/bin/env python3
"""Neighbour search between two clouds on the MI355X: what a call costs.

  (a) 64 problems of 10 000 queries against 10 000 data points (both uniform in the unit cube, from seeds; "voxel size"
      0.05, about the spacing of such a cloud): k-NN at k = 1, 8 and 30, hybrid search at (2 voxels, 30) and the uncapped
      radius search at 2 voxels (count-then-fill: two calls of the library) -- each in ONE call, as 64 calls, and as the
      numpy restatement (tests/search_reference.py) on the same host for one problem (times 64: extrapolated);
  (b) one pair of 300 000 x 300 000 points at k = 8;
  (c) one partial-overlap pair: 10 000 queries, half of them outside the data's box (the data cloud shifted by half its
      extent), k = 8, with "knn_fallbacks" recorded, and the same pair with "knn_ring_cap" = 0 (every query scanned);
  (d) one radius call whose rows average about 2 000 entries (2 000 queries, 10 000 data points, radius 0.42), so that
      the cost of the quadratic rank pass is on record; the single call with an exact size hint and a hybrid search
      of the same radius (which ranks nothing) are timed beside the count-then-fill pair.

Every timing is a host clock around a Python call that ends in a device synchronise, after `--warmup` untimed calls:
median, minimum and maximum of `--reps` (at least nine; the numpy restatement: two).  Needs an MI355X: there is no
CPU path.

    python scripts/bench_search.py --reps 9 --warmup 2 --out profiles/search/bench_search.json"""
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
import search_reference as S  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "bench_search.json"))
    a = ap.parse_args()
    if a.reps < 9:
        sys.exit("at least nine runs")
    if tp.device_count() < 1:
        sys.exit("bench_search.py needs an MI355X")
    B, N, vox = 64, 10000, 0.05
    data = [np.random.default_rng(100 + b).random((N, 3)) for b in range(B)]
    query = [np.random.default_rng(500 + b).random((N, 3)) for b in range(B)]
    out = dict(reps=a.reps, warmup=a.warmup, problems=B, points=N, voxel=vox, knn_ring_cap=tp.get_icp_option("knn_ring_cap"))
    work = [("knn_k1", lambda d, q: tp.knn_search_batch(d, q, 1), lambda d, q: S.knn_search(d, q, 1)),
            ("knn_k8", lambda d, q: tp.knn_search_batch(d, q, 8), lambda d, q: S.knn_search(d, q, 8)),
            ("knn_k30", lambda d, q: tp.knn_search_batch(d, q, 30), lambda d, q: S.knn_search(d, q, 30)),
            ("hybrid_2vox_30", lambda d, q: tp.hybrid_search_batch(d, q, 2 * vox, 30),
             lambda d, q: S.hybrid_search(d, q, 2 * vox, 30)),
            ("radius_2vox", lambda d, q: tp.radius_search_batch(d, q, 2 * vox), lambda d, q: S.radius_search(d, q, 2 * vox))]
    for name, dev, host in work:
        row = dict(one_call=timed(lambda: dev(data, query), a.reps, a.warmup),
                   single_calls=timed(lambda: [dev([d], [q]) for d, q in zip(data, query)], a.reps, a.warmup))
        if name.startswith("knn"):
            dev(data, query)
            row["knn_fallbacks"] = tp.get_icp_option("knn_fallbacks")
        if name.startswith("radius"):
            row["entries"] = int(sum(len(r[0]) for r in dev(data, query)))
        if not a.no_host:
            got, ref = dev(data[:1], query[:1])[0], host(data[0], query[0])
            row["numpy_one_problem"] = timed(lambda: host(data[0], query[0]), 2, 0)
            row["numpy_64_problems_ms_extrapolated"] = B * row["numpy_one_problem"]["median_ms"]
            row["equal_to_numpy"] = bool(all(np.array_equal(x, y) for x, y in zip(got, ref)))
        out[name] = row
        print(name, row, file=sys.stderr, flush=True)

    big_d, big_q = np.random.default_rng(7).random((300000, 3)), np.random.default_rng(8).random((300000, 3))
    out["big_300k_k8"] = timed(lambda: tp.knn_search(big_d, big_q, 8), a.reps, a.warmup)
    out["big_300k_k8"]["knn_fallbacks"] = tp.get_icp_option("knn_fallbacks")
    print("big", out["big_300k_k8"], file=sys.stderr, flush=True)

    shifted = data[0] + [0.5, 0.0, 0.0]  # half of it outside the data's box
    cap = tp.get_icp_option("knn_ring_cap")
    part = dict(queries=N, outside=int((shifted[:, 0] > data[0][:, 0].max()).sum()),
                rings=timed(lambda: tp.knn_search(data[0], shifted, 8), a.reps, a.warmup))
    part["knn_fallbacks"] = tp.get_icp_option("knn_fallbacks")
    try:
        tp.set_icp_option("knn_ring_cap", 0)
        part["scan_only"] = timed(lambda: tp.knn_search(data[0], shifted, 8), a.reps, a.warmup)
        part["scan_only_fallbacks"] = tp.get_icp_option("knn_fallbacks")
    finally:
        tp.set_icp_option("knn_ring_cap", cap)
    out["partial_overlap_k8"] = part
    print("partial", part, file=sys.stderr, flush=True)

    long_q = query[0][:2000]
    rows = tp.radius_search(data[0], long_q, 0.42)
    total = len(rows[0])
    out["long_rows"] = dict(queries=len(long_q), data=N, radius=0.42, entries=total, mean_row=total / len(long_q),
                            longest_row=int(np.diff(rows[2]).max()),
                            count_then_fill=timed(lambda: tp.radius_search(data[0], long_q, 0.42), a.reps, a.warmup),
                            one_call_with_hint=timed(lambda: tp.radius_search(data[0], long_q, 0.42, max_total=total),
                                                     a.reps, a.warmup),
                            hybrid_100_same_radius=timed(lambda: tp.hybrid_search(data[0], long_q, 0.42, 100), a.reps,
                                                         a.warmup))
    print("long rows", out["long_rows"], file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
